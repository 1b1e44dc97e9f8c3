// The four owners of csrc/lm_own.h against the stub runtime of tests/cpp/hip_stub (a table of live handles, a k-th-call failure): what
// is live after every operation, by the stub's table AND by the header's own counts, and the order of frees and allocations.
// Stand-alone (tests/test_own_cpu.py builds it plain and under ASan + UBSan); prints "OK <checks>".
#include "lm_own.h"

#include <cstdio>
#include <utility>

using namespace lmd;

static long g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// the stub's table and the header's counts agree on (device, pinned, streams, events), and the stub saw no bad free
static bool live_is(long dv, long pn, long st, long ev) {
    return stub.bad == 0 && stub.count('d') == dv && stub.count('p') == pn && stub.count('s') == st && stub.count('e') == ev &&
           g_live[OWN_DEV] == dv && g_live[OWN_PINNED] == pn && g_live[OWN_STREAM] == st && g_live[OWN_EVENT] == ev;
}

template <typename O, typename Make>
static int lifecycle(Make make, int kind) {
    const auto only = [&](long n) { return live_is(kind == 0 ? n : 0, kind == 1 ? n : 0, kind == 2 ? n : 0, kind == 3 ? n : 0); };
    { O a; CHECK(!a && a.get() == nullptr && only(0)); }                       // empty: nothing to release
    { O a; CHECK(make(a) == hipSuccess && a && only(1)); }                     // construct, destroy
    CHECK(only(0));
    { O a; make(a); O b(std::move(a)); CHECK(!a && b && only(1)); }            // move-construct
    CHECK(only(0));
    {
        O a, b; make(a); make(b);
        const auto hb = b.get();
        CHECK(only(2));
        a = std::move(b);                                                        // move-assign onto a non-empty owner: a's old handle goes
        CHECK(a.get() == hb && !b && only(1));
        O& self = a;
        a = std::move(self);                                                     // self-move keeps it
        CHECK(a.get() == hb && only(1));
        a.reset(); CHECK(!a && only(0));
        a.reset(); CHECK(only(0));                                               // ... and a second reset frees nothing twice
    }
    { O a; make(a); const auto h0 = a.get(); make(a); CHECK(a && only(1)); (void)h0; }   // creating again releases the first
    { O a; make(a); const auto h = a.release(); CHECK(!a && only(1)); O b(h); CHECK(b.get() == h && only(1)); }   // hand out, take back: counted once
    CHECK(only(0));
    { O a; stub.arm(1); CHECK(make(a) != hipSuccess && !a && only(0)); stub.arm(0); }    // a failed create leaves it empty
    return 0;
}

static int test_grow() {
    DevBuf<int> b;
    CHECK(b.grow(100) == hipSuccess && b.size() == 100 && live_is(1, 0, 0, 0));
    int* p = b.get();
    stub.log.clear();
    CHECK(b.grow(100) == hipSuccess && b.grow(7) == hipSuccess && b.get() == p && b.size() == 100 && stub.log.empty());   // large enough: kept
    CHECK(b.grow(101) == hipSuccess && b.size() == 101 && stub.log == "fa" && live_is(1, 0, 0, 0));    // released BEFORE the allocation
    stub.arm(1);
    CHECK(b.grow(500) != hipSuccess && !b && b.size() == 0 && live_is(0, 0, 0, 0));                    // a failed grow: empty, count 0
    stub.arm(0);
    CHECK(b.grow(3) == hipSuccess && b.size() == 3);
    PinnedBuf<char> h;
    stub.log.clear();
    CHECK(h.grow(10) == hipSuccess && h.grow(10) == hipSuccess && h.grow(11) == hipSuccess && stub.log == "afa" && live_is(1, 1, 0, 0));
    DevBuf<short> v;
    CHECK(upload_vec(v, std::vector<short>{1, 2, 3}) == hipSuccess && v.size() == 3 && v.get()[2] == 3);
    CHECK(upload_vec(v, std::vector<short>()) == hipSuccess && v.size() == 1 && live_is(2, 1, 0, 0));   // an empty list still has an address
    return 0;
}

// the shape of ensure_device / ensure_lane: a dozen owners of all four kinds, filled by a function that returns at the first failure
struct Dozen {
    DevBuf<unsigned char> arena, aux;
    PinnedBuf<unsigned char> blocks, table;
    Stream lane[3], copy;
    Event ev[3];
    DevBuf<int> lut;
    bool ready = false;
};
#define TRY(e) do { if ((e) != hipSuccess) return false; } while (0)
static bool fill(Dozen& d) {
    if (d.ready) return true;
    TRY(d.arena.alloc(4096)); TRY(d.aux.alloc(512));
    TRY(d.blocks.alloc(256, hipHostMallocMapped)); TRY(d.table.alloc(128));
    for (Stream& s : d.lane) TRY(s.create(hipStreamNonBlocking));
    TRY(d.copy.create(hipStreamNonBlocking, 1));
    for (Event& e : d.ev) TRY(e.create(hipEventDisableTiming));
    TRY(d.lut.alloc(64));
    return d.ready = true;
}
static const long N_FILL = 12;

static int test_ensure_shape() {
    { Dozen d; stub.arm(0); CHECK(fill(d) && stub.calls == N_FILL && live_is(3, 2, 4, 3)); }
    CHECK(live_is(0, 0, 0, 0));
    for (long k = 1; k <= N_FILL; ++k) {
        {   // the k-th call fails: what came into being before it is owned, and goes with the struct
            Dozen d; stub.arm(k);
            CHECK(!fill(d) && !d.ready && (long)stub.live.size() == k - 1);
        }
        CHECK(live_is(0, 0, 0, 0));
        {   // ... and a second attempt after the failed one starts at the top: every member releases what it holds before it creates
            // again -- never more live than one full set, no handle left without an owner -- and the struct's end frees everything
            Dozen d; stub.arm(k);
            CHECK(!fill(d));
            stub.arm(0); stub.log.clear();
            CHECK(fill(d) && d.ready && live_is(3, 2, 4, 3));
            long frees = 0; for (char c : stub.log) frees += c == 'f';
            CHECK(frees == k - 1 && (long)stub.log.size() == N_FILL + k - 1);
            CHECK(fill(d) && stub.calls == N_FILL);      // ready: a further call creates nothing
        }
        CHECK(live_is(0, 0, 0, 0));
        {   // ... also when the second attempt fails as well, at any later call
            Dozen d; stub.arm(k); CHECK(!fill(d));
            stub.arm(N_FILL + 1 - k); CHECK(!fill(d) && (long)stub.live.size() <= N_FILL);
        }
        CHECK(live_is(0, 0, 0, 0));
    }
    stub.arm(0);
    return 0;
}

int main() {
    if (lifecycle<DevBuf<float>>([](DevBuf<float>& b) { return b.alloc(16); }, 0)) return 1;
    if (lifecycle<PinnedBuf<float>>([](PinnedBuf<float>& b) { return b.alloc(16, hipHostMallocMapped); }, 1)) return 1;
    if (lifecycle<Stream>([](Stream& s) { return s.create(hipStreamNonBlocking); }, 2)) return 1;
    if (lifecycle<Stream>([](Stream& s) { return s.create(hipStreamNonBlocking, 1); }, 2)) return 1;
    if (lifecycle<Event>([](Event& e) { return e.create(hipEventDisableTiming); }, 3)) return 1;
    if (test_grow()) return 1;
    if (!live_is(0, 0, 0, 0)) { std::printf("FAILED: live after test_grow\n"); return 1; }
    if (test_ensure_shape()) return 1;
    std::printf("OK %ld\n", g_checks);
    return 0;
}
