// reduce_host.cpp -- csrc/lm_reduce.h on the host: lmx::span / lmx::weight, lmx::colour_pixel (through lmx::pixel, the per-source-pixel
// load and conversion k_reduce stages), lmx::depth_nearest / lmx::depth_min_valid and lmx::plan_tile, with a memory read that dereferences
// the address, over a source that ENDS where its malloc block ends.  Built by tests/test_reduce_cpu.py with g++ -ffp-contract=off, plain
// and under ASan / UBSan, and compared there with tests/reduce_reference.py.  No GPU, nothing loaded into Python.
//   reduce_host image IN OUT   IN: 16 int64 (kind, swap_rb, matrix, width, height, row_stride, plane_stride, offset, nbytes, num_x, den_x,
//                              num_y, den_y, mode, pipeline, 0), one double (scale), with pipeline != 0: 13 int32 (black, gain[3], ccm[9])
//                              and 4096 tone bytes, then nbytes source bytes.  The source is copied to the last nbytes of a block of
//                              offset + nbytes bytes.  mode 0: colour, 1: depth NEAREST, 2: depth MIN_VALID.
//                              OUT: the whole reduced image, one uint32 per pixel (B | G << 8 | R << 16, or the depth)
//   reduce_host axis num den n      per reduced pixel X < R one line "first count w0 w1 ..." (the taps of lmx::span and their lmx::weight)
//   reduce_host finish NUM_X NUM_Y   lmx::finish_fast against lmx::finish for every accumulator 0 .. 256 num_x num_y, lmx::small_div against /
//   reduce_host plan num_x den_x num_y den_y     "tw th sw sh lds_bytes", and the largest patch any tile position needs in a 4096-pixel side
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lm_reduce.h"

static std::vector<unsigned char> read_all(const char* path) {
    std::vector<unsigned char> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    unsigned char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

// the kernel's loads, on the host: typed reads at the address itself (a misaligned u16 / u32 read is UBSan's to report)
struct HostLd {
    lmx::u32 b8(lmx::addr_t p) const { return *reinterpret_cast<const uint8_t*>(p); }
    lmx::u32 b16(lmx::addr_t p) const { return *reinterpret_cast<const uint16_t*>(p); }
    lmx::u32 b32(lmx::addr_t p) const { return *reinterpret_cast<const uint32_t*>(p); }
};
struct HostTone {
    const unsigned char* t;
    lmx::u32 operator()(lmx::u32 i) const { return i < 4096u ? t[i] : (std::abort(), 0u); }
};

static int image(const char* in_path, const char* out_path) {
    const std::vector<unsigned char> in = read_all(in_path);
    int64_t hd[16];
    double scale;
    size_t head = sizeof(hd) + 8;
    if (in.size() < head) { std::fprintf(stderr, "bad input size\n"); return 2; }
    std::memcpy(hd, in.data(), sizeof(hd));
    std::memcpy(&scale, in.data() + sizeof(hd), 8);
    lmi::RawPipe pipe = lmi::RawPipe();
    std::vector<unsigned char> tone(4096, 0);
    if (hd[14]) {
        int32_t p[13];
        if (in.size() < head + sizeof(p) + 4096) { std::fprintf(stderr, "bad input size\n"); return 2; }
        std::memcpy(p, in.data() + head, sizeof(p));
        pipe.black = p[0];
        for (int k = 0; k < 3; ++k) pipe.gain[k] = (lmx::u32)p[1 + k];
        for (int k = 0; k < 9; ++k) pipe.ccm[k] = p[4 + k];
        std::memcpy(tone.data(), in.data() + head + sizeof(p), 4096);
        head += sizeof(p) + 4096;
    }
    const size_t offset = (size_t)hd[7], nbytes = (size_t)hd[8];
    if (in.size() != head + nbytes) { std::fprintf(stderr, "bad input size\n"); return 2; }
    unsigned char* block = static_cast<unsigned char*>(std::malloc(offset + nbytes));      // the source ends where the block ends
    if (!block) return 2;
    std::memcpy(block + offset, in.data() + head, nbytes);
    lmq::Src s;
    s.data = (lmx::addr_t)reinterpret_cast<uintptr_t>(block + offset);
    s.kind = (int)hd[0]; s.swap_rb = (int)hd[1]; s.matrix = (int)hd[2]; s.width = (int)hd[3]; s.height = (int)hd[4];
    s.row_stride = hd[5]; s.plane_stride = hd[6]; s.scale = (float)scale;
    s.dwords = s.kind == LMQ_PX4 && s.data % 4 == 0 && s.row_stride % 4 == 0;      // as the library sets it
    const lmx::Ratio r = {(int)hd[9], (int)hd[10], (int)hd[11], (int)hd[12]};
    const int mode = (int)hd[13];
    const int rw = lmx::reduced_size(s.width, r.num_x, r.den_x), rh = lmx::reduced_size(s.height, r.num_y, r.den_y);
    std::vector<uint32_t> out((size_t)rw * (size_t)rh);
    const HostTone ht = {tone.data()};
    for (int Y = 0; Y < rh; ++Y)
        for (int X = 0; X < rw; ++X)
            out[(size_t)Y * rw + X] = mode == 0 ? lmx::colour_pixel(s, pipe, r, X, Y, HostLd(), ht)
                                    : mode == 1 ? lmx::depth_nearest(s, r, X, Y, HostLd()) : lmx::depth_min_valid(s, r, X, Y, HostLd());
    std::free(block);
    FILE* f = std::fopen(out_path, "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 4, out.size(), f);
    std::fclose(f);
    std::printf("OK %d %d\n", rw, rh);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "image")) return image(argv[2], argv[3]);
    if (argc == 5 && !std::strcmp(argv[1], "axis")) {
        const int num = std::atoi(argv[2]), den = std::atoi(argv[3]), n = std::atoi(argv[4]);
        if (num < den || den < 1 || n < 1) return 2;
        const int R = lmx::reduced_size(n, num, den);
        std::printf("OK %d\n", R);
        for (int X = 0; X < R; ++X) {
            const lmx::Span sp = lmx::span(X, num, den);
            std::printf("%d %d", sp.first, sp.count);
            for (int k = 0; k < sp.count; ++k) std::printf(" %d", lmx::weight(X, sp.first + k, num, den));
            // (the neighbours of the span weigh nothing)
            std::printf(" | %d %d\n", lmx::weight(X, sp.first - 1, num, den), lmx::weight(X, sp.first + sp.count, num, den));
        }
        return 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "plan")) {
        const lmx::Ratio r = {std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5])};
        const lmx::Tile t = lmx::plan_tile(r);
        int need_w = 0, need_h = 0;
        for (int X0 = 0; X0 < 4096; ++X0) {
            const lmx::Span a = lmx::span(X0, r.num_x, r.den_x), b = lmx::span(X0 + t.tw - 1, r.num_x, r.den_x);
            const lmx::Span c = lmx::span(X0, r.num_y, r.den_y), d = lmx::span(X0 + t.th - 1, r.num_y, r.den_y);
            if (b.first + b.count - a.first > need_w) need_w = b.first + b.count - a.first;
            if (d.first + d.count - c.first > need_h) need_h = d.first + d.count - c.first;
        }
        std::printf("OK %d %d %d %d %u %d %d\n", t.tw, t.th, t.sw, t.sh, t.lds_bytes, need_w, need_h);
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "finish")) {
        // every accumulator a ratio can produce, and a margin beyond: the float quotient with its correction against the division
        const lmx::u32 n = (lmx::u32)(std::atoi(argv[2]) * std::atoi(argv[3]));
        if (n < 1 || n > 16384) return 2;
        const float inv = 1.0f / (float)n;
        for (lmx::u32 acc = 0; acc <= 256u * n; ++acc)
            if (lmx::finish_fast(acc, n, inv) != lmx::finish(acc, n)) { std::printf("DIFFERS at %u\n", acc); return 1; }
        for (int den = 1; den <= 16; ++den)
            for (int v = 0; v < 65536; ++v)
                if (lmx::small_div(v, 1.0f / (float)den) != v / den) { std::printf("small_div DIFFERS at %d / %d\n", v, den); return 1; }
        std::printf("OK %u\n", 256u * n + 1u);
        return 0;
    }
    std::fprintf(stderr, "usage: reduce_host image IN OUT | axis NUM DEN N | plan NUM_X DEN_X NUM_Y DEN_Y\n");
    return 2;
}
