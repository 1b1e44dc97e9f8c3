// ingest_raw_host.cpp -- csrc/lm_ingest_raw.h, the raw part of csrc/lm_rectify.h and csrc/lm_ingest_check.cpp on the host: the code
// k_ingest_raw runs per lane (lane_window, load_span, the unpackers, the three reflected rows, the N-bit site rule, the pipeline), the
// taps k_rectify_raw blends, and the descriptor check's raw formats, with the memory reads replaced by loaders that CHECK every load and
// the AMD builtins emulated.  Sources end exactly where their heap allocation ends (ASan guards the byte behind).  Checked:
//   lane code, for every lane of every case
//     * every load is 16-byte aligned;
//     * every load is the `safe` block or holds at least one source byte that a kept pixel needs (a byte of its own sample or of one of
//       its eight reflected neighbours) -- so it lies in the page of a byte that exists;
//     * the bytes a load holds beyond the allocation (poison here) and the safe block's content (poison too) never reach a pixel;
//     * the 16 output pixels equal the definition: shift, mirror, crop, and the per-pixel rule of include/linemod_hip.h restated below;
//   rectify taps: every load reads bytes of a sample inside the source, at most 16 samples per output pixel, none for a pixel whose taps
//     all lie outside, and the blend equals four taps of this file's own rule;
//   refusals: each refusal of the descriptor check for the raw formats with its exact words, what it fills for a good descriptor, and
//     lmc::process_bayer8.
// Prints "OK <checks>"; any failure prints the case and exits 1.  g++ -fsanitize=address,undefined; never loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lm_ingest_check.h"
#include "lm_rectify.h"

using lmi::addr_t;
using lmi::u32;

static unsigned long long g_checks = 0, g_loads = 0, g_safe_loads = 0, g_lane_pixels = 0;
static bool g_failed = false;
static char g_case[400];
static void fail(const char* what) {
    if (!g_failed) printf("FAILED %s: %s\n", g_case, what);
    g_failed = true;
}

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

// storage 0 .. 6 as lm_ingest_raw.h numbers them: u16 with 10 / 12 / 14 / 16 bits, 10p, 12p, one byte
static int bits_of(int st) { static const int b[7] = {10, 12, 14, 16, 10, 12, 8}; return b[st]; }
static int row_bits_of(int st) { return st < 4 ? 16 : bits_of(st); }
static bool container(int st) { return st < 4; }

struct Source {
    uint8_t* alloc = nullptr;       // the heap block; the source's last byte is its last byte
    size_t alloc_bytes = 0;
    uint8_t* data = nullptr;
    long long row_stride = 0, row_bytes = 0;
    int w = 0, h = 0, st = 0;
    ~Source() { free(alloc); }
    addr_t addr(long long byte, int y) const { return (addr_t)(uintptr_t)(data + (long long)y * row_stride + byte); }
    // the header's words: the container's low N bits, clamped; bits [N c, N c + N) of a packed row
    int sample(int x, int y, std::vector<addr_t>* need) const {
        const uint8_t* row = data + (long long)y * row_stride;
        const int N = bits_of(st);
        if (st == 6) { if (need) need->push_back(addr(x, y)); return row[x]; }
        if (container(st)) {
            if (need) { need->push_back(addr(2 * x, y)); need->push_back(addr(2 * x + 1, y)); }
            const int s = row[2 * x] | row[2 * x + 1] << 8, top = (1 << N) - 1;
            return s < top ? s : top;
        }
        const int k = (N * x) >> 3;
        if (need) { need->push_back(addr(k, y)); need->push_back(addr(k + 1, y)); }
        return ((row[k] | row[k + 1] << 8) >> ((N * x) & 7)) & ((1 << N) - 1);
    }
};

static void make_source(Source& s, int w, int h, int st, int offset, int pad) {
    s.w = w; s.h = h; s.st = st;
    s.row_bytes = ((long long)w * row_bits_of(st) + 7) / 8;
    s.row_stride = s.row_bytes + pad;
    s.alloc_bytes = (size_t)(offset + (h - 1) * s.row_stride + s.row_bytes);
    s.alloc = static_cast<uint8_t*>(malloc(s.alloc_bytes));
    s.data = s.alloc + offset;
    static const uint8_t edge[] = {0, 1, 2, 3, 127, 128, 253, 254, 255};
    // (containers: random high bytes too -- bits above N are set in most samples, and some samples are small)
    for (size_t i = 0; i < s.alloc_bytes; ++i) s.alloc[i] = rnd() % 4 == 0 ? edge[rnd() % sizeof edge] : (uint8_t)rnd();
    if (container(st))
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                if (rnd() % 2) s.data[(long long)y * s.row_stride + 2 * x + 1] &= (uint8_t)((1 << (bits_of(st) - 8)) - 1);
}

// ---- the pipelines
struct Pipe { lmi::RawPipe p; uint8_t tone[4096]; };
struct HostTone {
    const uint8_t* t;
    u32 operator()(u32 i) const { if (i >= 4096u) abort(); return t[i]; }
};
static Pipe g_pipes[3];
static void make_pipes() {
    Pipe& id = g_pipes[0];
    id.p.black = 0;
    for (int c = 0; c < 3; ++c) id.p.gain[c] = 1024;
    for (int k = 0; k < 9; ++k) id.p.ccm[k] = k % 4 == 0 ? 1024 : 0;
    for (int i = 0; i < 4096; ++i) id.tone[i] = (uint8_t)(i >> 4);
    Pipe& pin = g_pipes[1];         // the header's pin
    pin.p.black = 64; pin.p.gain[0] = 2048; pin.p.gain[1] = 1024; pin.p.gain[2] = 1536;
    for (int k = 0; k < 9; ++k) pin.p.ccm[k] = k % 4 == 0 ? 1536 : -256;
    for (int i = 0; i < 4096; ++i) pin.tone[i] = (uint8_t)((7 * i + 3) & 255);
    Pipe& hard = g_pipes[2];        // the extremes: a gain of 65535, matrix rows of +8192 and of -8192, a random table
    hard.p.black = 3; hard.p.gain[0] = 65535; hard.p.gain[1] = 700; hard.p.gain[2] = 4000;
    const int m[9] = {8192, 8192, 8192, -8192, -8192, -8192, -3000, 5000, -900};
    for (int k = 0; k < 9; ++k) hard.p.ccm[k] = m[k];
    for (int i = 0; i < 4096; ++i) hard.tone[i] = (uint8_t)rnd();
}

// ---- the rule, restated: explicit reflected indices, one pixel at a time, 64-bit.  pattern 0 .. 3 = RGGB, GRBG, GBRG, BGGR, 4 = mono.
static int refl(int i, int n) { return i == -1 ? 1 : i == n ? n - 2 : i; }
static u32 rule(const Source& s, int pattern, const Pipe& q, int x, int y, std::vector<addr_t>* need) {
    auto S = [&](int xx, int yy) {
        const int rx = refl(xx, s.w), ry = refl(yy, s.h);
        if (rx < 0 || rx >= s.w || ry < 0 || ry >= s.h) abort();
        const long long v = (long long)s.sample(rx, ry, need) - q.p.black;
        return v > 0 ? v : 0;
    };
    long long R, G, B;
    if (pattern == 4) R = G = B = S(x, y);
    else {
        const long long c = S(x, y);
        const long long h = (S(x - 1, y) + S(x + 1, y) + 1) >> 1, v = (S(x, y - 1) + S(x, y + 1) + 1) >> 1;
        const long long p = (S(x - 1, y) + S(x + 1, y) + S(x, y - 1) + S(x, y + 1) + 2) >> 2;
        const long long d = (S(x - 1, y - 1) + S(x + 1, y - 1) + S(x - 1, y + 1) + S(x + 1, y + 1) + 2) >> 2;
        const int red_x = pattern & 1, red_y = pattern >> 1, dx = (x ^ red_x) & 1, dy = (y ^ red_y) & 1;
        if (dx == 0 && dy == 0) { R = c; G = p; B = d; }
        else if (dx == 1 && dy == 1) { B = c; G = p; R = d; }
        else if (dx == 1 && dy == 0) { G = c; R = h; B = v; }
        else { G = c; B = h; R = v; }
    }
    const int N = bits_of(s.st);
    const long long in[3] = {R, G, B};
    long long x2[3], out[3];
    for (int c = 0; c < 3; ++c) {
        const long long t = ((in[c] << (16 - N)) * (long long)q.p.gain[c] + 512) >> 10;
        x2[c] = t < 65535 ? t : 65535;
    }
    for (int i = 0; i < 3; ++i) {
        long long t = ((long long)q.p.ccm[3 * i] * x2[0] + (long long)q.p.ccm[3 * i + 1] * x2[1] + (long long)q.p.ccm[3 * i + 2] * x2[2] + 512) >> 10;
        t = t < 0 ? 0 : t > 65535 ? 65535 : t;
        out[i] = q.tone[t >> 4];
    }
    return (u32)out[2] | (u32)out[1] << 8 | (u32)out[0] << 16;
}

// ---- the lane code
struct CheckedLoad {
    const Source* s;
    addr_t safe;
    const std::vector<addr_t>* need;
    lmi::Vec16 operator()(addr_t p) const {
        ++g_loads; ++g_checks;
        if (p % 16) fail("a load that is not 16-byte aligned");
        if (p == safe) { ++g_safe_loads; return lmi::Vec16{0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu}; }
        bool needed = false;
        for (addr_t n : *need) needed = needed || (n >= p && n < p + 16);
        if (!needed) fail("a load outside `safe` that holds no byte a kept pixel needs");
        const addr_t lo = (addr_t)(uintptr_t)s->alloc, hi = lo + s->alloc_bytes;
        uint8_t b[16];
        for (int i = 0; i < 16; ++i) b[i] = (p + i >= lo && p + i < hi) ? *reinterpret_cast<const uint8_t*>((uintptr_t)(p + i)) : 0xA5;
        lmi::Vec16 v;
        memcpy(&v, b, 16);
        return v;
    }
};

// one frame: every lane of a w x h window at (crop_x, crop_y) of the source (the lane code takes any w: a lane keeps what lies inside)
static void run_case(const Source& s, int pattern, const Pipe& q, int w, int h, int crop_x, int crop_y, bool flip, int shift_x, int shift_y) {
    alignas(16) static uint8_t safe_block[16];
    const addr_t safe = (addr_t)(uintptr_t)safe_block;
    lmi::RawSrc src;
    src.data = (addr_t)(uintptr_t)s.data; src.row_stride = s.row_stride; src.width = s.w; src.height = s.h;
    src.crop_x = crop_x; src.crop_y = crop_y; src.kind = lm_raw_kind(s.st, pattern);
    for (int y = 0; y < h; ++y)
        for (int x0 = 0; x0 < w; x0 += 16) {
            snprintf(g_case, sizeof g_case, "storage %d pattern %d source %d x %d at %p stride %lld window %d x %d at (%d, %d) flip %d shift (%d, %d) black %d lane (%d, %d)",
                     s.st, pattern, s.w, s.h, (void*)s.data, s.row_stride, w, h, crop_x, crop_y, (int)flip, shift_x, shift_y, q.p.black, x0, y);
            u32 expect[16];
            std::vector<addr_t> need;
            for (int j = 0; j < 16; ++j) {
                const int xs = x0 + j - shift_x, ys = y - shift_y;
                expect[j] = 0;
                if (xs < 0 || xs >= w || ys < 0 || ys >= h) continue;       // (a window narrower than a lane: the row goes on to the lane's end)
                const int u = flip ? w - 1 - xs : xs;
                expect[j] = rule(s, pattern, q, crop_x + u, crop_y + ys, &need);
            }
            const lmi::Lane L = lmi::lane_window(w, h, x0, y, flip, shift_x, shift_y);
            u32 P[16];
            lmi::raw_lane_pixels(src, q.p, L, safe, CheckedLoad{&s, safe, &need}, HostTone{q.tone}, P);
            for (int j = 0; j < 16; ++j) {          // k_ingest's arrange
                const int k = flip ? 15 - j : j;
                const u32 got = (k >= L.klo && k < L.khi) ? P[k] : 0u;
                ++g_checks; ++g_lane_pixels;
                if (got != expect[j]) fail("an output pixel differs from the rule");
            }
            if (g_failed) return;
        }
}

static std::vector<int> crops(int max, bool six) {
    std::vector<int> v;
    const int want[6] = {0, 1, 2, 3, max - 1, max};
    for (int i = 0; i < 6; ++i) {
        if (!six && (i == 2 || i == 3 || i == 4)) continue;       // y: {0, 1, max}
        bool dup = want[i] < 0 || want[i] > max;
        for (int u : v) dup = dup || u == want[i];
        if (!dup) v.push_back(want[i]);
    }
    return v;
}

static bool lane_cases() {
    // source size and the window taken from it, as tests/cpp/ingest_bayer_host.cpp: the tiny sources have both reflections land on one
    // column or row, a window of the source's own size has all four edges reflect at once.  crop_x 0 .. 3 reaches all four bit phases of
    // 10p (10 (c0 - 1) & 7 = 6, 0, 2, 4) and both of 12p.  The last two: odd sizes, for mono alone.
    const int sizes[][4] = {{2, 2, 2, 2}, {2, 2, 1, 1}, {2, 4, 2, 4}, {2, 4, 1, 2}, {4, 2, 4, 2}, {4, 2, 2, 1}, {18, 6, 16, 4}, {18, 6, 18, 6},
                            {34, 8, 16, 6}, {34, 8, 32, 5}, {34, 8, 34, 8}, {3, 3, 3, 3}, {21, 5, 17, 3}};
    const int shifts[3][2] = {{0, 0}, {3, -2}, {-5, 1}};
    unsigned long long phases10 = 0, phases12 = 0, n = 0;
    for (int st = 0; st < 7; ++st)
        for (const auto& z : sizes)
            for (int offset = 0; offset < 4; ++offset)
                for (int pad : {0, 3}) {
                    if (container(st) && (offset % 2)) continue;        // containers: base offsets 0 and 2, row padding 0 and 2
                    const int rpad = container(st) && pad ? 2 : pad;
                    Source s;
                    make_source(s, z[0], z[1], st, offset, rpad);
                    for (int pattern = 0; pattern < 5; ++pattern) {
                        if (pattern < 4 && (z[0] % 2 || z[1] % 2)) continue;
                        if (pattern == 4 && st == 6) continue;          // (one byte per sample is an 8-bit Bayer format under a pipeline: no mono)
                        for (int cx : crops(z[0] - z[2], true))
                            for (int cy : crops(z[1] - z[3], false))
                                for (int flip = 0; flip < 2; ++flip)
                                    for (const auto& sh : shifts) {
                                        const long long c0 = (long long)cx + (flip ? z[2] - 16 + sh[0] : -sh[0]);
                                        if (st == 4) phases10 |= 1ull << ((10 * (c0 - 1)) & 7);
                                        if (st == 5) phases12 |= 1ull << ((12 * (c0 - 1)) & 7);
                                        run_case(s, pattern, g_pipes[n++ % 3], z[2], z[3], cx, cy, flip != 0, sh[0], sh[1]);
                                        if (g_failed) return false;
                                    }
                    }
                }
    if (phases10 != 0x55 || phases12 != 0x11) { printf("FAILED: bit phases reached: 10p %llx, 12p %llx\n", phases10, phases12); return false; }
    if (g_safe_loads == 0 || g_safe_loads == g_loads) { printf("FAILED: %llu of %llu loads went to the safe block\n", g_safe_loads, g_loads); return false; }
    return true;
}

// ---- the rectify taps
struct CheckedLd {
    const Source* s;
    unsigned* count;
    bool inside(addr_t p, int n) const {
        const addr_t lo = (addr_t)(uintptr_t)s->data;
        if (p < lo) return false;
        const long long off = (long long)(p - lo), y = off / s->row_stride, x = off % s->row_stride;
        return y < s->h && x + n <= s->row_bytes;
    }
    u32 b8(addr_t p) const {
        ++*count; ++g_checks;
        if (container(s->st)) fail("a byte load in a container tap");
        if (!inside(p, 1)) { fail("a tap load outside the source"); return 0xA5u; }
        return *reinterpret_cast<const uint8_t*>((uintptr_t)p);
    }
    u32 b16(addr_t p) const {
        *count += 2; ++g_checks;
        if (!container(s->st) || p % 2) fail("a 16-bit load in a packed tap, or a misaligned one");
        if (!inside(p, 2)) { fail("a tap load outside the source"); return 0xA5A5u; }
        uint16_t v;
        memcpy(&v, reinterpret_cast<const void*>((uintptr_t)p), 2);
        return v;
    }
    u32 b32(addr_t) const { fail("a 32-bit load in a raw tap"); return 0; }
};

static u32 own_blend(const Source& s, int pattern, const Pipe& q, int qx, int qy) {
    const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;
    u32 t[4];
    for (int b = 0; b < 2; ++b)
        for (int a = 0; a < 2; ++a) {
            const int x = ix + a, y = iy + b;
            t[2 * b + a] = (x < 0 || x >= s.w || y < 0 || y >= s.h) ? 0u : rule(s, pattern, q, x, y, nullptr);
        }
    const long long w[4] = {(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay};
    u32 out = 0;
    for (int sh = 0; sh < 24; sh += 8) {
        long long v = 512;
        for (int k = 0; k < 4; ++k) v += w[k] * ((t[k] >> sh) & 0xFF);
        out |= (u32)(v >> 10) << sh;
    }
    return out;
}

static bool tap_cases() {
    const int sizes[][2] = {{2, 2}, {2, 4}, {4, 2}, {18, 6}, {34, 8}, {3, 5}};
    unsigned long long n = 0;
    for (int st = 0; st < 7; ++st)
        for (const auto& z : sizes)
            for (int offset : {0, 3})
                for (int pad : {0, 3}) {
                    Source s;
                    make_source(s, z[0], z[1], st, container(st) ? offset / 2 * 2 : offset, container(st) ? pad / 2 * 2 : pad);
                    lmq::Src q;
                    q.data = (addr_t)(uintptr_t)s.data; q.row_stride = s.row_stride; q.plane_stride = 0; q.width = s.w; q.height = s.h;
                    q.swap_rb = 0; q.matrix = 0; q.dwords = false; q.scale = 1.0f;
                    for (int pattern = 0; pattern < 5; ++pattern) {
                        if (pattern < 4 && (z[0] % 2 || z[1] % 2)) continue;
                        if (pattern == 4 && st == 6) continue;
                        q.kind = lm_raw_kind(st, pattern);
                        const Pipe& pipe = g_pipes[n++ % 3];
                        for (int iy = -2; iy <= s.h + 1; ++iy)
                            for (int ix = -2; ix <= s.w + 1; ++ix)
                                for (int f = 0; f < 4; ++f) {
                                    static const int frac[4][2] = {{0, 0}, {31, 1}, {13, 13}, {1, 31}};
                                    const int qx = 32 * ix + frac[f][0], qy = 32 * iy + frac[f][1];
                                    if (qx > 32 * s.w + 32 || qy > 32 * s.h + 32) continue;
                                    snprintf(g_case, sizeof g_case, "taps: storage %d pattern %d source %d x %d stride %lld map entry (%d, %d)", st, pattern, s.w, s.h, s.row_stride, qx, qy);
                                    unsigned bytes = 0;
                                    const u32 got = lmq::colour_pixel_raw(q, pipe.p, qx, qy, CheckedLd{&s, &bytes}, HostTone{pipe.tone});
                                    ++g_checks;
                                    if (got != own_blend(s, pattern, pipe, qx, qy)) fail("a rectified pixel differs from the blend of four taps of the rule");
                                    if (bytes > (pattern == 4 ? 4u : 16u) * (st == 6 ? 1u : 2u)) fail("more loads than the samples of one output pixel");
                                    const bool inside = ix + 1 >= 0 && ix < s.w && iy + 1 >= 0 && iy < s.h;
                                    if (!inside && bytes) fail("a load for an output pixel whose four taps lie outside");
                                    if (g_failed) return false;
                                }
                    }
                }
    return true;
}

// ---- the descriptor check
static bool expect_words(const lmc::Geometry& g, const lm_image_desc& im, const std::string& words) {
    LmIngestImage img;
    memset(&img, 0xAB, sizeof img);
    int matrix = -1;
    const std::string got = lmc::check_image(g, im, 0, lm_ingest_opts{0, 0, 0}, &img, g.role == lmc::COLOUR ? &matrix : nullptr);
    ++g_checks;
    if (got != words) { printf("FAILED refusal (format %d): got \"%s\", want \"%s\"\n", im.format, got.c_str(), words.c_str()); return false; }
    return true;
}

static bool refusal_cases() {
    lm_config c = lm_config();
    c.width = 160; c.height = 80;
    lm_rectification_desc rect = lm_rectification_desc();
    rect.source.width = 208; rect.source.height = 120; rect.ideal.width = 176; rect.ideal.height = 96;
    lm_registration_desc reg = lm_registration_desc();
    reg.depth.width = 96; reg.depth.height = 64; reg.colour.width = 208; reg.colour.height = 120;
    static const char* const tiles[5] = {"LM_PIX_BAYER_RGGB", "LM_PIX_BAYER_GRBG", "LM_PIX_BAYER_GBRG", "LM_PIX_BAYER_BGGR", "LM_PIX_MONO"};
    static const char* const suffix[6] = {"10", "12", "14", "16", "10P", "12P"};
    const std::string who = "colour image of frame 0: ";
    bool ok = true;
    for (int st = 0; st < 6; ++st)
        for (int pat = 0; pat < 5; ++pat) {
            const std::string n = std::string(tiles[pat]) + suffix[st];
            const long long row = (204ll * row_bits_of(st) + 7) / 8;       // 408, 255 (10p), 306 (12p)
            lm_image_desc im = lm_image_desc();
            im.data = reinterpret_cast<const void*>(static_cast<uintptr_t>(container(st) ? 0x7F0012340002ull : 0x7F0012340003ull));
            im.width = 204; im.height = 98; im.row_stride = row + (container(st) ? 2 : 3); im.format = LM_PIX_RAW | st << 4 | pat; im.crop_x = 3; im.crop_y = 1; im.scale = 1.0f;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), im, "");
            ok = ok && expect_words(lmc::plain(c, lmc::DEPTH), im, "depth image of frame 0: " + n + " is a colour format");
            ok = ok && expect_words(lmc::raw_depth(c, reg, false), im, "raw depth image of frame 0: " + n + " is a colour format");
            // half a tile at the source's edge; mono may have any size
            const std::string even = pat == 4 ? "" : who + "width and height of a " + n + " source must be even";
            lm_image_desc e = im;
            e.width = 203;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, even);
            e = im; e.height = 99;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, even);
            // a row holds the source's width: 2 * width container bytes, ceil(width * N / 8) packed bytes
            e = im; e.row_stride = row;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, "");
            e = im; e.row_stride = row - (container(st) ? 2 : 1);
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, who + "row_stride smaller than a window row");
            e = im; e.row_stride = 0;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, who + "row_stride smaller than a window row");
            // containers are u16 sources; packed rows lie anywhere
            const std::string u16 = container(st) ? who + "data and row_stride of a u16 source must be multiples of 2" : "";
            e = im; e.data = static_cast<const uint8_t*>(im.data) + 1;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, u16);
            e = im; e.row_stride = row + 1;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, u16);
            // the flags of the YUV formats and every other bit name nothing
            for (int bit : {(int)LM_PIX_YUV_BT709, (int)LM_PIX_YUV_FULL, 0x400, 0x800, 0x2000, 0x10000, 0x40000000}) {
                e = im; e.format |= bit;
                ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, who + "unknown pixel format " + std::to_string(e.format));
            }
            e = im; e.data = nullptr;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, who + "null data pointer");
            e = im; e.crop_x = 45;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, who + "0 <= roi.x && roi.x + roi.width <= m.cols && 0 <= roi.y && roi.y + roi.height <= m.rows failed: "
                                                                   "window 160 x 80 at (45, 1) in a 204 x 98 source");
            // the rectified route: the source camera's size, a source row
            const long long srow = (208ll * row_bits_of(st) + 7) / 8;
            e = im; e.width = 208; e.height = 120; e.row_stride = srow;
            ok = ok && expect_words(lmc::rectified(c, rect, lmc::COLOUR, false), e, "");
            ok = ok && expect_words(lmc::rectified(c, rect, lmc::COLOUR, true), e, "");
            e.row_stride = srow - (container(st) ? 2 : 1);
            ok = ok && expect_words(lmc::rectified(c, rect, lmc::COLOUR, false), e, "rectification: " + who + "row_stride smaller than a source row");
            ok = ok && expect_words(lmc::rectified(c, rect, lmc::DEPTH, false), e, "depth image of frame 0: " + n + " is a colour format");
            // what a good descriptor fills
            LmIngestImage img;
            memset(&img, 0xAB, sizeof img);
            int matrix = -1;
            ++g_checks;
            if (!lmc::check_image(lmc::plain(c, lmc::COLOUR), im, 0, lm_ingest_opts{0, 0, 0}, &img, &matrix).empty() || img.kind != LM_INGEST_RAW + 8 * st + pat ||
                img.kind < 14 || lm_raw_storage(img.kind) != st || lm_raw_pattern(img.kind) != pat || lm_raw_bits(st) != bits_of(st) || lm_raw_row_bits(st) != row_bits_of(st) ||
                img.src_w != 204 || img.src_h != 98 || img.crop_x != 3 || img.crop_y != 1 || img.row_stride != im.row_stride || img.plane_stride != 0 || img.aligned != 0 ||
                img.swap_rb != 0 || matrix != 0 || lm_ingest_family(img.kind) != LM_INGEST_FAMILY_RAW || img.data != im.data) {
                printf("FAILED: the fields of a good %s descriptor\n", n.c_str());
                ok = false;
            }
            // ... and an 8-bit Bayer kind is not touched by a raw descriptor's path
            const LmIngestImage before = img;
            lmc::process_bayer8(&img);
            ++g_checks;
            if (memcmp(&before, &img, sizeof img)) { printf("FAILED: process_bayer8 changed a %s image\n", n.c_str()); ok = false; }
        }
    // patterns 5 .. 15 and storages 0x60 .. 0xF0 name nothing; the values the earlier formats pin as unknown stay so
    lm_image_desc im = lm_image_desc();
    im.data = &im; im.width = 204; im.height = 98; im.row_stride = 408;
    for (int pat = 5; pat < 16; ++pat)
        for (int st : {0, 0x10, 0x40, 0x50}) {
            im.format = LM_PIX_RAW | st | pat;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), im, who + "unknown pixel format " + std::to_string(im.format));
        }
    for (int st = 0x60; st < 0x100; st += 0x10)
        for (int pat : {0, 3, 4}) {
            im.format = LM_PIX_RAW | st | pat;
            ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), im, who + "unknown pixel format " + std::to_string(im.format));
        }
    for (int bad : {13, 14, 15, 20, 99, -1, 0x300, LM_PIX_NV12 | 0x80, LM_PIX_NV12 | 0x400, LM_PIX_BAYER_RGGB8 | LM_PIX_YUV_FULL, LM_PIX_GRAY8 | LM_PIX_YUV_BT709, -0x1000, (int)0x80001000u}) {
        im.format = bad;
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), im, who + "unknown pixel format " + std::to_string(bad));
    }
    // the named values
    ++g_checks;
    if (LM_PIX_RAW != 0x1000 || LM_PIX_BAYER_RGGB10 != 0x1000 || LM_PIX_BAYER_BGGR10 != 0x1003 || LM_PIX_MONO10 != 0x1004 || LM_PIX_BAYER_GRBG12 != 0x1011 ||
        LM_PIX_MONO12 != 0x1014 || LM_PIX_BAYER_GBRG14 != 0x1022 || LM_PIX_MONO14 != 0x1024 || LM_PIX_BAYER_RGGB16 != 0x1030 || LM_PIX_MONO16 != 0x1034 ||
        LM_PIX_BAYER_RGGB10P != 0x1040 || LM_PIX_MONO10P != 0x1044 || LM_PIX_BAYER_BGGR12P != 0x1053 || LM_PIX_MONO12P != 0x1054) { printf("FAILED: LM_PIX_* values\n"); ok = false; }
    // an 8-bit Bayer image under a pipeline: the raw kind of its pattern, N = 8, the general path; everything else as it was
    for (int k = 0; k < 4; ++k) {
        lm_image_desc b = lm_image_desc();
        b.data = reinterpret_cast<const void*>(static_cast<uintptr_t>(0x7F0012340000ull));
        b.width = 208; b.height = 98; b.row_stride = 208; b.format = LM_PIX_BAYER_RGGB8 + k; b.scale = 1.0f;
        LmIngestImage img, was;
        int matrix = -1;
        ++g_checks;
        if (!lmc::check_image(lmc::plain(c, lmc::COLOUR), b, 0, lm_ingest_opts{0, 0, 0}, &img, &matrix).empty() || img.kind != LM_INGEST_BAYER_RGGB + k || img.aligned != 1) {
            printf("FAILED: an 8-bit Bayer descriptor\n"); ok = false;
        }
        was = img;
        lmc::process_bayer8(&img);
        if (img.kind != lm_raw_kind(LM_RAW_U8, k) || lm_ingest_family(img.kind) != LM_INGEST_FAMILY_RAW || lm_raw_bits(lm_raw_storage(img.kind)) != 8 || lm_raw_pattern(img.kind) != k ||
            img.aligned != 0 || img.data != was.data || img.row_stride != was.row_stride || img.src_w != 208 || img.src_h != 98) { printf("FAILED: process_bayer8\n"); ok = false; }
    }
    {
        lm_image_desc g8 = lm_image_desc();
        g8.data = &g8; g8.width = 204; g8.height = 98; g8.row_stride = 204; g8.format = LM_PIX_GRAY8;
        LmIngestImage img;
        int matrix = -1;
        ++g_checks;
        if (!lmc::check_image(lmc::plain(c, lmc::COLOUR), g8, 0, lm_ingest_opts{0, 0, 0}, &img, &matrix).empty()) ok = false;
        lmc::process_bayer8(&img);
        if (img.kind != LM_INGEST_GRAY8) { printf("FAILED: process_bayer8 touched GRAY8\n"); ok = false; }
    }
    ++g_checks;
    if (lm_ingest_family(LM_INGEST_PX3) != LM_INGEST_FAMILY_RGB || lm_ingest_family(LM_INGEST_UYVY) != LM_INGEST_FAMILY_YUV ||
        lm_ingest_family(LM_INGEST_BAYER_BGGR) != LM_INGEST_FAMILY_BAYER || lm_ingest_family(LM_INGEST_RAW) != LM_INGEST_FAMILY_RAW) { printf("FAILED: lm_ingest_family\n"); ok = false; }
    return ok;
}

// the header's pins through this file's rule and through the lane code
static bool pins() {
    static const int src[4] = {100, 2000, 3000, 4095};
    static const u32 rggb[4] = {0x036FFC, 0x03EDFC, 0x03F1FC, 0x036FFC}, mono[4] = {0x569D7D, 0xFC196B, 0xFC6FFC, 0xFC55FC}, ident[4] = {0x069CFF, 0x067DFF, 0x06BBFF, 0x069CFF};
    for (int st : {1, 5}) {         // RGGB12 / MONO12 in containers, and packed
        Source s;
        make_source(s, 2, 2, st, 0, 0);
        if (st == 1) for (int i = 0; i < 4; ++i) { uint16_t v = (uint16_t)src[i]; memcpy(s.data + 2 * i, &v, 2); }
        else { const uint8_t b[6] = {0x64, 0x00, 0x7D, 0xB8, 0xFB, 0xFF}; memcpy(s.data, b, 6); }       // 100, 2000 | 3000, 4095
        for (int i = 0; i < 4; ++i) {
            g_checks += 3;
            if (s.sample(i & 1, i >> 1, nullptr) != src[i]) { printf("FAILED: the pin's samples, storage %d\n", st); return false; }
            if (rule(s, 0, g_pipes[1], i & 1, i >> 1, nullptr) != rggb[i] || rule(s, 4, g_pipes[1], i & 1, i >> 1, nullptr) != mono[i] ||
                rule(s, 0, g_pipes[0], i & 1, i >> 1, nullptr) != ident[i]) { printf("FAILED: the header's pins, storage %d pixel %d\n", st, i); return false; }
        }
        for (int pattern : {0, 4})
            for (int q = 0; q < 2; ++q) run_case(s, pattern, g_pipes[q], 2, 2, 0, 0, false, 0, 0);
    }
    // the packing pins
    Source p10, p12;
    make_source(p10, 4, 1, 4, 0, 0);
    make_source(p12, 2, 1, 5, 0, 0);
    const uint8_t b10[5] = {1, 8, 48, 192, 255}, b12[3] = {0xBC, 0x3A, 0x12};
    memcpy(p10.data, b10, 5); memcpy(p12.data, b12, 3);
    g_checks += 2;
    if (p10.sample(0, 0, nullptr) != 1 || p10.sample(1, 0, nullptr) != 2 || p10.sample(2, 0, nullptr) != 3 || p10.sample(3, 0, nullptr) != 1023 ||
        p12.sample(0, 0, nullptr) != 0xABC || p12.sample(1, 0, nullptr) != 0x123) { printf("FAILED: the packing pins\n"); return false; }
    run_case(p10, 4, g_pipes[0], 4, 1, 0, 0, false, 0, 0);
    run_case(p12, 4, g_pipes[1], 2, 1, 0, 0, true, 0, 0);
    return !g_failed;
}

int main() {
    make_pipes();
    if (!pins() || !lane_cases() || !tap_cases() || !refusal_cases() || g_failed) return 1;
    printf("OK %llu checks, %llu lane pixels, %llu loads, %llu of them to the safe block\n", g_checks, g_lane_pixels, g_loads, g_safe_loads);
    return 0;
}
