// ingest_bayer_host.cpp -- csrc/lm_ingest_bayer.h, the Bayer part of csrc/lm_rectify.h and csrc/lm_ingest_check.cpp on the host: the code
// k_ingest_bayer runs per lane (lane_window, load_span, the three reflected rows, the site rule), the 4 x 4 neighbourhood k_rectify_bayer
// blends from, and the descriptor check's Bayer rows, with the memory reads replaced by loaders that CHECK every load and the AMD
// builtins emulated.  Sources end exactly where their heap allocation ends (ASan guards the byte behind).  Checked:
//   lane code, for every lane of every case
//     * every load is 16-byte aligned;
//     * every load is the `safe` block or holds at least one source byte that a kept pixel needs (itself or one of its eight reflected
//       neighbours) -- so it lies in the page of a byte that exists;
//     * the bytes a load holds beyond the allocation (poison here) and the safe block's content (poison too) never reach a pixel;
//     * the 16 output pixels equal the definition: shift, mirror, crop, and the per-pixel rule restated below with explicit reflection;
//   rectify taps: every byte load lies inside the source, at most 16 per output pixel, and the blend equals four taps of this file's own;
//   refusals: each Bayer refusal of the descriptor check with its exact words, and what it fills for a good descriptor.
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

static unsigned long long g_checks = 0, g_loads = 0, g_safe_loads = 0;
static bool g_failed = false;
static char g_case[320];
static void fail(const char* what) {
    if (!g_failed) printf("FAILED %s: %s\n", g_case, what);
    g_failed = true;
}

struct Source {
    uint8_t* alloc = nullptr;       // the heap block; the source's last byte is its last byte
    size_t alloc_bytes = 0;
    uint8_t* data = nullptr;
    long long row_stride = 0;
    int w = 0, h = 0;
    ~Source() { free(alloc); }
    int at(int x, int y) const { return data[(long long)y * row_stride + x]; }
    addr_t addr(int x, int y) const { return (addr_t)(uintptr_t)(data + (long long)y * row_stride + x); }
};

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static void make_source(Source& s, int w, int h, int offset, int pad, bool aligned) {
    s.w = w; s.h = h;
    s.row_stride = aligned ? (w + 15) / 16 * 16 : w + pad;
    s.alloc_bytes = (size_t)(offset + (h - 1) * s.row_stride + w);
    if (aligned) {
        if (posix_memalign(reinterpret_cast<void**>(&s.alloc), 16, s.alloc_bytes)) abort();
    } else {
        s.alloc = static_cast<uint8_t*>(malloc(s.alloc_bytes));
    }
    s.data = s.alloc + offset;
    static const uint8_t edge[] = {0, 1, 2, 3, 127, 128, 253, 254, 255};
    for (size_t i = 0; i < s.alloc_bytes; ++i) s.alloc[i] = rnd() % 4 == 0 ? edge[rnd() % sizeof edge] : (uint8_t)rnd();
}

// ---- the rule, restated: explicit reflected indices, one pixel at a time.  pattern 0 .. 3 = RGGB, GRBG, GBRG, BGGR.
static int refl(int i, int n) { return i == -1 ? 1 : i == n ? n - 2 : i; }
static u32 rule(const Source& s, int pattern, int x, int y, std::vector<addr_t>* need) {
    auto S = [&](int xx, int yy) {
        const int rx = refl(xx, s.w), ry = refl(yy, s.h);
        if (rx < 0 || rx >= s.w || ry < 0 || ry >= s.h) abort();
        if (need) need->push_back(s.addr(rx, ry));
        return s.at(rx, ry);
    };
    const int c = S(x, y);
    const int h = (S(x - 1, y) + S(x + 1, y) + 1) >> 1, v = (S(x, y - 1) + S(x, y + 1) + 1) >> 1;
    const int p = (S(x - 1, y) + S(x + 1, y) + S(x, y - 1) + S(x, y + 1) + 2) >> 2;
    const int d = (S(x - 1, y - 1) + S(x + 1, y - 1) + S(x - 1, y + 1) + S(x + 1, y + 1) + 2) >> 2;
    const int red_x = pattern & 1, red_y = pattern >> 1, dx = (x ^ red_x) & 1, dy = (y ^ red_y) & 1;
    int R, G, B;
    if (dx == 0 && dy == 0) { R = c; G = p; B = d; }
    else if (dx == 1 && dy == 1) { B = c; G = p; R = d; }
    else if (dx == 1 && dy == 0) { G = c; R = h; B = v; }
    else { G = c; B = h; R = v; }
    return (u32)B | (u32)G << 8 | (u32)R << 16;
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
static void run_case(const Source& s, int pattern, int w, int h, int crop_x, int crop_y, bool flip, int shift_x, int shift_y, bool aligned) {
    alignas(16) static uint8_t safe_block[16];
    const addr_t safe = (addr_t)(uintptr_t)safe_block;
    lmi::BayerSrc src;
    src.data = (addr_t)(uintptr_t)s.data; src.row_stride = s.row_stride; src.width = s.w; src.height = s.h;
    src.crop_x = crop_x; src.crop_y = crop_y; src.kind = LM_INGEST_BAYER_RGGB + pattern;
    const long long col0 = (long long)crop_x + (flip ? w - 16 + shift_x : -shift_x);
    src.aligned = lmi::spans_aligned(src.data, s.row_stride, 0, col0, 1);
    if (src.aligned != aligned) fail("the fast-path condition is not what the case was built for");
    for (int y = 0; y < h; ++y)
        for (int x0 = 0; x0 < w; x0 += 16) {
            snprintf(g_case, sizeof g_case, "pattern %d source %d x %d at %p stride %lld window %d x %d at (%d, %d) flip %d shift (%d, %d) aligned %d lane (%d, %d)",
                     pattern, s.w, s.h, (void*)s.data, s.row_stride, w, h, crop_x, crop_y, (int)flip, shift_x, shift_y, (int)aligned, x0, y);
            u32 expect[16];
            std::vector<addr_t> need;
            for (int j = 0; j < 16; ++j) {
                const int xs = x0 + j - shift_x, ys = y - shift_y;
                expect[j] = 0;
                if (xs < 0 || xs >= w || ys < 0 || ys >= h) continue;       // (a window narrower than a lane: the row goes on to the lane's end)
                const int u = flip ? w - 1 - xs : xs;
                expect[j] = rule(s, pattern, crop_x + u, crop_y + ys, &need);
            }
            const lmi::Lane L = lmi::lane_window(w, h, x0, y, flip, shift_x, shift_y);
            u32 P[16];
            lmi::bayer_lane_pixels(src, L, safe, CheckedLoad{&s, safe, &need}, P);
            for (int j = 0; j < 16; ++j) {          // k_ingest's arrange
                const int k = flip ? 15 - j : j;
                const u32 got = (k >= L.klo && k < L.khi) ? P[k] : 0u;
                ++g_checks;
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
    // source size and the window taken from it.  The tiny sources: both reflections land on the same column or row.  A window of the
    // source's own size (crop 0 = max) has all four edges reflect at once; a smaller one leaves room for the crops.
    const int sizes[][4] = {{2, 2, 2, 2}, {2, 2, 1, 1}, {2, 4, 2, 4}, {2, 4, 1, 2}, {4, 2, 4, 2}, {4, 2, 2, 1}, {18, 6, 16, 4}, {18, 6, 18, 6},
                            {34, 8, 16, 6}, {34, 8, 32, 5}, {34, 8, 34, 8}};
    const int shifts[3][2] = {{0, 0}, {3, -2}, {-5, 1}};
    for (const auto& z : sizes)
        for (int offset = 0; offset < 4; ++offset)
            for (int pad : {0, 3}) {
                Source s;
                make_source(s, z[0], z[1], offset, pad, false);
                for (int pattern = 0; pattern < 4; ++pattern)
                    for (int cx : crops(z[0] - z[2], true))
                        for (int cy : crops(z[1] - z[3], false))
                            for (int flip = 0; flip < 2; ++flip)
                                for (const auto& sh : shifts) {
                                    const long long col0 = (long long)cx + (flip ? z[2] - 16 + sh[0] : -sh[0]);
                                    const bool fast = lmi::spans_aligned((addr_t)(uintptr_t)s.data, s.row_stride, 0, col0, 1);
                                    run_case(s, pattern, z[2], z[3], cx, cy, flip != 0, sh[0], sh[1], fast);
                                    if (g_failed) return false;
                                }
            }
    // the fast path: a 16-byte aligned source with an aligned stride, windows at multiples of 16 columns, every row position
    Source a;
    make_source(a, 64, 8, 0, 0, true);
    unsigned long long fast_cases = 0;
    for (int pattern = 0; pattern < 4; ++pattern)
        for (int cx : {0, 16, 32, 8})
            for (int cy : {0, 1, 2})
                for (int flip = 0; flip < 2; ++flip)
                    for (int sx : {0, 16, -16}) {
                        run_case(a, pattern, 32, 6, cx, cy, flip != 0, sx, cy == 1 ? -1 : 0, cx % 16 == 0);
                        fast_cases += cx % 16 == 0;
                        if (g_failed) return false;
                    }
    // ... and with the window as wide as the source: the fast path at both reflecting columns
    for (int pattern = 0; pattern < 4; ++pattern)
        for (int flip = 0; flip < 2; ++flip) {
            run_case(a, pattern, 64, 8, 0, 0, flip != 0, 0, 0, true);
            if (g_failed) return false;
        }
    if (g_safe_loads == 0 || g_safe_loads == g_loads || fast_cases == 0) { printf("FAILED: %llu of %llu loads went to the safe block\n", g_safe_loads, g_loads); return false; }
    return true;
}

// ---- the rectify taps
struct CheckedLd {
    const Source* s;
    unsigned* count;
    u32 b8(addr_t p) const {
        ++*count; ++g_checks;
        const addr_t lo = (addr_t)(uintptr_t)s->data;
        const long long off = (long long)(p - lo), y = off / s->row_stride, x = off % s->row_stride;
        if (p < lo || y >= s->h || x >= s->w) { fail("a tap load outside the source"); return 0xA5u; }
        return *reinterpret_cast<const uint8_t*>((uintptr_t)p);
    }
    u32 b16(addr_t) const { fail("a 16-bit load in a Bayer tap"); return 0; }
    u32 b32(addr_t) const { fail("a 32-bit load in a Bayer tap"); return 0; }
};

static u32 own_blend(const Source& s, int pattern, int qx, int qy) {
    const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;
    u32 t[4];
    for (int b = 0; b < 2; ++b)
        for (int a = 0; a < 2; ++a) {
            const int x = ix + a, y = iy + b;
            t[2 * b + a] = (x < 0 || x >= s.w || y < 0 || y >= s.h) ? 0u : rule(s, pattern, x, y, nullptr);
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
    const int sizes[][2] = {{2, 2}, {2, 4}, {4, 2}, {18, 6}, {34, 8}};
    for (const auto& z : sizes)
        for (int offset : {0, 3})
            for (int pad : {0, 3}) {
                Source s;
                make_source(s, z[0], z[1], offset, pad, false);
                lmq::Src q;
                q.data = (addr_t)(uintptr_t)s.data; q.row_stride = s.row_stride; q.plane_stride = 0; q.width = s.w; q.height = s.h;
                q.swap_rb = 0; q.matrix = 0; q.dwords = false; q.scale = 1.0f;
                // map entries on all four borders, in the corners and fully outside: every integer position from -2 to n + 1 (the map's clamp
                // is [-64, 32 n + 32]) with fractions 0, 1, 13 and 31
                for (int pattern = 0; pattern < 4; ++pattern) {
                    q.kind = LM_INGEST_BAYER_RGGB + pattern;
                    for (int iy = -2; iy <= s.h + 1; ++iy)
                        for (int ix = -2; ix <= s.w + 1; ++ix)
                            for (int f = 0; f < 4; ++f) {
                                static const int frac[4][2] = {{0, 0}, {31, 1}, {13, 13}, {1, 31}};
                                const int qx = 32 * ix + frac[f][0], qy = 32 * iy + frac[f][1];
                                if (qx > 32 * s.w + 32 || qy > 32 * s.h + 32) continue;
                                snprintf(g_case, sizeof g_case, "taps: pattern %d source %d x %d stride %lld map entry (%d, %d)", pattern, s.w, s.h, s.row_stride, qx, qy);
                                unsigned loads = 0;
                                const u32 got = lmq::colour_pixel_any(q, qx, qy, CheckedLd{&s, &loads});
                                ++g_checks;
                                if (got != own_blend(s, pattern, qx, qy)) fail("a rectified pixel differs from the blend of four taps of the rule");
                                if (loads > 16) fail("more than 16 byte loads for one output pixel");
                                const bool inside = ix + 1 >= 0 && ix < s.w && iy + 1 >= 0 && iy < s.h;
                                if (!inside && loads) fail("a load for an output pixel whose four taps lie outside");
                                if (g_failed) return false;
                            }
                }
            }
    return true;
}

// ---- the descriptor check
static bool expect_words(const lmc::Geometry& g, const lm_image_desc& im, const char* words) {
    LmIngestImage img;
    memset(&img, 0xAB, sizeof img);
    int matrix = -1;
    const std::string got = lmc::check_image(g, im, 0, lm_ingest_opts{0, 0, 0}, &img, g.role == lmc::COLOUR ? &matrix : nullptr);
    ++g_checks;
    if (got != words) { printf("FAILED refusal: got \"%s\", want \"%s\"\n", got.c_str(), words); return false; }
    return true;
}

static bool refusal_cases() {
    lm_config c = lm_config();
    c.width = 160; c.height = 80;
    lm_rectification_desc rect = lm_rectification_desc();
    rect.source.width = 208; rect.source.height = 120; rect.ideal.width = 176; rect.ideal.height = 96;
    lm_registration_desc reg = lm_registration_desc();
    reg.depth.width = 96; reg.depth.height = 64; reg.colour.width = 208; reg.colour.height = 120;
    static const char* const names[4] = {"LM_PIX_BAYER_RGGB8", "LM_PIX_BAYER_GRBG8", "LM_PIX_BAYER_GBRG8", "LM_PIX_BAYER_BGGR8"};
    bool ok = true;
    for (int k = 0; k < 4; ++k) {
        lm_image_desc im = lm_image_desc();
        im.data = reinterpret_cast<const void*>(static_cast<uintptr_t>(0x7F0012340003ull));
        im.width = 204; im.height = 98; im.row_stride = 207; im.format = LM_PIX_BAYER_RGGB8 + k; im.crop_x = 3; im.crop_y = 1; im.scale = 1.0f;
        const std::string n = names[k];
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), im, "");
        ok = ok && expect_words(lmc::plain(c, lmc::DEPTH), im, ("depth image of frame 0: " + n + " is a colour format").c_str());
        ok = ok && expect_words(lmc::raw_depth(c, reg, false), im, ("raw depth image of frame 0: " + n + " is a colour format").c_str());
        lm_image_desc e = im;
        e.width = 205; e.row_stride = 208;
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, ("colour image of frame 0: width and height of a " + n + " source must be even").c_str());
        e = im; e.height = 99;
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, ("colour image of frame 0: width and height of a " + n + " source must be even").c_str());
        e = im; e.row_stride = 159;
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, "colour image of frame 0: row_stride smaller than a window row");
        e = im; e.row_stride = 203;         // a window row fits, the source's does not: the neighbours of the window's last column lie there
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, "colour image of frame 0: row_stride smaller than a window row");
        e = im; e.row_stride = 204;
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, "");
        e = im; e.format |= LM_PIX_YUV_BT709;
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, ("colour image of frame 0: unknown pixel format " + std::to_string(e.format)).c_str());
        e = im; e.format |= LM_PIX_YUV_FULL;
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, ("colour image of frame 0: unknown pixel format " + std::to_string(e.format)).c_str());
        e = im; e.data = nullptr;
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, "colour image of frame 0: null data pointer");
        e = im; e.crop_x = 45;
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), e, "colour image of frame 0: 0 <= roi.x && roi.x + roi.width <= m.cols && 0 <= roi.y && roi.y + roi.height <= m.rows failed: "
                                                         "window 160 x 80 at (45, 1) in a 204 x 98 source");
        // the rectified route: the source camera's size, a source row
        e = im; e.width = 208; e.height = 120; e.row_stride = 208;
        ok = ok && expect_words(lmc::rectified(c, rect, lmc::COLOUR, false), e, "");
        ok = ok && expect_words(lmc::rectified(c, rect, lmc::COLOUR, true), e, "");
        e.row_stride = 207;
        ok = ok && expect_words(lmc::rectified(c, rect, lmc::COLOUR, false), e, "rectification: colour image of frame 0: row_stride smaller than a source row");
        ok = ok && expect_words(lmc::rectified(c, rect, lmc::DEPTH, false), e, ("depth image of frame 0: " + n + " is a colour format").c_str());
        // what a good descriptor fills
        LmIngestImage img;
        memset(&img, 0xAB, sizeof img);
        int matrix = -1;
        ++g_checks;
        if (!lmc::check_image(lmc::plain(c, lmc::COLOUR), im, 0, lm_ingest_opts{0, 0, 0}, &img, &matrix).empty() || img.kind != LM_INGEST_BAYER_RGGB + k ||
            img.src_w != 204 || img.src_h != 98 || img.crop_x != 3 || img.crop_y != 1 || img.row_stride != 207 || img.plane_stride != 0 || img.aligned != 0 ||
            img.swap_rb != 0 || matrix != 0 || lm_ingest_family(img.kind) != LM_INGEST_FAMILY_BAYER) {
            printf("FAILED: the fields of a good %s descriptor\n", names[k]);
            ok = false;
        }
    }
    // 13, 14 and 15 stay unknown, with and without a flag
    for (int bad : {13, 14, 15, 20, 13 | LM_PIX_YUV_BT709}) {
        lm_image_desc im = lm_image_desc();
        im.data = &im; im.width = 204; im.height = 98; im.row_stride = 204; im.format = bad;
        ok = ok && expect_words(lmc::plain(c, lmc::COLOUR), im, ("colour image of frame 0: unknown pixel format " + std::to_string(bad)).c_str());
    }
    ++g_checks;
    if (lm_ingest_family(LM_INGEST_PX3) != LM_INGEST_FAMILY_RGB || lm_ingest_family(LM_INGEST_PLANAR) != LM_INGEST_FAMILY_RGB ||
        lm_ingest_family(LM_INGEST_GRAY8) != LM_INGEST_FAMILY_YUV || lm_ingest_family(LM_INGEST_UYVY) != LM_INGEST_FAMILY_YUV ||
        lm_ingest_family(LM_INGEST_BAYER_RGGB) != LM_INGEST_FAMILY_BAYER) { printf("FAILED: lm_ingest_family\n"); ok = false; }
    return ok;
}

int main() {
    // the pinned 2 x 2 table of include/linemod_hip.h through this file's rule and through the lane code
    {
        Source s;
        make_source(s, 2, 2, 0, 0, false);
        s.data[0] = 1; s.data[1] = 2; s.data[2] = 3; s.data[3] = 4;
        static const u32 table[4][4] = {{0x010304, 0x010204, 0x010304, 0x010304}, {0x020103, 0x020303, 0x020303, 0x020403},
                                        {0x030102, 0x030302, 0x030302, 0x030402}, {0x040301, 0x040201, 0x040301, 0x040301}};
        for (int pattern = 0; pattern < 4; ++pattern)
            for (int i = 0; i < 4; ++i) {
                ++g_checks;
                if (rule(s, pattern, i & 1, i >> 1, nullptr) != table[pattern][i]) { printf("FAILED: the 2 x 2 table, pattern %d pixel %d\n", pattern, i); return 1; }
            }
    }
    if (!lane_cases() || !tap_cases() || !refusal_cases() || g_failed) return 1;
    printf("OK %llu checks, %llu loads, %llu of them to the safe block\n", g_checks, g_loads, g_safe_loads);
    return 0;
}
