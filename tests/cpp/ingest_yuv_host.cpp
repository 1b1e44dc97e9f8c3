// ingest_yuv_host.cpp -- csrc/lm_ingest_yuv.h on the host: the code k_ingest_yuv runs per lane (lane_window, load_span, the chroma spans,
// the byte selectors, the conversion), with the memory read replaced by a loader that CHECKS every 16-byte load and the AMD builtins
// emulated.  Sources end exactly where their heap allocation ends (ASan guards the byte behind), at base offsets 0 .. 3 with row strides
// of bytes + 3, and 16-byte aligned ones for the fast path.  Checked, for every lane of every case:
//   * every load is 16-byte aligned;
//   * every load is the `safe` block or holds at least one byte of the source that a kept pixel needs (its luma byte, the bytes of the
//     chroma pair that covers it) -- so it lies in the page of a byte that exists;
//   * the bytes a load holds beyond the allocation (poison here) and the safe block's content (poison too) never reach a pixel;
//   * the 16 output pixels equal the definition: shift, mirror, crop, and the per-pixel rule in 64-bit integers with a table of its own.
// Prints "OK <checks>"; any failure prints the case and exits 1.  g++ -fsanitize=address,undefined; never loaded into Python.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lm_ingest_yuv.h"

using lmi::addr_t;
using lmi::u32;

static const long long TABLE[4][6] = {{16, 1220542, 1673527, -852492, -409993, 2116026},
                                      {16, 1220945, 1879825, -558796, -223607, 2215014},
                                      {0, 1048576, 1470104, -748826, -360853, 1858077},
                                      {0, 1048576, 1651297, -490864, -196424, 1945738}};

static long long floor_shift20(long long v) { return v >= 0 ? v >> 20 : -((-v + (1 << 20) - 1) >> 20); }
static u32 clamp8(long long v) { return (u32)(v < 0 ? 0 : v > 255 ? 255 : v); }
static u32 rule(int Y, int U, int V, int row) {
    const long long* t = TABLE[row];
    const long long y = (Y - t[0] > 0 ? Y - t[0] : 0) * t[1], u = U - 128, v = V - 128, h = 1 << 19;
    return clamp8(floor_shift20(y + h + t[5] * u)) | clamp8(floor_shift20(y + h + t[3] * v + t[4] * u)) << 8 | clamp8(floor_shift20(y + h + t[2] * v)) << 16;
}

struct Source {
    uint8_t* alloc = nullptr;       // the heap block; the source's last byte is its last byte
    size_t alloc_bytes = 0;
    uint8_t* data = nullptr;
    long long row_stride = 0, plane_stride = 0;
    int w = 0, h = 0, kind = 0;
    ~Source() { free(alloc); }
};

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static void make_source(Source& s, int kind, int w, int h, int offset, bool aligned) {
    const bool nv = kind == LM_INGEST_NV12 || kind == LM_INGEST_NV21, p422 = kind == LM_INGEST_YUY2 || kind == LM_INGEST_UYVY;
    const long long row_bytes = (long long)w * (p422 ? 2 : 1);
    s.kind = kind; s.w = w; s.h = h;
    s.row_stride = aligned ? (row_bytes + 15) / 16 * 16 : row_bytes + 3;
    s.plane_stride = nv ? (aligned ? h * s.row_stride + 32 : h * s.row_stride + 5) : 0;
    const long long bytes = nv ? s.plane_stride + (h / 2 - 1) * s.row_stride + row_bytes : (h - 1) * s.row_stride + row_bytes;
    s.alloc_bytes = (size_t)(offset + bytes);
    if (aligned) {
        if (posix_memalign(reinterpret_cast<void**>(&s.alloc), 16, s.alloc_bytes)) abort();
    } else {
        s.alloc = static_cast<uint8_t*>(malloc(s.alloc_bytes));
    }
    s.data = s.alloc + offset;
    static const uint8_t edge[] = {0, 1, 15, 16, 17, 127, 128, 129, 235, 239, 240, 241, 254, 255};
    for (size_t i = 0; i < s.alloc_bytes; ++i) s.alloc[i] = rnd() % 4 == 0 ? edge[rnd() % sizeof edge] : (uint8_t)rnd();
}

// the samples of source pixel (c, r), from the layout's definition
static void samples(const Source& s, int c, int r, int* Y, int* U, int* V, std::vector<addr_t>* need) {
    const uint8_t* d = s.data;
    auto at = [&](long long off) { if (need) need->push_back((addr_t)(uintptr_t)(d + off)); return (int)d[off]; };
    *U = *V = 128;
    if (s.kind == LM_INGEST_GRAY8) {
        *Y = at(r * s.row_stride + c);
    } else if (s.kind == LM_INGEST_NV12 || s.kind == LM_INGEST_NV21) {
        *Y = at(r * s.row_stride + c);
        const long long uv = s.plane_stride + (r / 2) * s.row_stride + 2 * (c / 2);
        const int first = at(uv), second = at(uv + 1);
        *U = s.kind == LM_INGEST_NV12 ? first : second; *V = s.kind == LM_INGEST_NV12 ? second : first;
    } else {
        const long long m = r * s.row_stride + 4 * (c / 2);
        const int b[4] = {at(m), at(m + 1), at(m + 2), at(m + 3)};
        if (s.kind == LM_INGEST_YUY2) { *Y = b[2 * (c & 1)]; *U = b[1]; *V = b[3]; }
        else { *Y = b[1 + 2 * (c & 1)]; *U = b[0]; *V = b[2]; }
    }
}

static unsigned long long g_checks = 0, g_loads = 0, g_safe_loads = 0;
static bool g_failed = false;
static char g_case[256];
static void fail(const char* what) {
    if (!g_failed) printf("FAILED %s: %s\n", g_case, what);
    g_failed = true;
}

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

// one frame: every lane of a w x h detector frame from the window at (crop_x, crop_y) of the source
static void run_case(const Source& s, int w, int h, int crop_x, int crop_y, bool flip, int shift_x, int shift_y, int matrix, bool aligned) {
    alignas(16) static uint8_t safe_block[16];
    const addr_t safe = (addr_t)(uintptr_t)safe_block;
    lmi::Src src;
    src.data = (addr_t)(uintptr_t)s.data; src.row_stride = s.row_stride; src.plane_stride = s.plane_stride;
    src.crop_x = crop_x; src.crop_y = crop_y; src.kind = s.kind; src.matrix = matrix;
    const int bpp = (s.kind == LM_INGEST_YUY2 || s.kind == LM_INGEST_UYVY) ? 2 : 1;
    const long long col0 = (long long)crop_x + (flip ? w - 16 + shift_x : -shift_x);
    src.aligned = lmi::spans_aligned(src.data, s.row_stride, s.plane_stride, col0, bpp);
    if (src.aligned != aligned) fail("the fast-path condition is not what the case was built for");
    for (int y = 0; y < h; ++y)
        for (int x0 = 0; x0 < w; x0 += 16) {
            snprintf(g_case, sizeof g_case, "kind %d matrix %d source %p stride %lld crop (%d, %d) flip %d shift (%d, %d) aligned %d lane (%d, %d)", s.kind,
                     matrix, (void*)s.data, s.row_stride, crop_x, crop_y, (int)flip, shift_x, shift_y, (int)aligned, x0, y);
            // the definition, pixel by pixel: expected output and the source bytes the lane needs
            u32 expect[16];
            std::vector<addr_t> need;
            for (int j = 0; j < 16; ++j) {
                const int xs = x0 + j - shift_x, ys = y - shift_y;
                expect[j] = 0;
                if (xs < 0 || xs >= w || ys < 0 || ys >= h) continue;
                const int u = flip ? w - 1 - xs : xs;
                int Y, U, V;
                samples(s, crop_x + u, crop_y + ys, &Y, &U, &V, &need);
                expect[j] = s.kind == LM_INGEST_GRAY8 ? (u32)Y * 0x010101u : rule(Y, U, V, matrix);
            }
            const lmi::Lane L = lmi::lane_window(w, h, x0, y, flip, shift_x, shift_y);
            u32 P[16];
            lmi::yuv_lane_pixels(src, L, safe, CheckedLoad{&s, safe, &need}, P);
            for (int j = 0; j < 16; ++j) {          // k_ingest's arrange
                const int k = flip ? 15 - j : j;
                const u32 got = (k >= L.klo && k < L.khi) ? P[k] : 0u;
                ++g_checks;
                if (got != expect[j]) fail("an output pixel differs from the rule");
            }
            if (g_failed) return;
        }
}

int main() {
    const int kinds[5] = {LM_INGEST_GRAY8, LM_INGEST_NV12, LM_INGEST_NV21, LM_INGEST_YUY2, LM_INGEST_UYVY};
    const int W = 32, H = 6, SW = 38, SH = 10;          // the window and the unaligned sources: crop_x 0 .. 6, crop_y 0 .. 4
    const int shifts[5][2] = {{0, 0}, {3, -2}, {-5, 1}, {17, 0}, {-32, 0}};
    int matrix = 0;
    for (int kind : kinds) {
        for (int offset = 0; offset < 4; ++offset) {
            Source s;
            make_source(s, kind, SW, SH, offset, false);
            for (int crop_x : {0, 1, 2, 3, 5, 6})
                for (int crop_y : {0, 1, 3, 4})
                    for (int flip = 0; flip < 2; ++flip)
                        for (const auto& sh : shifts) {
                            // (the general path; offset 0 with crop_x 0 still fails the fast-path condition: the stride is odd)
                            run_case(s, W, H, crop_x, crop_y, flip != 0, sh[0], sh[1], matrix, false);
                            matrix = (matrix + 1) & 3;
                            if (g_failed) return 1;
                        }
        }
        // the fast path: a 16-byte aligned source with aligned strides, windows at multiples of 16 columns (YUY2 / UYVY: of 8), any row
        Source a;
        make_source(a, kind, 64, SH, 0, true);
        const bool p422 = kind == LM_INGEST_YUY2 || kind == LM_INGEST_UYVY;
        for (int crop_x : {0, 16, 32, 8, 24})
            for (int crop_y : {0, 1, 4})
                for (int flip = 0; flip < 2; ++flip)
                    for (int sx : {0, 16, -16}) {
                        const bool fast = crop_x % 16 == 0 || p422;
                        run_case(a, W, H, crop_x, crop_y, flip != 0, sx, crop_y == 1 ? -1 : 0, matrix, fast);
                        matrix = (matrix + 1) & 3;
                        if (g_failed) return 1;
                    }
    }
    // the conversion alone: the header's rule against this file's over a grid that holds every saturation side, for the four tables
    for (int row = 0; row < 4; ++row) {
        const lmi::YuvCoef c = lmi::yuv_coef(row);
        for (int Y = 0; Y < 256; ++Y)
            for (int U = 0; U < 256; U += (U % 16 == 15 || U % 16 == 0) ? 1 : 7)
                for (int V = 0; V < 256; V += (V % 16 == 15 || V % 16 == 0) ? 1 : 7) {
                    ++g_checks;
                    if (lmi::yuv_to_bgr(Y, U, V, c) != rule(Y, U, V, row)) {
                        printf("FAILED yuv_to_bgr(%d, %d, %d) row %d\n", Y, U, V, row);
                        return 1;
                    }
                }
    }
    if (g_safe_loads == 0 || g_safe_loads == g_loads) { printf("FAILED: %llu of %llu loads went to the safe block\n", g_safe_loads, g_loads); return 1; }
    printf("OK %llu checks, %llu loads, %llu of them to the safe block\n", g_checks, g_loads, g_safe_loads);
    return 0;
}
