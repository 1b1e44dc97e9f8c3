// lm_dev_reduce.h -- what the tiled kernels of the area-averaged reduction share on the device: k_reduce_conv (lm_k_reduce.hip, DESIGN.md
// section 18) and k_rectify_reduce (lm_k_rectify_reduce.hip, section 19) differ in phase A alone -- what a pixel of the patch under a tile
// is and how it gets into LDS.  Here: the memory reads lm_rectify.h / lm_reduce.h take as parameters, the run of reduced pixels under a
// tile (tile_run), the patch under that run (patch_of), phase B (hsum: the horizontal weighted sums, carried unrounded) and phase C
// (vsum: the vertical sums and the one rounded division).  All the arithmetic is lm_reduce.h's.
#pragma once
#include "lm_dev.h"
#include "lm_kernels.h"

namespace lmt {

using lmq::addr_t;

// the address is an integer, and a pointer made from an integer would be a generic one
struct GlobalLd {
    __device__ __forceinline__ u32 b8(addr_t p) const { return *reinterpret_cast<const __attribute__((address_space(1))) uint8_t*>(p); }
    __device__ __forceinline__ u32 b16(addr_t p) const { return *reinterpret_cast<const __attribute__((address_space(1))) uint16_t*>(p); }
    __device__ __forceinline__ u32 b32(addr_t p) const { return *reinterpret_cast<const __attribute__((address_space(1))) uint32_t*>(p); }
};

// the raw pipeline's tone table, read through the cache
struct GlobalTone {
    addr_t t;
    __device__ __forceinline__ u32 operator()(u32 i) const { return *reinterpret_cast<const __attribute__((address_space(1))) uint8_t*>(t + i); }
};

// the device copy of the raw pipeline, without its tone table (uniform: scalar loads)
__device__ __forceinline__ lmi::RawPipe load_pipe(const lm_raw_processing* raw) {
    lmi::RawPipe pipe = lmi::RawPipe();
    pipe.black = raw->black;
#pragma unroll
    for (int k = 0; k < 3; ++k) pipe.gain[k] = raw->gain[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) pipe.ccm[k] = raw->ccm[k];
    return pipe;
}

// the reduced pixels a tile's slot pixels come from along one axis: slot pixels [t0, t0 + tn) clipped to the frame, less the shift,
// mirrored -> [lo, lo + n) in the reduced geometry (n <= 0: the tile lies in the zero border)
struct Run { int lo, n; };
__device__ __forceinline__ Run tile_run(int t0, int tn, int size, int shift, bool flip, int crop) {
    const int end = t0 + tn < size ? t0 + tn : size;
    int s_lo = t0 - shift, s_hi = end - 1 - shift;
    s_lo = s_lo > 0 ? s_lo : 0; s_hi = s_hi < size - 1 ? s_hi : size - 1;
    Run r;
    r.n = s_hi - s_lo + 1;
    r.lo = crop + (flip ? size - 1 - s_hi : s_lo);
    return r;
}

// the pixels under the runs rx, ry: (sx0 .. sx0 + SW - 1, sy0 .. sy0 + SH - 1), all zero when a run is empty
struct Patch { int sx0, sy0, SW, SH; };
__device__ __forceinline__ Patch patch_of(const lmx::Ratio& q, const Run& rx, const Run& ry) {
    Patch p = {0, 0, 0, 0};
    if (rx.n > 0 && ry.n > 0) {
        const lmx::Span fx = lmx::span(rx.lo, q.num_x, q.den_x), lx_ = lmx::span(rx.lo + rx.n - 1, q.num_x, q.den_x);
        const lmx::Span fy = lmx::span(ry.lo, q.num_y, q.den_y), ly_ = lmx::span(ry.lo + ry.n - 1, q.num_y, q.den_y);
        p.sx0 = fx.first; p.SW = lx_.first + lx_.count - p.sx0;
        p.sy0 = fy.first; p.SH = ly_.first + ly_.count - p.sy0;
    }
    return p;
}

// phase B: H[r][col] = sum over the taps of reduced column rx.lo + col in patch row r of C[SH][SW] (B | G << 8 | R << 16 per pixel).  256
// is a multiple of tw: a lane keeps its column, so its span and weights are set up once
__device__ __forceinline__ void hsum(const lmx::Ratio& q, const Run& rx, int sx0, int SW, int SH, int tw, int ltw, int tid, const u32* C, u32* H) {
    const int col = tid & (tw - 1), X = rx.lo + col;
    const lmx::Span sp = lmx::span(X, q.num_x, q.den_x);
    const int a0 = X * q.num_x, b0 = sp.first * q.den_x;
    if (col < rx.n)
        for (int r = tid >> ltw; r < SH; r += 256 >> ltw) {
            const u32* row = C + lmi::mul24(r, SW) + (sp.first - sx0);
            u32 hbr = 0u, hg = 0u;
            for (int k = 0, b = b0; k < sp.count; ++k, b += q.den_x) {
                const u32 px = row[k], w = (u32)lmx::overlap(a0, q.num_x, b, q.den_x);
                hbr += lmi::umul24(w, px & 0xFF00FFu);          // (weights <= 16, sums <= 255 * 128: full-rate 24-bit products)
                hg += lmi::umul24(w, (px >> 8) & 0xFFu);
            }
            *reinterpret_cast<uint2*>(H + 2 * ((r << ltw) + col)) = make_uint2(hbr, hg);
        }
}

// phase C: reduced pixel (mx, my) of the tile's runs from H, as B | G << 8 | R << 16.  The rows under reduced row my, counted from the
// tile's first patch row: (ry.lo num_y) / den_y = sy0 is the one division (uniform), the lane's own offset is small (lmx::small_div)
__device__ __forceinline__ u32 vsum(const lmx::Ratio& q, const Run& rx, const Run& ry, int sy0, int ltw, int mx, int my, const u32* H) {
    const int col = mx - rx.lo, dy = my - ry.lo;
    const int rem = ry.lo * q.num_y - sy0 * q.den_y, v0 = rem + lmi::mul24(dy, q.num_y);
    const float inv_d = 1.0f / (float)q.den_y;
    const int first = lmx::small_div(v0, inv_d), count = lmx::small_div(v0 + q.num_y - 1, inv_d) - first + 1;
    u32 ab = 0u, ag = 0u, ar = 0u;
    for (int k = 0, b = lmi::mul24(first, q.den_y); k < count; ++k, b += q.den_y) {
        const uint2 h2 = *reinterpret_cast<const uint2*>(H + 2 * (((first + k) << ltw) + col));
        const u32 w = (u32)lmx::overlap(v0, q.num_y, b, q.den_y);
        ab += lmi::umul24(w, h2.x & 0xFFFFu); ag += lmi::umul24(w, h2.y); ar += lmi::umul24(w, h2.x >> 16);
    }
    const u32 n = (u32)(q.num_x * q.num_y);
    const float inv_n = 1.0f / (float)n;
    return lmx::finish_fast(ab, n, inv_n) | lmx::finish_fast(ag, n, inv_n) << 8 | lmx::finish_fast(ar, n, inv_n) << 16;
}

}  // namespace lmt
