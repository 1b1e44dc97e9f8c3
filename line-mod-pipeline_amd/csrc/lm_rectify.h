// lm_rectify.h -- the arithmetic of the lens rectification (lm_k_rectify.hip; the rule is written out in
// include/linemod_hip.h) as functions the host can run too: the fixed-point map of an ideal camera onto a pinhole + Brown-Conrady source
// camera (quant, build_map: host only, double), where an output pixel of a slot lies in the ideal geometry (place), which bytes of which
// plane a tap reads for every source kind (tap), the bilinear blend of the colour image (colour_pixel) and the nearest rule of the depth
// image (depth_pixel).  The memory read is a parameter -- ld.b8(address), ld.b16(address), ld.b32(address) -- so that
// tests/cpp/rectify_host.cpp drives exactly the kernel's loads with g++ under ASan / UBSan over sources that end where their allocation
// ends.  A load is issued only for a tap inside the source, and it reads bytes of that tap's pixel alone.  No GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "lm_ingest_yuv.h"
#include "lm_ingest_bayer.h"
#include "lm_ingest_raw.h"
#include "lm_ingest_float.h"

// the kinds of lm_kernels.h, repeated for a host program that includes this header alone
#ifndef LM_RECTIFY_KINDS
#define LM_RECTIFY_KINDS
enum { LMQ_PX3 = 0, LMQ_PX4 = 1, LMQ_PLANAR = 2, LMQ_U16 = 3, LMQ_F32 = 4 };      // = LM_INGEST_PX3 .. LM_INGEST_F32
#endif

namespace lmq {

typedef lmi::u32 u32;
typedef lmi::addr_t addr_t;

// ---- the map (host, double: every operation rounded on its own in the order written, no contraction)
// quant(s, n): -64 if s is not finite; otherwise rint(32 s), ties to even, clamped into [-64, 32 n + 32]
inline int32_t quant(double s, int n) {
    if (!__builtin_isfinite(s)) return -64;
    const double r = __builtin_rint(32.0 * s), lo = -64.0, hi = 32.0 * (double)n + 32.0;
    return (int32_t)(r < lo ? lo : r > hi ? hi : r);
}

struct Cam { double fx, fy, cx, cy, k1, k2, p1, p2, k3; int width, height; };

// map[2 * (j * ideal.width + i)] = qx, [.. + 1] = qy of ideal pixel (i, j): the forward Brown model of the source camera at the ideal
// camera's normalised coordinate.  table (2 floats per ideal pixel, anything allowed) replaces (sx, sy) when it is not null.
inline void build_map(const Cam& s, const Cam& d, const float* table, int32_t* map) {
    for (int j = 0; j < d.height; ++j)
        for (int i = 0; i < d.width; ++i) {
            const size_t at = 2 * ((size_t)j * (size_t)d.width + (size_t)i);
            double sx, sy;
            if (table) { sx = (double)table[at]; sy = (double)table[at + 1]; }
            else {
                const double x = ((double)i - d.cx) / d.fx, y = ((double)j - d.cy) / d.fy;
                const double r2 = x * x + y * y;
                const double rad = 1.0 + r2 * (s.k1 + r2 * (s.k2 + r2 * s.k3));
                const double xd = x * rad + ((2.0 * s.p1) * (x * y) + s.p2 * (r2 + 2.0 * (x * x)));
                const double yd = y * rad + (s.p1 * (r2 + 2.0 * (y * y)) + (2.0 * s.p2) * (x * y));
                sx = s.fx * xd + s.cx; sy = s.fy * yd + s.cy;
            }
            map[at] = quant(sx, s.width); map[at + 1] = quant(sy, s.height);
        }
}

// ---- where output pixel (x, y) of a w x h frame lies in the ideal geometry: xs = x - shift_x, ys = y - shift_y, outside the frame: the
// zero border; u = flip ? w - 1 - xs : xs; the ideal pixel is (crop_x + u, crop_y + ys)
struct Place { bool on; int mx, my; };
LMI_FN Place place(int w, int h, int x, int y, bool flip, int shift_x, int shift_y, int crop_x, int crop_y) {
    const int xs = x - shift_x, ys = y - shift_y;
    Place p;
    p.on = xs >= 0 && xs < w && ys >= 0 && ys < h;
    p.mx = crop_x + (flip ? w - 1 - xs : xs); p.my = crop_y + ys;
    return p;
}

// ---- a source image: every image of a rectified call has the source camera's width and height
struct Src {
    addr_t data;
    long long row_stride, plane_stride;
    int width, height;
    int kind, swap_rb, matrix;
    bool dwords;        // LMQ_PX4: data and row_stride are multiples of 4, a pixel is read as one dword
    float scale;
};

// (B | G << 8 | R << 16) of source pixel (x, y), 0 outside the source.  What is read, per kind:
//   PX3      bytes 3 x .. 3 x + 2 of row y                                   PX4  bytes 4 x .. 4 x + 2 of row y (one dword 4 x .. 4 x + 3 when `dwords`)
//   PLANAR   byte x of row y of each of the three planes                     GRAY8  byte x of row y
//   NV12/21  byte x of row y; bytes 2 (x >> 1), 2 (x >> 1) + 1 of row y >> 1 of the chroma plane
//   YUY2     of the 4 bytes at 4 (x >> 1) of row y: byte 2 (x & 1), byte 1, byte 3;  UYVY: byte 2 (x & 1) + 1, byte 0, byte 2
//   float kinds (KIND >= LM_INGEST_FLOAT)  the pixel's own three elements, or its one: lmf::float_tap, converted by lmf::to_u8 with s.scale
template <int KIND, class Ld>
LMI_FN u32 tap(const Src& s, int x, int y, Ld ld) {
    if (x < 0 || x >= s.width || y < 0 || y >= s.height) return 0u;
    const addr_t row = s.data + (addr_t)((long long)y * s.row_stride);
    u32 px = 0u;
    if constexpr (KIND >= LM_INGEST_FLOAT) {
        px = lmf::float_tap<KIND>(row, s.plane_stride, s.scale, x, ld);
    } else if (KIND == LMQ_PX3) {
        const addr_t p = row + 3u * (u32)x;
        px = ld.b8(p) | ld.b8(p + 1) << 8 | ld.b8(p + 2) << 16;
    } else if (KIND == LMQ_PX4) {
        const addr_t p = row + 4u * (u32)x;
        px = s.dwords ? ld.b32(p) & 0xFFFFFFu : ld.b8(p) | ld.b8(p + 1) << 8 | ld.b8(p + 2) << 16;
    } else if (KIND == LMQ_PLANAR) {
        const addr_t p = row + (u32)x;
        px = ld.b8(p) | ld.b8(p + (addr_t)s.plane_stride) << 8 | ld.b8(p + 2 * (addr_t)s.plane_stride) << 16;
    } else if (KIND == LM_INGEST_GRAY8) {
        return ld.b8(row + (u32)x) * 0x010101u;
    } else if (KIND == LM_INGEST_NV12 || KIND == LM_INGEST_NV21) {
        const addr_t pc = s.data + (addr_t)(s.plane_stride + (long long)(y >> 1) * s.row_stride) + 2u * (u32)(x >> 1);
        const int Y = (int)ld.b8(row + (u32)x), c0 = (int)ld.b8(pc), c1 = (int)ld.b8(pc + 1);
        return lmi::yuv_to_bgr(Y, KIND == LM_INGEST_NV12 ? c0 : c1, KIND == LM_INGEST_NV12 ? c1 : c0, lmi::yuv_coef(s.matrix));
    } else {
        const addr_t pm = row + 4u * (u32)(x >> 1);
        const u32 yb = 2u * (u32)(x & 1);
        if (KIND == LM_INGEST_YUY2) return lmi::yuv_to_bgr((int)ld.b8(pm + yb), (int)ld.b8(pm + 1), (int)ld.b8(pm + 3), lmi::yuv_coef(s.matrix));
        return lmi::yuv_to_bgr((int)ld.b8(pm + yb + 1), (int)ld.b8(pm), (int)ld.b8(pm + 2), lmi::yuv_coef(s.matrix));
    }
    return s.swap_rb ? (px & 0xFF00u) | (px >> 16) | (px & 0xFFu) << 16 : px;
}

// the blend of one channel (bits sh .. sh + 7 of the taps): exact weight products, sum 1024
LMI_FN u32 blend(u32 t00, u32 t10, u32 t01, u32 t11, int w00, int w10, int w01, int w11, int sh) {
    const int v = lmi::mul24(w00, (int)((t00 >> sh) & 0xFFu)) + lmi::mul24(w10, (int)((t10 >> sh) & 0xFFu)) + lmi::mul24(w01, (int)((t01 >> sh) & 0xFFu)) +
                  lmi::mul24(w11, (int)((t11 >> sh) & 0xFFu));
    return (u32)((v + 512) >> 10) << sh;
}

// Rc at the map entry (qx, qy), as B | G << 8 | R << 16
template <int KIND, class Ld>
LMI_FN u32 colour_pixel(const Src& s, int qx, int qy, Ld ld) {
    const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;
    const u32 t00 = tap<KIND>(s, ix, iy, ld), t10 = tap<KIND>(s, ix + 1, iy, ld), t01 = tap<KIND>(s, ix, iy + 1, ld), t11 = tap<KIND>(s, ix + 1, iy + 1, ld);
    const int w00 = (32 - ax) * (32 - ay), w10 = ax * (32 - ay), w01 = (32 - ax) * ay, w11 = ax * ay;
    return blend(t00, t10, t01, t11, w00, w10, w01, w11, 0) | blend(t00, t10, t01, t11, w00, w10, w01, w11, 8) | blend(t00, t10, t01, t11, w00, w10, w01, w11, 16);
}

// ---- raw Bayer sources (s.kind = LM_INGEST_BAYER_*; lm_ingest_bayer.h, the rule: include/linemod_hip.h).  The tap at (x, y) is the
// demosaiced pixel (x, y) of the whole source and 0 outside it, as for every kind; the reflection serves the NEIGHBOURS of a tap that is
// inside.  Taps are converted before the blend.  The four taps (ix .. ix + 1, iy .. iy + 1) of an output pixel share the 4 x 4 raw
// neighbourhood (ix - 1 .. ix + 2, iy - 1 .. iy + 2): 16 byte loads where four taps on their own take 36.  A byte is loaded only where an
// inside tap needs it -- its column and its row lie within 1 of an inside tap's -- and then from its reflected place, inside the source.
template <class Ld>
LMI_FN void bayer_taps(const Src& s, int ix, int iy, Ld ld, u32 (&t)[4]) {
    const bool cx0 = ix >= 0 && ix < s.width, cx1 = ix + 1 >= 0 && ix + 1 < s.width;
    const bool cy0 = iy >= 0 && iy < s.height, cy1 = iy + 1 >= 0 && iy + 1 < s.height;
    const bool needx[4] = {cx0, cx0 || cx1, cx0 || cx1, cx1}, needy[4] = {cy0, cy0 || cy1, cy0 || cy1, cy1};
    int N[4][4];
    LMI_UNROLL
    for (int j = 0; j < 4; ++j) {
        const addr_t row = s.data + (addr_t)((long long)lmi::bayer_reflect(iy - 1 + j, s.height) * s.row_stride);
    LMI_UNROLL
        for (int i = 0; i < 4; ++i) {
            N[j][i] = 0;
            if (needx[i] && needy[j]) N[j][i] = (int)ld.b8(row + (u32)lmi::bayer_reflect(ix - 1 + i, s.width));
        }
    }
    LMI_UNROLL
    for (int b = 0; b < 2; ++b)
    LMI_UNROLL
        for (int a = 0; a < 2; ++a) {
            const bool on = (a ? cx1 : cx0) && (b ? cy1 : cy0);
            const u32 px = lmi::bayer_pixel(N[b + 1][a + 1], N[b + 1][a] + N[b + 1][a + 2], N[b][a + 1] + N[b + 2][a + 1],
                                            N[b][a] + N[b][a + 2] + N[b + 2][a] + N[b + 2][a + 2], lmi::bayer_dx(s.kind, ix + a), lmi::bayer_dy(s.kind, iy + b));
            t[2 * b + a] = on ? px : 0u;
        }
}

// Rc at the map entry (qx, qy) of a Bayer source, as B | G << 8 | R << 16
template <class Ld>
LMI_FN u32 colour_pixel_bayer(const Src& s, int qx, int qy, Ld ld) {
    const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;
    u32 t[4];
    bayer_taps(s, ix, iy, ld, t);
    const int w00 = (32 - ax) * (32 - ay), w10 = ax * (32 - ay), w01 = (32 - ax) * ay, w11 = ax * ay;
    return blend(t[0], t[1], t[2], t[3], w00, w10, w01, w11, 0) | blend(t[0], t[1], t[2], t[3], w00, w10, w01, w11, 8) | blend(t[0], t[1], t[2], t[3], w00, w10, w01, w11, 16);
}

// Rc at the map entry (qx, qy) of a raw source (s.kind >= LM_INGEST_RAW; lm_ingest_raw.h): the blend of four PROCESSED taps
template <class Ld, class Tone>
LMI_FN u32 colour_pixel_raw(const Src& s, const lmi::RawPipe& p, int qx, int qy, Ld ld, Tone tone) {
    const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;
    lmi::RawSrc r;
    r.data = s.data; r.row_stride = s.row_stride; r.width = s.width; r.height = s.height; r.crop_x = r.crop_y = 0; r.kind = s.kind;
    u32 t[4];
    lmi::raw_taps(r, p, ix, iy, ld, tone, t);
    const int w00 = (32 - ax) * (32 - ay), w10 = ax * (32 - ay), w01 = (32 - ax) * ay, w11 = ax * ay;
    return blend(t[0], t[1], t[2], t[3], w00, w10, w01, w11, 0) | blend(t[0], t[1], t[2], t[3], w00, w10, w01, w11, 8) | blend(t[0], t[1], t[2], t[3], w00, w10, w01, w11, 16);
}

// convertTo(CV_16UC1) of a float depth value times `scale`, k_ingest's rule: ONE single-precision multiply; NaN, +-inf and everything
// <= 0 -> 0, everything >= 65535 -> 65535, otherwise round to nearest, ties to even
LMI_FN u32 to_u16(float v, float scale) {
    const float t = v * scale;
    if (!(t > 0.0f) || t == __builtin_inff()) return 0u;
    if (t >= 65535.0f) return 65535u;
    return (u32)__builtin_rintf(t);
}

// Rd at the map entry (qx, qy): the nearest source pixel, 0 outside
template <class Ld>
LMI_FN u32 depth_pixel(const Src& s, int qx, int qy, Ld ld) {
    const int x = (qx + 16) >> 5, y = (qy + 16) >> 5;
    if (x < 0 || x >= s.width || y < 0 || y >= s.height) return 0u;
    const addr_t row = s.data + (addr_t)((long long)y * s.row_stride);
    if (s.kind == LMQ_U16) return ld.b16(row + 2u * (u32)x);
    const u32 bits = ld.b32(row + 4u * (u32)x);
    float v;
    __builtin_memcpy(&v, &bits, 4);
    return to_u16(v, s.scale);
}

// the format switch: one branch per lane, uniform over the image
template <class Ld>
LMI_FN u32 colour_pixel_any(const Src& s, int qx, int qy, Ld ld) {
    switch (s.kind) {
    case LMQ_PX3: return colour_pixel<LMQ_PX3>(s, qx, qy, ld);
    case LMQ_PX4: return colour_pixel<LMQ_PX4>(s, qx, qy, ld);
    case LMQ_PLANAR: return colour_pixel<LMQ_PLANAR>(s, qx, qy, ld);
    case LM_INGEST_GRAY8: return colour_pixel<LM_INGEST_GRAY8>(s, qx, qy, ld);
    case LM_INGEST_NV12: return colour_pixel<LM_INGEST_NV12>(s, qx, qy, ld);
    case LM_INGEST_NV21: return colour_pixel<LM_INGEST_NV21>(s, qx, qy, ld);
    case LM_INGEST_YUY2: return colour_pixel<LM_INGEST_YUY2>(s, qx, qy, ld);
    case LM_INGEST_UYVY: return colour_pixel<LM_INGEST_UYVY>(s, qx, qy, ld);
    case LM_INGEST_FLOAT + 0: return colour_pixel<LM_INGEST_FLOAT + 0>(s, qx, qy, ld);
    case LM_INGEST_FLOAT + 1: return colour_pixel<LM_INGEST_FLOAT + 1>(s, qx, qy, ld);
    case LM_INGEST_FLOAT + 2: return colour_pixel<LM_INGEST_FLOAT + 2>(s, qx, qy, ld);
    case LM_INGEST_FLOAT + 3: return colour_pixel<LM_INGEST_FLOAT + 3>(s, qx, qy, ld);
    case LM_INGEST_FLOAT + 4: return colour_pixel<LM_INGEST_FLOAT + 4>(s, qx, qy, ld);
    case LM_INGEST_FLOAT + 5: return colour_pixel<LM_INGEST_FLOAT + 5>(s, qx, qy, ld);
    case LM_INGEST_FLOAT + 6: return colour_pixel<LM_INGEST_FLOAT + 6>(s, qx, qy, ld);
    case LM_INGEST_FLOAT + 7: return colour_pixel<LM_INGEST_FLOAT + 7>(s, qx, qy, ld);
    default: return colour_pixel_bayer(s, qx, qy, ld);
    }
}

}  // namespace lmq
