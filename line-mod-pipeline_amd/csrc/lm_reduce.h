// lm_reduce.h -- the arithmetic of the area-averaged reduction (lm_k_reduce.hip; the rule is written out in
// include/linemod_hip.h) as functions the host can run too, in the manner of lm_rectify.h: which source pixels lie under a reduced pixel
// (span) and with which integer weight (weight), the converted source pixel of every colour kind (pixel: lm_rectify.h's tap for the RGB,
// grey and YUV kinds, the 3 x 3 neighbourhood of a mosaic site through lm_ingest_bayer.h's / lm_ingest_raw.h's own functions), the whole
// rule of one reduced colour pixel (box over any pixel source; colour_pixel: over a source's own pixels), the two depth rules (nearest, min_valid over any depth
// image -- lm_rectify_reduce.h puts the rectified images under them; depth_nearest, depth_min_valid: over a source) and the tile a workgroup of
// k_reduce takes for a ratio (plan_tile: host).  The memory read and the tone table's read are parameters, so tests/cpp/reduce_host.cpp
// drives exactly the kernel's loads with g++ under ASan / UBSan over sources that end where their allocation ends.  A load is issued only
// for a pixel inside the source, and it reads bytes of that pixel (a mosaic site: of its reflected neighbours) alone.  No GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "lm_rectify.h"

namespace lmx {

typedef lmi::u32 u32;
typedef lmi::addr_t addr_t;

// source pixels per reduced pixel = num / den per axis, 1 <= den <= 16, den <= num <= 8 den, in lowest terms
struct Ratio { int num_x, den_x, num_y, den_y; };

// (a reduced source has sides of at most 32768 pixels, lm_ingest_check.cpp: 2 (n + 1) num stays far inside an int)

// R = floor(n den / num): the reduced pixels of a side of n source pixels
LMI_FN int reduced_size(int n, int num, int den) { return (int)(((long long)n * den) / num); }

// The source pixels with a non-zero weight under reduced pixel X: [first, first + count), count <= ceil(num / den) + 1 <= 9
struct Span { int first, count; };
LMI_FN Span span(int X, int num, int den) {
    Span s;
    s.first = (X * num) / den;
    s.count = ((X + 1) * num - 1) / den - s.first + 1;
    return s;
}

// the overlap of reduced pixel X = [X num, (X + 1) num) and source pixel i = [i den, (i + 1) den), in units of 1 / den source pixel
// (overlap: with the products a0 = X num and b0 = i den done by the caller, who steps b0 by den from tap to tap)
LMI_FN int overlap(int a0, int num, int b0, int den) {
    const int a1 = a0 + num, b1 = b0 + den;
    const int lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
    return hi > lo ? hi - lo : 0;
}
LMI_FN int weight(int X, int i, int num, int den) { return overlap(X * num, num, i * den, den); }

// v / den for 0 <= v < 65536 and 1 <= den <= 16 with inv = 1.0f / den, without an integer division: (v + 0.5) / den lies at least 1 / 32
// from an integer and the two roundings move it by less than 65536 * 2^-23 = 1 / 128.  For a tile's own coordinates.
LMI_FN int small_div(int v, float inv) { return (int)(((float)v + 0.5f) * inv); }

// no tone table: the kinds that have no raw pipeline never call it
struct NoTone { LMI_FN u32 operator()(u32) const { return 0u; } };

// c, hs, vs, ds of mosaic site (x, y): its sample and the sums of its horizontal, vertical and diagonal neighbours, the neighbours
// reflected at the SOURCE's edges (lmi::bayer_reflect) -- nine samples, each read from its own place inside the source
template <class At>
LMI_FN void site_sums(int x, int y, int w, int h, At at, int& c, int& hs, int& vs, int& ds) {
    const int xl = lmi::bayer_reflect(x - 1, w), xr = lmi::bayer_reflect(x + 1, w), yu = lmi::bayer_reflect(y - 1, h), yd = lmi::bayer_reflect(y + 1, h);
    c = at(x, y);
    hs = at(xl, y) + at(xr, y);
    vs = at(x, yu) + at(x, yd);
    ds = at(xl, yu) + at(xr, yu) + at(xl, yd) + at(xr, yd);
}

template <class Ld>
struct ByteAt {
    addr_t data; long long row_stride; Ld ld;
    LMI_FN int operator()(int x, int y) const { return (int)ld.b8(data + (addr_t)((long long)y * row_stride) + (u32)x); }
};
template <class Ld>
struct RawAt {
    const lmi::RawSrc& r; const lmi::RawPipe& p; Ld ld;
    LMI_FN int operator()(int x, int y) const { return lmi::raw_sample(r, p, x, y, ld); }
};

// The CONVERTED pixel (x, y) of a colour source, B | G << 8 | R << 16, 0 outside the source: what every tap of the blend is.  KIND is one
// of lm_rectify.h's tap kinds, or LM_INGEST_BAYER_RGGB for the four 8-bit Bayer kinds (the demosaic of the whole source, s.kind names the
// tile), or LM_INGEST_RAW for the raw kinds (demosaic and pipeline; s.kind names storage and pattern).
template <int KIND, class Ld, class Tone>
LMI_FN u32 pixel(const lmq::Src& s, const lmi::RawPipe& p, int x, int y, Ld ld, Tone tone) {
    if (KIND == LM_INGEST_BAYER_RGGB) {
        if (x < 0 || x >= s.width || y < 0 || y >= s.height) return 0u;
        int c, hs, vs, ds;
        const ByteAt<Ld> at = {s.data, s.row_stride, ld};
        site_sums(x, y, s.width, s.height, at, c, hs, vs, ds);
        return lmi::bayer_pixel(c, hs, vs, ds, lmi::bayer_dx(s.kind, x), lmi::bayer_dy(s.kind, y));
    } else if (KIND == LM_INGEST_RAW) {
        if (x < 0 || x >= s.width || y < 0 || y >= s.height) return 0u;
        lmi::RawSrc r;
        r.data = s.data; r.row_stride = s.row_stride; r.width = s.width; r.height = s.height; r.crop_x = r.crop_y = 0; r.kind = s.kind;
        const int pat = lm_raw_pattern(s.kind), up = 16 - lm_raw_bits(lm_raw_storage(s.kind));
        if (pat == LM_RAW_MONO) {
            const int v = lmi::raw_sample(r, p, x, y, ld);
            return lmi::raw_pipeline(v, v, v, up, p, tone);
        }
        int c, hs, vs, ds, R, G, B;
        const RawAt<Ld> at = {r, p, ld};
        site_sums(x, y, s.width, s.height, at, c, hs, vs, ds);
        lmi::raw_channels(c, hs, vs, ds, (x ^ pat) & 1, (y ^ (pat >> 1)) & 1, R, G, B);
        return lmi::raw_pipeline(R, G, B, up, p, tone);
    } else {
        return lmq::tap<KIND>(s, x, y, ld);
    }
}

// (acc + N / 2) / N of one channel's weighted sum, N = num_x num_y <= 16384: acc <= 255 N, the sum stays below 2^22
LMI_FN u32 finish(u32 acc, u32 n) { return (acc + (n >> 1)) / n; }
// the same with inv = 1.0f / n: the float quotient of t = acc + n / 2 < 2^23 (exact in a float) is off by at most one, and the remainder
// says which way.  tests/cpp/reduce_host.cpp enumerates every accumulator of a ratio against `/`.
LMI_FN u32 finish_fast(u32 acc, u32 n, float inv) {
    const u32 t = acc + (n >> 1);
    u32 q = (u32)((float)t * inv);
    const int r = (int)t - (int)lmi::umul24(q, n);
    q = r < 0 ? q - 1u : r >= (int)n ? q + 1u : q;
    return q;
}

// Reduced pixel (X, Y) of ANY image, B | G << 8 | R << 16: every pixel under the footprint -- at(x, y), already B | G << 8 | R << 16 --
// times wx wy.  The horizontal sums are carried unrounded (<= 255 * 128 each), blue and red side by side in one word.
template <class At>
LMI_FN u32 box(const Ratio& r, int X, int Y, At at) {
    const Span sx = span(X, r.num_x, r.den_x), sy = span(Y, r.num_y, r.den_y);
    const int ax = X * r.num_x, ay = Y * r.num_y;
    u32 ab = 0u, ag = 0u, ar = 0u;
    for (int j = 0, by = sy.first * r.den_y; j < sy.count; ++j, by += r.den_y) {
        u32 hbr = 0u, hg = 0u;
        for (int i = 0, bx = sx.first * r.den_x; i < sx.count; ++i, bx += r.den_x) {
            const u32 px = at(sx.first + i, sy.first + j), w = (u32)overlap(ax, r.num_x, bx, r.den_x);
            hbr += lmi::umul24(w, px & 0xFF00FFu);          // (every factor and every sum of this function stays below 2^24)
            hg += lmi::umul24(w, (px >> 8) & 0xFFu);
        }
        const u32 w = (u32)overlap(ay, r.num_y, by, r.den_y);
        ab += lmi::umul24(w, hbr & 0xFFFFu); ag += lmi::umul24(w, hg); ar += lmi::umul24(w, hbr >> 16);
    }
    const u32 n = (u32)(r.num_x * r.num_y);
    const float inv = 1.0f / (float)n;
    return finish_fast(ab, n, inv) | finish_fast(ag, n, inv) << 8 | finish_fast(ar, n, inv) << 16;
}

template <int KIND, class Ld, class Tone>
struct PixelAt {
    const lmq::Src& s; const lmi::RawPipe& p; Ld ld; Tone tone;
    LMI_FN u32 operator()(int x, int y) const { return pixel<KIND>(s, p, x, y, ld, tone); }
};

// Reduced colour pixel (X, Y) of a source: the box over its converted pixels
template <int KIND, class Ld, class Tone>
LMI_FN u32 colour_pixel_of(const lmq::Src& s, const lmi::RawPipe& p, const Ratio& r, int X, int Y, Ld ld, Tone tone) {
    const PixelAt<KIND, Ld, Tone> at = {s, p, ld, tone};
    return box(r, X, Y, at);
}

// the kind switch: one branch per reduced pixel, uniform over the image
template <class Ld, class Tone>
LMI_FN u32 colour_pixel(const lmq::Src& s, const lmi::RawPipe& p, const Ratio& r, int X, int Y, Ld ld, Tone tone) {
    switch (s.kind) {
    case LMQ_PX3: return colour_pixel_of<LMQ_PX3>(s, p, r, X, Y, ld, tone);
    case LMQ_PX4: return colour_pixel_of<LMQ_PX4>(s, p, r, X, Y, ld, tone);
    case LMQ_PLANAR: return colour_pixel_of<LMQ_PLANAR>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_GRAY8: return colour_pixel_of<LM_INGEST_GRAY8>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_NV12: return colour_pixel_of<LM_INGEST_NV12>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_NV21: return colour_pixel_of<LM_INGEST_NV21>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_YUY2: return colour_pixel_of<LM_INGEST_YUY2>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_UYVY: return colour_pixel_of<LM_INGEST_UYVY>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 0: return colour_pixel_of<LM_INGEST_FLOAT + 0>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 1: return colour_pixel_of<LM_INGEST_FLOAT + 1>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 2: return colour_pixel_of<LM_INGEST_FLOAT + 2>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 3: return colour_pixel_of<LM_INGEST_FLOAT + 3>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 4: return colour_pixel_of<LM_INGEST_FLOAT + 4>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 5: return colour_pixel_of<LM_INGEST_FLOAT + 5>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 6: return colour_pixel_of<LM_INGEST_FLOAT + 6>(s, p, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 7: return colour_pixel_of<LM_INGEST_FLOAT + 7>(s, p, r, X, Y, ld, tone);
    default: return s.kind >= LM_INGEST_RAW ? colour_pixel_of<LM_INGEST_RAW>(s, p, r, X, Y, ld, tone) : colour_pixel_of<LM_INGEST_BAYER_RGGB>(s, p, r, X, Y, ld, tone);
    }
}

// to_u16 of depth pixel (x, y), 0 outside the source
template <class Ld>
LMI_FN u32 depth_value(const lmq::Src& s, int x, int y, Ld ld) {
    if (x < 0 || x >= s.width || y < 0 || y >= s.height) return 0u;
    const addr_t row = s.data + (addr_t)((long long)y * s.row_stride);
    if (s.kind == LMQ_U16) return ld.b16(row + 2u * (u32)x);
    const u32 bits = ld.b32(row + 4u * (u32)x);
    float v;
    __builtin_memcpy(&v, &bits, 4);
    return lmq::to_u16(v, s.scale);
}

template <class Ld>
struct DepthAt {
    const lmq::Src& s; Ld ld;
    LMI_FN u32 operator()(int x, int y) const { return depth_value(s, x, y, ld); }
};

// NEAREST over ANY depth image at(x, y): the pixel that contains the footprint's centre
template <class At>
LMI_FN u32 nearest(const Ratio& r, int X, int Y, At at) {
    return at(((2 * X + 1) * r.num_x) / (2 * r.den_x), ((2 * Y + 1) * r.num_y) / (2 * r.den_y));
}
template <class Ld>
LMI_FN u32 depth_nearest(const lmq::Src& s, const Ratio& r, int X, int Y, Ld ld) {
    const DepthAt<Ld> at = {s, ld};
    return nearest(r, X, Y, at);
}

// a source pixel's centre lies in the footprint: 2 X num <= (2 i + 1) den < 2 (X + 1) num
LMI_FN bool centre_inside(int X, int i, int num, int den) {
    const int c = (2 * i + 1) * den;
    return 2 * X * num <= c && c < 2 * (X + 1) * num;
}

// MIN_VALID over ANY depth image at(x, y): the smallest non-zero value among the pixels whose centre lies in the footprint, 0 when there is none
template <class At>
LMI_FN u32 min_valid(const Ratio& r, int X, int Y, At at) {
    const Span sx = span(X, r.num_x, r.den_x), sy = span(Y, r.num_y, r.den_y);
    u32 best = 0xFFFFFFFFu;
    for (int j = 0; j < sy.count; ++j) {
        if (!centre_inside(Y, sy.first + j, r.num_y, r.den_y)) continue;
        for (int i = 0; i < sx.count; ++i) {
            if (!centre_inside(X, sx.first + i, r.num_x, r.den_x)) continue;
            const u32 v = at(sx.first + i, sy.first + j);
            if (v != 0u && v < best) best = v;
        }
    }
    return best == 0xFFFFFFFFu ? 0u : best;
}
template <class Ld>
LMI_FN u32 depth_min_valid(const lmq::Src& s, const Ratio& r, int X, int Y, Ld ld) {
    const DepthAt<Ld> at = {s, ld};
    return min_valid(r, X, Y, at);
}

// ---- the tile of a workgroup of k_reduce (host).  A workgroup writes tw x th slot pixels (tw * th <= 256, powers of two) and stages the
// converted source pixels under them -- at most sw x sh -- and their horizontal sums (sh x tw, two words each) in LDS.  The tile starts at
// 32 x 8 and is halved, the longer side of the source patch first, until the footprint fits LDS_BUDGET: bounded at 8 : 1 on both axes.
enum { LDS_BUDGET = 24 * 1024 };
struct Tile { int tw, th, sw, sh; u32 lds_bytes; };
// the source pixels under t consecutive reduced pixels, at most (the first may begin anywhere inside a source pixel)
inline int patch_side(int t, int num, int den) { return (t * num + den - 1) / den + 1; }
inline Tile plan_tile(const Ratio& r) {
    Tile t;
    t.tw = 32; t.th = 8;
    for (;;) {
        t.sw = patch_side(t.tw, r.num_x, r.den_x); t.sh = patch_side(t.th, r.num_y, r.den_y);
        t.lds_bytes = (u32)(t.sw * t.sh * 4 + t.sh * t.tw * 8);
        if (t.lds_bytes <= (u32)LDS_BUDGET || (t.tw == 1 && t.th == 1)) return t;
        if (t.th == 1 || (t.tw > 1 && t.sw >= 2 * t.sh)) t.tw >>= 1; else t.th >>= 1;
    }
}

}  // namespace lmx
