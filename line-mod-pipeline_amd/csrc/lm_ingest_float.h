// lm_ingest_float.h -- the float colour sources of k_ingest_float / k_rectify_float / k_reduce_conv / k_rectify_reduce_float (lm_k_ingest.hip,
// lm_k_rectify.hip, lm_k_reduce.hip, lm_k_rectify_reduce.hip, DESIGN.md section 13 "Float sources"; the rule is written out in
// include/linemod_hip.h) as functions the host can run too, in the manner of lm_ingest_yuv.h: the conversion of one channel (to_u8), the
// exact widening of a binary16 (half_to_float), the two conversions of the way out (from_u8_f32, from_u8_f16), float_lane_pixels, which
// turns a lane's span of 16 float pixels into its 16 (B | G << 8 | R << 16) registers, and the tap of the tiled routes (float_tap).  The
// memory read is a parameter and lm_ingest_yuv.h's lane_window and load_span are used as they are, so tests/cpp/ingest_float_host.cpp
// drives exactly this code with g++ under ASan / UBSan over sources that end where their allocation ends, and checks every load the
// kernel would issue.  No GPU.
#pragma once
#include <stdint.h>

#include "lm_ingest_bayer.h"

// LmIngestImage::kind of a float colour source: LM_INGEST_FLOAT (lm_ingest_bayer.h: the fifth family) + element * 4 + shape
//   shape 0 = three interleaved channels, 1 = four (the fourth ignored), 2 = three planes, 3 = grey;  element 0 = binary32, 1 = binary16
enum { LM_FLOAT_PX3 = 0, LM_FLOAT_PX4 = 1, LM_FLOAT_PLANAR = 2, LM_FLOAT_GRAY = 3 };
LMI_FN int lm_float_kind(int half, int shape) { return LM_INGEST_FLOAT + half * 4 + shape; }
LMI_FN int lm_float_half(int kind) { return ((kind - LM_INGEST_FLOAT) >> 2) & 1; }
LMI_FN int lm_float_shape(int kind) { return (kind - LM_INGEST_FLOAT) & 3; }

namespace lmf {

typedef lmi::u32 u32;
typedef lmi::addr_t addr_t;

LMI_FN float as_float(u32 bits) {
    float v;
    __builtin_memcpy(&v, &bits, 4);
    return v;
}
LMI_FN u32 as_bits(float v) {
    u32 bits;
    __builtin_memcpy(&bits, &v, 4);
    return bits;
}

// a * b as ONE single-precision multiply, rounded to nearest, never fused into anything (the host build: -ffp-contract=off)
LMI_FN float mul_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}

// the binary32 value of a binary16 bit pattern: exact, subnormals included (v_cvt_f32_f16; the library's denormal mode keeps them)
LMI_FN float half_to_float(u32 h) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned short b = (unsigned short)h;
    _Float16 x;
    __builtin_memcpy(&x, &b, 2);
    return (float)x;
#else
    const u32 sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    if (e == 31u) return as_float(sign | 0x7F800000u | m << 13);
    if (e != 0u) return as_float(sign | (e + 112u) << 23 | m << 13);
    const float f = (float)m * 5.9604644775390625e-8f;          // m * 2^-24: exact
    return as_float(sign | as_bits(f));
#endif
}

// to_u8 of one channel (include/linemod_hip.h): t = v * scale; NaN and everything <= 0 -> 0, everything >= 255 (+inf too) -> 255,
// otherwise round to nearest, ties to even (v_rndne_f32)
LMI_FN u32 to_u8(float v, float scale) {
    const float t = mul_rn(v, scale);
    if (!(t > 0.0f)) return 0u;
    if (t >= 255.0f) return 255u;
    return (u32)__builtin_rintf(t);
}

// ---- the way out (lm_export_frames): channel value c = 0 .. 255 as f = (float)c * scale, one multiply; binary16: f rounded once,
// nearest, ties to even, overflowing to +inf (v_cvt_f16_f32).  scale is finite and positive: f is never NaN and never negative.
LMI_FN u32 from_u8_f32(u32 c, float scale) { return as_bits(mul_rn((float)c, scale)); }
LMI_FN u32 float_to_half(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 x = (_Float16)f;
    unsigned short b;
    __builtin_memcpy(&b, &x, 2);
    return b;
#else
    const u32 bits = as_bits(f), sign = (bits >> 16) & 0x8000u, x = bits & 0x7FFFFFFFu;
    if (x > 0x7F800000u) return sign | 0x7E00u;
    if (x >= 0x47800000u) return sign | 0x7C00u;                // 65536 and beyond, +inf
    if (x < 0x38800000u)                                        // below 2^-14: a binary16 subnormal, in units of 2^-24 (the product is exact)
        return sign | (u32)__builtin_rintf(as_float(x) * 16777216.0f);
    u32 h = ((x >> 23) - 112u) << 10 | ((x & 0x7FFFFFu) >> 13);
    const u32 rem = x & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;     // (the carry runs into the exponent, up to 0x7C00 = +inf)
    return sign | h;
#endif
}
LMI_FN u32 from_u8_f16(u32 c, float scale) { return float_to_half(mul_rn((float)c, scale)); }

// ---- the float source of one lane.  Source pixel k of the lane is column c0 + k of source row r, c0 = crop_x + uL (negative where the
// shift reaches beyond the window: those k are not kept).
struct Src {
    addr_t data;
    long long row_stride, plane_stride;
    int crop_x, crop_y, kind, swap_rb;
    bool aligned;
    float scale;
};

// element i of a span's dwords
template <int ES>
LMI_FN float element(const u32* D, int i) {
    if (ES == 4) return as_float(D[i]);
    return half_to_float((D[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
}

LMI_FN u32 pack(u32 c0, u32 c1, u32 c2, int swap_rb) { return swap_rb ? c2 | c1 << 8 | c0 << 16 : c0 | c1 << 8 | c2 << 16; }

// NCH interleaved channels of ES bytes (NCH = 1: grey, B = G = R; NCH = 4: the fourth is ignored): ONE span of 16 NCH ES bytes -- 32 .. 256,
// its 2 .. 17 loads in flight together
template <int ES, int NCH, class Load>
LMI_FN void interleaved_pixels(const Src& s, const lmi::Lane& L, addr_t safe, Load ld, u32 (&P)[16]) {
    constexpr int PB = ES * NCH, NB = 16 * PB;
    const long long c0 = (long long)s.crop_x + L.uL, r = (long long)s.crop_y + L.ys;
    const addr_t p = s.data + (addr_t)(r * s.row_stride + c0 * PB);
    u32 D[NB / 4];
    lmi::load_span<NB>(p, p + (addr_t)(PB * L.klo), p + (addr_t)(PB * L.khi), s.aligned, safe, ld, D);
    LMI_UNROLL
    for (int k = 0; k < 16; ++k) {
        const u32 a = to_u8(element<ES>(D, NCH * k), s.scale);
        if (NCH == 1) P[k] = a * 0x010101u;
        else P[k] = pack(a, to_u8(element<ES>(D, NCH * k + 1), s.scale), to_u8(element<ES>(D, NCH * k + 2), s.scale), s.swap_rb);
    }
}

// three planes of ES bytes per pixel, plane_stride apart: three spans of 16 ES bytes
template <int ES, class Load>
LMI_FN void planar_pixels(const Src& s, const lmi::Lane& L, addr_t safe, Load ld, u32 (&P)[16]) {
    constexpr int NB = 16 * ES;
    const long long c0 = (long long)s.crop_x + L.uL, r = (long long)s.crop_y + L.ys;
    const addr_t p = s.data + (addr_t)(r * s.row_stride + c0 * ES), lo = (addr_t)(ES * L.klo), hi = (addr_t)(ES * L.khi);
    const addr_t p1 = p + (addr_t)s.plane_stride, p2 = p + 2 * (addr_t)s.plane_stride;
    u32 A[NB / 4], B[NB / 4], C[NB / 4];
    lmi::load_span<NB>(p, p + lo, p + hi, s.aligned, safe, ld, A);
    lmi::load_span<NB>(p1, p1 + lo, p1 + hi, s.aligned, safe, ld, B);
    lmi::load_span<NB>(p2, p2 + lo, p2 + hi, s.aligned, safe, ld, C);
    LMI_UNROLL
    for (int k = 0; k < 16; ++k)
        P[k] = pack(to_u8(element<ES>(A, k), s.scale), to_u8(element<ES>(B, k), s.scale), to_u8(element<ES>(C, k), s.scale), s.swap_rb);
}

template <int ES, class Load>
LMI_FN void float_lane_pixels_of(const Src& s, const lmi::Lane& L, addr_t safe, Load ld, u32 (&P)[16]) {
    switch (lm_float_shape(s.kind)) {
    case LM_FLOAT_PX3: interleaved_pixels<ES, 3>(s, L, safe, ld, P); break;
    case LM_FLOAT_PX4: interleaved_pixels<ES, 4>(s, L, safe, ld, P); break;
    case LM_FLOAT_PLANAR: planar_pixels<ES>(s, L, safe, ld, P); break;
    default: interleaved_pixels<ES, 1>(s, L, safe, ld, P); break;
    }
}

// the (B, G, R, 0) registers of a lane's 16 source pixels, for the kinds of this header (the kind is uniform: scalar branches)
template <class Load>
LMI_FN void float_lane_pixels(const Src& s, const lmi::Lane& L, addr_t safe, Load ld, u32 (&P)[16]) {
    if (lm_float_half(s.kind)) float_lane_pixels_of<2>(s, L, safe, ld, P);
    else float_lane_pixels_of<4>(s, L, safe, ld, P);
}

// ---- the tap of the tiled routes: pixel x of the row at `row` (inside the source: the caller's test), as c0 | c1 << 8 | c2 << 16 in
// MEMORY order, from naturally aligned element loads -- ld.b32 / ld.b16 of the pixel's own elements alone
template <int KIND, class Ld>
LMI_FN u32 float_tap(addr_t row, long long plane_stride, float scale, int x, Ld ld) {
    constexpr int HALF = ((KIND - LM_INGEST_FLOAT) >> 2) & 1, SHAPE = (KIND - LM_INGEST_FLOAT) & 3, ES = HALF ? 2 : 4;
    const auto el = [&](addr_t p) { return to_u8(HALF ? half_to_float(ld.b16(p)) : as_float(ld.b32(p)), scale); };
    if (SHAPE == LM_FLOAT_GRAY) return el(row + (u32)(ES * x)) * 0x010101u;
    if (SHAPE == LM_FLOAT_PLANAR) {
        const addr_t p = row + (u32)(ES * x);
        return el(p) | el(p + (addr_t)plane_stride) << 8 | el(p + 2 * (addr_t)plane_stride) << 16;
    }
    const addr_t p = row + (u32)((SHAPE == LM_FLOAT_PX3 ? 3 : 4) * ES * x);
    return el(p) | el(p + ES) << 8 | el(p + 2 * ES) << 16;
}

}  // namespace lmf
