// lm_ingest_raw.h -- the high-bit raw colour sources and the raw pipeline of k_ingest_raw / k_rectify_raw (lm_k_ingest.hip, lm_k_rectify.hip,
// DESIGN.md section 13 "High-bit raw sources and the raw pipeline"; the rule is written out in include/linemod_hip.h) as functions the host
// can run too, in the manner of lm_ingest_bayer.h: how a sample lies in a row (raw_row: 8 / 10 / 12 / 16 bits per sample of the row's
// little-endian bit string -- the u16 containers, PFNC's 10p and 12p, and the 8-bit Bayer formats under a pipeline), the N-bit bilinear
// demosaic with the channels kept apart (raw_channels), the pipeline of one pixel (raw_pipeline: gains, matrix, tone table),
// raw_lane_pixels, which turns a lane's three reflected source rows into its 16 (B | G << 8 | R << 16) registers, and the four taps of a
// rectified pixel (raw_taps).  The memory read and the tone table's read are parameters and lm_ingest_yuv.h's lane_window and load_span
// are used as they are, so tests/cpp/ingest_raw_host.cpp drives exactly this code with g++ under ASan / UBSan over sources that end where
// their allocation ends, and checks every load the kernel would issue.  No GPU.
#pragma once
#include <stdint.h>

#include "lm_ingest_bayer.h"

// LmIngestImage::kind of a raw source: LM_INGEST_RAW + storage * 8 + pattern (lm_ingest_bayer.h: the fourth family).
//   pattern 0 .. 3 = red_x | red_y << 1 as the 8-bit Bayer kinds, 4 = mono
//   storage 0 .. 3 = 10 / 12 / 14 / 16 bits in a u16, 4 = 10p, 5 = 12p (the public format's bits 4 .. 7 >> 4), 6 = one byte per sample: an
//           8-bit Bayer format while a pipeline is set
enum { LM_RAW_U16_10 = 0, LM_RAW_U16_12 = 1, LM_RAW_U16_14 = 2, LM_RAW_U16_16 = 3, LM_RAW_P10 = 4, LM_RAW_P12 = 5, LM_RAW_U8 = 6 };
enum { LM_RAW_MONO = 4 };
LMI_FN int lm_raw_kind(int storage, int pattern) { return LM_INGEST_RAW + storage * 8 + pattern; }
LMI_FN int lm_raw_storage(int kind) { return (kind - LM_INGEST_RAW) >> 3; }
LMI_FN int lm_raw_pattern(int kind) { return (kind - LM_INGEST_RAW) & 7; }
// N: the bits of a sample;  the bits a sample takes in its row
LMI_FN int lm_raw_bits(int storage) { return storage < LM_RAW_P10 ? 10 + 2 * storage : storage == LM_RAW_P10 ? 10 : storage == LM_RAW_P12 ? 12 : 8; }
LMI_FN int lm_raw_row_bits(int storage) { return storage < LM_RAW_P10 ? 16 : lm_raw_bits(storage); }

namespace lmi {

// bits s .. s + 31 of the 64 bits {hi, lo} (v_alignbit_b32; s = 0 .. 31)
LMI_FN u32 funnel_bits(u32 hi, u32 lo, u32 s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return (u32)((((uint64_t)hi << 32) | lo) >> (s & 31u));
#endif
}
// a * b of two values below 2^24 whose product fits 32 bits (v_mul_u32_u24: full rate)
LMI_FN u32 umul24(u32 a, u32 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    if (a >= (1u << 24) || b >= (1u << 24) || (uint64_t)a * b > 0xFFFFFFFFull) __builtin_trap();
    return a * b;
#endif
}

// lm_raw_processing without its table: black level, Q10 gains (R, G, B), Q10 matrix (rows = output R, G, B).  The table is read through
// tone(i), i = 0 .. 4095.
struct RawPipe { int black; u32 gain[3]; int ccm[9]; };

// Steps 3 - 6 of the rule for one pixel: its N-bit (r, g, b), up = 16 - N.  32-bit throughout: x <= 65535 and gain <= 65535, so
// x * gain + 512 < 2^32 (unsigned); |ccm| <= 8192, so |sum| <= 3 * 8192 * 65535 + 512 < 2^31 (signed, every factor within 24 bits).
template <class Tone>
LMI_FN u32 raw_pipeline(int r, int g, int b, int up, const RawPipe& p, Tone tone) {
    const int v[3] = {r, g, b};
    int x[3];
    LMI_UNROLL
    for (int c = 0; c < 3; ++c) {
        const u32 t = (umul24((u32)v[c] << up, p.gain[c]) + 512u) >> 10;
        x[c] = (int)(t < 65535u ? t : 65535u);
    }
    u32 out[3];
    LMI_UNROLL
    for (int i = 0; i < 3; ++i) {
        const int y = (mul24(p.ccm[3 * i], x[0]) + mul24(p.ccm[3 * i + 1], x[1]) + mul24(p.ccm[3 * i + 2], x[2]) + 512) >> 10;
        out[i] = tone((u32)(y < 0 ? 0 : y > 65535 ? 65535 : y) >> 4) & 0xFFu;
    }
    return out[2] | out[1] << 8 | out[0] << 16;
}

// N-bit (R, G, B) of a site: lm_ingest_bayer.h's bayer_pixel with the channels kept apart (a channel no longer fits a byte)
LMI_FN void raw_channels(int c, int hs, int vs, int ds, int dx, int dy, int& r, int& g, int& b) {
    const bool green = dx != dy;
    const int a1 = green ? (hs + 1) >> 1 : c, a2 = green ? (vs + 1) >> 1 : (ds + 2) >> 2;
    g = green ? c : (hs + vs + 2) >> 2;
    r = dy ? a2 : a1; b = dy ? a1 : a2;
}

struct RawSrc {
    addr_t data;
    long long row_stride;
    int width, height;          // of the SOURCE: its edges reflect, the window's do not
    int crop_x, crop_y, kind;
};

// Samples c0 - 1 .. c0 + 16 of source row `row` as V[0 .. 17], clamped to maxv and less the black level; [vlo, vhi): the samples of the
// row the lane needs.  SB = the bits a sample takes in the row: sample c is bits [SB c, SB c + SB) of the row read as a little-endian
// bit string (a u16 container is just that with SB = 16, a byte with SB = 8).  The needed bytes are [SB vlo >> 3, (SB vhi + 7) >> 3); the
// span starts at byte SB (c0 - 1) >> 3 (floor: c0 - 1 may be negative, such samples are not needed and not loaded) and the bit phase
// SB (c0 - 1) & 7 is the same for the whole lane: ONE funnel shift of the span puts every sample at a compile-time position.
template <int SB, class Load>
LMI_FN void raw_row(const RawSrc& s, long long row, long long c0, long long vlo, long long vhi, int maxv, int black, addr_t safe, Load ld, int (&V)[18]) {
    constexpr int NB = SB == 16 ? 48 : 32;          // bytes of the span: 18 samples and at most 6 bits of phase -> 18, 24, 28, 36
    constexpr int NE = (18 * SB + 31) / 32;
    const addr_t base = s.data + (addr_t)(row * s.row_stride);
    const long long bit0 = (long long)SB * (c0 - 1);
    const bool any = vlo < vhi;
    const addr_t blo = base + (addr_t)(any ? (SB * vlo) >> 3 : 0), bhi = base + (addr_t)(any ? (SB * vhi + 7) >> 3 : 0);
    u32 D[NB / 4], E[NE + 1];
    load_span<NB>(base + (addr_t)(bit0 >> 3), blo, bhi, false, safe, ld, D);
    const u32 ph = (u32)(bit0 & 7);
    LMI_UNROLL
    for (int i = 0; i < NE; ++i) E[i] = (SB & 7) ? funnel_bits(D[i + 1], D[i], ph) : D[i];
    E[NE] = 0u;
    LMI_UNROLL
    for (int j = 0; j < 18; ++j) {
        const int w = (SB * j) >> 5, o = (SB * j) & 31;
        const u32 bits = o + SB <= 32 ? E[w] >> o : funnel_bits(E[w + 1], E[w], (u32)o);
        int v = (int)(bits & ((1u << SB) - 1u));
        v = v < maxv ? v : maxv;
        V[j] = v > black ? v - black : 0;
    }
}

// The 16 source pixels of a lane through black level, demosaic and pipeline: pixel k is column c0 + k of source row r (c0 = crop_x + uL,
// r = crop_y + ys).  A Bayer pattern needs samples c0 - 1 .. c0 + 16 of rows r - 1, r, r + 1, reflected as bayer_lane_pixels reflects
// them; mono needs the kept samples of row r alone.  The range handed to raw_row is the kept columns (Bayer: +- 1) clipped to the source:
// every load that is issued holds a byte of it.
template <int SB, class Load, class Tone>
LMI_FN void raw_lane_rows(const RawSrc& s, const RawPipe& p, const Lane& L, int bits, addr_t safe, Load ld, Tone tone, u32 (&P)[16]) {
    const long long c0 = (long long)s.crop_x + L.uL;
    const int r = s.crop_y + L.ys;
    const bool any = L.klo < L.khi, mono = lm_raw_pattern(s.kind) == LM_RAW_MONO;
    const int halo = mono ? 0 : 1, maxv = (1 << bits) - 1, up = 16 - bits;
    long long vlo = c0 + L.klo - halo, vhi = c0 + L.khi + halo;
    vlo = vlo < 0 ? 0 : vlo; vhi = vhi > s.width ? s.width : vhi;
    if (!any) vlo = vhi = 0;
    int C[18];
    raw_row<SB>(s, r, c0, vlo, vhi, maxv, p.black, safe, ld, C);
    if (mono) {
    LMI_UNROLL
        for (int k = 0; k < 16; ++k) P[k] = raw_pipeline(C[k + 1], C[k + 1], C[k + 1], up, p, tone);
        return;
    }
    const int rup = r == 0 ? 1 : r - 1, rdn = r == s.height - 1 ? r - 1 : r + 1;
    int T[18];
    raw_row<SB>(s, rup, c0, vlo, vhi, maxv, p.black, safe, ld, T);
    if (rup != rdn) {
        int B[18];
        raw_row<SB>(s, rdn, c0, vlo, vhi, maxv, p.black, safe, ld, B);
    LMI_UNROLL
        for (int j = 0; j < 18; ++j) T[j] += B[j];
    } else {
    LMI_UNROLL
        for (int j = 0; j < 18; ++j) T[j] += T[j];
    }
    const int kl = (int)-c0, kr = (int)(s.width - 1 - c0);
    const int pat = lm_raw_pattern(s.kind), ph = ((int)(c0 & 1) ^ pat) & 1, dy = (r ^ (pat >> 1)) & 1;
    LMI_UNROLL
    for (int k = 0; k < 16; ++k) {
        const bool first = k == kl, last = k == kr;
        const int cl = first ? C[k + 2] : C[k], cr = last ? C[k] : C[k + 2];
        const int tl = first ? T[k + 2] : T[k], tr = last ? T[k] : T[k + 2];
        int R, G, B;
        raw_channels(C[k + 1], cl + cr, T[k + 1], tl + tr, (k & 1) ^ ph, dy, R, G, B);
        P[k] = raw_pipeline(R, G, B, up, p, tone);
    }
}

// the storage switch: uniform over the image
template <class Load, class Tone>
LMI_FN void raw_lane_pixels(const RawSrc& s, const RawPipe& p, const Lane& L, addr_t safe, Load ld, Tone tone, u32 (&P)[16]) {
    const int st = lm_raw_storage(s.kind), bits = lm_raw_bits(st);
    if (st < LM_RAW_P10) raw_lane_rows<16>(s, p, L, bits, safe, ld, tone, P);
    else if (st == LM_RAW_P10) raw_lane_rows<10>(s, p, L, bits, safe, ld, tone, P);
    else if (st == LM_RAW_P12) raw_lane_rows<12>(s, p, L, bits, safe, ld, tone, P);
    else raw_lane_rows<8>(s, p, L, bits, safe, ld, tone, P);
}

// ---- the rectified route.  Sample (x, y) of the source, inside it, clamped and less the black level: what is read is the sample's own
// bytes -- one byte, one aligned u16, or the two bytes k, k + 1 of a packed sample (k = N x >> 3; N + (N x & 7) > 8: it always has both).
template <class Ld>
LMI_FN int raw_sample(const RawSrc& s, const RawPipe& p, int x, int y, Ld ld) {
    const int st = lm_raw_storage(s.kind), bits = lm_raw_bits(st);
    const addr_t row = s.data + (addr_t)((long long)y * s.row_stride);
    int v;
    if (st == LM_RAW_U8) v = (int)ld.b8(row + (u32)x);
    else if (st < LM_RAW_P10) v = (int)ld.b16(row + 2u * (u32)x);
    else {
        const u32 bit = (u32)bits * (u32)x, k = bit >> 3;
        v = (int)(((ld.b8(row + k) | ld.b8(row + k + 1u) << 8) >> (bit & 7u)) & ((1u << bits) - 1u));
    }
    const int maxv = (1 << bits) - 1;
    v = v < maxv ? v : maxv;
    return v > p.black ? v - p.black : 0;
}

// The four taps (ix .. ix + 1, iy .. iy + 1) of a rectified pixel, each the PROCESSED pixel of the whole source and 0 outside it; the
// conversion comes before the blend.  A Bayer pattern shares the 4 x 4 neighbourhood as lmq::bayer_taps does: a sample is loaded only
// where an inside tap needs it, and then from its reflected place, inside the source.  Mono: the four samples themselves.
template <class Ld, class Tone>
LMI_FN void raw_taps(const RawSrc& s, const RawPipe& p, int ix, int iy, Ld ld, Tone tone, u32 (&t)[4]) {
    const bool cx0 = ix >= 0 && ix < s.width, cx1 = ix + 1 >= 0 && ix + 1 < s.width;
    const bool cy0 = iy >= 0 && iy < s.height, cy1 = iy + 1 >= 0 && iy + 1 < s.height;
    const int pat = lm_raw_pattern(s.kind), up = 16 - lm_raw_bits(lm_raw_storage(s.kind));
    if (pat == LM_RAW_MONO) {
    LMI_UNROLL
        for (int b = 0; b < 2; ++b)
    LMI_UNROLL
            for (int a = 0; a < 2; ++a) {
                t[2 * b + a] = 0u;
                if ((a ? cx1 : cx0) && (b ? cy1 : cy0)) {
                    const int v = raw_sample(s, p, ix + a, iy + b, ld);
                    t[2 * b + a] = raw_pipeline(v, v, v, up, p, tone);
                }
            }
        return;
    }
    const bool needx[4] = {cx0, cx0 || cx1, cx0 || cx1, cx1}, needy[4] = {cy0, cy0 || cy1, cy0 || cy1, cy1};
    int N[4][4];
    LMI_UNROLL
    for (int j = 0; j < 4; ++j)
    LMI_UNROLL
        for (int i = 0; i < 4; ++i) {
            N[j][i] = 0;
            if (needx[i] && needy[j]) N[j][i] = raw_sample(s, p, bayer_reflect(ix - 1 + i, s.width), bayer_reflect(iy - 1 + j, s.height), ld);
        }
    LMI_UNROLL
    for (int b = 0; b < 2; ++b)
    LMI_UNROLL
        for (int a = 0; a < 2; ++a) {
            t[2 * b + a] = 0u;
            if ((a ? cx1 : cx0) && (b ? cy1 : cy0)) {
                int R, G, B;
                raw_channels(N[b + 1][a + 1], N[b + 1][a] + N[b + 1][a + 2], N[b][a + 1] + N[b + 2][a + 1], N[b][a] + N[b][a + 2] + N[b + 2][a] + N[b + 2][a + 2],
                             ((ix + a) ^ pat) & 1, ((iy + b) ^ (pat >> 1)) & 1, R, G, B);
                t[2 * b + a] = raw_pipeline(R, G, B, up, p, tone);
            }
        }
}

}  // namespace lmi
