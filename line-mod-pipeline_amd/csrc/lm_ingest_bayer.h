// lm_ingest_bayer.h -- the raw Bayer colour sources of k_ingest_bayer / k_rectify_bayer (lm_k_ingest.hip, lm_k_rectify.hip, DESIGN.md
// section 13 "Bayer sources"; the rule is written out in include/linemod_hip.h) as functions the host can run too, in the manner of
// lm_ingest_yuv.h: the site classification, the five averages of the bilinear demosaic and bayer_lane_pixels, which turns a lane's three
// reflected source rows into its 16 (B | G << 8 | R << 16) registers.  The memory read is a parameter and lm_ingest_yuv.h's lane_window
// and load_span are used as they are, so tests/cpp/ingest_bayer_host.cpp drives exactly this code with g++ under ASan / UBSan over
// sources that end where their allocation ends, and checks every load the kernel would issue.  No GPU.
#pragma once
#include <stdint.h>

#include "lm_ingest_yuv.h"

// LmIngestImage::kind of a Bayer colour source: kind - LM_INGEST_BAYER_RGGB = red_x | red_y << 1, the red sample's place in the 2 x 2 tile
enum { LM_INGEST_BAYER_RGGB = 10, LM_INGEST_BAYER_GRBG = 11, LM_INGEST_BAYER_GBRG = 12, LM_INGEST_BAYER_BGGR = 13 };

// the first kind of a high-bit raw source or of an 8-bit Bayer source under a raw pipeline: lm_ingest_raw.h's, every kind from here on
enum { LM_INGEST_RAW = 14 };

// the first kind of a float colour source: lm_ingest_float.h's, every kind from here on (the raw kinds end at 14 + 6 * 8 + 4)
enum { LM_INGEST_FLOAT = 128 };

// whose frame is this: k_ingest's / k_rectify's (RGB in some order), k_ingest_yuv's (grey, YUV), k_ingest_bayer's, k_ingest_raw's or
// k_ingest_float's -- the kernels' "not mine" test and the host's counters
enum { LM_INGEST_FAMILY_RGB = 0, LM_INGEST_FAMILY_YUV = 1, LM_INGEST_FAMILY_BAYER = 2, LM_INGEST_FAMILY_RAW = 3, LM_INGEST_FAMILY_FLOAT = 4,
       LM_INGEST_FAMILIES = 5 };
LMI_FN int lm_ingest_family(int colour_kind) {
    return colour_kind >= LM_INGEST_FLOAT ? LM_INGEST_FAMILY_FLOAT : colour_kind >= LM_INGEST_RAW ? LM_INGEST_FAMILY_RAW
         : colour_kind >= LM_INGEST_BAYER_RGGB ? LM_INGEST_FAMILY_BAYER : colour_kind >= LM_INGEST_GRAY8 ? LM_INGEST_FAMILY_YUV : LM_INGEST_FAMILY_RGB;
}

namespace lmi {

// coordinate i of a side of n >= 2 samples, reflected without repeating the edge: -1 -> 1, n -> n - 2 (an even distance: the colour
// of the site is kept).  Only i in [-1, n] is ever asked for.
LMI_FN int bayer_reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

// site of pixel (x, y): dx = 0 in a red column, dy = 0 in a red row
LMI_FN int bayer_dx(int kind, int x) { return (x ^ (kind - LM_INGEST_BAYER_RGGB)) & 1; }
LMI_FN int bayer_dy(int kind, int y) { return (y ^ ((kind - LM_INGEST_BAYER_RGGB) >> 1)) & 1; }

// The pixel of a site from its sample c and the SUMS of its neighbours: hs = left + right, vs = above + below, ds = the four diagonals.
//     h = (hs + 1) >> 1   v = (vs + 1) >> 1   p = (hs + vs + 2) >> 2   d = (ds + 2) >> 2
//     red site (0, 0): R = c, G = p, B = d        blue site (1, 1): B = c, G = p, R = d
//     green in a red row (1, 0): G = c, R = h, B = v        green in a blue row (0, 1): G = c, B = h, R = v
// -> a green site keeps c and takes (h, v), the others take p and (c, d); the row decides which of the pair is red.
LMI_FN u32 bayer_pixel(int c, int hs, int vs, int ds, int dx, int dy) {
    const bool green = dx != dy;
    const int a1 = green ? (hs + 1) >> 1 : c, a2 = green ? (vs + 1) >> 1 : (ds + 2) >> 2;
    const int g = green ? c : (hs + vs + 2) >> 2;
    const int r = dy ? a2 : a1, b = dy ? a1 : a2;
    return (u32)b | (u32)g << 8 | (u32)r << 16;
}

struct BayerSrc {
    addr_t data;
    long long row_stride;
    int width, height;          // of the SOURCE: its edges reflect, the window's do not
    int crop_x, crop_y, kind;
    bool aligned;               // spans_aligned with one byte per pixel: a lane's first column lies on a 16-byte boundary
};

// Bytes c0 - 1 .. c0 + 16 of source row `row` as V[0 .. 17] (column c0 + k is V[k + 1]); [vlo, vhi): the columns of the row the lane needs.
// Fast path: three aligned vectors from c0 - 16, of which the outer two hold one needed byte each (the neighbouring lanes' vectors: cache
// hits); general path: load_span's three vectors from c0 - 1.
template <class Load>
LMI_FN void bayer_row(const BayerSrc& s, long long row, long long c0, long long vlo, long long vhi, addr_t safe, Load ld, int (&V)[18]) {
    const addr_t base = s.data + (addr_t)(row * s.row_stride), p = base + (addr_t)c0;
    u32 E[5];
    if (s.aligned) {
        u32 D[12];
        load_span<48>(p - 16u, base + (addr_t)vlo, base + (addr_t)vhi, true, safe, ld, D);
    LMI_UNROLL
        for (int i = 0; i < 5; ++i) E[i] = funnel(D[4 + i], D[3 + i], 3);
    } else {
        u32 D[8];
        load_span<32>(p - 1u, base + (addr_t)vlo, base + (addr_t)vhi, false, safe, ld, D);
    LMI_UNROLL
        for (int i = 0; i < 5; ++i) E[i] = D[i];
    }
    LMI_UNROLL
    for (int j = 0; j < 18; ++j) V[j] = (int)((E[j / 4] >> (8 * (j & 3))) & 0xFFu);
}

// The 16 source pixels of a lane, demosaiced: pixel k is column c0 + k of source row r (c0 = crop_x + uL, r = crop_y + ys).  It needs
// columns c0 - 1 .. c0 + 16 of rows r - 1, r, r + 1.  Rows reflect by the choice of the row address: at r = 0 and r = h - 1 the rows above
// and below are the same row, which is loaded once.  Columns reflect by a select between registers: column -1 is column 1, the right
// neighbour of the pixel that misses it, and column w is column w - 2.  The range handed to load_span is the kept columns +- 1 clipped to
// the source: every load that is issued holds a byte of it, and the reflected columns 1 and w - 2 lie inside it (w >= 2).
template <class Load>
LMI_FN void bayer_lane_pixels(const BayerSrc& s, const Lane& L, addr_t safe, Load ld, u32 (&P)[16]) {
    const long long c0 = (long long)s.crop_x + L.uL;
    const int r = s.crop_y + L.ys;
    const bool any = L.klo < L.khi;
    long long vlo = c0 + L.klo - 1, vhi = c0 + L.khi + 1;
    vlo = vlo < 0 ? 0 : vlo; vhi = vhi > s.width ? s.width : vhi;
    if (!any) vlo = vhi = 0;
    const int up = r == 0 ? 1 : r - 1, dn = r == s.height - 1 ? r - 1 : r + 1;
    int C[18], T[18];
    bayer_row(s, r, c0, vlo, vhi, safe, ld, C);
    bayer_row(s, up, c0, vlo, vhi, safe, ld, T);
    if (up != dn) {
        int B[18];
        bayer_row(s, dn, c0, vlo, vhi, safe, ld, B);
    LMI_UNROLL
        for (int j = 0; j < 18; ++j) T[j] += B[j];
    } else {
    LMI_UNROLL
        for (int j = 0; j < 18; ++j) T[j] += T[j];
    }
    // pixel k's left neighbour is index k, its right neighbour index k + 2: the pixel in column 0 takes its right one for the left, the
    // pixel in column w - 1 its left one for the right
    const int kl = (int)-c0, kr = (int)(s.width - 1 - c0);
    const int ph = bayer_dx(s.kind, (int)(c0 & 1)), dy = bayer_dy(s.kind, r);
    LMI_UNROLL
    for (int k = 0; k < 16; ++k) {
        const bool first = k == kl, last = k == kr;
        const int cl = first ? C[k + 2] : C[k], cr = last ? C[k] : C[k + 2];
        const int tl = first ? T[k + 2] : T[k], tr = last ? T[k] : T[k + 2];
        P[k] = bayer_pixel(C[k + 1], cl + cr, T[k + 1], tl + tr, (k & 1) ^ ph, dy);
    }
}

}  // namespace lmi
