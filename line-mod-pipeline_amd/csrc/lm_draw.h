// lm_draw.h -- the rule of lm_export_frames (include/linemod_hip.h) as functions the host can run too: a primitive's
// record with its constants (make_rec), coverage per kind (covered), the blend, the un-shift / un-mirror index (frame_x, frame_y), the
// forward YUV conversion and its coefficient selects.  k_export (lm_k_export.hip), the planner (lmh::plan_export) and
// tests/cpp/export_host.cpp run exactly this code: everything is integer arithmetic, 32-bit wherever the bounds below allow it.
// Bounds (checked by lmc::check_export_prim): coordinates in [-8192, 8191], a frame of at most 8192 x 8192, thickness 1 .. 64.  A pixel
// and a primitive's point are then at most 16383 apart per axis: a squared distance is at most 2 * 16383^2 = 536805378, four times it
// 2147221512 < 2^31; a dot or cross product of two such vectors at most 536805378; only 4 cross^2 (< 2^61) needs 64 bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LMW_FN __host__ __device__ __forceinline__
#else
#define LMW_FN inline
#endif

namespace lmw {

typedef uint32_t u32;

enum { RING = 0, SEGMENT = 1, BOX = 2 };      // LM_DRAW_RING, LM_DRAW_SEGMENT, LM_DRAW_BOX
enum { COORD_MIN = -8192, COORD_MAX = 8191, FRAME_MAX = 8192, THICK_MAX = 64 };
// a workgroup's tile of the exported image (k_export: 256 lanes of 4 x 2 pixels; lmh::plan_export bins by it).  Even: an NV12 chroma block
// lies in one tile, and in one lane.
enum { TILE_W = 64, TILE_H = 32 };

// One primitive as the kernel reads it, 64 bytes: the caller's numbers, the per-kind constants and the conservative bounding box the
// planner bins by (the primitive's own box inflated by its thickness, in frame coordinates, NOT clipped).
//   RING     a = (2 r + t)^2, b = (2 r - t)^2 or 0 for a disc (every q >= 0)
//   SEGMENT  a, b = d = B - A;  c = L2 = |d|^2;  d = t^2;  k64 = t^2 L2
//   BOX      a, b = x0 + t, x1 - t;  c, d = y0 + t, y1 - t   (the inner rectangle; empty when a > b or c > d)
struct Rec {
    int kind, x0, y0, x1, y1;
    u32 colour;             // b | g << 8 | r << 16 | a << 24
    int a, b, c, d;
    long long k64;
    int bx0, by0, bx1, by1;
};
static_assert(sizeof(Rec) == 64, "a record is four 16-byte vectors");

LMW_FN Rec make_rec(int kind, int x0, int y0, int x1, int y1, int t, u32 colour) {
    Rec r;
    r.kind = kind; r.x0 = x0; r.y0 = y0; r.x1 = x1; r.y1 = y1; r.colour = colour;
    r.a = r.b = r.c = r.d = 0; r.k64 = 0;
    if (kind == RING) {
        const int rad = x1;
        r.a = (2 * rad + t) * (2 * rad + t);
        r.b = 2 * rad >= t ? (2 * rad - t) * (2 * rad - t) : 0;
        r.bx0 = x0 - rad - t; r.bx1 = x0 + rad + t; r.by0 = y0 - rad - t; r.by1 = y0 + rad + t;
    } else if (kind == SEGMENT) {
        r.a = x1 - x0; r.b = y1 - y0;
        r.c = r.a * r.a + r.b * r.b;
        r.d = t * t;
        r.k64 = (long long)r.d * (long long)r.c;
        r.bx0 = (x0 < x1 ? x0 : x1) - t; r.bx1 = (x0 < x1 ? x1 : x0) + t;
        r.by0 = (y0 < y1 ? y0 : y1) - t; r.by1 = (y0 < y1 ? y1 : y0) + t;
    } else {
        r.a = x0 + t; r.b = x1 - t; r.c = y0 + t; r.d = y1 - t;
        r.bx0 = x0 - t; r.bx1 = x1 + t; r.by0 = y0 - t; r.by1 = y1 + t;
    }
    return r;
}

// 4 |v|^2 of a vector between a pixel and a primitive's point
LMW_FN u32 q4(int dx, int dy) { return 4u * (u32)(dx * dx + dy * dy); }

LMW_FN bool ring_covered(const Rec& r, int x, int y) {
    const u32 q = q4(x - r.x0, y - r.y0);
    return q < (u32)r.a && q >= (u32)r.b;
}

// the pixel centre's distance to the segment is at most t / 2, round caps
LMW_FN bool segment_covered(const Rec& r, int x, int y) {
    const int wx = x - r.x0, wy = y - r.y0;
    const int s = wx * r.a + wy * r.b;
    if (r.c == 0 || s <= 0) return q4(wx, wy) <= (u32)r.d;
    if (s >= r.c) return q4(x - r.x1, y - r.y1) <= (u32)r.d;
    const long long cross = (long long)(wx * r.b - wy * r.a);
    return 4 * cross * cross <= r.k64;
}

LMW_FN bool box_covered(const Rec& r, int x, int y) {
    const bool outer = x >= r.x0 && x <= r.x1 && y >= r.y0 && y <= r.y1;
    const bool inner = x >= r.a && x <= r.b && y >= r.c && y <= r.d;
    return outer && !inner;
}

LMW_FN bool covered(const Rec& r, int x, int y) {
    return r.kind == RING ? ring_covered(r, x, y) : r.kind == SEGMENT ? segment_covered(r, x, y) : box_covered(r, x, y);
}

// round(c (255 - a) / 255 + p a / 255), exactly (all 2^24 triples): a = 255 gives p, a = 0 gives c
LMW_FN u32 blend(u32 c, u32 p, u32 a) {
    const u32 t = c * (255u - a) + p * a + 128u;
    return (t + (t >> 8)) >> 8;
}
// the pixel B | G << 8 | R << 16 under the record's colour
LMW_FN u32 blend_pixel(u32 px, u32 colour) {
    const u32 a = colour >> 24;
    return blend(px & 0xFFu, colour & 0xFFu, a) | blend((px >> 8) & 0xFFu, (colour >> 8) & 0xFFu, a) << 8 |
           blend((px >> 16) & 0xFFu, (colour >> 16) & 0xFFu, a) << 16;
}

// The ingest's options undone: window pixel (u, v) of the exported image shows frame pixel (frame_x(u), frame_y(v)), (0, 0, 0) where
// that lies outside the frame.  dest_x / dest_y are the inverses (the planner maps a primitive's box into the exported image with them).
LMW_FN int frame_x(int u, int w, int flip, int shift_x) { return (flip ? w - 1 - u : u) + shift_x; }
LMW_FN int frame_y(int v, int shift_y) { return v + shift_y; }
LMW_FN int dest_x(int x, int w, int flip, int shift_x) { return flip ? w - 1 - (x - shift_x) : x - shift_x; }
LMW_FN int dest_y(int y, int shift_y) { return y - shift_y; }

// ---- BGR -> YUV, the forward conversion of an NV12 destination: round(coefficient * 2^16) of the standard matrices, 32-bit signed
// integers, >> an arithmetic shift.  Luma per pixel; chroma per 2 x 2 block from the SUMS of its four pixels (at most 1020 per channel:
// |32768 * 1020 * 2| + (128 << 18) + (1 << 17) < 2^31).
struct FwdCoef { int y0, cyr, cyg, cyb, cur, cug, cub, cvr, cvg, cvb; };
// row = LM_PIX_YUV_BT709 >> 8 | LM_PIX_YUV_FULL >> 8, as lmi::yuv_coef.  Selects, not a table in memory: `row` is uniform.
LMW_FN FwdCoef fwd_coef(int row) {
    FwdCoef c;
    c.y0  = row < 2 ? 16 : 0;
    c.cyr = row == 0 ? 16829 : row == 1 ? 11966 : row == 2 ? 19595 : 13933;
    c.cyg = row == 0 ? 33039 : row == 1 ? 40254 : row == 2 ? 38470 : 46871;
    c.cyb = row == 0 ? 6416 : row == 1 ? 4064 : row == 2 ? 7471 : 4732;
    c.cur = row == 0 ? -9714 : row == 1 ? -6596 : row == 2 ? -11058 : -7509;
    c.cug = row == 0 ? -19071 : row == 1 ? -22189 : row == 2 ? -21710 : -25259;
    c.cub = row < 2 ? 28784 : 32768;
    c.cvr = row < 2 ? 28784 : 32768;
    c.cvg = row == 0 ? -24103 : row == 1 ? -26145 : row == 2 ? -27439 : -29763;
    c.cvb = row == 0 ? -4681 : row == 1 ? -2639 : row == 2 ? -5329 : -3005;
    return c;
}
LMW_FN int sat8(int x) { return x < 0 ? 0 : x > 255 ? 255 : x; }
LMW_FN int luma(int R, int G, int B, const FwdCoef& c) { return sat8((c.cyr * R + c.cyg * G + c.cyb * B + (c.y0 << 16) + 32768) >> 16); }
LMW_FN int chroma_u(int sR, int sG, int sB, const FwdCoef& c) { return sat8((c.cur * sR + c.cug * sG + c.cub * sB + (128 << 18) + (1 << 17)) >> 18); }
LMW_FN int chroma_v(int sR, int sG, int sB, const FwdCoef& c) { return sat8((c.cvr * sR + c.cvg * sG + c.cvb * sB + (128 << 18) + (1 << 17)) >> 18); }

}  // namespace lmw
