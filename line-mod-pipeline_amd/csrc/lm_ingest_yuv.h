// lm_ingest_yuv.h -- the index arithmetic of k_ingest / k_ingest_yuv (lm_k_ingest.hip) as functions the host can run too:
// a lane's window (lane_window), the span loader (load_span), the fast-path condition (spans_aligned) and, for the grey and YUV source
// formats, the byte ranges per plane, the byte selectors and the integer conversion (yuv_to_bgr).  The memory read is a parameter
// (ld(address) -> the 16 bytes at a 16-byte aligned address) and the two AMD builtins are emulated off the device, so
// tests/cpp/ingest_yuv_host.cpp drives exactly this code with g++ under ASan / UBSan over sources that end where their allocation
// ends, and checks every load the kernel would issue.  No GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LMI_FN __host__ __device__ __forceinline__
#define LMI_UNROLL _Pragma("unroll")
#else
#define LMI_FN inline
#define LMI_UNROLL
#endif

// how a pixel of a grey / YUV colour source lies in memory (LmIngestImage::kind; the kinds below 5 are lm_kernels.h's)
enum { LM_INGEST_GRAY8 = 5, LM_INGEST_NV12 = 6, LM_INGEST_NV21 = 7, LM_INGEST_YUY2 = 8, LM_INGEST_UYVY = 9 };

namespace lmi {

typedef uint32_t u32;
typedef unsigned long long addr_t;
struct Vec16 { u32 x, y, z, w; };

// bytes s .. s + 3 of the 8 bytes {hi, lo} (v_alignbyte_b32; s = 0 .. 3)
LMI_FN u32 funnel(u32 hi, u32 lo, u32 s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
    return (u32)((((uint64_t)hi << 32) | lo) >> (8u * (s & 3u)));
#endif
}
// v_perm_b32: every selector byte picks 0-3 a byte of lo, 4-7 a byte of hi, 0x0c a zero byte (the only selectors in use)
LMI_FN u32 perm(u32 hi, u32 lo, u32 sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    u32 r = 0;
    for (int i = 0; i < 4; ++i) {
        const u32 s = (sel >> (8 * i)) & 0xFFu;
        if (s < 8u) r |= (u32)((both >> (8u * s)) & 0xFFu) << (8 * i);
        else if (s != 0x0cu) __builtin_trap();
    }
    return r;
#endif
}
// a * b of two values that fit 24 signed bits (v_mul_i32_i24 / v_mad_i32_i24: full rate, where the 32-bit multiply runs at a quarter)
LMI_FN int mul24(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    if (a < -(1 << 23) || a >= (1 << 23) || b < -(1 << 23) || b >= (1 << 23)) __builtin_trap();
    return a * b;
#endif
}

// The NB bytes at address a as NB / 4 dwords, whatever a's alignment.  Only 16-byte ALIGNED loads are issued, and a load reads the
// source only where it holds at least one byte of [vlo, vhi) -- the bytes of the span the caller will keep (inside the window, hence
// inside the source): such a load lies inside the page of a byte that exists, so it cannot fault however the source is aligned and
// wherever it ends.  Every other load is pointed at `safe` (the frame arena: 16-byte aligned memory of the detector's own) and its
// dwords read as zero: the loads stay unconditional, so all of a lane's loads are in flight together (a branch around each would
// put a wait behind each).  aligned (per image, from the descriptor: every span of the image starts on a 16-byte boundary) is the
// fast path, NB / 16 loads straight into D; the general path loads one vector more, rotates by whole dwords ((a >> 2) & 3) and
// funnels by bytes (a & 3).
template <int NB, class Load>
LMI_FN void load_span(addr_t a, addr_t vlo, addr_t vhi, bool aligned, addr_t safe, Load ld, u32 (&D)[NB / 4]) {
    constexpr int ND = NB / 4, NV = NB / 16;
    const bool any = vlo < vhi;         // (an empty range lies nowhere: no load may be placed by it)
    if (aligned) {
    LMI_UNROLL
        for (int v = 0; v < NV; ++v) {
            const addr_t p = a + 16u * v;
            const bool on = any && p < vhi && p + 16u > vlo;
            const Vec16 r = ld(on ? p : safe);
            D[4 * v] = on ? r.x : 0u; D[4 * v + 1] = on ? r.y : 0u; D[4 * v + 2] = on ? r.z : 0u; D[4 * v + 3] = on ? r.w : 0u;
        }
        return;
    }
    u32 R[ND + 4];
    const addr_t base = a & ~(addr_t)15;
    LMI_UNROLL
    for (int v = 0; v <= NV; ++v) {
        const addr_t p = base + 16u * v;
        const bool on = any && p < vhi && p + 16u > vlo;
        const Vec16 r = ld(on ? p : safe);
        R[4 * v] = on ? r.x : 0u; R[4 * v + 1] = on ? r.y : 0u; R[4 * v + 2] = on ? r.z : 0u; R[4 * v + 3] = on ? r.w : 0u;
    }
    // (bit selects, v_bfi_b32: written as `cond ? R[i + 2] : R[i]` the compiler indexes R dynamically and moves it to scratch memory)
    const u32 by2 = (a & 8u) ? ~0u : 0u, by1 = (a & 4u) ? ~0u : 0u;
    LMI_UNROLL
    for (int i = 0; i <= ND + 1; ++i) R[i] = (R[i + 2] & by2) | (R[i] & ~by2);
    LMI_UNROLL
    for (int i = 0; i <= ND; ++i) R[i] = (R[i + 1] & by1) | (R[i] & ~by1);
    const u32 s = (u32)a & 3u;
    LMI_UNROLL
    for (int i = 0; i < ND; ++i) D[i] = funnel(R[i + 1], R[i], s);
}

// The 16 output pixels x0 .. x0 + 15 of output row y: they come from source row crop_y + ys and from the 16 consecutive window
// columns uL .. uL + 15 (ascending, or descending when mirrored); the lane keeps source pixel k of that span for k in [klo, khi).
struct Lane { int ys, uL, klo, khi; };
LMI_FN Lane lane_window(int w, int h, int x0, int y, bool flip, int shift_x, int shift_y) {
    Lane L;
    L.ys = y - shift_y;
    L.uL = flip ? w - 16 - x0 + shift_x : x0 - shift_x;
    const int lo = -L.uL, hi = w - L.uL;
    L.klo = lo > 0 ? lo : 0; L.khi = hi < 16 ? hi : 16;
    if (L.ys < 0 || L.ys >= h || L.khi < L.klo) L.khi = L.klo = 0;
    return L;
}

// The fast-path condition of one image: every span of every plane starts on a 16-byte boundary.  A lane's first source column is
// col0 + 16 n (col0 = crop_x - shift_x, or crop_x + W - 16 + shift_x when mirrored) and 16 pixels are a multiple of 16 bytes in
// every format, so the spans of a plane with `bpp` bytes per pixel start at data (+ planes) + row * row_stride + (col0 + 16 n) * bpp.
// NV12 / NV21: bpp 1 -- the chroma span of an EVEN first column c0 starts at byte 2 * (c0 >> 1) = c0 of its row, behind plane_stride.
// YUY2 / UYVY: bpp 2 -- the macropixel span of an even c0 starts at byte 4 * (c0 >> 1) = 2 c0.
LMI_FN bool spans_aligned(addr_t data, long long row_stride, long long plane_stride, long long col0, int bpp) {
    return data % 16 == 0 && row_stride % 16 == 0 && plane_stride % 16 == 0 && ((col0 * bpp) % 16 + 16) % 16 == 0;
}

// ---- YUV -> BGR, an exact integer rule (include/linemod_hip.h): 32-bit signed integers, >> an arithmetic shift
//     y = max(0, Y - Y0) * CY;  u = U - 128;  v = V - 128
//     R = sat8((y + (1 << 19) + CVR v) >> 20);  G = sat8((y + (1 << 19) + CVG v + CUG u) >> 20);  B = sat8((y + (1 << 19) + CUB u) >> 20)
struct YuvCoef { int y0, cy, cvr, cvg, cug, cub; };
// row = LM_PIX_YUV_BT709 >> 8 | LM_PIX_YUV_FULL >> 8: 0 BT.601 limited (OpenCV's ITUR_BT_601_* constants), 1 BT.709 limited, 2 BT.601 full,
// 3 BT.709 full (rows 1 - 3: round(coefficient * 2^20) of the standard matrices).  Selects, not a table in memory: `row` is uniform.
LMI_FN YuvCoef yuv_coef(int row) {
    YuvCoef c;
    c.y0  = row < 2 ? 16 : 0;
    c.cy  = row == 0 ? 1220542 : row == 1 ? 1220945 : 1048576;
    c.cvr = row == 0 ? 1673527 : row == 1 ? 1879825 : row == 2 ? 1470104 : 1651297;
    c.cvg = row == 0 ? -852492 : row == 1 ? -558796 : row == 2 ? -748826 : -490864;
    c.cug = row == 0 ? -409993 : row == 1 ? -223607 : row == 2 ? -360853 : -196424;
    c.cub = row == 0 ? 2116026 : row == 1 ? 2215014 : row == 2 ? 1858077 : 1945738;
    return c;
}
LMI_FN int sat8(int x) { return x < 0 ? 0 : x > 255 ? 255 : x; }
// what a chroma pair adds to the three channels, the rounding term included: once per pair, shared by the pixels it covers
struct Chroma { int r, g, b; };
LMI_FN Chroma chroma_terms(int U, int V, const YuvCoef& c) {
    const int u = U - 128, v = V - 128;
    Chroma t;
    t.r = mul24(c.cvr, v) + (1 << 19);
    t.g = mul24(c.cvg, v) + mul24(c.cug, u) + (1 << 19);
    t.b = mul24(c.cub, u) + (1 << 19);
    return t;
}
// the pixel as k_ingest keeps it: B | G << 8 | R << 16
LMI_FN u32 luma_pixel(int Y, const Chroma& t, const YuvCoef& c) {
    const int d = Y - c.y0, y = mul24(d > 0 ? d : 0, c.cy);
    return (u32)sat8((y + t.b) >> 20) | (u32)sat8((y + t.g) >> 20) << 8 | (u32)sat8((y + t.r) >> 20) << 16;
}
LMI_FN u32 yuv_to_bgr(int Y, int U, int V, const YuvCoef& c) { return luma_pixel(Y, chroma_terms(U, V, c), c); }

// ---- the grey and YUV sources of one lane.  Source pixel k of the lane is column c0 + k of source row r, c0 = crop_x + uL (negative
// where the shift reaches beyond the window: those k are not kept).  Chroma is replicated: pixel k takes the chroma pair
// ((c0 + k) >> 1) - (c0 >> 1) = (k + odd) >> 1 of the lane's chroma span, odd = c0 & 1 -- 8 pairs when c0 is even and 9 when it is odd.
// The pairs that cover the kept pixels [klo, khi) are pairs (klo + odd) >> 1 .. (khi - 1 + odd) >> 1: their bytes are the [vlo, vhi) of
// the chroma span, inside the source because the source's width (and, 4:2:0, its height) is even.
struct Src {
    addr_t data;
    long long row_stride, plane_stride;
    int crop_x, crop_y, kind, matrix;
    bool aligned;
};

// Y[k] and the pair terms T[j] -> P[k] = B | G << 8 | R << 16.  Pixel k takes pair (k + odd) >> 1: k / 2 for even k; for odd k the
// pair behind or in front, a select between two registers (never a dynamic index).
LMI_FN void convert16(const int (&Y)[16], const Chroma (&T)[9], bool odd, const YuvCoef& c, u32 (&P)[16]) {
    LMI_UNROLL
    for (int k = 0; k < 16; k += 2) {
        P[k] = luma_pixel(Y[k], T[k / 2], c);
        Chroma t;
        t.r = odd ? T[k / 2 + 1].r : T[k / 2].r; t.g = odd ? T[k / 2 + 1].g : T[k / 2].g; t.b = odd ? T[k / 2 + 1].b : T[k / 2].b;
        P[k + 1] = luma_pixel(Y[k + 1], t, c);
    }
}

// LM_INGEST_GRAY8: one span of 16 bytes, B = G = R = the byte
template <class Load>
LMI_FN void gray_pixels(const Src& s, const Lane& L, addr_t safe, Load ld, u32 (&P)[16]) {
    const long long c0 = (long long)s.crop_x + L.uL, r = (long long)s.crop_y + L.ys;
    const addr_t p = s.data + (addr_t)(r * s.row_stride + c0);
    u32 D[4];
    load_span<16>(p, p + L.klo, p + L.khi, s.aligned, safe, ld, D);
    LMI_UNROLL
    for (int k = 0; k < 16; ++k) P[k] = perm(0u, D[k / 4], 0x0c000000u | 0x010101u * (u32)(k & 3));
}

// LM_INGEST_NV12 / NV21: 16 bytes of the Y plane, and 16 (c0 even) or 18 (odd) bytes of chroma row r >> 1, which starts plane_stride
// behind the Y plane and has the Y plane's row stride: byte 2 * (c >> 1) of it is U (NV21: V) of column c, the next byte the other.
template <class Load>
LMI_FN void nv_pixels(const Src& s, const Lane& L, addr_t safe, Load ld, u32 (&P)[16]) {
    const long long c0 = (long long)s.crop_x + L.uL, r = (long long)s.crop_y + L.ys;
    const int odd = (int)(c0 & 1);
    const addr_t py = s.data + (addr_t)(r * s.row_stride + c0);
    const addr_t pc = s.data + (addr_t)(s.plane_stride + (r >> 1) * s.row_stride + (c0 - odd));
    const bool any = L.klo < L.khi;
    const addr_t clo = pc + (any ? 2u * (u32)((L.klo + odd) >> 1) : 0u), chi = pc + (any ? 2u * (u32)((L.khi - 1 + odd) >> 1) + 2u : 0u);
    u32 D[4], Cd[8];
    load_span<16>(py, py + L.klo, py + L.khi, s.aligned, safe, ld, D);
    load_span<32>(pc, clo, chi, s.aligned, safe, ld, Cd);
    const YuvCoef c = yuv_coef(s.matrix);
    const u32 sel = s.kind == LM_INGEST_NV21 ? 0x02030001u : 0x03020100u;     // (U, V) of both pairs of a dword
    Chroma T[9];
    LMI_UNROLL
    for (int j = 0; j < 9; ++j) {
        const u32 uv = perm(0u, Cd[j / 2], sel) >> (16 * (j & 1));
        T[j] = chroma_terms((int)(uv & 0xFFu), (int)((uv >> 8) & 0xFFu), c);
    }
    int Y[16];
    LMI_UNROLL
    for (int k = 0; k < 16; ++k) Y[k] = (int)((D[k / 4] >> (8 * (k & 3))) & 0xFFu);
    convert16(Y, T, odd != 0, c, P);
}

// LM_INGEST_YUY2 / UYVY: 4 bytes per pair of columns, Y0 U Y1 V or U Y0 V Y1, at byte 4 * (c >> 1) of the row: 32 (c0 even) or 36 (odd)
// bytes.  Column c takes Y0 when it is even and Y1 when it is odd.
template <class Load>
LMI_FN void yuv422_pixels(const Src& s, const Lane& L, addr_t safe, Load ld, u32 (&P)[16]) {
    const long long c0 = (long long)s.crop_x + L.uL, r = (long long)s.crop_y + L.ys;
    const int odd = (int)(c0 & 1);
    const addr_t pm = s.data + (addr_t)(r * s.row_stride + 2 * (c0 - odd));
    const bool any = L.klo < L.khi;
    const addr_t mlo = pm + (any ? 4u * (u32)((L.klo + odd) >> 1) : 0u), mhi = pm + (any ? 4u * (u32)((L.khi - 1 + odd) >> 1) + 4u : 0u);
    u32 M[12];
    load_span<48>(pm, mlo, mhi, s.aligned, safe, ld, M);
    const YuvCoef c = yuv_coef(s.matrix);
    const u32 sel = s.kind == LM_INGEST_UYVY ? 0x02000301u : 0x03010200u;     // -> Y0 Y1 U V
    Chroma T[9];
    LMI_UNROLL
    for (int j = 0; j < 9; ++j) {
        M[j] = perm(0u, M[j], sel);
        T[j] = chroma_terms((int)((M[j] >> 16) & 0xFFu), (int)(M[j] >> 24), c);
    }
    int Y[16];
    LMI_UNROLL
    for (int k = 0; k < 16; k += 2) {       // column c0 + k is the first of its pair unless c0 is odd, column c0 + k + 1 the other way round
        Y[k] = (int)(odd ? (M[k / 2] >> 8) & 0xFFu : M[k / 2] & 0xFFu);
        Y[k + 1] = (int)(odd ? M[k / 2 + 1] & 0xFFu : (M[k / 2] >> 8) & 0xFFu);
    }
    convert16(Y, T, odd != 0, c, P);
}

// the (B, G, R, 0) registers of a lane's 16 source pixels, for the kinds of this header
template <class Load>
LMI_FN void yuv_lane_pixels(const Src& s, const Lane& L, addr_t safe, Load ld, u32 (&P)[16]) {
    if (s.kind == LM_INGEST_GRAY8) gray_pixels(s, L, safe, ld, P);
    else if (s.kind == LM_INGEST_NV12 || s.kind == LM_INGEST_NV21) nv_pixels(s, L, safe, ld, P);
    else yuv422_pixels(s, L, safe, ld, P);
}

}  // namespace lmi
