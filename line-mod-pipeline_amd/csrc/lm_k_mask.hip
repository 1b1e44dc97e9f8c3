// lm_k_mask.hip -- Detector::match's per-modality masks: the quantised images of the masked slots of a
// call ANDed with their masks, between the last quantiser and the linear memories (lm_detector.hip enqueue_preprocess).
//   colour: quant[l][0] &= mask_l at every level l, mask_l = the level-0 mask resized with INTER_NEAREST l times = mask0[y << l][x << l]
//   depth:  quant[0][1] &= mask_0 only: every depth level above reads quant[0][1] at (2y, 2x) (the linear memories of level 1,
//           k_nn_half for the levels above), the same NN rule as the mask's, so the one masking is exact at every level.
// A byte-wise, memory-bound pass: each lane ANDs 16 quantised bytes with 16 mask bytes (dwordx4 loads and stores).  The level-1 mask
// bytes are the even bytes of two dwordx4 loads of row 2y, gathered with v_perm_b32.
//
// k_mask_rule (below) computes such a level-0 mask on the device from the slot's resident frame: the sticky mask rules of
// lm_set_mask_rule.
#include "lm_dev.h"
#include "lm_kernels.h"

namespace {

// OpenCV copyTo semantics: a nonzero mask byte keeps the pixel.  Per byte 0xFF where v's byte is nonzero, 0x00 where it is zero.
__device__ __forceinline__ u32 keep_bytes(u32 v) {
    const u32 t = (v | ((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u;   // bit 7 of a byte: the byte is nonzero (no carry leaves a byte)
    return t | (t - (t >> 7));                                           // 0x80 -> 0xFF, 0x00 -> 0x00
}

// Bytes 0 and 2 of lo, then bytes 0 and 2 of hi (v_perm_b32: selector 0-3 picks a byte of the second operand, 4-7 of the first).
__device__ __forceinline__ u32 even_bytes(u32 lo, u32 hi) { return __builtin_amdgcn_perm(hi, lo, 0x06040200u); }

}  // namespace

// One launch over up to LM_MASK_SLOTS masked slots: blockIdx.y = entry of the table, blockIdx.x * 256 + threadIdx.x = a 16-byte vector of the
// entry's planes, the colour levels (0 .. L-1) first, then depth level 0.  An entry without a colour (depth) mask skips those planes.
// Rows of 16-byte multiples (a.vec_rows): a vector lies inside one row; other widths take the per-byte form below.
// (Outside the anonymous namespace: rocprofv3 lists it as k_match_mask.)
__global__ __launch_bounds__(256) void k_match_mask(LmMaskArgs a) {
    const u32 e = blockIdx.y;
    const u8* cm = a.cmask[e];
    const u8* dm = a.dmask[e];
    u32 v = blockIdx.x * 256u + threadIdx.x;
    const u32 cvec = cm ? a.vec_begin[a.levels] : 0u;
    if (v >= cvec + (dm ? a.vec_depth : 0u)) return;
    u8* slot = a.frame + (size_t)a.slot[e] * a.slot_stride;
    int l = 0, m = 0;
    const u8* mask = cm;
    if (v >= cvec) { v -= cvec; m = 1; mask = dm; }
    else while (l + 1 < a.levels && v >= a.vec_begin[l + 1]) ++l;
    if (m == 0) v -= a.vec_begin[l];
    const u32 w = a.w[l];
    u8* q = slot + a.off_quant[l][m] + (size_t)v * 16u;
    uint4 qv = *reinterpret_cast<const uint4*>(q);
    u32 mw[4];
    if (a.vec_rows) {
        const u32 vpr = w >> 4;
        const u32 y = v / vpr, x = (v - y * vpr) * 16u;
        const u8* row = mask + (size_t)(y << l) * a.mask_pitch;
        if (l == 0) {
            const uint4 mv = *reinterpret_cast<const uint4*>(row + x);
            mw[0] = mv.x; mw[1] = mv.y; mw[2] = mv.z; mw[3] = mv.w;
        } else if (l == 1) {
            const uint4 m0 = *reinterpret_cast<const uint4*>(row + 2 * x);
            const uint4 m1 = *reinterpret_cast<const uint4*>(row + 2 * x + 16);
            mw[0] = even_bytes(m0.x, m0.y); mw[1] = even_bytes(m0.z, m0.w);
            mw[2] = even_bytes(m1.x, m1.y); mw[3] = even_bytes(m1.z, m1.w);
        } else {
            // (levels 2+ of deeper pyramids: column (x + k) << l is a multiple of 4, the wanted byte is the low byte of its dword)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                u32 r = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    r |= (*reinterpret_cast<const u32*>(row + ((size_t)(x + 4 * k + b) << l)) & 0xFFu) << (8 * b);
                mw[k] = r;
            }
        }
    } else {
        // rows that are not 16-byte multiples (other frame widths): each byte finds its own row and column
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            u32 r = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const u32 i = v * 16u + 4u * k + b, y = i / w, x = i - y * w;
                r |= (u32)mask[(size_t)(y << l) * a.mask_pitch + ((size_t)x << l)] << (8 * b);
            }
            mw[k] = r;
        }
    }
    qv.x &= keep_bytes(mw[0]); qv.y &= keep_bytes(mw[1]); qv.z &= keep_bytes(mw[2]); qv.w &= keep_bytes(mw[3]);
    *reinterpret_cast<uint4*>(q) = qv;
}

void lmk_match_mask(hipStream_t s, const LmMaskArgs& a) {
    u32 most = 0;
    for (int e = 0; e < a.n; ++e) {
        const u32 nv = (a.cmask[e] ? a.vec_begin[a.levels] : 0u) + (a.dmask[e] ? a.vec_depth : 0u);
        most = nv > most ? nv : most;
    }
    if (!most) return;
    hipLaunchKernelGGL(k_match_mask, dim3((most + 255) / 256, (unsigned)a.n), dim3(256), 0, s, a);
}

// ---- mask rules -------------------------------------------------------------------------------------------------------------------
namespace {

// bit k of b (k < 4) -> byte k = 0xFF / 0x00 (the products' bits i + {0, 7, 14, 21} are all different: no carries)
__device__ __forceinline__ u32 expand4(u32 b) { return ((b * 0x00204081u) & 0x01010101u) * 0xFFu; }

}  // namespace

// One launch over the ruled slots of a call: blockIdx.y = entry of the table, blockIdx.x = a strip of a.rows_out rows over the frame's
// whole width.  A row of the mask is ceil(w / 64) 64-bit words in LDS, bit x % 64 of word x / 64 = pixel x; pixels outside the image are 0
// bits and rows outside the image 0 words, which IS the clipped window of the dilation.
//   1  seed: a lane gates 8 consecutive pixels (one 16-byte depth load and three 8-byte colour loads where the rows allow it, a.vec) and
//      writes their byte of the row's words, for the strip's rows and the `grow` rows above and below it
//   2  a thread per (row, word): the OR of the 2 grow + 1 rows of the word and of its two neighbours, then the horizontal dilation of the
//      middle word as ORs of shifted words in doubling steps (the neighbours carry the bits that cross a word border), then the rectangle
//   3  a thread per 16 pixels: its 16 bits expanded to 0 / 255 bytes, one dwordx4 store into the slot's rule plane
// No scratch, no atomics: a pure function of the frame.
__global__ __launch_bounds__(256) void k_mask_rule(LmRuleArgs a) {
    extern __shared__ __attribute__((aligned(16))) u64 rule_lds[];
    __shared__ int divtab[512];
    const u32 e = blockIdx.y;
    const LmRule ru = a.rule[a.kind[e]];
    const int w = a.w, h = a.h, nw = (w + 63) >> 6, r = ru.grow;
    const int y0 = (int)blockIdx.x * a.rows_out;
    const int rows_out = min(a.rows_out, h - y0);
    const int rows_in = rows_out + 2 * r;                  // image rows y0 - r .. y0 + rows_out + r - 1
    u64* S = rule_lds;                                     // [rows_in][nw] seed words
    u64* R = rule_lds + (size_t)(a.rows_out + 2 * LM_RULE_MAX_GROW) * nw;      // [rows_out][nw] result words
    const size_t so = (size_t)a.slot[e] * a.slot_stride;
    if (ru.use_hsv) {
        for (int i = threadIdx.x; i < 512; i += 256) divtab[i] = a.divtab[i];
        __syncthreads();
    }
    // ---- 1: seed bytes
    {
        u8* Sb = reinterpret_cast<u8*>(S);
        const int bpr = nw * 8;                            // bytes per row of words
        for (int t = threadIdx.x; t < rows_in * bpr; t += 256) {
            const int rr = t / bpr, j = t - rr * bpr;
            const int y = y0 - r + rr, x = 8 * j;
            u32 bits = 0;
            if (y >= 0 && y < h && x < w) {
                const size_t px = (size_t)y * w + x;
                const int npx = min(8, w - x);
                bits = (1u << npx) - 1u;
                if (ru.use_depth) {
                    const u16* dp = reinterpret_cast<const u16*>(reinterpret_cast<const u8*>(a.depth) + so) + px;
                    u32 dd[4] = {0, 0, 0, 0};
                    if (a.vec) {
                        const u32x4 v = ld16(dp);
                        dd[0] = v.x; dd[1] = v.y; dd[2] = v.z; dd[3] = v.w;
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k) if (k < npx) dd[k >> 1] |= (u32)dp[k] << (16 * (k & 1));
                    }
                    u32 in = 0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int d = (int)((dd[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
                        in |= (u32)(d == 0 ? ru.keep_invalid != 0 : (d >= ru.zmin && d <= ru.zmax)) << k;
                    }
                    bits &= in;
                }
                if (ru.use_hsv) {
                    const u8* cp = a.bgr + so + px * 3;
                    u32 cc[6] = {0, 0, 0, 0, 0, 0};
                    if (a.vec) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const u32x2 v = *reinterpret_cast<const u32x2*>(cp + 8 * k);
                            cc[2 * k] = v.x; cc[2 * k + 1] = v.y;
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < 24; ++k) if (k < 3 * npx) cc[k >> 2] |= (u32)cp[k] << (8 * (k & 3));
                    }
                    u32 in = 0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int b = (int)((cc[(3 * k) >> 2] >> (8 * ((3 * k) & 3))) & 0xFFu);
                        const int g = (int)((cc[(3 * k + 1) >> 2] >> (8 * ((3 * k + 1) & 3))) & 0xFFu);
                        const int c = (int)((cc[(3 * k + 2) >> 2] >> (8 * ((3 * k + 2) & 3))) & 0xFFu);
                        in |= (u32)hsv_in_range(b, g, c, ru.hsv, divtab) << k;
                    }
                    bits &= in;
                }
            }
            Sb[t] = (u8)bits;
        }
    }
    __syncthreads();
    // ---- 2: dilation and rectangle
    for (int t = threadIdx.x; t < rows_out * nw; t += 256) {
        const int ro = t / nw, i = t - ro * nw;
        u64 lf = 0, c = 0, rt = 0;
        for (int k = 0; k <= 2 * r; ++k) {                // S rows ro .. ro + 2r = image rows y - r .. y + r
            const u64* row = S + (size_t)(ro + k) * nw;
            c |= row[i];
            if (i > 0) lf |= row[i - 1];
            if (i + 1 < nw) rt |= row[i + 1];
        }
        // A: OR of the bits at x .. x + r, B: at x - r .. x.  A neighbour word is dilated too, without ITS neighbour: what it lacks
        // sits within r <= 16 bits of its far end, and the middle word takes at most 16 bits of its near end.
        u64 A = c, B = c;
        int span = 1;                                      // A, B hold the OR over `span` positions
        while (span <= r) {
            const int s = min(span, r + 1 - span);
            A |= (A >> s) | (rt << (64 - s)); rt |= rt >> s;
            B |= (B << s) | (lf >> (64 - s)); lf |= lf << s;
            span += s;
        }
        u64 m = A | B;
        const int y = y0 + ro;
        const int lo = max(ru.rx - 64 * i, 0), hi = min(ru.rx + ru.rw - 64 * i, 64);
        if (y < ru.ry || y >= ru.ry + ru.rh || hi <= lo) m = 0;
        else m &= (hi == 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
        R[t] = m;
    }
    __syncthreads();
    // ---- 3: bits -> bytes
    u8* plane = a.plane[e];
    const int vpr = nw * 4;                                // 16-byte vectors per row of the plane (mask_pitch = 64 nw)
    for (int t = threadIdx.x; t < rows_out * vpr; t += 256) {
        const int ro = t / vpr, v = t - ro * vpr;
        const u32 b = (u32)(R[ro * nw + (v >> 2)] >> (16 * (v & 3))) & 0xFFFFu;
        u32x4 o;
        o.x = expand4(b & 15u); o.y = expand4((b >> 4) & 15u); o.z = expand4((b >> 8) & 15u); o.w = expand4(b >> 12);
        st16(plane + (size_t)(y0 + ro) * a.mask_pitch + 16u * v, o);
    }
}

static size_t mask_rule_lds(int w, int rows_out) { return (size_t)(2 * rows_out + 2 * LM_RULE_MAX_GROW) * ((w + 63) / 64) * sizeof(u64); }

bool lmk_mask_rule_fits(int w) { return mask_rule_lds(w, 8) <= 60 * 1024; }

void lmk_mask_rule(hipStream_t s, LmRuleArgs& a) {
    if (!a.n) return;
    // strips of 64 rows keep the halo rows (2 grow per strip) a small share; few frames take strips of 16 rows for more workgroups
    int rows = (size_t)a.n * ((a.h + 63) / 64) >= 512 ? 64 : 16;
    while (rows > 8 && mask_rule_lds(a.w, rows) > 40 * 1024) rows >>= 1;
    a.rows_out = rows;
    // a lane's 8 pixels: depth (px * 2) 16-byte aligned, colour (px * 3) 8-byte aligned, at every row start of every slot
    a.vec = a.w % 8 == 0 && a.slot_stride % 16 == 0 && reinterpret_cast<uintptr_t>(a.bgr) % 8 == 0 &&
            reinterpret_cast<uintptr_t>(a.depth) % 16 == 0;
    hipLaunchKernelGGL(k_mask_rule, dim3((unsigned)((a.h + rows - 1) / rows), (unsigned)a.n), dim3(256), mask_rule_lds(a.w, rows), s, a);
}
