// lm_k_mask.hip -- Detector::match's per-modality masks: the quantised images of the masked slots of a
// call ANDed with their masks, between the last quantiser and the linear memories (lm_detector.hip enqueue_preprocess).
//   colour: quant[l][0] &= mask_l at every level l, mask_l = the level-0 mask resized with INTER_NEAREST l times = mask0[y << l][x << l]
//   depth:  quant[0][1] &= mask_0 only: every depth level above reads quant[0][1] at (2y, 2x) (lmk_linear_memories of level 1,
//           lmk_nn_half for the levels above), the same NN rule as the mask's, so the one masking is exact at every level.
// A byte-wise, memory-bound pass: each lane ANDs 16 quantised bytes with 16 mask bytes (dwordx4 loads and stores).  The level-1 mask
// bytes are the even bytes of two dwordx4 loads of row 2y, gathered with v_perm_b32.
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
