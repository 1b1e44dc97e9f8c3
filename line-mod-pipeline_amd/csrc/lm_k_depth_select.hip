// lm_k_depth_select.hip -- k_depth_select for gfx950 (CDNA4, wave64): the depth check's sorted order statistic of many crops of resident depth
// frames (include/linemod_hip.h lm_depth_select_begin), and its launcher.
//
// Per query: the element at 0-based index `rank` of the ascending sort of t = (d <= 1) ? 65535 : d over the crop [x0, x1) x [y0, y1).  An exact
// radix select over the 16-bit key in two passes over the crop (tens of KB, L2-resident after the first): a histogram of the high bytes, the bin
// that holds the rank (lm_depth_select.h, the step the host runs too), then a histogram of the low bytes of the values in that bin.
//
// One workgroup per query and k_depth_counts' access pattern: thread t takes the 8-pixel pieces t, t + 256, .. of the crop, eight independent
// 2-byte loads each, nothing outside [x0, x1) of the crop's rows.
//
// Contention.  Depth crops are smooth: most pixels of a crop share one high byte, and 256 lanes adding 1 to one LDS word would serialise.  So a
// lane counts in registers: it keeps ONE open run (bin, count) across its whole walk and touches LDS only when the bin changes and once at
// the end -- on a smooth crop a handful of atomics per lane instead of one per pixel.  The histograms are private to a wave (4 x 256 words), so
// the closing flush of an all-equal crop is 64 adds to a word, once.  All of it is integer addition: the sums, and with them the chosen bins,
// do not depend on the order of arrival.  Counters are 32-bit (a crop is at most a frame).
#include "lm_dev.h"
#include "lm_depth_select.h"

namespace {

constexpr int SEL_WAVES = 4;

// One pass over the crop: the histogram of key(t) over the pixels that `take` admits, into hist[wave][256] (zeroed by the caller).
// PASS 0: key = t >> 8, every pixel.  PASS 1: key = t & 255, the pixels with t >> 8 == hi.
template <int PASS, bool NAIVE>
__device__ __forceinline__ void sel_pass(const u16* __restrict__ img, int w, int x0, int y0, int cw, int ch, int hi, u32* hist) {
    const int tid = (int)threadIdx.x;
    u32* mine = NAIVE ? hist : hist + (tid >> 6) * LM_SEL_BINS;
    const int pr = (cw + 7) >> 3;                      // pieces per row
    const int np = pr * ch;
    int run_bin = -1; u32 run_n = 0;                   // the lane's open run
    for (int p = tid; p < np; p += 256) {
        const int r = p / pr, c = (p - r * pr) << 3;
        const u16* src = img + (size_t)(y0 + r) * w + x0 + c;
        const int m = cw - c < 8 ? cw - c : 8;
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = k < m ? (int)src[k] : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int t = v[k] <= 1 ? 65535 : v[k];
            const bool ok = k < m && (PASS == 0 || (t >> 8) == hi);
            const int key = PASS == 0 ? (t >> 8) : (t & 255);
            if (!ok) continue;
            if (NAIVE) { atomicAdd(&mine[key], 1u); continue; }
            if (key == run_bin) { ++run_n; continue; }
            if (run_n) atomicAdd(&mine[run_bin], run_n);
            run_bin = key; run_n = 1;
        }
    }
    if (!NAIVE && run_n) atomicAdd(&mine[run_bin], run_n);
}

// hist[wave][256] -> tot[256] (the waves' sums) and coarse[16]; every thread then reads the same choice.
template <bool NAIVE>
__device__ __forceinline__ LmSelBin sel_choose(u32* hist, u32* tot, u32* coarse, u32 rank) {
    const int tid = (int)threadIdx.x;
    __syncthreads();
    u32 s = hist[tid];
    if (!NAIVE) {
#pragma unroll
        for (int wv = 1; wv < SEL_WAVES; ++wv) s += hist[wv * LM_SEL_BINS + tid];
    }
    tot[tid] = s;
    __syncthreads();
    if (tid < LM_SEL_COARSE) {
        u32 cs = 0;
#pragma unroll
        for (int k = 0; k < LM_SEL_BINS / LM_SEL_COARSE; ++k) cs += tot[tid * (LM_SEL_BINS / LM_SEL_COARSE) + k];
        coarse[tid] = cs;
    }
    __syncthreads();
    return lm_select_bin256(tot, coarse, rank);
}

template <bool NAIVE>
__global__ __launch_bounds__(256) void k_depth_select(LmDepthSelArgs a) {
    __shared__ u32 hist[SEL_WAVES * LM_SEL_BINS];
    __shared__ u32 tot[LM_SEL_BINS];
    __shared__ u32 coarse[LM_SEL_COARSE];
    const int tid = (int)threadIdx.x;
    const u32 qi = blockIdx.x;
    const LmDepthSelQuery q = a.q[qi];
    const int cw = q.x1 - q.x0, ch = q.y1 - q.y0;
    if (cw <= 0 || ch <= 0) {                          // an empty crop: 65535 (uniform over the workgroup: no barrier is skipped by a part of it)
        if (tid == 0) a.out[qi] = (u16)65535;
        return;
    }
    const u16* img = reinterpret_cast<const u16*>(reinterpret_cast<const u8*>(a.depth) + (size_t)q.slot * a.slot_stride);
    for (int k = tid; k < SEL_WAVES * LM_SEL_BINS; k += 256) hist[k] = 0u;
    __syncthreads();
    sel_pass<0, NAIVE>(img, a.w, q.x0, q.y0, cw, ch, 0, hist);
    const LmSelBin hi = sel_choose<NAIVE>(hist, tot, coarse, (u32)q.rank);
    __syncthreads();                                   // (every thread has read tot / coarse)
    for (int k = tid; k < SEL_WAVES * LM_SEL_BINS; k += 256) hist[k] = 0u;
    __syncthreads();
    sel_pass<1, NAIVE>(img, a.w, q.x0, q.y0, cw, ch, hi.bin, hist);
    const LmSelBin lo = sel_choose<NAIVE>(hist, tot, coarse, hi.rank);
    if (tid == 0) a.out[qi] = (u16)((hi.bin << 8) | lo.bin);
}

}  // namespace

void lmk_depth_select(hipStream_t s, const LmDepthSelArgs& a, bool naive_histogram) {
    if (a.n == 0) return;
    if (naive_histogram) hipLaunchKernelGGL(k_depth_select<true>, dim3(a.n), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_depth_select<false>, dim3(a.n), dim3(256), 0, s, a);
}
