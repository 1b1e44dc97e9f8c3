// lm_k_select.hip -- the feature selection of addTemplate on the GPU: what lmh::select_color / lmh::select_depth
// (lm_extract.cpp) make of a candidate list, feature for feature.  Host side: lm_detector_gen.hip (lm_add_templates_slots,
// lm_add_templates_rendered, lm_stage_select).
//   One workgroup per list.  The host sorts (score descending, equal scores in list order) and walks the sorted list cyclically; it keeps
//   a candidate iff it lies at least `distance` from everything kept, and relaxes the distance by one after every full walk.  Within one
//   walk the distance is fixed and the kept set only grows, so a candidate that has failed stays failed: "the next one the host keeps" is
//   the alive candidate with the smallest 64-bit key (~score bits | list index; scores are non-negative floats, which order like their
//   bits).  No sort: per pick one block reduction of that minimum, then every thread tests its alive candidates against the one new
//   feature.  When nothing is alive the walk has ended: relax, and evaluate every candidate against the kept set again.
//   A thread owns the candidates tid, tid + T, ...; their alive bits are the thread's own words of a global scratch bitmap (word j of
//   thread t = candidates (32 j + b) T + t), so nothing but the 63 kept positions, the label counts and the reduction lives in LDS.
//   Integer and compare arithmetic only, but for the depth scores' division, which is IEEE single precision like the host's (__fdiv_rn).
//   No atomics on floats: the result does not depend on the order in which anything runs.
#include "lm_dev.h"
#include "lm_kernels.h"

namespace {

constexpr int kSelT = LM_SELECT_THREADS;
constexpr unsigned long long kNone = ~0ull;

__device__ __forceinline__ unsigned long long sel_block_min(unsigned long long v, unsigned long long* wave_min) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_down(v, o, 64);
        v = t < v ? t : v;
    }
    __syncthreads();                                   // (the previous reduction's readers are done with wave_min)
    if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = wave_min[0];
    for (int k = 1; k < kSelT / 64; ++k) m = wave_min[k] < m ? wave_min[k] : m;
    return m;
}

// pick_scattered's test against one kept feature (xy: x in the low half, y in the high half, both int16)
__device__ __forceinline__ bool sel_far(u32 xy, u32 kxy, float d2) {
    const int dx = (int)(int16_t)(xy & 0xFFFFu) - (int)(int16_t)(kxy & 0xFFFFu);
    const int dy = (int)(int16_t)(xy >> 16) - (int)(int16_t)(kxy >> 16);
    return (float)(dx * dx + dy * dy) >= d2;
}

__global__ __launch_bounds__(LM_SELECT_THREADS) void k_select(const LmSelList* lists, const LmGenCand* cand, u32* skey, u32* alive_all,
                                                              lm_feature* features, int* n_out) {
    __shared__ int lab_cnt[8];
    __shared__ u32 kept[LM_MAX_FEATURES + 1];
    __shared__ unsigned long long wave_min[kSelT / 64];
    const LmSelList L = lists[blockIdx.x];
    const int tid = threadIdx.x;
    const u32 n = L.n;
    const int want = L.want;
    if (want <= 0 || n < (u32)want) {                  // (uniform) too few: the host's select_* returns false before it touches anything
        if (tid == 0) n_out[blockIdx.x] = want <= 0 ? 0 : -1;
        return;
    }
    const LmGenCand* c = cand + L.lo;
    u32* key = skey + L.lo;
    u32* alive = alive_all + L.alive_lo;
    lm_feature* out = features + (size_t)blockIdx.x * LM_MAX_FEATURES;
    // the sort key's high word: ~bits of the score, depth: of the score divided by the number of candidates of its label in this list
    if (L.depth) {
        if (tid < 8) lab_cnt[tid] = 0;
        __syncthreads();
        int mine[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (u32 i = tid; i < n; i += kSelT) {
            const int lab = c[i].label & 7;
#pragma unroll
            for (int b = 0; b < 8; ++b) mine[b] += lab == b ? 1 : 0;
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) if (mine[b]) atomicAdd(&lab_cnt[b], mine[b]);
        __syncthreads();
        for (u32 i = tid; i < n; i += kSelT) key[i] = ~__float_as_uint(__fdiv_rn(c[i].score, (float)lab_cnt[c[i].label & 7]));
    } else {
        for (u32 i = tid; i < n; i += kSelT) key[i] = ~__float_as_uint(c[i].score);
    }
    const u32 nwords = (n + 32u * kSelT - 1) / (32u * kSelT);      // alive words of this thread
    float distance = L.distance, d2 = distance * distance;
    int nk = 0;
    for (;;) {
        // a new walk: every candidate against the whole kept set (a kept one fails against itself while d2 > 0)
        bool fresh = true;
        for (;;) {
            unsigned long long best = kNone;
            const u32 newest = nk ? kept[nk - 1] : 0u;
            for (u32 j = 0; j < nwords; ++j) {
                u32 w;
                if (fresh) {
                    w = 0;
                    for (u32 b = 0; b < 32; ++b) {
                        const u32 i = (j * 32u + b) * kSelT + tid;
                        if (i >= n) break;
                        const u32 xy = *reinterpret_cast<const u32*>(&c[i]);
                        bool ok = true;
                        for (int k = 0; k < nk && ok; ++k) ok = sel_far(xy, kept[k], d2);
                        if (ok) {
                            w |= 1u << b;
                            const unsigned long long kk = ((unsigned long long)key[i] << 32) | i;
                            best = kk < best ? kk : best;
                        }
                    }
                    alive[(size_t)j * kSelT + tid] = w;
                } else {
                    const u32 w0 = alive[(size_t)j * kSelT + tid];
                    w = w0;
                    for (u32 r = w0; r; r &= r - 1) {
                        const u32 b = (u32)__ffs(r) - 1u;
                        const u32 i = (j * 32u + b) * kSelT + tid;
                        const u32 xy = *reinterpret_cast<const u32*>(&c[i]);
                        if (!sel_far(xy, newest, d2)) { w &= ~(1u << b); continue; }
                        const unsigned long long kk = ((unsigned long long)key[i] << 32) | i;
                        best = kk < best ? kk : best;
                    }
                    if (w != w0) alive[(size_t)j * kSelT + tid] = w;
                }
            }
            fresh = false;
            const unsigned long long g = sel_block_min(best, wave_min);
            if (g == kNone) break;                     // the walk is past its last candidate
            const u32 i = (u32)g;
            const LmGenCand pc = c[i];
            if (i % kSelT == (u32)tid) {               // the owner: the walk has passed the candidate, whatever d2 says
                const u32 bit = i / kSelT;
                alive[(size_t)(bit >> 5) * kSelT + tid] &= ~(1u << (bit & 31u));
                kept[nk] = *reinterpret_cast<const u32*>(&c[i]);
                out[nk] = lm_feature{pc.x, pc.y, pc.label};
            }
            ++nk;
            if (nk == want) {
                if (tid == 0) n_out[blockIdx.x] = nk;
                return;
            }
            __syncthreads();                           // kept[nk - 1] is visible
        }
        distance -= 1.0f;
        d2 = distance * distance;
        // Below zero the host's walk would never end (every position left is kept already): lists with repeated positions only
        if (distance < 0.0f) {
            if (tid == 0) n_out[blockIdx.x] = -1;
            return;
        }
        __syncthreads();
    }
}

}  // namespace

void lmk_select(hipStream_t s, const LmSelList* lists, int n_lists, const LmGenCand* cand, u32* skey, u32* alive, lm_feature* features,
                int* n_out) {
    if (n_lists > 0) hipLaunchKernelGGL(k_select, dim3((unsigned)n_lists), dim3(kSelT), 0, s, lists, cand, skey, alive, features, n_out);
}
