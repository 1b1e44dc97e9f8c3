// lm_k_eval.hip -- pose-error evaluation on the GPU: the kernels behind lm_pose_error_vsd, lm_pose_error_add and
// lm_stage_vsd_counts (Benchmark.cpp's calculateErrorHodan, calculateErrorLM and calculateErrorLMAmbigous).  Host side: lm_detector_eval.hip.
//   Hodan    lmk_gen_zbuffer renders the GT and the estimated pose of every query as two views -> k_eval_vsd counts the pixels of
//            calculateVisibilityMasks' rules (wave ballots + popcounts, per-block sums in LDS, one integer atomic per block and counter)
//   ADD      k_eval_transform: R v + t of both poses and the per-vertex distance
//   ADD-S    k_eval_transform (both clouds) -> k_eval_adds: LDS-tiled all pairs, the running minimum of the squared length, one
//            atomicMin on its bits per GT vertex and estimate slice
//   mean     k_eval_final (per-vertex result, a double sum per block) -> k_eval_mean (one fixed-order sum per query)
// -ffp-contract=off (build.py) keeps every product and sum apart, in the order written (the contract).
#include "lm_dev.h"
#include "lm_kernels.h"

namespace {

constexpr int kEvalTile = 256;
constexpr int kAddsGt = 4;                               // GT vertices per lane of k_eval_adds
constexpr int kAddsGtBlock = kEvalTile * kAddsGt;       // GT vertices per block
constexpr int kAddsEstSlice = 1024;                     // estimate vertices per block (grid.y slices the estimate cloud)
constexpr u32 kInfBits = 0x7f800000u;

// Benchmark::calculateVisibilityMasks on CV_16U images, one pixel (the reference's saturating subtractions and 16-bit thresholds):
// bit 0 rendered GT (> 1), 1 rendered estimate, 2 visible GT, 3 visible estimate, 4 intersection, 5 union, 6 visible in both with
// |gt - est| <= tau.
__device__ __forceinline__ u32 vsd_bits(int g, int e, int d, int delta, int tau) {
    const bool rg = g > 1, re = e > 1;
    const bool og = (g > d ? g - d : 0) > delta, oe = (e > d ? e - d : 0) > delta;
    const bool vg = rg && !og;
    const bool ve = (re && !oe) || (vg && e != 0);        // estimateVisibility |= groundTruthVisibility & estimateDepthRender
    const bool in = vg && ve;
    const int ad = g > e ? g - e : e - g;
    return (rg ? 1u : 0u) | (re ? 2u : 0u) | (vg ? 4u : 0u) | (ve ? 8u : 0u) | (in ? 16u : 0u) | ((vg || ve) ? 32u : 0u) |
           ((in && ad <= tau) ? 64u : 0u);
}

// grid (pixel blocks, query); query q's renders are views 2q (GT) and 2q + 1 (estimate).  FromZ: z-buffers (u32, gen_z_to_mm) or,
// for the stage hook, depth images (u16).  counts[q][8] must be zero on entry.
template <bool FromZ, int PerThread>
__global__ __launch_bounds__(256) void k_eval_vsd(const void* renders, const u16* scenes, const int* scene_idx, size_t npx, int delta, int tau,
                                                  u32* counts) {
    const int q = blockIdx.y;
    const u16* sc = scenes + (size_t)scene_idx[q] * npx;
    const u32* zg = reinterpret_cast<const u32*>(renders) + (size_t)(2 * q) * npx;
    const u16* hg = reinterpret_cast<const u16*>(renders) + (size_t)(2 * q) * npx;
    u32 c[7] = {0, 0, 0, 0, 0, 0, 0};
    const size_t p0 = (size_t)blockIdx.x * (kEvalTile * PerThread) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < PerThread; ++k) {
        const size_t p = p0 + (size_t)k * kEvalTile;
        u32 b = 0;
        if (p < npx) {
            int g, e;
            if (FromZ) { g = gen_z_to_mm(zg[p]); e = gen_z_to_mm(zg[npx + p]); }
            else { g = hg[p]; e = hg[npx + p]; }
            b = vsd_bits(g, e, sc[p], delta, tau);
        }
#pragma unroll
        for (int j = 0; j < 7; ++j) c[j] += (u32)__popcll(__ballot((b >> j) & 1u));
    }
    __shared__ u32 part[kEvalTile / 64][8];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0)
        for (int j = 0; j < 7; ++j) part[wv][j] = c[j];
    __syncthreads();
    if (threadIdx.x < 7) {
        u32 s = 0;
        for (int w = 0; w < kEvalTile / 64; ++w) s += part[w][threadIdx.x];
        if (s) atomicAdd(&counts[(size_t)q * 8 + threadIdx.x], s);
    }
}

// One pose's point: R v + t, row-major R, left to right.
__device__ __forceinline__ float3 eval_apply(const float* P, float x, float y, float z) {
    float3 r;
    r.x = P[0] * x + P[1] * y + P[2] * z + P[9];
    r.y = P[3] * x + P[4] * y + P[5] * z + P[10];
    r.z = P[6] * x + P[7] * y + P[8] * z + P[11];
    return r;
}

// grid (vertex blocks, query); q[24] = R_gt[9] t_gt[3] R_est[9] t_est[3].  ADD: dist[q][k] = |gt_k - est_k|.  ADD-S: both clouds
// (gt / est [q][m], float4) and the minimum's start (+inf bits).
__global__ __launch_bounds__(256) void k_eval_transform(const float* xyz, int step, int m, const float* queries, int symmetric, float4* gt,
                                                        float4* est, u32* minbits, float* dist) {
    const int k = blockIdx.x * kEvalTile + threadIdx.x;
    const int q = blockIdx.y;
    if (k >= m) return;
    const size_t v = (size_t)k * step;
    const float x = xyz[3 * v], y = xyz[3 * v + 1], z = xyz[3 * v + 2];
    const float* Q = queries + 24 * (size_t)q;
    const float3 a = eval_apply(Q, x, y, z), b = eval_apply(Q + 12, x, y, z);
    const size_t o = (size_t)q * m + k;
    if (symmetric) {
        gt[o] = make_float4(a.x, a.y, a.z, 0.f);
        est[o] = make_float4(b.x, b.y, b.z, 0.f);
        minbits[o] = kInfBits;
    } else {
        const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
        dist[o] = sqrtf(dx * dx + dy * dy + dz * dz);
    }
}

// grid (GT blocks, estimate slices, query).  Each lane keeps kAddsGt GT vertices and the running minimum of their squared lengths;
// the slice's estimate vertices pass through LDS, every lane reading the same one (a broadcast).  NaN never lowers a minimum (fminf),
// as `tmpDiff < absDifference` never takes one.  Squared lengths are >= +0, so their bits order like the floats: atomicMin is exact.
__global__ __launch_bounds__(256) void k_eval_adds(const float4* gt, const float4* est, int m, u32* minbits) {
    const int q = blockIdx.z;
    const int g0 = blockIdx.x * kAddsGtBlock + threadIdx.x;
    const int e0 = blockIdx.y * kAddsEstSlice;
    const float4* G = gt + (size_t)q * m;
    const float4* E = est + (size_t)q * m;
    __shared__ float4 tile[kEvalTile];
    float gx[kAddsGt], gy[kAddsGt], gz[kAddsGt], mn[kAddsGt];
#pragma unroll
    for (int j = 0; j < kAddsGt; ++j) {
        const int k = g0 + j * kEvalTile;
        const float4 p = G[k < m ? k : m - 1];
        gx[j] = p.x; gy[j] = p.y; gz[j] = p.z; mn[j] = __uint_as_float(kInfBits);
    }
    const int e1 = min(m, e0 + kAddsEstSlice);
    for (int t0 = e0; t0 < e1; t0 += kEvalTile) {
        const int nt = min(kEvalTile, e1 - t0);
        __syncthreads();
        if ((int)threadIdx.x < nt) tile[threadIdx.x] = E[t0 + threadIdx.x];
        __syncthreads();
        for (int i = 0; i < nt; ++i) {
            const float4 e = tile[i];
#pragma unroll
            for (int j = 0; j < kAddsGt; ++j) {
                const float dx = gx[j] - e.x, dy = gy[j] - e.y, dz = gz[j] - e.z;
                mn[j] = fminf(mn[j], dx * dx + dy * dy + dz * dz);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kAddsGt; ++j) {
        const int k = g0 + j * kEvalTile;
        if (k < m) atomicMin(&minbits[(size_t)q * m + k], __float_as_uint(mn[j]));
    }
}

// grid (vertex blocks, query): the per-vertex result (ADD-S: sqrt of the minimum, never above the reference's start 999999) and the
// block's sum in double, reduced in a fixed tree -> part[q][block]
__global__ __launch_bounds__(256) void k_eval_final(const u32* minbits, float* dist, int m, int symmetric, double* part) {
    const int k = blockIdx.x * kEvalTile + threadIdx.x;
    const int q = blockIdx.y;
    __shared__ double s[kEvalTile];
    double v = 0.0;
    if (k < m) {
        const size_t o = (size_t)q * m + k;
        float d;
        if (symmetric) {
            d = sqrtf(__uint_as_float(minbits[o]));
            d = d < 999999.f ? d : 999999.f;
            dist[o] = d;
        } else {
            d = dist[o];
        }
        v = (double)d;
    }
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = kEvalTile / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)q * gridDim.x + blockIdx.x] = s[0];
}

// one block per query: the block sums in a fixed order, mean = (float)(sum / m)
__global__ __launch_bounds__(256) void k_eval_mean(const double* part, int nb, int m, float* mean) {
    const int q = blockIdx.x;
    __shared__ double s[kEvalTile];
    double v = 0.0;
    for (int i = threadIdx.x; i < nb; i += kEvalTile) v += part[(size_t)q * nb + i];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = kEvalTile / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) mean[q] = (float)(s[0] / (double)m);
}

inline unsigned cdiv(size_t n, size_t d) { return (unsigned)((n + d - 1) / d); }

constexpr int kVsdPerThread = 8;

}  // namespace

void lmk_eval_vsd(hipStream_t s, bool from_z, const void* renders, const u16* scenes, const int* scene_idx, int nq, size_t npx, int delta,
                  int tau, u32* counts) {
    const dim3 grid(cdiv(npx, (size_t)kEvalTile * kVsdPerThread), (unsigned)nq);
    if (from_z)
        hipLaunchKernelGGL((k_eval_vsd<true, kVsdPerThread>), grid, dim3(kEvalTile), 0, s, renders, scenes, scene_idx, npx, delta, tau, counts);
    else
        hipLaunchKernelGGL((k_eval_vsd<false, kVsdPerThread>), grid, dim3(kEvalTile), 0, s, renders, scenes, scene_idx, npx, delta, tau, counts);
}

size_t lmk_eval_add_parts(int m) { return cdiv((size_t)m, kEvalTile); }

void lmk_eval_add(hipStream_t s, const float* xyz, int step, int m, const float* queries, int nq, int symmetric, float4* gt, float4* est,
                  u32* minbits, float* dist, double* part, float* mean) {
    const unsigned nb = cdiv((size_t)m, kEvalTile);
    hipLaunchKernelGGL(k_eval_transform, dim3(nb, (unsigned)nq), dim3(kEvalTile), 0, s, xyz, step, m, queries, symmetric, gt, est, minbits, dist);
    if (symmetric)
        hipLaunchKernelGGL(k_eval_adds, dim3(cdiv((size_t)m, kAddsGtBlock), cdiv((size_t)m, kAddsEstSlice), (unsigned)nq), dim3(kEvalTile), 0, s,
                           gt, est, m, minbits);
    hipLaunchKernelGGL(k_eval_final, dim3(nb, (unsigned)nq), dim3(kEvalTile), 0, s, minbits, dist, m, symmetric, part);
    hipLaunchKernelGGL(k_eval_mean, dim3((unsigned)nq), dim3(kEvalTile), 0, s, part, (int)nb, m, mean);
}
