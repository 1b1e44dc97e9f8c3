// lm_k_icp.hip -- ICP pose refinement (HighLevelLinemodIcp): the scene cloud of prepareDepthForIcp and the
// rounds of ICP::registerModelToScene, batched over every pose of a query.  Host side: lm_detector_icp.hip.
//   scene cloud  k_icp_blur_z -> k_icp_keep_count -> k_icp_scan -> k_icp_scatter -> k_icp_normals
//   per pose     k_icp_normalise, then per level k_icp_level_src and per round k_icp_nn -> k_icp_select -> k_icp_picky -> k_icp_accum
//                -> k_icp_solve, and k_icp_finish.  Every round of every level is enqueued up front: a pose whose level is done (the
//                stop test, fewer than 6 pairs, a NaN) returns at once from the kernels of the remaining rounds.
// Positions of the scene cloud are float and bit-identical to the numpy restatement (tests/icp_reference.py): -ffp-contract=off and
// the same operation order.  Everything of the ICP is double except the 1-NN distances handed to the median, which are float.
#include "lm_dev.h"
#include "lm_kernels.h"

#include <algorithm>

namespace {

constexpr int kIcpTile = 256;
constexpr int kIcpK = 12;                      // neighbours of a normal (computeNormalsPC3d(..., 12, ...))
constexpr double kMadScale = 1.48257968;
constexpr double kFvalStart = 9999999999.0;
constexpr int kAcc = 29;                       // A^T A upper triangle (21) | A^T b (6) | pair count | sum of squared 6-column differences

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// Block sum of a u64 (256 threads), one atomic per block.  Integer: the order does not matter.
__device__ void block_add_u64(unsigned long long v, unsigned long long* dst) {
    __shared__ unsigned long long s[kIcpTile / 64];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kIcpTile / 64; ++w) t += s[w];
        atomicAdd(dst, t);
    }
}

__device__ __forceinline__ bool keep_z(u32 z, double mean) { return !(fabs((double)z - mean) > 300.0); }

// x' = M x (3x4 row-major), left-to-right sums as tests/icp_reference.py transform()
__device__ __forceinline__ void xform_p(const double* M, const double* x, double* y) {
    for (int r = 0; r < 3; ++r) y[r] = M[4 * r] * x[0] + M[4 * r + 1] * x[1] + M[4 * r + 2] * x[2] + M[4 * r + 3];
}
__device__ __forceinline__ void xform_n(const double* M, const double* x, double* y) {
    for (int r = 0; r < 3; ++r) y[r] = M[4 * r] * x[0] + M[4 * r + 1] * x[1] + M[4 * r + 2] * x[2];
}
// C = A B for 3x4 row-major rigid transforms (the implicit last row 0 0 0 1)
__device__ void compose(const double* A, const double* B, double* C) {
    double t[12];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) t[4 * r + c] = A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c] + A[4 * r + 2] * B[8 + c] + (c == 3 ? A[4 * r + 3] : 0.0);
    for (int k = 0; k < 12; ++k) C[k] = t[k];
}
__device__ void set_identity(double* M) { for (int k = 0; k < 12; ++k) M[k] = (k % 5 == 0) ? 1.0 : 0.0; }

// the normalised scene point j: ((x, y, z) - meanAvg) * scale
__device__ __forceinline__ void dst_pos(const float* scene, int j, const LmIcpPose& p, double* d) {
    for (int c = 0; c < 3; ++c) d[c] = ((double)scene[6 * (size_t)j + c] - p.mean_avg[c]) * p.scale;
}

// Eigenvector of the smallest eigenvalue of a symmetric 3x3 (cyclic Jacobi, fixed sweeps, double).
__device__ void smallest_eigvec(double a00, double a01, double a02, double a11, double a12, double a22, double* n) {
    double a[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 10; ++sweep) {
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            if (a[p][q] == 0.0) continue;
            const double th = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
            const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double kp = a[k][p], kq = a[k][q]; a[k][p] = c * kp - s * kq; a[k][q] = s * kp + c * kq; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double pk = a[p][k], qk = a[q][k]; a[p][k] = c * pk - s * qk; a[q][k] = s * pk + c * qk; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double kp = v[k][p], kq = v[k][q]; v[k][p] = c * kp - s * kq; v[k][q] = s * kp + c * kq; }
        }
    }
    int m = 0;
    if (a[1][1] < a[m][m]) m = 1;
    if (a[2][2] < a[m][m]) m = 2;
    const double x = m == 0 ? v[0][0] : (m == 1 ? v[0][1] : v[0][2]);
    const double y = m == 0 ? v[1][0] : (m == 1 ? v[1][1] : v[1][2]);
    const double z = m == 0 ? v[2][0] : (m == 1 ? v[2][1] : v[2][2]);
    const double l = sqrt(x * x + y * y + z * z);
    n[0] = x / l; n[1] = y / l; n[2] = z / l;
}

}  // namespace

// ---- scene cloud.  counts: [0] bbox pixels with z kept by the 300 mm test, [1] points written = [0] / step.  zsum: sum of z (u64).
// (Outside the anonymous namespace: rocprofv3 lists the kernels by these names.)

// 3x3 box blur (REFLECT_101, (sum + 4) / 9) of the bbox's pixels, in the bbox's row-major order
__global__ __launch_bounds__(256) void k_icp_blur_z(const u16* depth, int W, int H, int x0, int y0, int bw, int bh, u32* z,
                                                    unsigned long long* zsum) {
    const int k = blockIdx.x * kIcpTile + threadIdx.x;
    unsigned long long v = 0;
    if (k < bw * bh) {
        const int u = x0 + k % bw, r = y0 + k / bw;
        u32 s = 0;
        for (int dy = -1; dy <= 1; ++dy) {
            const u16* row = depth + (size_t)reflect101(r + dy, H) * W;
            for (int dx = -1; dx <= 1; ++dx) s += row[reflect101(u + dx, W)];
        }
        v = (s + 4) / 9;
        z[k] = (u32)v;
    }
    block_add_u64(v, zsum);
}

__global__ __launch_bounds__(256) void k_icp_keep_count(const u32* z, int npx, const unsigned long long* zsum, u32* blockcnt) {
    __shared__ u32 cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const double mean = (double)*zsum / (double)npx;
    const int k = blockIdx.x * kIcpTile + threadIdx.x;
    const bool keep = k < npx && keep_z(z[k], mean);
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) atomicAdd(&cnt, (u32)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = cnt;
}

// exclusive scan of the block counts (a few hundred) by one thread: deterministic and far below a microsecond per hundred blocks
__global__ void k_icp_scan(const u32* blockcnt, int nblocks, int step, u32* blockoff, u32* counts) {
    if (threadIdx.x != 0) return;
    u32 s = 0;
    for (int b = 0; b < nblocks; ++b) { blockoff[b] = s; s += blockcnt[b]; }
    counts[0] = s;
    counts[1] = s / (u32)step;
}

__global__ __launch_bounds__(256) void k_icp_scatter(const u32* z, int npx, const unsigned long long* zsum, int x0, int y0, int bw,
                                                     float fx, float fy, float cx, float cy, int step, const u32* blockoff,
                                                     const u32* counts, float* out) {
    __shared__ u32 wave_cnt[kIcpTile / 64];
    const double mean = (double)*zsum / (double)npx;
    const int k = blockIdx.x * kIcpTile + threadIdx.x;
    const bool keep = k < npx && keep_z(z[k], mean);
    const unsigned long long b = __ballot(keep);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wave_cnt[w] = (u32)__popcll(b);
    __syncthreads();
    if (!keep) return;
    u32 j = blockoff[blockIdx.x] + (u32)__popcll(b & ((1ull << lane) - 1ull));
    for (int i = 0; i < w; ++i) j += wave_cnt[i];
    if (j % (u32)step != 0 || j / (u32)step >= counts[1]) return;
    const float zf = (float)z[k];
    const float u = (float)(x0 + k % bw), v = (float)(y0 + k / bw);
    float* o = out + 6 * (size_t)(j / (u32)step);
    o[0] = zf == 0.0f ? 0.0f : ((u - cx) / fx) * zf;
    o[1] = zf == 0.0f ? 0.0f : ((v - cy) / fy) * zf;
    o[2] = zf;
}

// Normal of every scene point: its 12 nearest neighbours (float squared distance, ties to the lower index, itself included) through
// LDS tiles of candidates, a sorted 12-entry list in registers, the mean-centred covariance in double, Jacobi, oriented to n . p <= 0.
__global__ __launch_bounds__(256) void k_icp_normals(float* cloud, const u32* counts) {
    __shared__ float tile[kIcpTile][3];
    const int n = (int)counts[1];
    const int i = blockIdx.x * kIcpTile + threadIdx.x;
    if (blockIdx.x * kIcpTile >= n) return;                      // block-uniform
    float px = 0, py = 0, pz = 0;
    if (i < n) { px = cloud[6 * (size_t)i]; py = cloud[6 * (size_t)i + 1]; pz = cloud[6 * (size_t)i + 2]; }
    float bd[kIcpK];
    int bi[kIcpK];
#pragma unroll
    for (int k = 0; k < kIcpK; ++k) { bd[k] = INFINITY; bi[k] = -1; }
    for (int t0 = 0; t0 < n; t0 += kIcpTile) {
        const int j = t0 + threadIdx.x;
        __syncthreads();
        if (j < n) { tile[threadIdx.x][0] = cloud[6 * (size_t)j]; tile[threadIdx.x][1] = cloud[6 * (size_t)j + 1]; tile[threadIdx.x][2] = cloud[6 * (size_t)j + 2]; }
        __syncthreads();
        const int m = min(kIcpTile, n - t0);
        for (int c = 0; c < m; ++c) {
            const float dx = tile[c][0] - px, dy = tile[c][1] - py, dz = tile[c][2] - pz;
            float cd = dx * dx + dy * dy + dz * dz;
            if (!(cd < bd[kIcpK - 1])) continue;
            int ci = t0 + c;
#pragma unroll
            for (int k = 0; k < kIcpK; ++k) {
                // (d, index) order: the carried entry may tie an entry further down and has the lower index (ties to the lower index)
                if (cd < bd[k] || (cd == bd[k] && (unsigned)ci < (unsigned)bi[k])) {
                    const float td = bd[k]; const int ti = bi[k]; bd[k] = cd; bi[k] = ci; cd = td; ci = ti;
                }
            }
        }
    }
    if (i >= n) return;
    double mx = 0, my = 0, mz = 0;
    int kk = 0;
#pragma unroll
    for (int k = 0; k < kIcpK; ++k)
        if (bi[k] >= 0) { mx += cloud[6 * (size_t)bi[k]]; my += cloud[6 * (size_t)bi[k] + 1]; mz += cloud[6 * (size_t)bi[k] + 2]; ++kk; }
    mx /= kk; my /= kk; mz /= kk;
    double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
#pragma unroll
    for (int k = 0; k < kIcpK; ++k) {
        if (bi[k] < 0) continue;
        const double dx = cloud[6 * (size_t)bi[k]] - mx, dy = cloud[6 * (size_t)bi[k] + 1] - my, dz = cloud[6 * (size_t)bi[k] + 2] - mz;
        c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
    }
    double nv[3];
    smallest_eigvec(c00, c01, c02, c11, c12, c22, nv);
    if (nv[0] * px + nv[1] * py + nv[2] * pz > 0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
    float* o = cloud + 6 * (size_t)i;
    o[3] = (float)nv[0]; o[4] = (float)nv[1]; o[5] = (float)nv[2];
}

// ---- ICP.  One block per pose: meanAvg, scale (fixed-order LDS reductions), the normalised model src0 and the state of the pose.
__global__ __launch_bounds__(256) void k_icp_normalise(const float* model, int nm, const float* scene, int ns, LmIcpPose* st, double* src0) {
    __shared__ double red[kIcpTile][4];
    LmIcpPose& p = st[blockIdx.y];
    double* out = src0 + (size_t)blockIdx.y * nm * 6;
    double P[12];
    for (int k = 0; k < 12; ++k) P[k] = p.P[k];
    const int t = threadIdx.x;
    auto reduce = [&](double a, double b, double c, double d, double* res) {
        red[t][0] = a; red[t][1] = b; red[t][2] = c; red[t][3] = d;
        __syncthreads();
        for (int o = kIcpTile / 2; o > 0; o >>= 1) {
            if (t < o) for (int q = 0; q < 4; ++q) red[t][q] += red[t + o][q];
            __syncthreads();
        }
        for (int q = 0; q < 4; ++q) res[q] = red[0][q];
        __syncthreads();
    };
    double s[4] = {0, 0, 0, 0}, r[4];
    for (int i = t; i < nm; i += kIcpTile) {
        double m[3] = {model[6 * (size_t)i], model[6 * (size_t)i + 1], model[6 * (size_t)i + 2]}, y[3];
        xform_p(P, m, y);
        s[0] += y[0]; s[1] += y[1]; s[2] += y[2];
    }
    reduce(s[0], s[1], s[2], 0, r);
    double ms[3] = {r[0] / nm, r[1] / nm, r[2] / nm};
    s[0] = s[1] = s[2] = 0;
    for (int j = t; j < ns; j += kIcpTile) { s[0] += scene[6 * (size_t)j]; s[1] += scene[6 * (size_t)j + 1]; s[2] += scene[6 * (size_t)j + 2]; }
    reduce(s[0], s[1], s[2], 0, r);
    double mu[3];
    for (int c = 0; c < 3; ++c) mu[c] = 0.5 * (ms[c] + r[c] / ns);
    s[0] = s[1] = 0;
    for (int i = t; i < nm; i += kIcpTile) {
        double m[3] = {model[6 * (size_t)i], model[6 * (size_t)i + 1], model[6 * (size_t)i + 2]}, y[3];
        xform_p(P, m, y);
        const double a = y[0] - mu[0], b = y[1] - mu[1], c = y[2] - mu[2];
        s[0] += sqrt(a * a + b * b + c * c);
    }
    for (int j = t; j < ns; j += kIcpTile) {
        const double a = scene[6 * (size_t)j] - mu[0], b = scene[6 * (size_t)j + 1] - mu[1], c = scene[6 * (size_t)j + 2] - mu[2];
        s[1] += sqrt(a * a + b * b + c * c);
    }
    reduce(s[0], s[1], 0, 0, r);
    const double scale = (double)nm / (0.5 * (r[0] + r[1]));
    for (int i = t; i < nm; i += kIcpTile) {
        double m[3] = {model[6 * (size_t)i], model[6 * (size_t)i + 1], model[6 * (size_t)i + 2]};
        double nn[3] = {model[6 * (size_t)i + 3], model[6 * (size_t)i + 4], model[6 * (size_t)i + 5]}, y[3], yn[3];
        xform_p(P, m, y);
        xform_n(P, nn, yn);
        double* o = out + 6 * (size_t)i;
        for (int c = 0; c < 3; ++c) { o[c] = (y[c] - mu[c]) * scale; o[3 + c] = yn[c]; }
    }
    if (t == 0) {
        for (int c = 0; c < 3; ++c) p.mean_avg[c] = mu[c];
        p.scale = scale;
        set_identity(p.pose);
        set_identity(p.posex);
        p.done = 1;
    }
}

// Start of a level: srcL = every s-th row of pose . src0 (normals rotated), and the level's state of the pose reset.
__global__ __launch_bounds__(256) void k_icp_level_src(LmIcpPose* st, const double* src0, int nm, int s, int nL, int max_it, double* srcL) {
    LmIcpPose& p = st[blockIdx.y];
    const int i = blockIdx.x * kIcpTile + threadIdx.x;
    if (i < nL) {
        const double* x = src0 + ((size_t)blockIdx.y * nm + (size_t)i * s) * 6;
        double* y = srcL + ((size_t)blockIdx.y * nm + i) * 6;
        xform_p(p.pose, x, y);
        xform_n(p.pose, x + 3, y + 3);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        set_identity(p.posex);
        p.fval_old = kFvalStart;
        p.fval_perc = 0.0;
        p.it = 0;
        p.done = max_it > 0 ? 0 : 1;
    }
}

// Exact 1-NN of moved = posex . srcL among dstL (rows 0, s, 2s, ... of the normalised scene): grid = src tile x dst chunk x pose,
// the chunk's dst points through LDS, strict < in ascending order (ties to the lower index).  Result per (pose, chunk, src point).
__global__ __launch_bounds__(256) void k_icp_nn(const LmIcpPose* st, const double* srcL, int nm, int nL, const float* scene, int s, int ndL,
                                                int chunk, LmIcpNN* part) {
    __shared__ double tile[kIcpTile][3];
    const LmIcpPose& p = st[blockIdx.z];
    if (p.done) return;                                           // block-uniform
    const int i = blockIdx.x * kIcpTile + threadIdx.x;
    double m[3] = {0, 0, 0};
    if (i < nL) xform_p(p.posex, srcL + ((size_t)blockIdx.z * nm + i) * 6, m);
    const int j0 = blockIdx.y * chunk, j1 = min(ndL, j0 + chunk);
    double best = INFINITY;
    int bj = -1;
    for (int t0 = j0; t0 < j1; t0 += kIcpTile) {
        __syncthreads();
        const int j = t0 + threadIdx.x;
        if (j < j1) dst_pos(scene, j * s, p, tile[threadIdx.x]);
        __syncthreads();
        const int cnt = min(kIcpTile, j1 - t0);
        for (int c = 0; c < cnt; ++c) {
            const double dx = m[0] - tile[c][0], dy = m[1] - tile[c][1], dz = m[2] - tile[c][2];
            const double d = dx * dx + dy * dy + dz * dz;
            if (d < best) { best = d; bj = t0 + c; }
        }
    }
    if (i < nL) {
        LmIcpNN& r = part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * nm + i];
        r.d = best; r.j = bj;
    }
}

// Lower median of the float keys (values >= 0: their bits order like unsigned ints): 4 radix passes of 8 bits in LDS.
template <typename F>
__device__ float radix_select(int m, int k, F value) {
    __shared__ u32 hist[256];
    __shared__ u32 sh_prefix, sh_k;
    u32 prefix = 0, mask = 0;
    if (threadIdx.x == 0) sh_k = (u32)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = threadIdx.x; b < 256; b += blockDim.x) hist[b] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += blockDim.x) {
            const u32 v = __float_as_uint(value(i));
            if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            u32 kk = sh_k, b = 0;
            while (b < 255 && kk >= hist[b]) { kk -= hist[b]; ++b; }
            sh_k = kk;
            sh_prefix = prefix | (b << shift);
        }
        __syncthreads();
        prefix = sh_prefix;
        mask |= 255u << shift;
    }
    return __uint_as_float(prefix);
}

// One block per pose: merge the chunk minima (ties to the lower chunk = lower index), float distances, median and MAD, the rejection
// threshold, and the picky table of the round cleared.
__global__ __launch_bounds__(1024) void k_icp_select(LmIcpPose* st, const LmIcpNN* part, int nchunks, int nm, int nL, float* nd, int* nidx,
                                                     unsigned long long* keys, int ns, double rejection_scale) {
    LmIcpPose& p = st[blockIdx.x];
    if (p.done) return;
    float* d = nd + (size_t)blockIdx.x * nm;
    int* ix = nidx + (size_t)blockIdx.x * nm;
    for (int i = threadIdx.x; i < nL; i += blockDim.x) {
        double best = INFINITY;
        int bj = -1;
        for (int c = 0; c < nchunks; ++c) {
            const LmIcpNN& r = part[((size_t)blockIdx.x * nchunks + c) * nm + i];
            if (r.d < best) { best = r.d; bj = r.j; }
        }
        d[i] = (float)best;
        ix[i] = bj;
    }
    unsigned long long* kp = keys + (size_t)blockIdx.x * ns;
    for (int j = threadIdx.x; j < ns; j += blockDim.x) kp[j] = ~0ull;
    __syncthreads();
    const int k = (nL - 1) / 2;
    const float med = radix_select(nL, k, [&](int i) { return d[i]; });
    const float mad = radix_select(nL, k, [&](int i) { return fabsf(d[i] - med); });
    if (threadIdx.x == 0) p.thr = rejection_scale * kMadScale * (double)mad + (double)med;
}

// Picky step: per dst point the kept pair of the smallest distance, ties to the lower src index: 64-bit atomicMin of (d bits, src index).
__global__ __launch_bounds__(256) void k_icp_picky(const LmIcpPose* st, const float* nd, const int* nidx, int nm, int nL, unsigned long long* keys, int ns) {
    const LmIcpPose& p = st[blockIdx.y];
    if (p.done) return;
    const int i = blockIdx.x * kIcpTile + threadIdx.x;
    if (i >= nL) return;
    const float d = nd[(size_t)blockIdx.y * nm + i];
    if (!((double)d < p.thr)) return;
    const int j = nidx[(size_t)blockIdx.y * nm + i];
    if (j < 0) return;                                            // no finite distance
    atomicMin(keys + (size_t)blockIdx.y * ns + j, ((unsigned long long)__float_as_uint(d) << 32) | (u32)i);
}

// Normal equations of the point-to-plane step over the pairs (s from srcL, d and n from dstL), one partial of kAcc doubles per block in a
// fixed reduction order; k_icp_solve adds the partials in block order.
__global__ __launch_bounds__(256) void k_icp_accum(const LmIcpPose* st, const unsigned long long* keys, int ns, int ndL, const double* srcL, int nm,
                                                   const float* scene, int s, double* acc) {
    __shared__ double red[kIcpTile / 64][kAcc];
    const LmIcpPose& p = st[blockIdx.y];
    if (p.done) return;
    const int j = blockIdx.x * kIcpTile + threadIdx.x;
    double v[kAcc];
#pragma unroll
    for (int q = 0; q < kAcc; ++q) v[q] = 0;
    if (j < ndL) {
        const unsigned long long key = keys[(size_t)blockIdx.y * ns + j];
        if (key != ~0ull) {
            const int i = (int)(u32)key;
            const double* sp = srcL + ((size_t)blockIdx.y * nm + i) * 6;
            double dp[3];
            dst_pos(scene, j * s, p, dp);
            const float* sc = scene + 6 * (size_t)j * s;
            const double n0 = sc[3], n1 = sc[4], n2 = sc[5];
            double a[6] = {sp[1] * n2 - sp[2] * n1, sp[2] * n0 - sp[0] * n2, sp[0] * n1 - sp[1] * n0, n0, n1, n2};
            const double b = (dp[0] - sp[0]) * n0 + (dp[1] - sp[1]) * n1 + (dp[2] - sp[2]) * n2;
            int q = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) v[q++] = a[r] * a[c];
#pragma unroll
            for (int r = 0; r < 6; ++r) v[21 + r] = a[r] * b;
            v[27] = 1.0;
            const double e0 = sp[0] - dp[0], e1 = sp[1] - dp[1], e2 = sp[2] - dp[2], e3 = sp[3] - n0, e4 = sp[4] - n1, e5 = sp[5] - n2;
            v[28] = e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3 + e4 * e4 + e5 * e5;
        }
    }
#pragma unroll
    for (int q = 0; q < kAcc; ++q)
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_down(v[q], o, 64);
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q < kAcc; ++q) red[threadIdx.x >> 6][q] = v[q];
    __syncthreads();
    if (threadIdx.x < kAcc) {
        double t = 0;
        for (int w = 0; w < kIcpTile / 64; ++w) t += red[w][threadIdx.x];
        acc[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kAcc + threadIdx.x] = t;
    }
}

// One thread per pose: the 6x6 solve (Gaussian elimination, partial pivoting), PoseX, fval and the stop test.  When the level of the pose
// ends (stop test, rounds used up, fewer than 6 pairs, NaN) pose = PoseX . pose and the pose is marked done.
__global__ void k_icp_solve(LmIcpPose* st, int np, const double* acc, int nblk, int nL, int max_it, double tolp) {
    const int pi = blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= np) return;
    LmIcpPose& p = st[pi];
    if (p.done) return;
    double v[kAcc];
    for (int q = 0; q < kAcc; ++q) v[q] = 0;
    for (int b = 0; b < nblk; ++b)
        for (int q = 0; q < kAcc; ++q) v[q] += acc[((size_t)pi * nblk + b) * kAcc + q];
    bool stop = v[27] < 6.0;
    if (!stop) {
        double A[6][7];
        int q = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) { A[r][c] = v[q]; A[c][r] = v[q]; ++q; }
        for (int r = 0; r < 6; ++r) A[r][6] = v[21 + r];
        for (int c = 0; c < 6; ++c) {
            int piv = c;
            for (int r = c + 1; r < 6; ++r) if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
            if (piv != c) for (int k = 0; k < 7; ++k) { const double t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; }
            for (int r = c + 1; r < 6; ++r) {
                const double f = A[r][c] / A[c][c];
                for (int k = c; k < 7; ++k) A[r][k] -= f * A[c][k];
            }
        }
        double x[6];
        for (int r = 5; r >= 0; --r) {
            double t = A[r][6];
            for (int k = r + 1; k < 6; ++k) t -= A[r][k] * x[k];
            x[r] = t / A[r][r];
        }
        for (int k = 0; k < 6; ++k) if (!isfinite(x[k])) stop = true;
        if (!stop) {
            const double cx = cos(x[0]), sx = sin(x[0]), cy = cos(x[1]), sy = sin(x[1]), cz = cos(x[2]), sz = sin(x[2]);
            // Rz . Ry . Rx
            double* M = p.posex;
            M[0] = cz * cy; M[1] = cz * sy * sx - sz * cx; M[2] = cz * sy * cx + sz * sx; M[3] = x[3];
            M[4] = sz * cy; M[5] = sz * sy * sx + cz * cx; M[6] = sz * sy * cx - cz * sx; M[7] = x[4];
            M[8] = -sy;     M[9] = cy * sx;                M[10] = cy * cx;                M[11] = x[5];
            const double fval = sqrt(v[28]) / (double)nL;
            p.fval_perc = fval / p.fval_old;
            p.fval_old = fval;
            p.it += 1;
            stop = (p.fval_perc < 1.0 + tolp && p.fval_perc > 1.0 - tolp) || p.it >= max_it;
        }
    }
    if (stop) {
        compose(p.posex, p.pose, p.pose);
        p.done = 1;
    }
}

// Undo the normalisation and apply the initial pose: out = [R | t / scale + meanAvg - R meanAvg] . P  (4x4 row-major).
__global__ void k_icp_finish(const LmIcpPose* st, int np, double* out) {
    const int pi = blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= np) return;
    const LmIcpPose& p = st[pi];
    double T[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = p.pose[4 * r + c];
        T[4 * r + 3] = p.pose[4 * r + 3] / p.scale + p.mean_avg[r] - (p.pose[4 * r] * p.mean_avg[0] + p.pose[4 * r + 1] * p.mean_avg[1] + p.pose[4 * r + 2] * p.mean_avg[2]);
    }
    double R[12];
    compose(T, p.P, R);
    double* o = out + 16 * (size_t)pi;
    for (int k = 0; k < 12; ++k) o[k] = R[k];
    o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 1;
}

// ---- launchers
static inline unsigned blocks(long long n) { return (unsigned)((n + kIcpTile - 1) / kIcpTile); }

void lmk_icp_scene(hipStream_t st, const u16* depth, int W, int H, int x0, int y0, int bw, int bh, float fx, float fy, float cx, float cy,
                   int step, LmIcpSceneScratch sc, float* out) {
    const int npx = bw * bh;
    const unsigned nb = blocks(npx);
    hipLaunchKernelGGL(k_icp_blur_z, dim3(nb), dim3(kIcpTile), 0, st, depth, W, H, x0, y0, bw, bh, sc.z, sc.zsum);
    hipLaunchKernelGGL(k_icp_keep_count, dim3(nb), dim3(kIcpTile), 0, st, sc.z, npx, sc.zsum, sc.blockcnt);
    hipLaunchKernelGGL(k_icp_scan, dim3(1), dim3(64), 0, st, sc.blockcnt, (int)nb, step, sc.blockoff, sc.counts);
    hipLaunchKernelGGL(k_icp_scatter, dim3(nb), dim3(kIcpTile), 0, st, sc.z, npx, sc.zsum, x0, y0, bw, fx, fy, cx, cy, step, sc.blockoff,
                       sc.counts, out);
    hipLaunchKernelGGL(k_icp_normals, dim3(blocks(npx / step + 1)), dim3(kIcpTile), 0, st, out, sc.counts);
}

int lmk_icp_nn_chunks(int ndL) { return std::max(1, std::min(32, (ndL + 2047) / 2048)); }

void lmk_icp_register(hipStream_t st, const float* model, int nm, const float* scene, int ns, int np, const LmIcpLevel* levels, int nlevels,
                      double rejection_scale, LmIcpScratch w, double* out) {
    hipLaunchKernelGGL(k_icp_normalise, dim3(1, np), dim3(kIcpTile), 0, st, model, nm, scene, ns, w.st, w.src0);
    for (int l = 0; l < nlevels; ++l) {
        const LmIcpLevel& L = levels[l];
        if (L.rounds == 0) continue;                                       // the level never iterates: pose = I . pose
        hipLaunchKernelGGL(k_icp_level_src, dim3(blocks(L.nL), np), dim3(kIcpTile), 0, st, w.st, w.src0, nm, L.s, L.nL, L.rounds, w.srcL);
        const int nchunks = lmk_icp_nn_chunks(L.ndL);
        const int chunk = (L.ndL + nchunks - 1) / nchunks;
        const unsigned nblk = std::max(1u, blocks(L.ndL));
        for (int r = 0; r < L.rounds; ++r) {
            hipLaunchKernelGGL(k_icp_nn, dim3(blocks(L.nL), nchunks, np), dim3(kIcpTile), 0, st, w.st, w.srcL, nm, L.nL, scene, L.s, L.ndL,
                               chunk, w.part);
            hipLaunchKernelGGL(k_icp_select, dim3(np), dim3(1024), 0, st, w.st, w.part, nchunks, nm, L.nL, w.nd, w.nidx, w.keys, ns,
                               rejection_scale);
            hipLaunchKernelGGL(k_icp_picky, dim3(blocks(L.nL), np), dim3(kIcpTile), 0, st, w.st, w.nd, w.nidx, nm, L.nL, w.keys, ns);
            hipLaunchKernelGGL(k_icp_accum, dim3(nblk, np), dim3(kIcpTile), 0, st, w.st, w.keys, ns, L.ndL, w.srcL, nm, scene, L.s, w.acc);
            hipLaunchKernelGGL(k_icp_solve, dim3((np + 63) / 64), dim3(64), 0, st, w.st, np, w.acc, (int)nblk, L.nL, L.rounds, L.tolp);
        }
    }
    hipLaunchKernelGGL(k_icp_finish, dim3((np + 63) / 64), dim3(64), 0, st, w.st, np, out);
}
