// lm_k_icp.hip -- ICP pose refinement (HighLevelLinemodIcp): the scene cloud of prepareDepthForIcp and the
// rounds of ICP::registerModelToScene, batched over every query of a chunk and every pose of its queries.
// Host side: lm_detector_icp.hip; the chunks, scratch offsets, level records and grids: lm_host.h plan_icp_batch / plan_icp_levels.
//   scene cloud  k_icp_blur_z -> k_icp_keep_count -> k_icp_scan -> k_icp_scatter -> k_icp_normals, the query = blockIdx.y
//   per pose     k_icp_normalise, then per level k_icp_level_src and per round k_icp_nn -> k_icp_select -> k_icp_picky -> k_icp_accum
//                -> k_icp_solve, and k_icp_finish.  The pose index runs over the chunk; a pose carries its query (LmIcpPose::q).  Every
//                round of every level is enqueued up front, as many as the chunk's longest query runs: a pose whose level is done (the
//                stop test, fewer than 6 pairs, a NaN, or its own query's rounds used up) returns at once from the remaining kernels.
// A grid is sized for the chunk's largest query.  A workgroup outside its own query's extent returns at once, block-uniformly, and
// every decomposition that enters a sum or a tie -- the 1-NN chunks, the partials of the normal equations, the tiles of the normals --
// is derived from the query's own record, never from gridDim: a pose's bytes do not depend on the company its query keeps.
// Positions of the scene cloud are float and bit-identical to the numpy restatement (tests/icp_reference.py): -ffp-contract=off and
// the same operation order.  Everything of the ICP is double except the 1-NN distances handed to the median, which are float.
#include "lm_dev.h"
#include "lm_kernels.h"
#include "lm_host.h"

#include <algorithm>

namespace {

constexpr int kIcpTile = LM_ICP_TILE;
constexpr int kIcpK = 12;                      // neighbours of a normal (computeNormalsPC3d(..., 12, ...))
constexpr double kMadScale = 1.48257968;
constexpr double kFvalStart = 9999999999.0;
constexpr int kAcc = LM_ICP_ACC;               // A^T A upper triangle (21) | A^T b (6) | pair count | sum of squared 6-column differences

template <typename T>
__device__ __forceinline__ T* at(u8* base, u64 off) { return reinterpret_cast<T*>(base + off); }

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
__global__ __launch_bounds__(256) void k_icp_blur_z(const LmIcpSceneRec* recs, u8* base, int W, int H, unsigned long long* zsum) {
    const LmIcpSceneRec& q = recs[blockIdx.y];
    if ((int)blockIdx.x >= q.nb) return;                         // block-uniform: a tile past this query's pixels
    const u16* depth = q.depth;
    u32* z = at<u32>(base, q.z);
    const int bw = q.bw;
    const int k = blockIdx.x * kIcpTile + threadIdx.x;
    unsigned long long v = 0;
    if (k < q.npx) {
        const int u = q.x0 + k % bw, r = q.y0 + k / bw;
        u32 s = 0;
        for (int dy = -1; dy <= 1; ++dy) {
            const u16* row = depth + (size_t)reflect101(r + dy, H) * W;
            for (int dx = -1; dx <= 1; ++dx) s += row[reflect101(u + dx, W)];
        }
        v = (s + 4) / 9;
        z[k] = (u32)v;
    }
    block_add_u64(v, zsum + blockIdx.y);
}

// (the mean divides by the query's own pixel count)
__global__ __launch_bounds__(256) void k_icp_keep_count(const LmIcpSceneRec* recs, u8* base, const unsigned long long* zsum) {
    __shared__ u32 cnt;
    const LmIcpSceneRec& q = recs[blockIdx.y];
    if ((int)blockIdx.x >= q.nb) return;                         // block-uniform
    const u32* z = at<u32>(base, q.z);
    const int npx = q.npx;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const double mean = (double)zsum[blockIdx.y] / (double)npx;
    const int k = blockIdx.x * kIcpTile + threadIdx.x;
    const bool keep = k < npx && keep_z(z[k], mean);
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) atomicAdd(&cnt, (u32)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0) at<u32>(base, q.blockcnt)[blockIdx.x] = cnt;
}

// exclusive scan of a query's block counts (a few hundred) by one thread: deterministic and far below a microsecond per hundred blocks
__global__ void k_icp_scan(const LmIcpSceneRec* recs, u8* base, int step, u32* counts) {
    if (threadIdx.x != 0) return;
    const LmIcpSceneRec& q = recs[blockIdx.x];
    const u32* blockcnt = at<u32>(base, q.blockcnt);
    u32* blockoff = at<u32>(base, q.blockoff);
    u32 s = 0;
    for (int b = 0; b < q.nb; ++b) { blockoff[b] = s; s += blockcnt[b]; }
    counts[2 * blockIdx.x] = s;
    counts[2 * blockIdx.x + 1] = s / (u32)step;
}

__global__ __launch_bounds__(256) void k_icp_scatter(const LmIcpSceneRec* recs, u8* base, const unsigned long long* zsum, int step,
                                                     const u32* counts) {
    __shared__ u32 wave_cnt[kIcpTile / 64];
    const LmIcpSceneRec& q = recs[blockIdx.y];
    if ((int)blockIdx.x >= q.nb) return;                         // block-uniform
    const u32* z = at<u32>(base, q.z);
    const int npx = q.npx, bw = q.bw;
    const float fx = q.fx, fy = q.fy, cx = q.cx, cy = q.cy;
    const double mean = (double)zsum[blockIdx.y] / (double)npx;
    const int k = blockIdx.x * kIcpTile + threadIdx.x;
    const bool keep = k < npx && keep_z(z[k], mean);
    const unsigned long long b = __ballot(keep);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wave_cnt[w] = (u32)__popcll(b);
    __syncthreads();
    if (!keep) return;
    u32 j = at<u32>(base, q.blockoff)[blockIdx.x] + (u32)__popcll(b & ((1ull << lane) - 1ull));
    for (int i = 0; i < w; ++i) j += wave_cnt[i];
    if (j % (u32)step != 0 || j / (u32)step >= counts[2 * blockIdx.y + 1]) return;
    const float zf = (float)z[k];
    const float u = (float)(q.x0 + k % bw), v = (float)(q.y0 + k / bw);
    float* o = at<float>(base, q.cloud) + 6 * (size_t)(j / (u32)step);
    o[0] = zf == 0.0f ? 0.0f : ((u - cx) / fx) * zf;
    o[1] = zf == 0.0f ? 0.0f : ((v - cy) / fy) * zf;
    o[2] = zf;
}

// Normal of every scene point: its 12 nearest neighbours (float squared distance, ties to the lower index, itself included) through
// LDS tiles of candidates, a sorted 12-entry list in registers, the mean-centred covariance in double, Jacobi, oriented to n . p <= 0.
// The tiles walked are the query's own cloud's.
__global__ __launch_bounds__(256) void k_icp_normals(const LmIcpSceneRec* recs, u8* base, const u32* counts) {
    __shared__ float tile[kIcpTile][3];
    float* cloud = at<float>(base, recs[blockIdx.y].cloud);
    const int n = (int)counts[2 * blockIdx.y + 1];
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
__global__ __launch_bounds__(256) void k_icp_normalise(const LmIcpRegRec* recs, u8* base, LmIcpPose* st) {
    __shared__ double red[kIcpTile][4];
    LmIcpPose& p = st[blockIdx.y];
    const LmIcpRegRec& q = recs[p.q];
    const float* model = q.model;
    const float* scene = at<float>(base, q.cloud);
    const int nm = q.nm, ns = q.ns;
    double* out = at<double>(base, q.src0) + (size_t)p.li * nm * 6;
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
// A pose whose own query never iterates at this level is left as it is (done, pose = I . pose): the reset follows the query's rounds.
__global__ __launch_bounds__(256) void k_icp_level_src(const LmIcpRegRec* recs, const LmIcpLevel* lev, int nlevels, int l, u8* base, LmIcpPose* st) {
    LmIcpPose& p = st[blockIdx.y];
    const LmIcpLevel& L = lev[p.q * nlevels + l];
    if (L.rounds == 0) return;                                    // block-uniform
    const LmIcpRegRec& q = recs[p.q];
    const int nm = q.nm, s = L.s;
    const int i = blockIdx.x * kIcpTile + threadIdx.x;
    if (i < L.nL) {
        const double* x = at<double>(base, q.src0) + ((size_t)p.li * nm + (size_t)i * s) * 6;
        double* y = at<double>(base, q.srcL) + ((size_t)p.li * nm + i) * 6;
        xform_p(p.pose, x, y);
        xform_n(p.pose, x + 3, y + 3);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        set_identity(p.posex);
        p.fval_old = kFvalStart;
        p.fval_perc = 0.0;
        p.it = 0;
        p.done = 0;
    }
}

// Exact 1-NN of moved = posex . srcL among dstL (rows 0, s, 2s, ... of the normalised scene): grid = src tile x dst chunk x pose,
// the chunk's dst points through LDS, strict < in ascending order (ties to the lower index).  Result per (pose, chunk, src point).
// The chunks are the query's own lm_icp_nn_chunks(ndL) of ceil(ndL / chunks) rows: a launch's grid.y is the chunk's largest.
__global__ __launch_bounds__(256) void k_icp_nn(const LmIcpRegRec* recs, const LmIcpLevel* lev, int nlevels, int l, u8* base, const LmIcpPose* st) {
    __shared__ double tile[kIcpTile][3];
    const LmIcpPose& p = st[blockIdx.z];
    if (p.done) return;                                           // block-uniform
    const LmIcpLevel& L = lev[p.q * nlevels + l];
    const int nL = L.nL, ndL = L.ndL, s = L.s;
    const int nchunks = lm_icp_nn_chunks(ndL);
    if ((int)(blockIdx.x * kIcpTile) >= nL || (int)blockIdx.y >= nchunks) return;   // block-uniform: outside this query's extent
    const LmIcpRegRec& q = recs[p.q];
    const int nm = q.nm;
    const float* scene = at<float>(base, q.cloud);
    const int chunk = (ndL + nchunks - 1) / nchunks;
    const int i = blockIdx.x * kIcpTile + threadIdx.x;
    double m[3] = {0, 0, 0};
    if (i < nL) xform_p(p.posex, at<double>(base, q.srcL) + ((size_t)p.li * nm + i) * 6, m);
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
        LmIcpNN& r = at<LmIcpNN>(base, q.part)[((size_t)p.li * q.nch_cap + blockIdx.y) * nm + i];
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
__global__ __launch_bounds__(1024) void k_icp_select(const LmIcpRegRec* recs, const LmIcpLevel* lev, int nlevels, int l, u8* base, LmIcpPose* st,
                                                     double rejection_scale) {
    LmIcpPose& p = st[blockIdx.x];
    if (p.done) return;
    const LmIcpRegRec& q = recs[p.q];
    const LmIcpLevel& L = lev[p.q * nlevels + l];
    const int nm = q.nm, ns = q.ns, nL = L.nL;
    const int nchunks = lm_icp_nn_chunks(L.ndL);                 // exactly the chunks k_icp_nn wrote for this query, lower chunk first
    const LmIcpNN* part = at<LmIcpNN>(base, q.part) + (size_t)p.li * q.nch_cap * nm;
    float* d = at<float>(base, q.nd) + (size_t)p.li * nm;
    int* ix = at<int>(base, q.nidx) + (size_t)p.li * nm;
    for (int i = threadIdx.x; i < nL; i += blockDim.x) {
        double best = INFINITY;
        int bj = -1;
        for (int c = 0; c < nchunks; ++c) {
            const LmIcpNN& r = part[(size_t)c * nm + i];
            if (r.d < best) { best = r.d; bj = r.j; }
        }
        d[i] = (float)best;
        ix[i] = bj;
    }
    unsigned long long* kp = at<unsigned long long>(base, q.keys) + (size_t)p.li * ns;
    for (int j = threadIdx.x; j < ns; j += blockDim.x) kp[j] = ~0ull;
    __syncthreads();
    const int k = (nL - 1) / 2;
    const float med = radix_select(nL, k, [&](int i) { return d[i]; });
    const float mad = radix_select(nL, k, [&](int i) { return fabsf(d[i] - med); });
    if (threadIdx.x == 0) p.thr = rejection_scale * kMadScale * (double)mad + (double)med;
}

// Picky step: per dst point the kept pair of the smallest distance, ties to the lower src index: 64-bit atomicMin of (d bits, src index).
__global__ __launch_bounds__(256) void k_icp_picky(const LmIcpRegRec* recs, const LmIcpLevel* lev, int nlevels, int l, u8* base, const LmIcpPose* st) {
    const LmIcpPose& p = st[blockIdx.y];
    if (p.done) return;
    const LmIcpRegRec& q = recs[p.q];
    const int nm = q.nm, nL = lev[p.q * nlevels + l].nL;
    const int i = blockIdx.x * kIcpTile + threadIdx.x;
    if (i >= nL) return;
    const float d = at<float>(base, q.nd)[(size_t)p.li * nm + i];
    if (!((double)d < p.thr)) return;
    const int j = at<int>(base, q.nidx)[(size_t)p.li * nm + i];
    if (j < 0) return;                                            // no finite distance
    atomicMin(at<unsigned long long>(base, q.keys) + (size_t)p.li * q.ns + j, ((unsigned long long)__float_as_uint(d) << 32) | (u32)i);
}

// Normal equations of the point-to-plane step over the pairs (s from srcL, d and n from dstL), one partial of kAcc doubles per block in a
// fixed reduction order; k_icp_solve adds the partials in block order.
// A query has max(1, ceil(ndL / 256)) partials of its own; the launch's grid.x is the chunk's largest.
__global__ __launch_bounds__(256) void k_icp_accum(const LmIcpRegRec* recs, const LmIcpLevel* lev, int nlevels, int l, u8* base, const LmIcpPose* st) {
    __shared__ double red[kIcpTile / 64][kAcc];
    const LmIcpPose& p = st[blockIdx.y];
    if (p.done) return;
    const LmIcpLevel& L = lev[p.q * nlevels + l];
    const int ndL = L.ndL, s = L.s;
    if ((int)blockIdx.x >= max(1, (ndL + kIcpTile - 1) / kIcpTile)) return;   // block-uniform: past this query's partials
    const LmIcpRegRec& q = recs[p.q];
    const int nm = q.nm;
    const float* scene = at<float>(base, q.cloud);
    const int j = blockIdx.x * kIcpTile + threadIdx.x;
    double v[kAcc];
#pragma unroll
    for (int q = 0; q < kAcc; ++q) v[q] = 0;
    if (j < ndL) {
        const unsigned long long key = at<unsigned long long>(base, q.keys)[(size_t)p.li * q.ns + j];
        if (key != ~0ull) {
            const int i = (int)(u32)key;
            const double* sp = at<double>(base, q.srcL) + ((size_t)p.li * nm + i) * 6;
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
        at<double>(base, q.acc)[((size_t)p.li * q.nblk_cap + blockIdx.x) * kAcc + threadIdx.x] = t;
    }
}

// One thread per pose: the 6x6 solve (Gaussian elimination, partial pivoting), PoseX, fval and the stop test.  When the level of the pose
// ends (stop test, rounds used up, fewer than 6 pairs, NaN) pose = PoseX . pose and the pose is marked done.
// The partials summed are the query's own max(1, ceil(ndL / 256)), in block order; the rounds a pose may run are its query's.
__global__ void k_icp_solve(const LmIcpRegRec* recs, const LmIcpLevel* lev, int nlevels, int l, u8* base, LmIcpPose* st, int np) {
    const int pi = blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= np) return;
    LmIcpPose& p = st[pi];
    if (p.done) return;
    const LmIcpRegRec& rec = recs[p.q];
    const LmIcpLevel& L = lev[p.q * nlevels + l];
    const int nblk = max(1, (L.ndL + kIcpTile - 1) / kIcpTile), nL = L.nL, max_it = L.rounds;
    const double tolp = L.tolp;
    const double* acc = at<double>(base, rec.acc) + (size_t)p.li * rec.nblk_cap * kAcc;
    double v[kAcc];
    for (int q = 0; q < kAcc; ++q) v[q] = 0;
    for (int b = 0; b < nblk; ++b)
        for (int q = 0; q < kAcc; ++q) v[q] += acc[(size_t)b * kAcc + q];
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

// ---- launchers: a plan's grids (lm_host.h) with the chunk's pointers; nothing is decided here
void lmk_icp_scene(hipStream_t st, const lmh::IcpChunkPlan& c, const LmIcpBatchArgs& a) {
    const unsigned nq = (unsigned)c.q.size();
    const dim3 px(c.g_px, nq), blk(kIcpTile);
    hipLaunchKernelGGL(k_icp_blur_z, px, blk, 0, st, a.scene, a.base, a.W, a.H, a.zsum);
    hipLaunchKernelGGL(k_icp_keep_count, px, blk, 0, st, a.scene, a.base, a.zsum);
    hipLaunchKernelGGL(k_icp_scan, dim3(nq), dim3(64), 0, st, a.scene, a.base, a.step, a.counts);
    hipLaunchKernelGGL(k_icp_scatter, px, blk, 0, st, a.scene, a.base, a.zsum, a.step, a.counts);
    hipLaunchKernelGGL(k_icp_normals, dim3(c.g_normals, nq), blk, 0, st, a.scene, a.base, a.counts);
}

void lmk_icp_register(hipStream_t st, const lmh::IcpLevelsPlan& plan, const LmIcpBatchArgs& a) {
    const unsigned np = (unsigned)plan.np;
    const dim3 blk(kIcpTile), per_pose((np + 63) / 64);
    hipLaunchKernelGGL(k_icp_normalise, dim3(1, np), blk, 0, st, a.reg, a.base, a.st);
    for (int l = 0; l < plan.nlevels; ++l) {
        const lmh::IcpLevelLaunch& g = plan.level[(size_t)l];
        if (g.rounds == 0) continue;                                       // the level iterates for no query: pose = I . pose
        hipLaunchKernelGGL(k_icp_level_src, dim3(g.g_src, np), blk, 0, st, a.reg, a.lev, a.nlevels, l, a.base, a.st);
        for (int r = 0; r < g.rounds; ++r) {
            hipLaunchKernelGGL(k_icp_nn, dim3(g.g_src, g.g_chunks, np), blk, 0, st, a.reg, a.lev, a.nlevels, l, a.base, a.st);
            hipLaunchKernelGGL(k_icp_select, dim3(np), dim3(1024), 0, st, a.reg, a.lev, a.nlevels, l, a.base, a.st, a.rejection_scale);
            hipLaunchKernelGGL(k_icp_picky, dim3(g.g_src, np), blk, 0, st, a.reg, a.lev, a.nlevels, l, a.base, a.st);
            hipLaunchKernelGGL(k_icp_accum, dim3(g.g_dst, np), blk, 0, st, a.reg, a.lev, a.nlevels, l, a.base, a.st);
            hipLaunchKernelGGL(k_icp_solve, per_pose, dim3(64), 0, st, a.reg, a.lev, a.nlevels, l, a.base, a.st, (int)np);
        }
    }
    hipLaunchKernelGGL(k_icp_finish, per_pose, dim3(64), 0, st, a.st, (int)np, a.out);
}

