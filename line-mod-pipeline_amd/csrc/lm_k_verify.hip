// lm_k_verify.hip -- the best-pose check of the ICP branch on the GPU (HighLevelLinemodIcp::estimateBestMatch's
// meanDepthDifference): per query, the pixels where the pose's render and the scene are both valid, eroded 3x3 twice, counted, and the
// sum of |scene - render| over them.  Host side: lm_detector_icp.hip (lm_icp_verify*); the render is lm_k_gen.hip's z-buffer.
//   m0(x, y) = render > 1 && scene > scene_min;  mask = erode3(erode3(m0)), a neighbour outside the image counting as set (cv::erode's
//   default border value).  On a rectangle that is "every in-image pixel of the 5x5 window is set in m0", which is what the kernel computes.
// One pass, no mask image: a block's m0 lives in wave ballots.  A wave reads 64 consecutive pixels of a row, two of them halo on either
// side; the ballot of m0 is the row segment's bit mask, the horizontal 5-tap AND is four shifts of it (exact for the 60 inner bits),
// the vertical one an AND of five such words from LDS.  Sums are integers: per block 32-bit, one atomic per block and counter.
#include "lm_dev.h"
#include "lm_kernels.h"

namespace {

constexpr int kVerCols = 60;                 // output columns of a tile: lanes 2 .. 61 of the 64 read
constexpr int kVerRows = 16;                 // output rows of a tile
constexpr int kVerHalo = 2;                  // two erosions
constexpr int kVerIn = kVerRows + 2 * kVerHalo;
constexpr int kVerWaves = 4;

// grid (pixel tiles, query); tiles run row-major, tiles_x to a row.  Query q's render is view q: a z-buffer (FromZ: u32, gen_z_to_mm)
// or a depth image (u16); its scene is scenes + scene_idx[q] * scene_stride.  out[q] = {u32 count, u32 unused, u64 sum}, zero on entry.
template <bool FromZ>
__global__ __launch_bounds__(64 * kVerWaves) void k_icp_verify(const void* renders, const u16* scenes, const int* scene_idx, size_t scene_stride,
                                                               int w, int h, int tiles_x, int scene_min, u32* out) {
    const int q = blockIdx.y;
    const size_t npx = (size_t)w * h;
    const u16* sc = scenes + (size_t)scene_idx[q] * scene_stride;
    const u32* zr = reinterpret_cast<const u32*>(renders) + (size_t)q * npx;
    const u16* hr = reinterpret_cast<const u16*>(renders) + (size_t)q * npx;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kVerCols, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kVerRows;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ unsigned long long hrow[kVerIn];      // per input row: m0 ANDed over x - 2 .. x + 2 (bits 2 .. 61 hold columns x0 .. x0 + 59)
    __shared__ u16 adiff[kVerRows][64];              // |scene - render| of the output rows
    __shared__ u32 part[kVerWaves][2];

    const int x = x0 - kVerHalo + lane;
    const bool xin = x >= 0 && x < w;
    for (int j = wv; j < kVerIn; j += kVerWaves) {
        const int y = y0 - kVerHalo + j;
        bool set = true;                              // outside the image: set
        int ad = 0;
        if (xin && y >= 0 && y < h) {
            const size_t p = (size_t)y * w + x;
            const int r = FromZ ? (int)gen_z_to_mm(zr[p]) : (int)hr[p];
            const int s = sc[p];
            set = r > 1 && s > scene_min;
            ad = s > r ? s - r : r - s;
        }
        const unsigned long long m = __ballot(set);
        if (lane == 0) hrow[j] = m & (m >> 1) & (m >> 2) & (m << 1) & (m << 2);
        if (j >= kVerHalo && j < kVerHalo + kVerRows) adiff[j - kVerHalo][lane] = (u16)ad;
    }
    __syncthreads();

    const int ncol = min(kVerCols, w - x0);          // >= 1: the grid covers the image exactly
    const unsigned long long cols = ((1ull << ncol) - 1ull) << kVerHalo;
    u32 cnt = 0, sum = 0;                             // cnt is wave-uniform; sum per lane: at most 4 x 65535
    for (int r = wv; r < kVerRows && y0 + r < h; r += kVerWaves) {
        const unsigned long long v = hrow[r] & hrow[r + 1] & hrow[r + 2] & hrow[r + 3] & hrow[r + 4] & cols;
        cnt += (u32)__popcll(v);
        if ((v >> lane) & 1ull) sum += adiff[r][lane];
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    if (lane == 0) { part[wv][0] = cnt; part[wv][1] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 c = 0, s = 0;                             // a tile's sum: at most 960 x 65535 < 2^32
        for (int k = 0; k < kVerWaves; ++k) { c += part[k][0]; s += part[k][1]; }
        if (c) {
            atomicAdd(&out[4 * (size_t)q], c);
            atomicAdd(reinterpret_cast<unsigned long long*>(&out[4 * (size_t)q + 2]), (unsigned long long)s);
        }
    }
}

}  // namespace

void lmk_icp_verify(hipStream_t s, bool from_z, const void* renders, const u16* scenes, const int* scene_idx, size_t scene_stride, int nq, int w,
                    int h, int scene_min, u32* out) {
    const int tiles_x = (w + kVerCols - 1) / kVerCols, tiles_y = (h + kVerRows - 1) / kVerRows;
    const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)nq), block(64 * kVerWaves);
    if (from_z)
        hipLaunchKernelGGL(k_icp_verify<true>, grid, block, 0, s, renders, scenes, scene_idx, scene_stride, w, h, tiles_x, scene_min, out);
    else
        hipLaunchKernelGGL(k_icp_verify<false>, grid, block, 0, s, renders, scenes, scene_idx, scene_stride, w, h, tiles_x, scene_min, out);
}
