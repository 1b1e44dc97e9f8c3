// lm_k_rectify.hip -- lens rectification as a stage of the ingest (lm_ingest_frames_rectified; the rule:
// include/linemod_hip.h): source frames in device memory, as the camera delivered them, resampled through the detector's fixed-point map
// into the slots' resident frames -- crop, mirror and shift of the ingest included, in ONE pass.  A gather: output pixel (x, y) looks up
// its ideal pixel (lmq::place), reads that pixel's map entry (qx, qy) and blends the four source taps around it (colour, lmq::colour_pixel)
// or takes the nearest source pixel (depth, lmq::depth_pixel).  All the arithmetic is lm_rectify.h's, which the host runs too.
// A lane owns FOUR consecutive output pixels of a row: 12 colour bytes (three dword stores) and 8 depth bytes (one dwordx2 store) when
// w % 4 == 0 -- the slots' case, W % 16 == 0 -- so a wave writes 256 consecutive pixels, and its lanes' taps are neighbours in the source
// (a lens map is locally smooth): the loads of one instruction fall into a few cache lines.  Wider runs per lane would spread one load
// instruction's addresses further apart.  Other widths (the stage hook) store byte by byte.  Loads are plain global loads of the taps'
// own bytes, each under its tap's inside-the-source test: nothing outside a source is ever read.
#include "lm_dev_ingest.h"

namespace {

using lmt::GlobalLd;

struct Entry { bool on; int qx, qy; };

// the map entries of the lane's four pixels for one image (colour and depth may have different windows)
__device__ __forceinline__ void entries(const LmIngestArgs& a, const LmIngestDesc& e, const LmIngestImage& im, int x0, int y, Entry (&E)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const lmq::Place p = lmq::place(a.w, a.h, x0 + k, y, e.flip_x != 0, e.shift_x, e.shift_y, im.crop_x, im.crop_y);
        E[k].on = p.on && x0 + k < a.w;
        E[k].qx = E[k].qy = 0;
        if (E[k].on) {
            const int2 q = reinterpret_cast<const int2*>(a.map)[(size_t)p.my * (size_t)a.mw + (size_t)p.mx];
            E[k].qx = q.x; E[k].qy = q.y;
        }
    }
}

// blockIdx.y = frame of the call, blockIdx.x * 256 + threadIdx.x = (row, group of 4 pixels).  Everything read from the descriptor is uniform
// over the workgroup: the format switches are scalar branches.  k_rectify takes the frames whose colour image is RGB in some order (and
// the frames of a depth-only stage call), k_rectify_yuv the grey and YUV ones, k_rectify_bayer the raw Bayer ones (its four taps
// share one 4 x 4 neighbourhood: lmq::colour_pixel_bayer) and k_rectify_raw the high-bit raw ones and the 8-bit Bayer ones under a raw
// pipeline (lmq::colour_pixel_raw: processed taps) and k_rectify_float the float ones (lmf::float_tap: a tap is the converted pixel), as
// k_ingest / k_ingest_yuv / k_ingest_bayer / k_ingest_raw / k_ingest_float are split (lm_ingest_family).
template <int FAMILY>
__device__ __forceinline__ void rectify_lane(const LmIngestArgs& a) {
    const int slot = a.first + (int)blockIdx.y;
    const LmIngestDesc e = a.table[slot];
    if (lm_ingest_family(e.colour.kind) != FAMILY) return;
    const int G = (a.w + 3) >> 2;
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (u32)G * (u32)a.h) return;
    const int y = (int)(i / (u32)G), x0 = ((int)i - y * G) * 4;
    const bool vec = (a.w & 3) == 0;
    Entry E[4];
    u32 P[4];
    if (a.out_bgr) {
        const lmq::Src s = lmt::make_src(e.colour, e.matrix, a.sw, a.sh);
        entries(a, e, e.colour, x0, y, E);
        lmt::with_kind<FAMILY>(s.kind, [&](auto kind) {
            constexpr int KIND = decltype(kind)::value;
            const lmi::RawPipe pipe = lmt::pipe_of<KIND>(a.raw);
            const auto tone = lmt::tone_of<KIND>(a.raw);
#pragma unroll
            for (int k = 0; k < 4; ++k) P[k] = E[k].on ? lmy::ideal_pixel<KIND>(s, pipe, E[k].qx, E[k].qy, GlobalLd(), tone) : 0u;
        });
        u8* o = a.out_bgr + (size_t)slot * a.out_stride + ((size_t)y * a.w + x0) * 3;
        if (vec) {
            u32* o4 = reinterpret_cast<u32*>(o);
            o4[0] = P[0] | P[1] << 24;
            o4[1] = P[1] >> 8 | P[2] << 16;
            o4[2] = P[2] >> 16 | P[3] << 8;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < a.w) { o[3 * k] = (u8)P[k]; o[3 * k + 1] = (u8)(P[k] >> 8); o[3 * k + 2] = (u8)(P[k] >> 16); }
        }
    }
    if (a.out_depth) {
        const lmq::Src s = lmt::make_src(e.depth, 0, a.sw, a.sh);
        entries(a, e, e.depth, x0, y, E);
#pragma unroll
        for (int k = 0; k < 4; ++k) P[k] = E[k].on ? lmq::depth_pixel(s, E[k].qx, E[k].qy, GlobalLd()) : 0u;
        u8* o = a.out_depth + (size_t)slot * a.out_stride + ((size_t)y * a.w + x0) * 2;
        if (vec) *reinterpret_cast<uint2*>(o) = make_uint2(P[0] | P[1] << 16, P[2] | P[3] << 16);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < a.w) reinterpret_cast<u16*>(o)[k] = (u16)P[k];
        }
    }
}

__global__ __launch_bounds__(256) void k_rectify(LmIngestArgs a) { rectify_lane<LM_INGEST_FAMILY_RGB>(a); }
__global__ __launch_bounds__(256) void k_rectify_yuv(LmIngestArgs a) { rectify_lane<LM_INGEST_FAMILY_YUV>(a); }
__global__ __launch_bounds__(256) void k_rectify_bayer(LmIngestArgs a) { rectify_lane<LM_INGEST_FAMILY_BAYER>(a); }
__global__ __launch_bounds__(256) void k_rectify_raw(LmIngestArgs a) { rectify_lane<LM_INGEST_FAMILY_RAW>(a); }
__global__ __launch_bounds__(256) void k_rectify_float(LmIngestArgs a) { rectify_lane<LM_INGEST_FAMILY_FLOAT>(a); }

}  // namespace

void lmk_rectify(hipStream_t s, const LmIngestArgs& a) {
    if (a.n <= 0 || a.w <= 0 || a.h <= 0) return;
    const u32 lanes = (u32)((a.w + 3) >> 2) * (u32)a.h;
    const dim3 grid((lanes + 255u) / 256u, (u32)a.n);
    if (a.n_family[LM_INGEST_FAMILY_RGB] > 0 && lmk_count_launch(LM_INGEST_FAMILY_RGB)) hipLaunchKernelGGL(k_rectify, grid, dim3(256), 0, s, a);
    if (a.n_family[LM_INGEST_FAMILY_YUV] > 0 && lmk_count_launch(LM_INGEST_FAMILY_YUV)) hipLaunchKernelGGL(k_rectify_yuv, grid, dim3(256), 0, s, a);
    if (a.n_family[LM_INGEST_FAMILY_BAYER] > 0 && lmk_count_launch(LM_INGEST_FAMILY_BAYER)) hipLaunchKernelGGL(k_rectify_bayer, grid, dim3(256), 0, s, a);
    if (a.n_family[LM_INGEST_FAMILY_RAW] > 0 && lmk_count_launch(LM_INGEST_FAMILY_RAW)) hipLaunchKernelGGL(k_rectify_raw, grid, dim3(256), 0, s, a);
    if (a.n_family[LM_INGEST_FAMILY_FLOAT] > 0 && lmk_count_launch(LM_INGEST_FAMILY_FLOAT)) hipLaunchKernelGGL(k_rectify_float, grid, dim3(256), 0, s, a);
}
