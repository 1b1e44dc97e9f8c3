// lm_k_rectify_reduce.hip -- lens rectification AND area-averaged reduction as ONE stage of the ingest (lm_ingest_frames_rectified_reduced,
// DESIGN.md section 19; the rule: include/linemod_hip.h): source frames in device memory at the camera's resolution and through the
// camera's lens, into the slots' resident frames.  The rule is cv::remap followed by cv::resize(INTER_AREA): the rectified image Rc of the
// whole IDEAL geometry (section 17), box-filtered by the reduction's ratio (section 18) -- but Rc never exists in memory.  It is
// k_reduce_conv's tiled form with another phase A (one "source pixel" is expensive here: a map entry, four taps each converted by its
// format's rule, a blend; and a reduced pixel's neighbours share their border pixels):
//   A  the patch of IDEAL pixels under the tile (lmx::plan_tile, at most sw x sh of them): consecutive lanes on consecutive ideal pixels
//      of a row read their map entries (int2), form the Rc pixel with lmy::ideal_pixel -- lm_rectify.h's colour_pixel /
//      colour_pixel_bayer / colour_pixel_raw, as k_rectify does -- and store it ONCE into LDS as B | G << 8 | R << 16: this file's part;
//   B, C  lm_dev_ingest.h's tiled_colour, shared with k_reduce_conv: horizontal sums carried unrounded, vertical sums, the one division.
// Depth is never blended: a lane takes its own pixel straight from memory before the colour work -- the reduction's rule (nearest /
// minimum of the valid) over the ideal pixels, each through its map entry and lmq::depth_pixel (lm_rectify_reduce.h).
// The taps of an ideal pixel may lie outside the source (an ideal camera may see more than the lens delivers): every tap stays under
// its inside-the-source test, so nothing outside a source is ever read; the map is read inside the ideal geometry alone.
// Five kernels by lm_ingest_family, as k_rectify's: the conversions' registers and code stay out of the plain kernel.
#include "lm_dev_ingest.h"

namespace {

using lmt::GlobalLd;

// The tile's column and row and the frame of the call come from the grid in one of two orders (a.frame_fast; DESIGN.md section 19 has both
// measured): blockIdx.y = frame, or blockIdx.x = frame so that the workgroups that read one patch of the map run together.  Everything
// read from the descriptor is uniform over the workgroup: the format switches are scalar branches and the barriers sit under uniform
// conditions.
// Phase A takes NB ideal pixels per lane and round, their map entries loaded together; six cover the 73 x 19 patch of 9/4 in ONE round
// (the bound is the vector arithmetic per ideal pixel, DESIGN.md section 19: a lane past the patch's end does none, and whole waves
// skip); the Bayer and raw conversions' registers leave room for one.
template <int FAMILY>
__device__ __forceinline__ void rectify_reduce_block(const LmIngestArgs& a, u32* lds) {
    constexpr int NB = FAMILY == LM_INGEST_FAMILY_BAYER || FAMILY == LM_INGEST_FAMILY_RAW ? 1 : 6;
    const int frame = a.frame_fast ? (int)blockIdx.x : (int)blockIdx.y, bx = a.frame_fast ? (int)blockIdx.y : (int)blockIdx.x;
    if (frame >= a.n) return;
    const int slot = a.first + frame;
    const LmIngestDesc e = a.table[slot];
    if (lm_ingest_family(e.colour.kind) != FAMILY) return;
    const auto depth = [&](int mx, int my) {
        const lmq::Src s = lmt::make_src(e.depth, 0, a.sw, a.sh);
        const lmy::Map m = {a.map, a.mw, a.mh};
        return a.depth_rule == LM_REDUCE_DEPTH_MIN_VALID ? lmy::depth_min_valid(s, m, a.depth, mx, my, GlobalLd()) : lmy::depth_nearest(s, m, a.depth, mx, my, GlobalLd());
    };
    lmt::tile_frame(a, e, slot, bx, depth, [&](const lmt::TileAt& t) {
        return lmt::tiled_colour(a, e, t, lds, [&](const lmt::Patch& pt, u32* C) {
            const lmq::Src s = lmt::make_src(e.colour, e.matrix, a.sw, a.sh);
            lmt::with_kind<FAMILY>(s.kind, [&](auto kind) {
                constexpr int KIND = decltype(kind)::value;
                const lmi::RawPipe pipe = lmt::pipe_of<KIND>(a.raw);
                const auto tone = lmt::tone_of<KIND>(a.raw);
                lmt::stage<NB>(pt, a.mw, a.mh, C, [&](int x, int y) { return GlobalLd().b64((lmt::addr_t)a.map + 8 * ((size_t)lmi::umul24((u32)y, (u32)a.mw) + (size_t)x)); },
                               [&](u32x2 q) { return lmy::ideal_pixel<KIND>(s, pipe, (int)q.x, (int)q.y, GlobalLd(), tone); });
            });
        });
    });
}

__global__ __launch_bounds__(256) void k_rectify_reduce(LmIngestArgs a) {
    extern __shared__ u32 lds[];
    rectify_reduce_block<LM_INGEST_FAMILY_RGB>(a, lds);
}
__global__ __launch_bounds__(256) void k_rectify_reduce_yuv(LmIngestArgs a) {
    extern __shared__ u32 lds[];
    rectify_reduce_block<LM_INGEST_FAMILY_YUV>(a, lds);
}
__global__ __launch_bounds__(256) void k_rectify_reduce_bayer(LmIngestArgs a) {
    extern __shared__ u32 lds[];
    rectify_reduce_block<LM_INGEST_FAMILY_BAYER>(a, lds);
}
__global__ __launch_bounds__(256) void k_rectify_reduce_raw(LmIngestArgs a) {
    extern __shared__ u32 lds[];
    rectify_reduce_block<LM_INGEST_FAMILY_RAW>(a, lds);
}
__global__ __launch_bounds__(256) void k_rectify_reduce_float(LmIngestArgs a) {
    extern __shared__ u32 lds[];
    rectify_reduce_block<LM_INGEST_FAMILY_FLOAT>(a, lds);
}

}  // namespace

void lmk_rectify_reduce(hipStream_t s, LmIngestArgs& a) {
    if (a.n <= 0 || a.w <= 0 || a.h <= 0) return;
    a.tile = lmx::plan_tile(a.colour);
    const u32 cols = (u32)((a.w + a.tile.tw - 1) / a.tile.tw), rows = (u32)((a.h + a.tile.th - 1) / a.tile.th);
    if (a.frame_fast && cols > 65535u) a.frame_fast = 0;          // (a grid's y holds 65535 blocks; a slot is far narrower)
    const dim3 grid = a.frame_fast ? dim3((u32)a.n, cols, rows) : dim3(cols, (u32)a.n, rows);
    const u32 lds = a.out_bgr ? a.tile.lds_bytes : 0u;
    if (a.n_family[LM_INGEST_FAMILY_RGB] > 0 && lmk_count_launch(LM_INGEST_FAMILY_RGB)) hipLaunchKernelGGL(k_rectify_reduce, grid, dim3(256), lds, s, a);
    if (a.n_family[LM_INGEST_FAMILY_YUV] > 0 && lmk_count_launch(LM_INGEST_FAMILY_YUV)) hipLaunchKernelGGL(k_rectify_reduce_yuv, grid, dim3(256), lds, s, a);
    if (a.n_family[LM_INGEST_FAMILY_BAYER] > 0 && lmk_count_launch(LM_INGEST_FAMILY_BAYER)) hipLaunchKernelGGL(k_rectify_reduce_bayer, grid, dim3(256), lds, s, a);
    if (a.n_family[LM_INGEST_FAMILY_RAW] > 0 && lmk_count_launch(LM_INGEST_FAMILY_RAW)) hipLaunchKernelGGL(k_rectify_reduce_raw, grid, dim3(256), lds, s, a);
    if (a.n_family[LM_INGEST_FAMILY_FLOAT] > 0 && lmk_count_launch(LM_INGEST_FAMILY_FLOAT)) hipLaunchKernelGGL(k_rectify_reduce_float, grid, dim3(256), lds, s, a);
}
