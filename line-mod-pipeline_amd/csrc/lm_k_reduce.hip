// lm_k_reduce.hip -- the area-averaged reduction as a stage of the ingest (lm_ingest_frames_reduced; the rule:
// include/linemod_hip.h): source frames in device memory at the camera's resolution, box-filtered down by a rational ratio into the
// slots' resident frames -- crop, mirror and shift of the ingest included, in ONE pass.  The traffic is the reverse of k_ingest's: the
// kernel reads ratio_x * ratio_y times what it writes.  A workgroup owns a tile of slot pixels, a lane one of them (lm_dev_ingest.h:
// tile_frame).  Two forms were built for every kind and measured side by side; each kernel keeps the one that was
// faster for its kinds:
//   k_reduce (RGB in some order: a tap is its own bytes, nothing to convert)  a lane walks its own footprint through
//      lmx::colour_pixel_of -- the rule as tests/cpp/reduce_host.cpp runs it on the host.  A footprint's border pixels are fetched by two
//      lanes per axis, from the cache; there is no barrier and no LDS, and that outweighs the second fetch.
//   k_reduce_conv (grey, YUV, Bayer, raw, float: a tap costs a matrix, a demosaic of nine samples, a pipeline, a float conversion per channel)  the tile (lmx::plan_tile: 32 x 8,
//      smaller for large ratios so that LDS stays bounded) works in three phases (lm_dev_ingest.h: tiled_colour):
//      A  the source patch under the tile, at most sw x sh pixels, is loaded with consecutive lanes on consecutive source pixels of a
//         row and CONVERTED ONCE per source pixel into LDS as B | G << 8 | R << 16 -- this file's part;
//      B  per (source row, tile column) the horizontal weighted sum, carried unrounded (<= 255 * 128: blue and red share a word), into LDS;
//      C  per slot pixel the vertical weighted sum of those, the one rounded division, and the store.
// Depth is never blended: a lane takes its pixel's nearest source pixel or the minimum of the valid ones under it, straight from
// memory (no source pixel belongs to two footprints by the centre test), before the colour work so that the two overlap.  All the
// arithmetic is lm_reduce.h's.  Every load is under its pixel's inside-the-source test: nothing outside a source is ever read.
#include "lm_dev_ingest.h"

namespace {

using lmt::GlobalLd;
using lmt::make_src;

// blockIdx.y = frame of the call, blockIdx.x and blockIdx.z = the tile's column and row.  Everything read from the descriptor is uniform
// over the workgroup: the format switches are scalar branches and the barriers sit under uniform conditions.  k_reduce takes the frames whose colour image is
// RGB in some order (and the frames of a depth-only stage call), k_reduce_conv the grey, YUV, Bayer, raw and float ones -- the split of
// k_ingest / k_ingest_yuv: the conversions' registers and code stay out of the plain kernel.  Colour and depth sources have sizes of
// their own here (src_w x src_h of each image).
template <bool CONV>
__device__ __forceinline__ void reduce_block(const LmIngestArgs& a, u32* lds) {
    const int slot = a.first + (int)blockIdx.y;
    const LmIngestDesc e = a.table[slot];
    if ((lm_ingest_family(e.colour.kind) != LM_INGEST_FAMILY_RGB) != CONV) return;
    const lmq::Src s = make_src(e.colour, e.matrix, e.colour.src_w, e.colour.src_h);
    const auto depth = [&](int mx, int my) {
        const lmq::Src sd = make_src(e.depth, 0, e.depth.src_w, e.depth.src_h);
        return a.depth_rule == LM_REDUCE_DEPTH_MIN_VALID ? lmx::depth_min_valid(sd, a.depth, mx, my, GlobalLd()) : lmx::depth_nearest(sd, a.depth, mx, my, GlobalLd());
    };
    lmt::tile_frame(a, e, slot, (int)blockIdx.x, depth, [&](const lmt::TileAt& t) {
        if constexpr (CONV) {
            // k_reduce_conv's phase A: four pixels per lane and round (more cost the conversions' registers their occupancy); a pixel is
            // the converted source pixel, made where it is fetched
            return lmt::tiled_colour(a, e, t, lds, [&](const lmt::Patch& pt, u32* C) {
                const auto fill = [&](auto kind) {
                    constexpr int KIND = decltype(kind)::value;
                    const lmi::RawPipe pipe = lmt::pipe_of<KIND>(a.raw);
                    const auto tone = lmt::tone_of<KIND>(a.raw);
                    lmt::stage<4>(pt, s.width, s.height, C, [&](int x, int y) { return lmx::pixel<KIND>(s, pipe, x, y, GlobalLd(), tone); }, [](u32 v) { return v; });
                };
                if (s.kind >= LM_INGEST_FLOAT) lmt::with_kind<LM_INGEST_FAMILY_FLOAT>(s.kind, fill);      // (four families in one kernel)
                else if (s.kind >= LM_INGEST_RAW) lmt::with_kind<LM_INGEST_FAMILY_RAW>(s.kind, fill);
                else if (s.kind >= LM_INGEST_BAYER_RGGB) lmt::with_kind<LM_INGEST_FAMILY_BAYER>(s.kind, fill);
                else lmt::with_kind<LM_INGEST_FAMILY_YUV>(s.kind, fill);
            });
        } else {
            // k_reduce: a lane walks its own footprint (lmx::colour_pixel_of)
            lmt::lane_colour(a, e, t, [&](int mx, int my) {
                u32 P = 0u;
                lmt::with_kind<LM_INGEST_FAMILY_RGB>(s.kind, [&](auto kind) {
                    P = lmx::colour_pixel_of<decltype(kind)::value>(s, lmi::RawPipe(), a.colour, mx, my, GlobalLd(), lmx::NoTone());
                });
                return P;
            });
            return true;
        }
    });
}

__global__ __launch_bounds__(256) void k_reduce(LmIngestArgs a) {
    extern __shared__ u32 lds[];
    reduce_block<false>(a, lds);
}
__global__ __launch_bounds__(256) void k_reduce_conv(LmIngestArgs a) {
    extern __shared__ u32 lds[];
    reduce_block<true>(a, lds);
}

}  // namespace

void lmk_reduce(hipStream_t s, LmIngestArgs& a) {
    if (a.n <= 0 || a.w <= 0 || a.h <= 0) return;
    a.tile = lmx::plan_tile(a.colour);
    const lmx::Tile planned = a.tile;
    const auto grid = [&a]() { return dim3((u32)((a.w + a.tile.tw - 1) / a.tile.tw), (u32)a.n, (u32)((a.h + a.tile.th - 1) / a.tile.th)); };
    if (a.n_family[LM_INGEST_FAMILY_RGB] > 0 && lmk_count_launch(LM_INGEST_FAMILY_RGB)) {
        a.tile = lmx::Tile{32, 8, 0, 0, 0u};          // (no patch: always a whole 32 x 8 tile)
        hipLaunchKernelGGL(k_reduce, grid(), dim3(256), 0, s, a);
    }
    a.tile = planned;
    const int n_conv = a.n_family[LM_INGEST_FAMILY_YUV] + a.n_family[LM_INGEST_FAMILY_BAYER] + a.n_family[LM_INGEST_FAMILY_RAW] + a.n_family[LM_INGEST_FAMILY_FLOAT];
    if (n_conv > 0 && lmk_count_launch(LMK_LAUNCH_REDUCE_CONV)) hipLaunchKernelGGL(k_reduce_conv, grid(), dim3(256), a.out_bgr ? a.tile.lds_bytes : 0u, s, a);
}
