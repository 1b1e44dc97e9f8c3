// lm_k_rectify_reduce.hip -- lens rectification AND area-averaged reduction as ONE stage of the ingest (lm_ingest_frames_rectified_reduced,
// DESIGN.md section 19; the rule: include/linemod_hip.h): source frames in device memory at the camera's resolution and through the
// camera's lens, into the slots' resident frames.  The rule is cv::remap followed by cv::resize(INTER_AREA): the rectified image Rc of the
// whole IDEAL geometry (section 17), box-filtered by the reduction's ratio (section 18) -- but Rc never exists in memory.  It is
// k_reduce_conv's tiled form with another phase A (one "source pixel" is expensive here: a map entry, four taps each converted by its
// format's rule, a blend; and a reduced pixel's neighbours share their border pixels):
//   A  the patch of IDEAL pixels under the tile (lmx::plan_tile, at most sw x sh of them): consecutive lanes on consecutive ideal pixels
//      of a row read their map entries (int2), form the Rc pixel with lm_rectify.h's colour_pixel / colour_pixel_bayer /
//      colour_pixel_raw -- the functions k_rectify calls -- and store it ONCE into LDS as B | G << 8 | R << 16;
//   B, C  lm_dev_reduce.h's hsum and vsum, shared with k_reduce_conv: horizontal sums carried unrounded, vertical sums, the one division.
// Depth is never blended: a lane takes its own pixel straight from memory before the colour work -- the reduction's rule (nearest /
// minimum of the valid) over the ideal pixels, each through its map entry and lmq::depth_pixel (lm_rectify_reduce.h).
// The taps of an ideal pixel may lie outside the source (an ideal camera may see more than the lens delivers): every tap stays under
// its inside-the-source test, so nothing outside a source is ever read; the map is read inside the ideal geometry alone.
// Four kernels by lm_ingest_family, as k_rectify's: the conversions' registers and code stay out of the plain kernel.
#include "lm_dev_reduce.h"
#include "lm_rectify_reduce.h"

namespace {

using lmq::addr_t;
using lmt::GlobalLd;
using lmt::GlobalTone;
using lmt::Run;

__device__ __forceinline__ lmq::Src make_src(const LmIngestImage& im, int matrix, int sw, int sh) {
    lmq::Src s;
    s.data = (addr_t)im.data; s.row_stride = im.row_stride; s.plane_stride = im.plane_stride;
    s.width = sw; s.height = sh;
    s.kind = im.kind; s.swap_rb = im.swap_rb; s.matrix = matrix;
    s.dwords = im.aligned != 0; s.scale = im.scale;
    return s;
}

// phase A: Rc of the ideal pixels (sx0 .. sx0 + SW - 1, sy0 .. sy0 + SH - 1) into C[SH][SW].  (idx + 0.5) / SW in float is the exact row
// for idx < 2^20.  NB pixels per lane and round, their map entries loaded together; six cover the 73 x 19 patch of 9/4 in ONE round (the
// bound is the vector arithmetic per ideal pixel, DESIGN.md section 19: a lane past the patch's end does none, and whole waves skip).
// The patch lies inside the ideal geometry (the window lies inside the reduced ideal geometry, and a span ends inside the ideal one);
// the clamp is a no-op that keeps the map's read inside the table whatever the arguments.
template <int KIND, int NB, class Tone>
__device__ __forceinline__ void stage(const lmq::Src& s, const lmi::RawPipe& p, Tone tone, const int2* map, int mw, int mh, int sx0, int sy0, int SW, int SH,
                                      u32* C) {
    const float inv = 1.0f / (float)SW;
    const int n = SW * SH;
    for (int base = (int)threadIdx.x; base < n; base += 256 * NB) {
        int2 q[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int at = base + 256 * k, idx = at < n ? at : n - 1;
            const int r = (int)(((float)idx + 0.5f) * inv), c = idx - lmi::mul24(r, SW);
            int x = sx0 + c, y = sy0 + r;
            x = x < mw - 1 ? x : mw - 1; x = x > 0 ? x : 0;
            y = y < mh - 1 ? y : mh - 1; y = y > 0 ? y : 0;
            q[k] = map[(size_t)lmi::umul24((u32)y, (u32)mw) + (size_t)x];
        }
#pragma unroll
        for (int k = 0; k < NB; ++k)
            if (base + 256 * k < n) C[base + 256 * k] = lmy::ideal_pixel<KIND>(s, p, q[k].x, q[k].y, GlobalLd(), tone);
    }
}

// The tile's column and row and the frame of the call come from the grid in one of two orders (a.frame_fast; DESIGN.md section 19 has both
// measured): blockIdx.y = frame, or blockIdx.x = frame so that the workgroups that read one patch of the map run together.  Everything
// read from the descriptor is uniform over the workgroup: the format switches are scalar branches and the barriers sit under uniform
// conditions.
template <int FAMILY>
__device__ __forceinline__ void rectify_reduce_block(const LmRectifyReduceArgs& a, u32* lds) {
    constexpr bool YUV = FAMILY == LM_INGEST_FAMILY_YUV, BAYER = FAMILY == LM_INGEST_FAMILY_BAYER, RAW = FAMILY == LM_INGEST_FAMILY_RAW;
    const int frame = a.frame_fast ? (int)blockIdx.x : (int)blockIdx.y, bx = a.frame_fast ? (int)blockIdx.y : (int)blockIdx.x;
    if (frame >= a.n) return;
    const int slot = a.first + frame;
    const LmIngestDesc e = a.table[slot];
    if (lm_ingest_family(e.colour.kind) != FAMILY) return;
    const int tw = a.tile.tw, th = a.tile.th, ltw = 31 - __clz(tw);
    const int x0 = bx << ltw, y0 = (int)blockIdx.z * th;
    const int tid = (int)threadIdx.x, lx = tid & (tw - 1), ly = tid >> ltw;
    const int x = x0 + lx, y = y0 + ly;
    const bool mine = ly < th && x < a.w && y < a.h;
    const bool flip = e.flip_x != 0;
    const int2* map = reinterpret_cast<const int2*>(a.map);
    // the depth pixel first: its loads are in flight while the colour phases run, the store comes last
    u32 depth_v = 0u;
    if (a.out_depth && mine) {
        const lmq::Place p = lmq::place(a.w, a.h, x, y, flip, e.shift_x, e.shift_y, e.depth.crop_x, e.depth.crop_y);
        if (p.on) {
            const lmq::Src s = make_src(e.depth, 0, a.sw, a.sh);
            const lmy::Map m = {a.map, a.mw, a.mh};
            depth_v = a.depth_rule == LM_REDUCE_DEPTH_MIN_VALID ? lmy::depth_min_valid(s, m, a.depth, p.mx, p.my, GlobalLd())
                                                                : lmy::depth_nearest(s, m, a.depth, p.mx, p.my, GlobalLd());
        }
    }
    if (a.out_bgr) {
        const lmx::Ratio q = a.colour;
        const Run rx = lmt::tile_run(x0, tw, a.w, e.shift_x, flip, e.colour.crop_x), ry = lmt::tile_run(y0, th, a.h, e.shift_y, false, e.colour.crop_y);
        const lmt::Patch pt = lmt::patch_of(q, rx, ry);
        const bool any = rx.n > 0 && ry.n > 0;
        if (pt.SW > a.tile.sw || pt.SH > a.tile.sh) return;          // (lmx::patch_side bounds both; never taken)
        u32* C = lds;
        u32* H = lds + a.tile.sw * a.tile.sh;
        if (any) {
            const lmq::Src s = make_src(e.colour, e.matrix, a.sw, a.sh);
            const lmi::RawPipe none = lmi::RawPipe();
            if (RAW) {
                const lmi::RawPipe pipe = lmt::load_pipe(a.raw);
                stage<LM_INGEST_RAW, 1>(s, pipe, GlobalTone{(addr_t)a.raw->tone}, map, a.mw, a.mh, pt.sx0, pt.sy0, pt.SW, pt.SH, C);
            } else if (BAYER) {
                stage<LM_INGEST_BAYER_RGGB, 1>(s, none, lmx::NoTone(), map, a.mw, a.mh, pt.sx0, pt.sy0, pt.SW, pt.SH, C);
            } else if (YUV) {
                switch (s.kind) {
                case LM_INGEST_GRAY8: stage<LM_INGEST_GRAY8, 6>(s, none, lmx::NoTone(), map, a.mw, a.mh, pt.sx0, pt.sy0, pt.SW, pt.SH, C); break;
                case LM_INGEST_NV12: stage<LM_INGEST_NV12, 6>(s, none, lmx::NoTone(), map, a.mw, a.mh, pt.sx0, pt.sy0, pt.SW, pt.SH, C); break;
                case LM_INGEST_NV21: stage<LM_INGEST_NV21, 6>(s, none, lmx::NoTone(), map, a.mw, a.mh, pt.sx0, pt.sy0, pt.SW, pt.SH, C); break;
                case LM_INGEST_YUY2: stage<LM_INGEST_YUY2, 6>(s, none, lmx::NoTone(), map, a.mw, a.mh, pt.sx0, pt.sy0, pt.SW, pt.SH, C); break;
                default: stage<LM_INGEST_UYVY, 6>(s, none, lmx::NoTone(), map, a.mw, a.mh, pt.sx0, pt.sy0, pt.SW, pt.SH, C); break;
                }
            } else {
                switch (s.kind) {
                case LM_INGEST_PX3: stage<LMQ_PX3, 6>(s, none, lmx::NoTone(), map, a.mw, a.mh, pt.sx0, pt.sy0, pt.SW, pt.SH, C); break;
                case LM_INGEST_PX4: stage<LMQ_PX4, 6>(s, none, lmx::NoTone(), map, a.mw, a.mh, pt.sx0, pt.sy0, pt.SW, pt.SH, C); break;
                default: stage<LMQ_PLANAR, 6>(s, none, lmx::NoTone(), map, a.mw, a.mh, pt.sx0, pt.sy0, pt.SW, pt.SH, C); break;
                }
            }
            __syncthreads();
            lmt::hsum(q, rx, pt.sx0, pt.SW, pt.SH, tw, ltw, tid, C, H);          // phase B
            __syncthreads();
        }
        if (mine) {
            u32 P = 0u;
            const lmq::Place p = lmq::place(a.w, a.h, x, y, flip, e.shift_x, e.shift_y, e.colour.crop_x, e.colour.crop_y);
            if (p.on) P = lmt::vsum(q, rx, ry, pt.sy0, ltw, p.mx, p.my, H);          // phase C
            u8* o = a.out_bgr + (size_t)slot * a.out_stride + (size_t)lmi::umul24((u32)y, (u32)a.w) * 3 + (size_t)(3 * x);
            o[0] = (u8)P; o[1] = (u8)(P >> 8); o[2] = (u8)(P >> 16);
        }
    }
    if (a.out_depth && mine) reinterpret_cast<u16*>(a.out_depth + (size_t)slot * a.out_stride)[lmi::umul24((u32)y, (u32)a.w) + (u32)x] = (u16)depth_v;
}

__global__ __launch_bounds__(256) void k_rectify_reduce(LmRectifyReduceArgs a) {
    extern __shared__ u32 lds[];
    rectify_reduce_block<LM_INGEST_FAMILY_RGB>(a, lds);
}
__global__ __launch_bounds__(256) void k_rectify_reduce_yuv(LmRectifyReduceArgs a) {
    extern __shared__ u32 lds[];
    rectify_reduce_block<LM_INGEST_FAMILY_YUV>(a, lds);
}
__global__ __launch_bounds__(256) void k_rectify_reduce_bayer(LmRectifyReduceArgs a) {
    extern __shared__ u32 lds[];
    rectify_reduce_block<LM_INGEST_FAMILY_BAYER>(a, lds);
}
__global__ __launch_bounds__(256) void k_rectify_reduce_raw(LmRectifyReduceArgs a) {
    extern __shared__ u32 lds[];
    rectify_reduce_block<LM_INGEST_FAMILY_RAW>(a, lds);
}

}  // namespace

void lmk_rectify_reduce(hipStream_t s, LmRectifyReduceArgs& a) {
    if (a.n <= 0 || a.w <= 0 || a.h <= 0) return;
    a.tile = lmx::plan_tile(a.colour);
    const u32 cols = (u32)((a.w + a.tile.tw - 1) / a.tile.tw), rows = (u32)((a.h + a.tile.th - 1) / a.tile.th);
    if (a.frame_fast && cols > 65535u) a.frame_fast = 0;          // (a grid's y holds 65535 blocks; a slot is far narrower)
    const dim3 grid = a.frame_fast ? dim3((u32)a.n, cols, rows) : dim3(cols, (u32)a.n, rows);
    const u32 lds = a.out_bgr ? a.tile.lds_bytes : 0u;
    if (a.n_rgb > 0) hipLaunchKernelGGL(k_rectify_reduce, grid, dim3(256), lds, s, a);
    if (a.n_yuv > 0) hipLaunchKernelGGL(k_rectify_reduce_yuv, grid, dim3(256), lds, s, a);
    if (a.n_bayer > 0) hipLaunchKernelGGL(k_rectify_reduce_bayer, grid, dim3(256), lds, s, a);
    if (a.n_raw > 0) hipLaunchKernelGGL(k_rectify_reduce_raw, grid, dim3(256), lds, s, a);
}
