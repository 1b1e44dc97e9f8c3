// lm_k_reduce.hip -- the area-averaged reduction as a stage of the ingest (lm_ingest_frames_reduced; the rule:
// include/linemod_hip.h): source frames in device memory at the camera's resolution, box-filtered down by a rational ratio into the
// slots' resident frames -- crop, mirror and shift of the ingest included, in ONE pass.  The traffic is the reverse of k_ingest's: the
// kernel reads ratio_x * ratio_y times what it writes.  A workgroup owns a tile of slot pixels, a lane one of them.  Two forms were built
// for every kind and measured side by side; each kernel keeps the one that was faster for its kinds:
//   k_reduce (RGB in some order: a tap is its own bytes, nothing to convert)  a lane walks its own footprint through
//      lmx::colour_pixel_of -- the rule as tests/cpp/reduce_host.cpp runs it on the host.  A footprint's border pixels are fetched by two
//      lanes per axis, from the cache; there is no barrier and no LDS, and that outweighs the second fetch.
//   k_reduce_conv (grey, YUV, Bayer, raw: a tap costs a matrix, a demosaic of nine samples, a pipeline)  the tile (lmx::plan_tile: 32 x 8,
//      smaller for large ratios so that LDS stays bounded) works in three phases:
//      A  the source patch under the tile, at most sw x sh pixels, is loaded with consecutive lanes on consecutive source pixels of a
//         row and CONVERTED ONCE per source pixel into LDS as B | G << 8 | R << 16;
//      B  per (source row, tile column) the horizontal weighted sum, carried unrounded (<= 255 * 128: blue and red share a word), into LDS;
//      C  per slot pixel the vertical weighted sum of those, the one rounded division, and the store.
// Depth is never blended: a lane takes its pixel's nearest source pixel or the minimum of the valid ones under it, straight from
// memory (no source pixel belongs to two footprints by the centre test), before the colour work so that the two overlap.  All the
// arithmetic is lm_reduce.h's.  Every load is under its pixel's inside-the-source test: nothing outside a source is ever read.
#include "lm_dev_reduce.h"

namespace {

using lmq::addr_t;
using lmt::GlobalLd;
using lmt::GlobalTone;
using lmt::Run;
using lmt::tile_run;

__device__ __forceinline__ lmq::Src make_src(const LmIngestImage& im, int matrix) {
    lmq::Src s;
    s.data = (addr_t)im.data; s.row_stride = im.row_stride; s.plane_stride = im.plane_stride;
    s.width = im.src_w; s.height = im.src_h;
    s.kind = im.kind; s.swap_rb = im.swap_rb; s.matrix = matrix;
    s.dwords = im.aligned != 0; s.scale = im.scale;
    return s;
}

// phase A: source pixels (sx0 .. sx0 + SW - 1, sy0 .. sy0 + SH - 1), converted, into C[SH][SW].  (idx + 0.5) / SW in float is the exact
// row for idx < 2^20: the quotient keeps 0.5 / SW away from an integer.  Four pixels per lane and round (more cost the conversions' registers their occupancy), their loads issued together: the
// patch lies inside the source (the window lies inside the reduced geometry, and a span ends inside the source), so the coordinates are
// clamped -- a no-op -- and the compiler is told so: the taps' inside tests fold away and nothing stands between the loads.
template <int KIND, class Tone>
__device__ __forceinline__ void stage(const lmq::Src& s, const lmi::RawPipe& p, Tone tone, int sx0, int sy0, int SW, int SH, u32* C) {
    constexpr int NB = 4;
    const float inv = 1.0f / (float)SW;
    const int n = SW * SH;
    for (int base = (int)threadIdx.x; base < n; base += 256 * NB) {
        u32 v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int at = base + 256 * k, idx = at < n ? at : n - 1;
            const int r = (int)(((float)idx + 0.5f) * inv), c = idx - lmi::mul24(r, SW);
            int x = sx0 + c, y = sy0 + r;
            x = x < s.width - 1 ? x : s.width - 1; x = x > 0 ? x : 0;
            y = y < s.height - 1 ? y : s.height - 1; y = y > 0 ? y : 0;
            __builtin_assume(x >= 0 && x < s.width && y >= 0 && y < s.height);
            v[k] = lmx::pixel<KIND>(s, p, x, y, GlobalLd(), tone);
        }
#pragma unroll
        for (int k = 0; k < NB; ++k)
            if (base + 256 * k < n) C[base + 256 * k] = v[k];
    }
}

// blockIdx.y = frame of the call, blockIdx.x and blockIdx.z = the tile's column and row.  Everything read from the descriptor is uniform
// over the workgroup: the format switches are scalar branches and the barriers sit under uniform conditions.  k_reduce takes the frames whose colour image is
// RGB in some order (and the frames of a depth-only stage call), k_reduce_conv the grey, YUV, Bayer and raw ones -- the split of
// k_ingest / k_ingest_yuv: the conversions' registers and code stay out of the plain kernel.
template <bool CONV>
__device__ __forceinline__ void reduce_block(const LmReduceArgs& a, u32* lds) {
    const int slot = a.first + (int)blockIdx.y;
    const LmIngestDesc e = a.table[slot];
    if ((lm_ingest_family(e.colour.kind) != LM_INGEST_FAMILY_RGB) != CONV) return;
    const int tw = a.tile.tw, th = a.tile.th, ltw = 31 - __clz(tw);
    const int x0 = (int)blockIdx.x << ltw, y0 = (int)blockIdx.z * th;
    const int tid = (int)threadIdx.x, lx = tid & (tw - 1), ly = tid >> ltw;
    const int x = x0 + lx, y = y0 + ly;
    const bool mine = ly < th && x < a.w && y < a.h;
    const bool flip = e.flip_x != 0;
    // the depth pixel first: its loads are in flight while the colour phases run, the store comes last
    u32 depth_v = 0u;
    if (a.out_depth && mine) {
        const lmq::Place p = lmq::place(a.w, a.h, x, y, flip, e.shift_x, e.shift_y, e.depth.crop_x, e.depth.crop_y);
        if (p.on) {
            const lmq::Src s = make_src(e.depth, 0);
            depth_v = a.depth_rule == LM_REDUCE_DEPTH_MIN_VALID ? lmx::depth_min_valid(s, a.depth, p.mx, p.my, GlobalLd())
                                                                : lmx::depth_nearest(s, a.depth, p.mx, p.my, GlobalLd());
        }
    }
    if (!CONV && a.out_bgr) {
        // k_reduce: a lane walks its own footprint (lmx::colour_pixel_of)
        if (mine) {
            u32 P = 0u;
            const lmq::Place p = lmq::place(a.w, a.h, x, y, flip, e.shift_x, e.shift_y, e.colour.crop_x, e.colour.crop_y);
            if (p.on) {
                const lmq::Src s = make_src(e.colour, e.matrix);
                const lmi::RawPipe pipe = lmi::RawPipe();
                if (s.kind == LM_INGEST_PX3) P = lmx::colour_pixel_of<LMQ_PX3>(s, pipe, a.colour, p.mx, p.my, GlobalLd(), lmx::NoTone());
                else if (s.kind == LM_INGEST_PX4) P = lmx::colour_pixel_of<LMQ_PX4>(s, pipe, a.colour, p.mx, p.my, GlobalLd(), lmx::NoTone());
                else P = lmx::colour_pixel_of<LMQ_PLANAR>(s, pipe, a.colour, p.mx, p.my, GlobalLd(), lmx::NoTone());
            }
            u8* o = a.out_bgr + (size_t)slot * a.out_stride + (size_t)lmi::umul24((u32)y, (u32)a.w) * 3 + (size_t)(3 * x);
            o[0] = (u8)P; o[1] = (u8)(P >> 8); o[2] = (u8)(P >> 16);
        }
    } else if (CONV && a.out_bgr) {
        const lmx::Ratio q = a.colour;
        const Run rx = tile_run(x0, tw, a.w, e.shift_x, flip, e.colour.crop_x), ry = tile_run(y0, th, a.h, e.shift_y, false, e.colour.crop_y);
        const lmt::Patch pt = lmt::patch_of(q, rx, ry);
        const bool any = rx.n > 0 && ry.n > 0;
        const int sx0 = pt.sx0, sy0 = pt.sy0, SW = pt.SW, SH = pt.SH;
        if (SW > a.tile.sw || SH > a.tile.sh) return;          // (lmx::patch_side bounds both; never taken)
        u32* C = lds;
        u32* H = lds + a.tile.sw * a.tile.sh;
        if (any) {
            const lmq::Src s = make_src(e.colour, e.matrix);
            lmi::RawPipe pipe = lmi::RawPipe();
            if (s.kind >= LM_INGEST_RAW) {
                pipe = lmt::load_pipe(a.raw);
                stage<LM_INGEST_RAW>(s, pipe, GlobalTone{(addr_t)a.raw->tone}, sx0, sy0, SW, SH, C);
            } else switch (s.kind) {
            case LM_INGEST_GRAY8: stage<LM_INGEST_GRAY8>(s, pipe, lmx::NoTone(), sx0, sy0, SW, SH, C); break;
            case LM_INGEST_NV12: stage<LM_INGEST_NV12>(s, pipe, lmx::NoTone(), sx0, sy0, SW, SH, C); break;
            case LM_INGEST_NV21: stage<LM_INGEST_NV21>(s, pipe, lmx::NoTone(), sx0, sy0, SW, SH, C); break;
            case LM_INGEST_YUY2: stage<LM_INGEST_YUY2>(s, pipe, lmx::NoTone(), sx0, sy0, SW, SH, C); break;
            case LM_INGEST_UYVY: stage<LM_INGEST_UYVY>(s, pipe, lmx::NoTone(), sx0, sy0, SW, SH, C); break;
            default: stage<LM_INGEST_BAYER_RGGB>(s, pipe, lmx::NoTone(), sx0, sy0, SW, SH, C); break;
            }
            __syncthreads();
            lmt::hsum(q, rx, sx0, SW, SH, tw, ltw, tid, C, H);          // phase B
            __syncthreads();
        }
        if (mine) {
            u32 P = 0u;
            const lmq::Place p = lmq::place(a.w, a.h, x, y, flip, e.shift_x, e.shift_y, e.colour.crop_x, e.colour.crop_y);
            if (p.on) P = lmt::vsum(q, rx, ry, sy0, ltw, p.mx, p.my, H);          // phase C
            u8* o = a.out_bgr + (size_t)slot * a.out_stride + (size_t)lmi::umul24((u32)y, (u32)a.w) * 3 + (size_t)(3 * x);
            o[0] = (u8)P; o[1] = (u8)(P >> 8); o[2] = (u8)(P >> 16);
        }
    }
    if (a.out_depth && mine) reinterpret_cast<u16*>(a.out_depth + (size_t)slot * a.out_stride)[lmi::umul24((u32)y, (u32)a.w) + (u32)x] = (u16)depth_v;
}

__global__ __launch_bounds__(256) void k_reduce(LmReduceArgs a) {
    extern __shared__ u32 lds[];
    reduce_block<false>(a, lds);
}
__global__ __launch_bounds__(256) void k_reduce_conv(LmReduceArgs a) {
    extern __shared__ u32 lds[];
    reduce_block<true>(a, lds);
}

}  // namespace

void lmk_reduce(hipStream_t s, LmReduceArgs& a) {
    if (a.n <= 0 || a.w <= 0 || a.h <= 0) return;
    a.tile = lmx::plan_tile(a.colour);
    const lmx::Tile planned = a.tile;
    const auto grid = [&a]() { return dim3((u32)((a.w + a.tile.tw - 1) / a.tile.tw), (u32)a.n, (u32)((a.h + a.tile.th - 1) / a.tile.th)); };
    if (a.n_rgb > 0) {
        a.tile = lmx::Tile{32, 8, 0, 0, 0u};          // (no patch: always a whole 32 x 8 tile)
        hipLaunchKernelGGL(k_reduce, grid(), dim3(256), 0, s, a);
    }
    a.tile = planned;
    if (a.n_conv > 0) hipLaunchKernelGGL(k_reduce_conv, grid(), dim3(256), a.out_bgr ? a.tile.lds_bytes : 0u, s, a);
}
