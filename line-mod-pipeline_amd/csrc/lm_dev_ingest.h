// lm_dev_ingest.h -- what the ingest kernels share on the device: lm_k_ingest.hip, lm_k_rectify.hip (section 17),
// lm_k_reduce.hip (section 18) and lm_k_rectify_reduce.hip (section 19).  The rules are host-and-device headers of their own (lm_ingest_yuv.h,
// lm_ingest_bayer.h, lm_ingest_raw.h, lm_rectify.h, lm_reduce.h, lm_rectify_reduce.h) and take their memory reads as parameters; here is
// what stands between a rule and a kernel, once:
//   the memory reads (GlobalLoad / load_span, GlobalLd, GlobalTone), the raw pipeline's device copy (load_pipe, pipe_of, tone_of), a
//   descriptor's image as a rule's source (make_src), the run-time kind as a template argument (with_kind);
//   the frame of the tiled kernels k_reduce, k_reduce_conv and k_rectify_reduce* (tile_frame: coordinates, the depth pixel first, the
//   stores; tiled_colour: the run of reduced pixels under a tile, the patch under that run, LDS, phase B = hsum, phase C = vsum), which
//   differ in phase A alone -- what a pixel of the patch is and how it gets into LDS (stage: one loop, a fetch and a make step).
// All the arithmetic is the rule headers'.  A new route writes its rule header, its phase A or lane body, and its launcher.
#pragma once
#include "lm_dev.h"
#include "lm_kernels.h"
#include "lm_rectify_reduce.h"

namespace lmt {

using lmq::addr_t;

// ---- memory reads: the address is an integer, and a pointer made from an integer would be a generic one
// 16 bytes at a 16-byte aligned address (global_load_dwordx4): the read lm_ingest_yuv.h's load_span takes as a parameter
struct GlobalLoad {
    __device__ __forceinline__ lmi::Vec16 operator()(addr_t p) const {
        const u32x4 r = *reinterpret_cast<const __attribute__((address_space(1))) u32x4*>(p);
        return lmi::Vec16{r.x, r.y, r.z, r.w};
    }
};
template <int NB>
__device__ __forceinline__ void load_span(addr_t a, addr_t vlo, addr_t vhi, bool aligned, addr_t safe, u32 (&D)[NB / 4]) {
    lmi::load_span<NB>(a, vlo, vhi, aligned, safe, GlobalLoad(), D);
}

// a tap's own bytes: the read lm_rectify.h and lm_reduce.h take as a parameter
struct GlobalLd {
    __device__ __forceinline__ u32 b8(addr_t p) const { return *reinterpret_cast<const __attribute__((address_space(1))) uint8_t*>(p); }
    __device__ __forceinline__ u32 b16(addr_t p) const { return *reinterpret_cast<const __attribute__((address_space(1))) uint16_t*>(p); }
    __device__ __forceinline__ u32 b32(addr_t p) const { return *reinterpret_cast<const __attribute__((address_space(1))) uint32_t*>(p); }
    __device__ __forceinline__ u32x2 b64(addr_t p) const { return *reinterpret_cast<const __attribute__((address_space(1))) u32x2*>(p); }
};

// The tone table of the raw pipeline (lm_ingest_raw.h takes its read as a parameter): bytes of the detector's 4 KB device copy, read
// through the cache (staging it in LDS per workgroup was timed and won nothing: DESIGN.md section 13).  The kinds that have no raw
// pipeline take lmx::NoTone.
struct GlobalTone {
    addr_t t;
    __device__ __forceinline__ u32 operator()(u32 i) const { return *reinterpret_cast<const __attribute__((address_space(1))) uint8_t*>(t + i); }
};

// the device copy of the raw pipeline, without its tone table (uniform: scalar loads)
__device__ __forceinline__ lmi::RawPipe load_pipe(const lm_raw_processing* raw) {
    lmi::RawPipe pipe = lmi::RawPipe();
    pipe.black = raw->black;
#pragma unroll
    for (int k = 0; k < 3; ++k) pipe.gain[k] = raw->gain[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) pipe.ccm[k] = raw->ccm[k];
    return pipe;
}

// what a kind's conversion reads beside its source: the pipeline and the tone table for LM_INGEST_RAW, nothing for every other kind
template <int KIND>
__device__ __forceinline__ lmi::RawPipe pipe_of(const lm_raw_processing* raw) {
    if constexpr (KIND == LM_INGEST_RAW) return load_pipe(raw);
    else return lmi::RawPipe();
}
template <int KIND>
__device__ __forceinline__ auto tone_of(const lm_raw_processing* raw) {
    if constexpr (KIND == LM_INGEST_RAW) return GlobalTone{(addr_t)raw->tone};
    else return lmx::NoTone();
}

// An image of the descriptor as lm_rectify.h's source, w x h: the source camera's size (the rectified routes: every image has it), or the
// image's own src_w x src_h (the reduced route: colour and depth sources may differ in size)
__device__ __forceinline__ lmq::Src make_src(const LmIngestImage& im, int matrix, int w, int h) {
    lmq::Src s;
    s.data = (addr_t)im.data; s.row_stride = im.row_stride; s.plane_stride = im.plane_stride;
    s.width = w; s.height = h;
    s.kind = im.kind; s.swap_rb = im.swap_rb; s.matrix = matrix;
    s.dwords = im.aligned != 0; s.scale = im.scale;
    return s;
}

// The run-time kind of a colour image of FAMILY as a template argument: f(Kind<K>()), K one of lm_rectify.h's tap kinds (the RGB storage
// kinds, the grey and YUV kinds, the eight float kinds LM_INGEST_FLOAT + element * 4 + shape), LM_INGEST_BAYER_RGGB for the four 8-bit Bayer
// kinds or LM_INGEST_RAW for the raw kinds (the rules read pattern and storage from the source's own kind).  The kind is uniform over the workgroup: scalar branches.
template <int K>
struct Kind { static constexpr int value = K; };
template <int FAMILY, class F>
__device__ __forceinline__ void with_kind(int kind, F f) {
    if constexpr (FAMILY == LM_INGEST_FAMILY_RAW) f(Kind<LM_INGEST_RAW>());
    else if constexpr (FAMILY == LM_INGEST_FAMILY_BAYER) f(Kind<LM_INGEST_BAYER_RGGB>());
    else if constexpr (FAMILY == LM_INGEST_FAMILY_FLOAT) {
        switch (kind - LM_INGEST_FLOAT) {
        case 0: f(Kind<LM_INGEST_FLOAT + 0>()); break;
        case 1: f(Kind<LM_INGEST_FLOAT + 1>()); break;
        case 2: f(Kind<LM_INGEST_FLOAT + 2>()); break;
        case 3: f(Kind<LM_INGEST_FLOAT + 3>()); break;
        case 4: f(Kind<LM_INGEST_FLOAT + 4>()); break;
        case 5: f(Kind<LM_INGEST_FLOAT + 5>()); break;
        case 6: f(Kind<LM_INGEST_FLOAT + 6>()); break;
        default: f(Kind<LM_INGEST_FLOAT + 7>()); break;
        }
    } else if constexpr (FAMILY == LM_INGEST_FAMILY_YUV) {
        switch (kind) {
        case LM_INGEST_GRAY8: f(Kind<LM_INGEST_GRAY8>()); break;
        case LM_INGEST_NV12: f(Kind<LM_INGEST_NV12>()); break;
        case LM_INGEST_NV21: f(Kind<LM_INGEST_NV21>()); break;
        case LM_INGEST_YUY2: f(Kind<LM_INGEST_YUY2>()); break;
        default: f(Kind<LM_INGEST_UYVY>()); break;
        }
    } else {
        switch (kind) {
        case LM_INGEST_PX3: f(Kind<LMQ_PX3>()); break;
        case LM_INGEST_PX4: f(Kind<LMQ_PX4>()); break;
        default: f(Kind<LMQ_PLANAR>()); break;
        }
    }
}

// ---- the tiled kernels.  A workgroup owns tile (bx, blockIdx.z) of tw x th slot pixels (a.tile; tw a power of two, tw th <= 256), lane
// tid the pixel (x, y) of it: `mine` when that pixel exists.
struct TileAt {
    int slot, tw, th, ltw, x0, y0, tid, x, y;
    bool mine, flip;
};

__device__ __forceinline__ void store_bgr(const LmIngestArgs& a, const TileAt& t, u32 P) {
    u8* o = a.out_bgr + (size_t)t.slot * a.out_stride + (size_t)lmi::umul24((u32)t.y, (u32)a.w) * 3 + (size_t)(3 * t.x);
    o[0] = (u8)P; o[1] = (u8)(P >> 8); o[2] = (u8)(P >> 16);
}

// the lane's colour pixel: pixel(mx, my) where the slot pixel lies on the image (lmq::place), 0 in the shift's border
template <class Pixel>
__device__ __forceinline__ void lane_colour(const LmIngestArgs& a, const LmIngestDesc& e, const TileAt& t, Pixel pixel) {
    if (!t.mine) return;
    u32 P = 0u;
    const lmq::Place p = lmq::place(a.w, a.h, t.x, t.y, t.flip, e.shift_x, e.shift_y, e.colour.crop_x, e.colour.crop_y);
    if (p.on) P = pixel(p.mx, p.my);
    store_bgr(a, t, P);
}

// The frame: the depth pixel first -- depth(mx, my), never blended; its loads are in flight while the colour phases run, the store comes
// last --, then colour(t), which writes the tile's colour pixels (false: the workgroup leaves at once).  A null plane is not written.
template <class Depth, class Colour>
__device__ __forceinline__ void tile_frame(const LmIngestArgs& a, const LmIngestDesc& e, int slot, int bx, Depth depth, Colour colour) {
    TileAt t;
    t.slot = slot; t.tw = a.tile.tw; t.th = a.tile.th; t.ltw = 31 - __clz(t.tw);
    t.x0 = bx << t.ltw; t.y0 = (int)blockIdx.z * t.th;
    t.tid = (int)threadIdx.x;
    const int ly = t.tid >> t.ltw;
    t.x = t.x0 + (t.tid & (t.tw - 1)); t.y = t.y0 + ly;
    t.mine = ly < t.th && t.x < a.w && t.y < a.h;
    t.flip = e.flip_x != 0;
    u32 depth_v = 0u;
    if (a.out_depth && t.mine) {
        const lmq::Place p = lmq::place(a.w, a.h, t.x, t.y, t.flip, e.shift_x, e.shift_y, e.depth.crop_x, e.depth.crop_y);
        if (p.on) depth_v = depth(p.mx, p.my);
    }
    if (a.out_bgr && !colour(t)) return;
    if (a.out_depth && t.mine) reinterpret_cast<u16*>(a.out_depth + (size_t)slot * a.out_stride)[lmi::umul24((u32)t.y, (u32)a.w) + (u32)t.x] = (u16)depth_v;
}

// the reduced pixels a tile's slot pixels come from along one axis: slot pixels [t0, t0 + tn) clipped to the frame, less the shift,
// mirrored -> [lo, lo + n) in the reduced geometry (n <= 0: the tile lies in the zero border)
struct Run { int lo, n; };
__device__ __forceinline__ Run tile_run(int t0, int tn, int size, int shift, bool flip, int crop) {
    const int end = t0 + tn < size ? t0 + tn : size;
    int s_lo = t0 - shift, s_hi = end - 1 - shift;
    s_lo = s_lo > 0 ? s_lo : 0; s_hi = s_hi < size - 1 ? s_hi : size - 1;
    Run r;
    r.n = s_hi - s_lo + 1;
    r.lo = crop + (flip ? size - 1 - s_hi : s_lo);
    return r;
}

// the pixels under the runs rx, ry: (sx0 .. sx0 + SW - 1, sy0 .. sy0 + SH - 1), all zero when a run is empty
struct Patch { int sx0, sy0, SW, SH; };
__device__ __forceinline__ Patch patch_of(const lmx::Ratio& q, const Run& rx, const Run& ry) {
    Patch p = {0, 0, 0, 0};
    if (rx.n > 0 && ry.n > 0) {
        const lmx::Span fx = lmx::span(rx.lo, q.num_x, q.den_x), lx_ = lmx::span(rx.lo + rx.n - 1, q.num_x, q.den_x);
        const lmx::Span fy = lmx::span(ry.lo, q.num_y, q.den_y), ly_ = lmx::span(ry.lo + ry.n - 1, q.num_y, q.den_y);
        p.sx0 = fx.first; p.SW = lx_.first + lx_.count - p.sx0;
        p.sy0 = fy.first; p.SH = ly_.first + ly_.count - p.sy0;
    }
    return p;
}

// phase A: the patch's pixels into C[SH][SW], B | G << 8 | R << 16 each: consecutive lanes on consecutive pixels of a row, NB pixels per
// lane and round.  fetch(x, y) is what pixel (x, y) loads first -- the loads of a round are issued together -- and make() turns that
// into the pixel.  (idx + 0.5) / SW in float is the exact row for idx < 2^20: the quotient keeps 0.5 / SW away from an integer.  The patch
// lies inside its gw x gh geometry (the window lies inside the reduced geometry, and a span ends inside the one it reduces), so the
// coordinates are clamped -- a no-op that keeps every read inside whatever the arguments -- and the compiler is told so: inside tests
// behind it fold away and nothing stands between the loads.  A lane past the patch's end makes nothing.
template <int NB, class Fetch, class Make>
__device__ __forceinline__ void stage(const Patch& pt, int gw, int gh, u32* C, const Fetch& fetch, const Make& make) {
    const int sx0 = pt.sx0, sy0 = pt.sy0, SW = pt.SW, SH = pt.SH;
    const float inv = 1.0f / (float)SW;
    const int n = SW * SH;
    for (int base = (int)threadIdx.x; base < n; base += 256 * NB) {
        decltype(fetch(0, 0)) v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int at = base + 256 * k, idx = at < n ? at : n - 1;
            const int r = (int)(((float)idx + 0.5f) * inv), c = idx - lmi::mul24(r, SW);
            int x = sx0 + c, y = sy0 + r;
            x = x < gw - 1 ? x : gw - 1; x = x > 0 ? x : 0;
            y = y < gh - 1 ? y : gh - 1; y = y > 0 ? y : 0;
            __builtin_assume(x >= 0 && x < gw && y >= 0 && y < gh);
            v[k] = fetch(x, y);
        }
#pragma unroll
        for (int k = 0; k < NB; ++k)
            if (base + 256 * k < n) C[base + 256 * k] = make(v[k]);
    }
}

// phase B: H[r][col] = sum over the taps of reduced column rx.lo + col in patch row r of C[SH][SW] (B | G << 8 | R << 16 per pixel).  256
// is a multiple of tw: a lane keeps its column, so its span and weights are set up once
__device__ __forceinline__ void hsum(const lmx::Ratio& q, const Run& rx, int sx0, int SW, int SH, int tw, int ltw, int tid, const u32* C, u32* H) {
    const int col = tid & (tw - 1), X = rx.lo + col;
    const lmx::Span sp = lmx::span(X, q.num_x, q.den_x);
    const int a0 = X * q.num_x, b0 = sp.first * q.den_x;
    if (col < rx.n)
        for (int r = tid >> ltw; r < SH; r += 256 >> ltw) {
            const u32* row = C + lmi::mul24(r, SW) + (sp.first - sx0);
            u32 hbr = 0u, hg = 0u;
            for (int k = 0, b = b0; k < sp.count; ++k, b += q.den_x) {
                const u32 px = row[k], w = (u32)lmx::overlap(a0, q.num_x, b, q.den_x);
                hbr += lmi::umul24(w, px & 0xFF00FFu);          // (weights <= 16, sums <= 255 * 128: full-rate 24-bit products)
                hg += lmi::umul24(w, (px >> 8) & 0xFFu);
            }
            *reinterpret_cast<uint2*>(H + 2 * ((r << ltw) + col)) = make_uint2(hbr, hg);
        }
}

// phase C: reduced pixel (mx, my) of the tile's runs from H, as B | G << 8 | R << 16.  The rows under reduced row my, counted from the
// tile's first patch row: (ry.lo num_y) / den_y = sy0 is the one division (uniform), the lane's own offset is small (lmx::small_div)
__device__ __forceinline__ u32 vsum(const lmx::Ratio& q, const Run& rx, const Run& ry, int sy0, int ltw, int mx, int my, const u32* H) {
    const int col = mx - rx.lo, dy = my - ry.lo;
    const int rem = ry.lo * q.num_y - sy0 * q.den_y, v0 = rem + lmi::mul24(dy, q.num_y);
    const float inv_d = 1.0f / (float)q.den_y;
    const int first = lmx::small_div(v0, inv_d), count = lmx::small_div(v0 + q.num_y - 1, inv_d) - first + 1;
    u32 ab = 0u, ag = 0u, ar = 0u;
    for (int k = 0, b = lmi::mul24(first, q.den_y); k < count; ++k, b += q.den_y) {
        const uint2 h2 = *reinterpret_cast<const uint2*>(H + 2 * (((first + k) << ltw) + col));
        const u32 w = (u32)lmx::overlap(v0, q.num_y, b, q.den_y);
        ab += lmi::umul24(w, h2.x & 0xFFFFu); ag += lmi::umul24(w, h2.y); ar += lmi::umul24(w, h2.x >> 16);
    }
    const u32 n = (u32)(q.num_x * q.num_y);
    const float inv_n = 1.0f / (float)n;
    return lmx::finish_fast(ab, n, inv_n) | lmx::finish_fast(ag, n, inv_n) << 8 | lmx::finish_fast(ar, n, inv_n) << 16;
}

// The tiled colour work of tile t (lmx::plan_tile: 32 x 8, smaller for large ratios so that LDS stays bounded): phase_a(patch, C) fills
// C[SH][SW] with the patch under the tile, then phase B, phase C and the store.  Everything the barriers sit under is uniform over the
// workgroup.  lds: a.tile.lds_bytes of them, C in front of H.
template <class PhaseA>
__device__ __forceinline__ bool tiled_colour(const LmIngestArgs& a, const LmIngestDesc& e, const TileAt& t, u32* lds, PhaseA phase_a) {
    const lmx::Ratio q = a.colour;
    const Run rx = tile_run(t.x0, t.tw, a.w, e.shift_x, t.flip, e.colour.crop_x), ry = tile_run(t.y0, t.th, a.h, e.shift_y, false, e.colour.crop_y);
    const Patch pt = patch_of(q, rx, ry);
    if (pt.SW > a.tile.sw || pt.SH > a.tile.sh) return false;          // (lmx::patch_side bounds both; never taken)
    u32* C = lds;
    u32* H = lds + a.tile.sw * a.tile.sh;
    if (rx.n > 0 && ry.n > 0) {
        phase_a(pt, C);
        __syncthreads();
        hsum(q, rx, pt.sx0, pt.SW, pt.SH, t.tw, t.ltw, t.tid, C, H);
        __syncthreads();
    }
    lane_colour(a, e, t, [&](int mx, int my) { return vsum(q, rx, ry, pt.sy0, t.ltw, mx, my, H); });
    return true;
}

}  // namespace lmt
