// lm_k_ingest.hip -- frames that already live in device memory, in the producer's format, into the resident slots (lm_ingest_frames,
// DESIGN.md section 13): crop -> channel order, YUV conversion or Bayer demosaic -> float-to-u16 -> mirror -> shift in ONE pass.
// Per image, output pixel (x, y) of the W x H frame:
//     xs = x - shift_x, ys = y - shift_y;  outside [0, W) x [0, H): 0  (zeros shifted in, as lm_upload_frame_shifted)
//     u  = flip_x ? W - 1 - xs : xs                                    (cv::flip(.., 1) of the cropped window)
//     p  = source pixel (crop_x + u, crop_y + ys);  colour: (B, G, R) of p (grey and YUV sources: lm_ingest_yuv.h's rule; raw Bayer
//          sources: lm_ingest_bayer.h's, which reads p's neighbours in the source too),  depth: to_u16(p)
// A byte-moving, memory-bound pass.  A lane owns 16 output pixels of a row (W % 16 == 0: 48 colour and 32 depth bytes, 16-byte aligned)
// and writes them with dwordx4 stores, the shift's border as zeros -- no memset in front of or behind the kernel.  Whatever flip and
// shift are, the 16 pixels come from 16 CONSECUTIVE source pixels (ascending, or descending when mirrored), so the lane reads one
// contiguous byte span per plane (load_span), turns it into 16 one-pixel registers and reverses, blanks and packs those.
#include <atomic>

#include "lm_dev_ingest.h"

namespace {

using lmi::addr_t;
using lmi::funnel;
using lmi::perm;
using lmt::GlobalLoad;
using lmt::load_span;

// convertTo(CV_16UC1) of a float depth value times `scale` (a choice): ONE single-precision multiply; NaN, +-inf and
// everything <= 0 -> 0, everything >= 65535 -> 65535, otherwise round to nearest, ties to even (v_rndne_f32).
__device__ __forceinline__ u32 to_u16(u32 bits, float scale) {
    const float t = __fmul_rn(__uint_as_float(bits), scale);
    if (!(t > 0.0f) || t == __builtin_inff()) return 0u;
    if (t >= 65535.0f) return 65535u;
    return (u32)__builtin_rintf(t);
}

// P[k] = source pixel k of the lane's span; Q[j] = output pixel j: mirrored (k = 15 - j) or not, pixels outside [klo, khi) blanked
__device__ __forceinline__ void arrange(const u32 (&P)[16], u32 (&Q)[16], bool flip, int klo, int khi) {
    u32 M[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) M[k] = (k >= klo && k < khi) ? P[k] : 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) Q[j] = flip ? M[15 - j] : M[j];
}

__device__ __forceinline__ void store16(u8* p, u32 a, u32 b, u32 c, u32 d) { *reinterpret_cast<uint4*>(p) = make_uint4(a, b, c, d); }

}  // namespace

// blockIdx.y = frame of the call (table entry first + blockIdx.y = its slot), blockIdx.x * 256 + threadIdx.x = (row, group of 16 pixels).
// Everything read from the descriptor is uniform over the workgroup: the format switches are scalar branches.
// Five kernels share this body.  k_ingest (FAMILY = LM_INGEST_FAMILY_RGB) takes the frames whose colour image is RGB in some order,
// k_ingest_yuv the frames whose colour image is grey or YUV (lm_ingest_yuv.h: the conversion's registers and instructions are no business
// of the byte-moving formats), k_ingest_bayer the raw Bayer frames (lm_ingest_bayer.h: a stencil over three source rows, no business of
// either), k_ingest_raw the high-bit raw frames and the 8-bit Bayer frames under a raw pipeline (lm_ingest_raw.h: unpacking, the same stencil
// on N-bit samples, gains, matrix and the tone table, read through `tone`), k_ingest_float the float colour frames (lm_ingest_float.h: one
// span of 32 .. 256 bytes or three planes' spans, every channel through to_u8); each leaves the others' frames at once (lm_ingest_family), and
// the host launches a kernel only when the call has a frame for it.
template <int FAMILY, class Tone>
__device__ __forceinline__ void ingest_lane(const LmIngestArgs& a, Tone tone) {
    constexpr bool YUV = FAMILY == LM_INGEST_FAMILY_YUV, BAYER = FAMILY == LM_INGEST_FAMILY_BAYER, RAW = FAMILY == LM_INGEST_FAMILY_RAW;
    constexpr bool FLOAT = FAMILY == LM_INGEST_FAMILY_FLOAT;
    const int slot = a.first + (int)blockIdx.y;
    const LmIngestDesc e = a.table[slot];
    if (lm_ingest_family(e.colour.kind) != FAMILY) return;
    const addr_t safe = (addr_t)a.out_bgr;          // (the frame arena: 16-byte aligned memory of the detector's own)
    const int G = a.w >> 4;
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (u32)(G * a.h)) return;
    const int y = (int)(i / (u32)G), x0 = ((int)i - y * G) * 16;
    const bool flip = e.flip_x != 0;
    // source pixel k of the span is column uL + k of the window; the lane keeps k in [klo, khi)
    const lmi::Lane L = lmi::lane_window(a.w, a.h, x0, y, flip, e.shift_x, e.shift_y);
    const int ys = L.ys, uL = L.uL, klo = L.klo, khi = L.khi;
    u32 P[16], Q[16];
    {
        const LmIngestImage& c = e.colour;
        const long long row = (long long)(c.crop_y + ys) * c.row_stride, col = c.crop_x + uL;
        const bool al = c.aligned != 0;
        if (RAW) {
            lmi::RawSrc src;
            src.data = (addr_t)c.data; src.row_stride = c.row_stride; src.width = c.src_w; src.height = c.src_h;
            src.crop_x = c.crop_x; src.crop_y = c.crop_y; src.kind = c.kind;
            lmi::raw_lane_pixels(src, lmt::load_pipe(a.raw), L, safe, GlobalLoad(), tone, P);
        } else if (BAYER) {
            lmi::BayerSrc src;
            src.data = (addr_t)c.data; src.row_stride = c.row_stride; src.width = c.src_w; src.height = c.src_h;
            src.crop_x = c.crop_x; src.crop_y = c.crop_y; src.kind = c.kind; src.aligned = al;
            lmi::bayer_lane_pixels(src, L, safe, GlobalLoad(), P);
        } else if (FLOAT) {
            lmf::Src src;
            src.data = (addr_t)c.data; src.row_stride = c.row_stride; src.plane_stride = c.plane_stride;
            src.crop_x = c.crop_x; src.crop_y = c.crop_y; src.kind = c.kind; src.swap_rb = c.swap_rb; src.aligned = al; src.scale = c.scale;
            lmf::float_lane_pixels(src, L, safe, GlobalLoad(), P);
        } else if (YUV) {
            lmi::Src src;
            src.data = (addr_t)c.data; src.row_stride = c.row_stride; src.plane_stride = c.plane_stride;
            src.crop_x = c.crop_x; src.crop_y = c.crop_y; src.kind = c.kind; src.matrix = e.matrix; src.aligned = al;
            lmi::yuv_lane_pixels(src, L, safe, GlobalLoad(), P);
        } else if (c.kind == LM_INGEST_PX3) {
            const addr_t p = (addr_t)c.data + (addr_t)(row + col * 3);
            u32 D[12];
            load_span<48>(p, p + 3 * klo, p + 3 * khi, al, safe, D);
#pragma unroll
            for (int t = 0; t < 4; ++t) {       // four pixels per three dwords (byte 3 of P is dropped below)
                P[4 * t] = D[3 * t];
                P[4 * t + 1] = funnel(D[3 * t + 1], D[3 * t], 3);
                P[4 * t + 2] = funnel(D[3 * t + 2], D[3 * t + 1], 2);
                P[4 * t + 3] = D[3 * t + 2] >> 8;
            }
        } else if (c.kind == LM_INGEST_PX4) {
            const addr_t p = (addr_t)c.data + (addr_t)(row + col * 4);
            load_span<64>(p, p + 4 * klo, p + 4 * khi, al, safe, P);
        } else {
            const addr_t p = (addr_t)c.data + (addr_t)(row + col);
            u32 A[4], B[4], C[4];
            load_span<16>(p, p + klo, p + khi, al, safe, A);
            load_span<16>(p + (addr_t)c.plane_stride, p + (addr_t)c.plane_stride + klo, p + (addr_t)c.plane_stride + khi, al, safe, B);
            load_span<16>(p + 2 * (addr_t)c.plane_stride, p + 2 * (addr_t)c.plane_stride + klo, p + 2 * (addr_t)c.plane_stride + khi, al, safe, C);
#pragma unroll
            for (int t = 0; t < 4; ++t) {       // byte k of the three planes -> pixel k
                const u32 lo = perm(B[t], A[t], 0x05010400u), hi = perm(B[t], A[t], 0x07030602u);
                P[4 * t] = perm(C[t], lo, 0x0c040100u);
                P[4 * t + 1] = perm(C[t], lo, 0x0c050302u);
                P[4 * t + 2] = perm(C[t], hi, 0x0c060100u);
                P[4 * t + 3] = perm(C[t], hi, 0x0c070302u);
            }
        }
        if (!YUV && !BAYER && !RAW && !FLOAT) {
            // (B, G, R, 0) of every pixel: sources in R, G, B order trade bytes 0 and 2
            const u32 sel = c.swap_rb ? 0x0c000102u : 0x0c020100u;
#pragma unroll
            for (int k = 0; k < 16; ++k) P[k] = perm(0u, P[k], sel);
        }
        arrange(P, Q, flip, klo, khi);
        u8* o = a.out_bgr + (size_t)slot * a.out_stride + ((size_t)y * a.w + x0) * 3;
        u32 O[12];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            O[3 * t] = perm(Q[4 * t + 1], Q[4 * t], 0x04020100u);
            O[3 * t + 1] = perm(Q[4 * t + 2], Q[4 * t + 1], 0x05040201u);
            O[3 * t + 2] = perm(Q[4 * t + 3], Q[4 * t + 2], 0x06050402u);
        }
        store16(o, O[0], O[1], O[2], O[3]);
        store16(o + 16, O[4], O[5], O[6], O[7]);
        store16(o + 32, O[8], O[9], O[10], O[11]);
    }
    if (a.out_depth) {
        const LmIngestImage& c = e.depth;
        const long long row = (long long)(c.crop_y + ys) * c.row_stride, col = c.crop_x + uL;
        const bool al = c.aligned != 0;
        if (c.kind == LM_INGEST_U16) {
            const addr_t p = (addr_t)c.data + (addr_t)(row + col * 2);
            u32 D[8];
            load_span<32>(p, p + 2 * klo, p + 2 * khi, al, safe, D);
#pragma unroll
            for (int t = 0; t < 8; ++t) { P[2 * t] = D[t] & 0xFFFFu; P[2 * t + 1] = D[t] >> 16; }
        } else {
            const addr_t p = (addr_t)c.data + (addr_t)(row + col * 4);
            u32 D[16];
            load_span<64>(p, p + 4 * klo, p + 4 * khi, al, safe, D);
#pragma unroll
            for (int k = 0; k < 16; ++k) P[k] = to_u16(D[k], c.scale);
        }
        arrange(P, Q, flip, klo, khi);
        u8* o = a.out_depth + (size_t)slot * a.out_stride + ((size_t)y * a.w + x0) * 2;
        store16(o, Q[0] | (Q[1] << 16), Q[2] | (Q[3] << 16), Q[4] | (Q[5] << 16), Q[6] | (Q[7] << 16));
        store16(o + 16, Q[8] | (Q[9] << 16), Q[10] | (Q[11] << 16), Q[12] | (Q[13] << 16), Q[14] | (Q[15] << 16));
    }
}

__global__ __launch_bounds__(256) void k_ingest(LmIngestArgs a) { ingest_lane<LM_INGEST_FAMILY_RGB>(a, lmx::NoTone()); }
__global__ __launch_bounds__(256) void k_ingest_yuv(LmIngestArgs a) { ingest_lane<LM_INGEST_FAMILY_YUV>(a, lmx::NoTone()); }
__global__ __launch_bounds__(256) void k_ingest_bayer(LmIngestArgs a) { ingest_lane<LM_INGEST_FAMILY_BAYER>(a, lmx::NoTone()); }
__global__ __launch_bounds__(256) void k_ingest_raw(LmIngestArgs a) { ingest_lane<LM_INGEST_FAMILY_RAW>(a, lmt::tone_of<LM_INGEST_RAW>(a.raw)); }
__global__ __launch_bounds__(256) void k_ingest_float(LmIngestArgs a) { ingest_lane<LM_INGEST_FAMILY_FLOAT>(a, lmx::NoTone()); }

static std::atomic<long long> g_launches[LMK_LAUNCH_KINDS];
bool lmk_count_launch(int kind) {
    g_launches[kind].fetch_add(1, std::memory_order_relaxed);
    return true;
}
long long lmk_launch_count(int kind) { return g_launches[kind].load(std::memory_order_relaxed); }

void lmk_ingest(hipStream_t s, const LmIngestArgs& a) {
    if (a.n <= 0) return;
    const u32 lanes = (u32)(a.w >> 4) * (u32)a.h;
    const dim3 grid((lanes + 255u) / 256u, (u32)a.n);
    if (a.n_family[LM_INGEST_FAMILY_RGB] > 0 && lmk_count_launch(LM_INGEST_FAMILY_RGB)) hipLaunchKernelGGL(k_ingest, grid, dim3(256), 0, s, a);
    if (a.n_family[LM_INGEST_FAMILY_YUV] > 0 && lmk_count_launch(LM_INGEST_FAMILY_YUV)) hipLaunchKernelGGL(k_ingest_yuv, grid, dim3(256), 0, s, a);
    if (a.n_family[LM_INGEST_FAMILY_BAYER] > 0 && lmk_count_launch(LM_INGEST_FAMILY_BAYER)) hipLaunchKernelGGL(k_ingest_bayer, grid, dim3(256), 0, s, a);
    if (a.n_family[LM_INGEST_FAMILY_RAW] > 0 && lmk_count_launch(LM_INGEST_FAMILY_RAW)) hipLaunchKernelGGL(k_ingest_raw, grid, dim3(256), 0, s, a);
    if (a.n_family[LM_INGEST_FAMILY_FLOAT] > 0 && lmk_count_launch(LM_INGEST_FAMILY_FLOAT)) hipLaunchKernelGGL(k_ingest_float, grid, dim3(256), 0, s, a);
}
