// lm_k_export.hip -- resident frames out again, with primitives drawn, in the consumer's format (lm_export_frames):
// slot frame -> un-shift / un-mirror -> primitives composited in list order -> channel order or BGR -> YUV -> the caller's memory, in ONE pass.
// The rule is lm_draw.h's (coverage, blend, index mapping, forward YUV): the host test program runs the same functions.
// A workgroup owns one lmw::TILE_W x TILE_H tile of the exported image, a lane a block of 4 x 2 window pixels (W % 16 == 0: a run of four
// lies inside the window or outside it, never across its edge).  Whatever flip and shift are, the four pixels of a row come from four
// CONSECUTIVE frame pixels: three dword loads when the run starts on a multiple of four frame pixels (shift_x % 4 == 0) and lies inside
// the frame, byte loads with zeros for the pixels outside it otherwise.  The eight pixels stay in registers, B | G << 8 | R << 16, in
// FRAME order while the primitives are walked (their coordinates are the frame's) and are mirrored afterwards.  A 2 x 2 chroma block of
// an NV12 destination lies inside one lane's block.  No atomics: every output byte has one writer, and only bytes inside the window are
// written -- dword stores where the address allows, byte stores where it does not.
#include "lm_dev.h"
#include "lm_kernels.h"
#include "lm_ingest_float.h"

namespace {

constexpr int CHUNK = 64;       // records staged per round: 4 KB of LDS

// the frame pixels x .. x + 3 of row y in ascending order, zeros outside the frame.  F: the slot's dense BGR8 frame (16-byte aligned, rows
// of 3 w bytes: a multiple of 48)
__device__ __forceinline__ void load_run(const u8* F, int w, int h, int x, int y, u32 (&P)[4]) {
    P[0] = P[1] = P[2] = P[3] = 0u;
    if (y < 0 || y >= h || x + 3 < 0 || x >= w) return;
    const u8* row = F + (size_t)y * (size_t)w * 3;
    if (x >= 0 && x + 3 < w && (x & 3) == 0) {
        const u32* q = reinterpret_cast<const u32*>(row + 3 * x);
        const u32 d0 = q[0], d1 = q[1], d2 = q[2];
        P[0] = d0 & 0xFFFFFFu;
        P[1] = (d0 >> 24) | (d1 & 0xFFFFu) << 8;
        P[2] = (d1 >> 16) | (d2 & 0xFFu) << 16;
        P[3] = d2 >> 8;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xk = x + k;
        if (xk >= 0 && xk < w) { const u8* p = row + 3 * xk; P[k] = (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16; }
    }
}

// four bytes at p, which lie inside the window: one dword where p is aligned, bytes where it is not
__device__ __forceinline__ void store4(u8* p, u32 v) {
    if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) { *reinterpret_cast<u32*>(p) = v; return; }
    p[0] = (u8)v; p[1] = (u8)(v >> 8); p[2] = (u8)(v >> 16); p[3] = (u8)(v >> 24);
}

__device__ __forceinline__ u32 swap_rb(u32 px) { return (px & 0xFF00u) | ((px >> 16) & 0xFFu) | (px & 0xFFu) << 16; }

// one row of four window pixels Q (B | G << 8 | R << 16, channel order already the destination's) at window position (u, v)
__device__ __forceinline__ void store_row(const LmExportImage& e, int u, int v, const u32 (&Q)[4]) {
    u8* row = e.data + (long long)(e.crop_y + v) * e.row_stride;
    if (e.kind == LM_EXPORT_PX3) {
        u8* p = row + (long long)(e.crop_x + u) * 3;
        const u32 d0 = Q[0] | Q[1] << 24, d1 = Q[1] >> 8 | Q[2] << 16, d2 = Q[2] >> 16 | Q[3] << 8;
        if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
            u32* q = reinterpret_cast<u32*>(p);
            q[0] = d0; q[1] = d1; q[2] = d2;
        } else {
            store4(p, d0); store4(p + 4, d1); store4(p + 8, d2);
        }
    } else if (e.kind == LM_EXPORT_PX4) {
        u8* p = row + (long long)(e.crop_x + u) * 4;
        const u32 A = 0xFF000000u;
        if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) *reinterpret_cast<uint4*>(p) = make_uint4(Q[0] | A, Q[1] | A, Q[2] | A, Q[3] | A);
        else { store4(p, Q[0] | A); store4(p + 4, Q[1] | A); store4(p + 8, Q[2] | A); store4(p + 12, Q[3] | A); }
    } else {        // LM_EXPORT_PLANAR
        u8* p = row + (e.crop_x + u);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s = 8 * c;
            store4(p + (long long)c * e.plane_stride, ((Q[0] >> s) & 0xFFu) | ((Q[1] >> s) & 0xFFu) << 8 | ((Q[2] >> s) & 0xFFu) << 16 | ((Q[3] >> s) & 0xFFu) << 24);
        }
    }
}

// ---- float destinations (k_export_float; the rule: lm_ingest_float.h's from_u8_f32 / from_u8_f16).  N elements of ES bytes at p, a
// multiple of ES, inside the window: the widest stores the address allows -- dwordx4, dwordx2, dwords, and for an odd binary16 address
// single elements.  E[i] holds element i's bits.
template <int ES, int N>
__device__ __forceinline__ void store_elements(u8* p, const u32 (&E)[N]) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (ES == 4) {
        if (N % 4 == 0 && (a & 15u) == 0) {
#pragma unroll
            for (int i = 0; i < N / 4; ++i) reinterpret_cast<uint4*>(p)[i] = make_uint4(E[4 * i], E[4 * i + 1], E[4 * i + 2], E[4 * i + 3]);
        } else if ((a & 7u) == 0) {
#pragma unroll
            for (int i = 0; i < N / 2; ++i) reinterpret_cast<uint2*>(p)[i] = make_uint2(E[2 * i], E[2 * i + 1]);
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) reinterpret_cast<u32*>(p)[i] = E[i];
        }
        return;
    }
    constexpr int ND = N / 2;
    u32 D[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) D[i] = E[2 * i] | E[2 * i + 1] << 16;
    if (ND % 4 == 0 && (a & 15u) == 0) {
#pragma unroll
        for (int i = 0; i < ND / 4; ++i) reinterpret_cast<uint4*>(p)[i] = make_uint4(D[4 * i], D[4 * i + 1], D[4 * i + 2], D[4 * i + 3]);
    } else if ((a & 7u) == 0) {
#pragma unroll
        for (int i = 0; i < ND / 2; ++i) reinterpret_cast<uint2*>(p)[i] = make_uint2(D[2 * i], D[2 * i + 1]);
    } else if ((a & 3u) == 0) {
#pragma unroll
        for (int i = 0; i < ND; ++i) reinterpret_cast<u32*>(p)[i] = D[i];
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) reinterpret_cast<u16*>(p)[i] = (u16)E[i];
    }
}

// one row of four window pixels Q at window position (u, v) of a float destination: 12 or 16 interleaved elements (alpha = 255 through
// the same conversion), or four per plane
template <int ES>
__device__ __forceinline__ void store_row_float(const LmExportImage& e, int u, int v, const u32 (&Q)[4]) {
    const auto conv = [&](u32 c) { return ES == 4 ? lmf::from_u8_f32(c, e.scale) : lmf::from_u8_f16(c, e.scale); };
    u8* row = e.data + (long long)(e.crop_y + v) * e.row_stride;
    if (e.kind == LM_EXPORT_PX3) {
        u32 E[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) { E[3 * i] = conv(Q[i] & 0xFFu); E[3 * i + 1] = conv((Q[i] >> 8) & 0xFFu); E[3 * i + 2] = conv((Q[i] >> 16) & 0xFFu); }
        store_elements<ES, 12>(row + (long long)(e.crop_x + u) * (3 * ES), E);
    } else if (e.kind == LM_EXPORT_PX4) {
        u32 E[16];
        const u32 alpha = conv(255u);
#pragma unroll
        for (int i = 0; i < 4; ++i) { E[4 * i] = conv(Q[i] & 0xFFu); E[4 * i + 1] = conv((Q[i] >> 8) & 0xFFu); E[4 * i + 2] = conv((Q[i] >> 16) & 0xFFu); E[4 * i + 3] = alpha; }
        store_elements<ES, 16>(row + (long long)(e.crop_x + u) * (4 * ES), E);
    } else {        // LM_EXPORT_PLANAR
        u8* p = row + (long long)(e.crop_x + u) * ES;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const u32 E[4] = {conv((Q[0] >> (8 * c)) & 0xFFu), conv((Q[1] >> (8 * c)) & 0xFFu), conv((Q[2] >> (8 * c)) & 0xFFu), conv((Q[3] >> (8 * c)) & 0xFFu)};
            store_elements<ES, 4>(p + (long long)c * e.plane_stride, E);
        }
    }
}

// NV12: the lane's 4 x 2 block (v even, both rows inside the window): two rows of luma, two chroma pairs from the block sums
__device__ __forceinline__ void store_nv12(const LmExportImage& e, int u, int v, const u32 (&Q)[2][4]) {
    const lmw::FwdCoef c = lmw::fwd_coef(e.matrix);
    int sb[2] = {0, 0}, sg[2] = {0, 0}, sr[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        u32 even = 0u, odd = 0u;        // Y0 | Y2 << 16 and Y1 | Y3 << 16 (interleaved by a permute, like the chroma below)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int B = (int)(Q[j][i] & 0xFFu), G = (int)((Q[j][i] >> 8) & 0xFFu), R = (int)((Q[j][i] >> 16) & 0xFFu);
            const u32 yy = (u32)lmw::luma(R, G, B, c) << (8 * (i & 2));
            if (i & 1) odd |= yy; else even |= yy;
            sb[i >> 1] += B; sg[i >> 1] += G; sr[i >> 1] += R;
        }
        store4(e.data + (long long)(e.crop_y + v + j) * e.row_stride + (e.crop_x + u), lmi::perm(odd, even, 0x06020400u));
    }
    // U0 V0 U1 V1, interleaved by a byte permute of (U0, U1) and (V0, V1) and NOT written as u | v << 8: hipcc folds the clamp, the shift
    // and that pack of two neighbouring bytes into v_ashr_pk_u8_i32 and takes the result's upper half for zero, but on the MI355X the
    // instruction leaves the destination's upper 16 bits as they were -- the second pair came out ORed with stale bits
    const u32 uu = (u32)lmw::chroma_u(sr[0], sg[0], sb[0], c) | (u32)lmw::chroma_u(sr[1], sg[1], sb[1], c) << 16;
    const u32 vv = (u32)lmw::chroma_v(sr[0], sg[0], sb[0], c) | (u32)lmw::chroma_v(sr[1], sg[1], sb[1], c) << 16;
    const u32 uv = lmi::perm(vv, uu, 0x06020400u);
    store4(e.data + e.plane_stride + (long long)((e.crop_y + v) >> 1) * e.row_stride + (e.crop_x + u), uv);
}

// blockIdx = (tile column, tile row, frame of the call).  Everything read from the frame's descriptor and the tile's list is uniform over
// the workgroup: the format switches and the primitive loop are scalar branches, and a tile with an empty list (most tiles of most
// frames) never enters the loop: a pure convert-and-copy.
// Two kernels share this body: k_export takes the frames with an 8-bit destination, k_export_float those with a float one (the
// conversions' and the wide stores' registers are no business of the byte-moving formats); each leaves the other's frames at once.
template <bool FLOAT>
__device__ __forceinline__ void export_block(const LmExportArgs& a, lmw::Rec* recs) {
    const int f = (int)blockIdx.z;
    const LmExportImage e = a.images[f];
    if ((e.es != 0) != FLOAT) return;
    const int tid = (int)threadIdx.x;
    const int u0 = (int)blockIdx.x * lmw::TILE_W + (tid & 15) * 4, v0 = (int)blockIdx.y * lmw::TILE_H + (tid >> 4) * 2;
    const bool live = u0 < a.w && v0 < a.h, row1 = v0 + 1 < a.h;
    const bool flip = e.flip_x != 0;
    // the lane's block in FRAME coordinates: columns xmin .. xmin + 3 (the window's u0 .. u0 + 3, descending when mirrored), rows y0, y0 + 1
    const int xmin = flip ? a.w - 4 - u0 + e.shift_x : u0 + e.shift_x, y0 = v0 + e.shift_y;
    const u8* F = a.frame + (size_t)(a.first + f) * a.slot_stride + a.off_bgr;
    u32 P[2][4];
    load_run(F, a.w, live ? a.h : 0, xmin, y0, P[0]);
    load_run(F, a.w, live && row1 ? a.h : 0, xmin, y0 + 1, P[1]);

    const u32 t = ((u32)f * (u32)a.tiles_y + blockIdx.y) * (u32)a.tiles_x + blockIdx.x;
    const u32 begin = a.tile_off[t], end = a.tile_off[t + 1];
    for (u32 base = begin; base < end; base += CHUNK) {
        const int n = (int)(end - base < (u32)CHUNK ? end - base : (u32)CHUNK);
        __syncthreads();        // (the last round's readers are done with the records)
        if (tid < 4 * n) reinterpret_cast<uint4*>(recs)[tid] = reinterpret_cast<const uint4*>(a.recs + a.idx[base + (u32)(tid >> 2)])[tid & 3];
        __syncthreads();
        if (!live) continue;
        for (int i = 0; i < n; ++i) {
            const lmw::Rec& r = recs[i];
            if (r.bx1 < xmin || r.bx0 > xmin + 3 || r.by1 < y0 || r.by0 > y0 + 1) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int y = y0 + j;
                if (y < 0 || y >= a.h) continue;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = xmin + k;
                    if (x >= 0 && x < a.w && lmw::covered(r, x, y)) P[j][k] = lmw::blend_pixel(P[j][k], r.colour);
                }
            }
        }
    }
    if (!live) return;
    u32 Q[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u32 px = flip ? P[j][3 - i] : P[j][i];
            Q[j][i] = e.swap_rb ? swap_rb(px) : px;
        }
    if constexpr (FLOAT) {
        if (e.es == 4) {
            store_row_float<4>(e, u0, v0, Q[0]);
            if (row1) store_row_float<4>(e, u0, v0 + 1, Q[1]);
        } else {
            store_row_float<2>(e, u0, v0, Q[0]);
            if (row1) store_row_float<2>(e, u0, v0 + 1, Q[1]);
        }
    } else {
        if (e.kind == LM_EXPORT_NV12) {
            if (row1) store_nv12(e, u0, v0, Q);      // (the frame's height is even: always)
            return;
        }
        store_row(e, u0, v0, Q[0]);
        if (row1) store_row(e, u0, v0 + 1, Q[1]);
    }
}

__global__ __launch_bounds__(256) void k_export(LmExportArgs a) {
    __shared__ __attribute__((aligned(16))) lmw::Rec recs[CHUNK];     // (staged as 16-byte vectors)
    export_block<false>(a, recs);
}
__global__ __launch_bounds__(256) void k_export_float(LmExportArgs a) {
    __shared__ __attribute__((aligned(16))) lmw::Rec recs[CHUNK];
    export_block<true>(a, recs);
}

}  // namespace

void lmk_export(hipStream_t s, const LmExportArgs& a) {
    if (a.n <= 0 || a.w <= 0 || a.h <= 0) return;
    const dim3 grid((u32)a.tiles_x, (u32)a.tiles_y, (u32)a.n);
    if (a.n_plain > 0 && lmk_count_launch(LMK_LAUNCH_EXPORT)) hipLaunchKernelGGL(k_export, grid, dim3(256), 0, s, a);
    if (a.n_float > 0 && lmk_count_launch(LMK_LAUNCH_EXPORT_FLOAT)) hipLaunchKernelGGL(k_export_float, grid, dim3(256), 0, s, a);
}
