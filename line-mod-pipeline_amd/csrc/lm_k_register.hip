// lm_k_register.hip -- a raw depth image, in the depth camera's own geometry, registered onto the colour camera (lm_ingest_frames_registered,
// DESIGN.md section 16; the rule: include/linemod_hip.h).  Two kernels, whatever the number of frames, behind the caller's memset of the
// z-buffer to the sentinel on the same stream:
//   k_register_scatter   one lane per RAW depth pixel of every frame (blockIdx.y = frame), row-major: lmr::project (lm_register.h) gives
//                        the colour pixel and the millimetres, and the lane takes the minimum into the (2 splat_x + 1) x (2 splat_y + 1)
//                        z-buffer words around it that lie in the window (atomicMin on u32: global_atomic_umin, no value returned).
//                        Neighbouring depth pixels land on neighbouring or equal words, so a wave's atomics stay in a few cache lines.
//                        The minimum does not depend on the order the lanes arrive in: the result is the same bits on every run.
//   k_register_resolve   one lane per two output pixels: sentinel -> 0, u32 -> u16, mirror and shift exactly as k_ingest places a depth
//                        window (xs = x - shift_x, ys = y - shift_y, outside: 0; u = flip_x ? W - 1 - xs : xs), one dword store.
// The z-buffer is kept in WINDOW coordinates: a colour pixel outside the window can reach no slot.
#include "lm_dev.h"
#include "lm_kernels.h"

namespace {

constexpr u32 Z_NONE = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void k_register_scatter(LmRegisterArgs a) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (u32)a.dw * (u32)a.dh) return;
    const LmIngestImage& e = a.table[a.first + (int)blockIdx.y].depth;
    const int row = (int)(i / (u32)a.dw), col = (int)i - row * a.dw;
    const u8* p = e.data + (long long)row * e.row_stride;
    const float t = e.kind == LM_INGEST_U16 ? (float)reinterpret_cast<const u16*>(p)[col] : reinterpret_cast<const float*>(p)[col] * e.scale;
    const float2 ray = reinterpret_cast<const float2*>(a.rays)[i];
    const lmr::Hit hit = lmr::project(a.rig, ray.x, ray.y, t);
    if (hit.dropped) return;
    // the window's columns [crop_x, crop_x + w) widened by the splat: compared in float (every bound is far below 2^24, so it is exact),
    // and only a u, v inside is converted to int
    const int x_lo = e.crop_x, x_hi = e.crop_x + a.w - 1, y_lo = e.crop_y, y_hi = e.crop_y + a.h - 1;
    if (!(hit.u >= (float)(x_lo - a.splat_x) && hit.u <= (float)(x_hi + a.splat_x) && hit.v >= (float)(y_lo - a.splat_y) &&
          hit.v <= (float)(y_hi + a.splat_y)))
        return;
    const int u = (int)hit.u, v = (int)hit.v;
    const int x0 = max(u - a.splat_x, x_lo), x1 = min(u + a.splat_x, x_hi), y0 = max(v - a.splat_y, y_lo), y1 = min(v + a.splat_y, y_hi);
    u32* z = a.zbuf + (size_t)blockIdx.y * (size_t)a.w * (size_t)a.h;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) atomicMin(z + (size_t)(y - y_lo) * a.w + (x - x_lo), hit.m);
}

__global__ __launch_bounds__(256) void k_register_resolve(LmRegisterArgs a) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    const int half = (a.w + 1) >> 1;
    if (i >= (u32)half * (u32)a.h) return;
    const int slot = a.first + (int)blockIdx.y;
    const LmIngestDesc& e = a.table[slot];
    const int y = (int)(i / (u32)half), x = ((int)i - y * half) * 2;
    const int ys = y - e.shift_y;
    const u32* z = a.zbuf + (size_t)blockIdx.y * (size_t)a.w * (size_t)a.h;
    u32 px[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int xs = x + k - e.shift_x;
        px[k] = 0u;
        if (xs >= 0 && xs < a.w && ys >= 0 && ys < a.h) {
            const u32 m = z[(size_t)ys * a.w + (e.flip_x ? a.w - 1 - xs : xs)];
            px[k] = m == Z_NONE ? 0u : m;
        }
    }
    u8* o = a.out + (size_t)slot * a.out_stride + ((size_t)y * a.w + x) * 2;
    if ((a.w & 1) == 0) *reinterpret_cast<u32*>(o) = px[0] | (px[1] << 16);
    else {      // (the stage hook's whole colour geometry may have an odd width: rows start on odd pixels, and the last lane of a row has one)
        reinterpret_cast<u16*>(o)[0] = (u16)px[0];
        if (x + 1 < a.w) reinterpret_cast<u16*>(o)[1] = (u16)px[1];
    }
}

}  // namespace

void lmk_register(hipStream_t s, const LmRegisterArgs& a) {
    if (a.n <= 0) return;
    const u32 raw = (u32)a.dw * (u32)a.dh, pairs = (u32)((a.w + 1) >> 1) * (u32)a.h;
    hipLaunchKernelGGL(k_register_scatter, dim3((raw + 255u) / 256u, (u32)a.n), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_register_resolve, dim3((pairs + 255u) / 256u, (u32)a.n), dim3(256), 0, s, a);
}
