// lm_k_gen.hip -- template-bank generation on the GPU: the kernels behind lm_add_templates_rendered, which
// make the same bank as the host generator (host/TemplateGenerator.cpp generate_templates) bit for bit.  Host side: lm_detector_gen.hip.
//   render   k_gen_vertices -> k_gen_zclear -> k_gen_raster (atomicMin on the float bits of window z) -> k_gen_resolve
//   rotate   k_gen_rotate (warp_rotate_u8 of the coverage into the slot's colour image, warp_rotate_u16 of the depth) -> k_gen_erode
//   masks    k_gen_flags per level: the nearest-neighbour mask pyramid read through the eroded level-0 mask, the colour rim and the
//            depth interior (shrink_mask once / twice, replicated borders)
//   depth    k_gen_rowdist: per label, the row distance to the nearest pixel outside the label's selection (the row pass of DIST_C)
//   lists    k_gen_cands: count pass, then write pass of the candidate lists, compacted in row-major order with ordered ballots
// Everything that rounds is restated in the host's operation order; the build's -ffp-contract=off keeps products and sums apart.
#include "lm_dev.h"
#include "lm_kernels.h"

namespace {

constexpr int kGenTile = 256;
constexpr u32 kZOne = 0x3f800000u;   // bits of 1.0f: glClear depth

// SoftRender::render_view's window coordinates: x, y, z, w (x = y = z = 0 when w <= 1e-6, as the host)
__global__ __launch_bounds__(256) void k_gen_vertices(const float* xyz, int nv, const float* vp_all, int W, int H, float4* sv) {
    const int i = blockIdx.x * kGenTile + threadIdx.x;
    const int v = blockIdx.y;
    if (i >= nv) return;
    const float* m = vp_all + 16 * (size_t)v;      // m[c * 4 + r] = Mat4::m[c][r]
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    const float cx = m[0] * x + m[4] * y + m[8] * z + m[12];
    const float cy = m[1] * x + m[5] * y + m[9] * z + m[13];
    const float cz = m[2] * x + m[6] * y + m[10] * z + m[14];
    const float cw = m[3] * x + m[7] * y + m[11] * z + m[15];
    float4 s;
    s.w = cw;
    if (cw > 1e-6f) {
        s.x = (cx / cw * 0.5f + 0.5f) * (float)W;
        s.y = (cy / cw * 0.5f + 0.5f) * (float)H;
        s.z = cz / cw * 0.5f + 0.5f;
    } else { s.x = s.y = s.z = 0.f; }
    sv[(size_t)v * nv + i] = s;
}

__global__ __launch_bounds__(256) void k_gen_zclear(u32* z, size_t n) {
    const size_t i = (size_t)blockIdx.x * kGenTile + threadIdx.x;
    if (i < n) z[i] = kZOne;
}

// One thread per (triangle, view) walks the triangle's clipped bbox.  A pixel's result depends only on the minimum accepted z, so an
// atomicMin on the bits (non-negative floats order like their bits; -0 is mapped to +0, NaN never passes) is exact in any order.
__global__ __launch_bounds__(256) void k_gen_raster(const float4* sv, int nv, const u32* idx, int ntri, int W, int H, u32* zbuf) {
    const int t = blockIdx.x * kGenTile + threadIdx.x;
    const int v = blockIdx.y;
    if (t >= ntri) return;
    const float4* s = sv + (size_t)v * nv;
    const float4 a = s[idx[3 * (size_t)t]], b = s[idx[3 * (size_t)t + 1]], c = s[idx[3 * (size_t)t + 2]];
    if (a.w <= 1e-6f || b.w <= 1e-6f || c.w <= 1e-6f) return;
    const float area = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x);
    if (area == 0) return;
    const int x0 = max(0, (int)floorf(fminf(a.x, fminf(b.x, c.x))));
    const int x1 = min(W - 1, (int)ceilf(fmaxf(a.x, fmaxf(b.x, c.x))));
    const int y0 = max(0, (int)floorf(fminf(a.y, fminf(b.y, c.y))));
    const int y1 = min(H - 1, (int)ceilf(fmaxf(a.y, fmaxf(b.y, c.y))));
    const float inv = 1.0f / area;
    u32* zb = zbuf + (size_t)v * W * H;
    for (int py = y0; py <= y1; ++py)
        for (int px = x0; px <= x1; ++px) {
            const float fx = px + 0.5f, fy = py + 0.5f;
            const float w0 = ((b.x - fx) * (c.y - fy) - (b.y - fy) * (c.x - fx)) * inv;
            const float w1 = ((c.x - fx) * (a.y - fy) - (c.y - fy) * (a.x - fx)) * inv;
            const float w2 = 1.0f - w0 - w1;
            if (w0 < 0 || w1 < 0 || w2 < 0) continue;
            float z = w0 * a.z + w1 * b.z + w2 * c.z;
            if (z < 0 || z > 1 || z != z) continue;
            if (z == 0.0f) z = 0.0f;                 // -0 (accepted by the host's z < zbuf) has the largest bits
            atomicMin(&zb[(size_t)(H - 1 - py) * W + px], __float_as_uint(z));
        }
}

// coverage 255 where some triangle was accepted (z < 1), depth = shader/depth.fs's linear depth in mm, R16 unorm
__global__ __launch_bounds__(256) void k_gen_resolve(const u32* zbuf, size_t n, u8* cov, u16* depth) {
    const size_t i = (size_t)blockIdx.x * kGenTile + threadIdx.x;
    if (i >= n) return;
    const u32 zb = zbuf[i];
    cov[i] = __uint_as_float(zb) < 1.0f ? 255 : 0;
    depth[i] = gen_z_to_mm(zb);
}

// warp_rotate_u8 / warp_rotate_u16 from fixed-point source-coordinate tables built on the host: tab = adelta[W] | bdelta[W] | X0[H] | Y0[H]
__device__ __forceinline__ void gen_src(const int* tab, int W, int H, int x, int y, int* X, int* Y) {
    *X = (tab[2 * W + y] + tab[x]) >> 5;
    *Y = (tab[2 * W + H + y] + tab[W + x]) >> 5;
}
__device__ __forceinline__ u8 gen_warp_u8(const u8* src, int W, int H, int X, int Y) {
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    auto at = [&](int yy, int xx) -> int { return (xx < 0 || yy < 0 || xx >= W || yy >= H) ? 0 : src[(size_t)yy * W + xx]; };
    const int v = at(sy, sx) * w00 + at(sy, sx + 1) * w01 + at(sy + 1, sx) * w10 + at(sy + 1, sx + 1) * w11;
    return (u8)((v + (1 << 14)) >> 15);
}
__device__ __forceinline__ u16 gen_warp_u16(const u16* src, int W, int H, int X, int Y) {
    const int sx = X >> 5, sy = Y >> 5;
    const float fx = (X & 31) / 32.0f, fy = (Y & 31) / 32.0f;
    auto at = [&](int yy, int xx) -> float { return (xx < 0 || yy < 0 || xx >= W || yy >= H) ? 0.f : (float)src[(size_t)yy * W + xx]; };
    const float v = at(sy, sx) * (1 - fx) * (1 - fy) + at(sy, sx + 1) * fx * (1 - fy) + at(sy + 1, sx) * (1 - fx) * fy +
                    at(sy + 1, sx + 1) * fx * fy;
    const long q = (long)rintf(v);
    return (u16)(q < 0 ? 0 : (q > 65535 ? 65535 : q));
}

// image i = (view img_view[i], angle img_angle[i]).  Writes the rotated coverage (rmask), the rotated depth (rdepth: read by the
// median of every template, also in colour-only mode), the colour image of the slot (the binarised colour = the coverage in all three
// channels) and, RGB-D, the slot's depth image.
__global__ __launch_bounds__(256) void k_gen_rotate(const u8* cov, const u16* dep, const int* img_view, const int* img_angle, const int* tabs,
                                                    int W, int H, u8* rmask, u16* rdepth, u8* bgr_slot, u16* depth_slot, size_t slot_stride) {
    const int p = blockIdx.x * kGenTile + threadIdx.x;
    const int i = blockIdx.y;
    const size_t npx = (size_t)W * H;
    if (p >= (int)npx) return;
    const int x = p % W, y = p / W;
    const int* tab = tabs + (size_t)img_angle[i] * (2 * W + 2 * H);
    const size_t vo = (size_t)img_view[i] * npx;
    int X, Y;
    gen_src(tab, W, H, x, y, &X, &Y);
    const u8 m = gen_warp_u8(cov + vo, W, H, X, Y);
    const u16 dz = gen_warp_u16(dep + vo, W, H, X, Y);
    rmask[(size_t)i * npx + p] = m;
    rdepth[(size_t)i * npx + p] = dz;
    u8* b = bgr_slot + (size_t)i * slot_stride + 3 * (size_t)p;
    b[0] = m; b[1] = m; b[2] = m;
    if (depth_slot) *reinterpret_cast<u16*>(reinterpret_cast<u8*>(depth_slot) + (size_t)i * slot_stride + 2 * (size_t)p) = dz;
}

// addTemplate's erode(maskRotated, 3x3): the border does not erode (neighbours outside the image are skipped)
__global__ __launch_bounds__(256) void k_gen_erode(const u8* rmask, int W, int H, u8* er) {
    const int p = blockIdx.x * kGenTile + threadIdx.x;
    const size_t npx = (size_t)W * H;
    if (p >= (int)npx) return;
    const int x = p % W, y = p / W;
    const u8* m = rmask + (size_t)blockIdx.y * npx;
    u8 v = 255;
    for (int j = -1; j <= 1; ++j)
        for (int i = -1; i <= 1; ++i) {
            const int yy = y + j, xx = x + i;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            v = min(v, m[(size_t)yy * W + xx]);
        }
    er[(size_t)blockIdx.y * npx + p] = v;
}

// The mask of level l at (x, y) is lm_add_template's nearest-neighbour pyramid: the level-0 mask at (x << l, y << l).
// flags bit 0: colour rim (mask > its 3x3 replicated minimum: shrink_mask once), bit 1: depth interior (5x5 replicated minimum != 0 --
// two 3x3 replicated minimum passes reach exactly the clamped 5x5 window).  An image without a mask (unmasked[image] != 0) has both
// bits set everywhere: extract_pyramid's `!masked` -- colour candidates anywhere, the whole level is the depth interior.
__global__ __launch_bounds__(256) void k_gen_flags(const u8* er, const int* unmasked, int W, int H, LmGenGeom g, int l, u8* flags) {
    const int w = g.w[l], h = g.h[l];
    const int p = blockIdx.x * kGenTile + threadIdx.x;
    if (p >= w * h) return;
    if (unmasked && unmasked[blockIdx.y]) { flags[(size_t)blockIdx.y * g.img_px + g.off[l] + p] = 3; return; }
    const int x = p % w, y = p / w;
    const u8* m = er + (size_t)blockIdx.y * W * H;
    auto at = [&](int yy, int xx) -> u8 {
        yy = min(max(yy, 0), h - 1); xx = min(max(xx, 0), w - 1);
        return m[(size_t)(yy << l) * W + (xx << l)];
    };
    u8 m3 = 255, m5 = 255;
    for (int j = -2; j <= 2; ++j)
        for (int i = -2; i <= 2; ++i) {
            const u8 v = at(y + j, x + i);
            m5 = min(m5, v);
            if (j >= -1 && j <= 1 && i >= -1 && i <= 1) m3 = min(m3, v);
        }
    flags[(size_t)blockIdx.y * g.img_px + g.off[l] + p] = (u8)((at(y, x) > m3 ? 1 : 0) | (m5 != 0 ? 2 : 0));
}

// DIST_C row pass: per label b, the distance along the row to the nearest pixel OUTSIDE sel_b = interior & (q & (1 << b)); 0xFFFF when
// the row has none (outside the image counts as far away, like the host's two raster sweeps).
__global__ __launch_bounds__(256) void k_gen_rowdist(const u8* flags, const u8* slot0, size_t slot_stride, LmGenGeom g, int l, u16* hp) {
    const int w = g.w[l], h = g.h[l];
    const int p = blockIdx.x * kGenTile + threadIdx.x;
    if (p >= w * h) return;
    const int x = p % w, y = p / w;
    const int i = blockIdx.y;
    const u8* fr = flags + (size_t)i * g.img_px + g.off[l] + (size_t)y * w;
    const u8* qr = slot0 + (size_t)i * slot_stride + g.q_off[l][1] + (size_t)y * w;
    u16* o = hp + (size_t)i * 8 * g.img_px + g.off[l] + p;
    const unsigned sel = (fr[x] & 2) ? qr[x] : 0u;
    for (int b = 0; b < 8; ++b) {
        u16 d = 0;
        if (sel & (1u << b)) {
            int best = 0xFFFF;
            for (int r = 1; r < w && r < best; ++r) {
                const int xl = x - r, xr = x + r;
                const bool zl = xl >= 0 && !((fr[xl] & 2) && (qr[xl] & (1u << b)));
                const bool zr = xr < w && !((fr[xr] & 2) && (qr[xr] & (1u << b)));
                if (zl || zr) { best = r; break; }
                if (xl < 0 && xr >= w) break;
            }
            d = (u16)best;
        }
        o[(size_t)b * g.img_px] = d;
    }
}

__device__ __forceinline__ int gen_label(unsigned q) {   // one-hot byte -> bin, -1 if not one-hot
    if (q == 0 || (q & (q - 1))) return -1;
    return __ffs(q) - 1;
}

// DIST_C column pass at (x, y) for label b: min over rows y' of max(|y - y'|, row distance at y'); rows beyond the image are far away
__device__ int gen_coldist(const u16* hb, int w, int h, int x, int y) {
    int best = hb[(size_t)y * w + x];
    if (best == 0xFFFF) best = INT_MAX;
    for (int r = 1; r < best && (y - r >= 0 || y + r < h); ++r) {
        int hv = INT_MAX;
        if (y - r >= 0) { const int t = hb[(size_t)(y - r) * w + x]; hv = min(hv, t == 0xFFFF ? INT_MAX : t); }
        if (y + r < h) { const int t = hb[(size_t)(y + r) * w + x]; hv = min(hv, t == 0xFFFF ? INT_MAX : t); }
        if (hv != INT_MAX) best = min(best, max(r, hv));
    }
    return best == INT_MAX ? (INT_MAX >> 2) : best;   // no zero anywhere: the host's FAR
}

// One workgroup per (row, list, image); list = level * M + modality.  pass 0 counts the row's candidates (and, for depth, its interior
// pixels), pass 1 writes them at rowoff in row-major order: ordered ballots within a wave, wave counts in LDS across the workgroup.
__global__ __launch_bounds__(256) void k_gen_cands(int pass, const u8* flags, const u16* hp, const u8* slot0, const u8* mag,
                                                   size_t slot_stride, LmGenGeom g, u32* cnt, u32* icnt,
                                                   const u32* rowoff, LmGenCand* out) {
    const int li = blockIdx.y, l = li / g.M, mod = li % g.M, i = blockIdx.z, y = blockIdx.x;
    const int w = g.w[l], h = g.h[l];
    if (y >= h) return;
    __shared__ u32 wave_cnt[kGenTile / 64];
    const u8* fr = flags + (size_t)i * g.img_px + g.off[l] + (size_t)y * w;
    const u8* qr = slot0 + (size_t)i * slot_stride + g.q_off[l][mod] + (size_t)y * w;
    const float* mr = reinterpret_cast<const float*>(mag + (size_t)i * slot_stride + g.mag_off[l]) + (size_t)y * w;   // (mod == 0 only)
    const size_t list = (size_t)i * g.L * g.M + li;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u32 base = pass ? rowoff[list * g.rows + y] : 0u, inner = 0;
    for (int x0 = 0; x0 < w; x0 += kGenTile) {
        const int x = x0 + threadIdx.x;
        bool keep = false;
        LmGenCand c;
        if (x < w) {
            const unsigned q = qr[x];
            if (mod == 0) {
                keep = (fr[x] & 1) && q != 0 && mr[x] > g.min_mag;
                if (keep) { c.label = gen_label(q); c.score = mr[x]; }
            } else {
                const bool in = fr[x] & 2;
                inner += in ? 1u : 0u;
                const int lab = gen_label(q);
                if (in && q != 255 && lab >= 0) {
                    const int d = gen_coldist(hp + (size_t)i * 8 * g.img_px + (size_t)lab * g.img_px + g.off[l], w, h, x, y);
                    keep = (float)d >= (float)g.et[l];
                    if (keep) { c.label = lab; c.score = (float)d; }
                }
            }
            c.x = (int16_t)x; c.y = (int16_t)y;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wave_cnt[wv] = (u32)__popcll(bal);
        __syncthreads();
        u32 before = 0, total = 0;
        for (int k = 0; k < kGenTile / 64; ++k) { if (k < wv) before += wave_cnt[k]; total += wave_cnt[k]; }
        if (pass && keep) out[base + before + (u32)__popcll(bal & ((1ull << lane) - 1ull))] = c;
        base += total;
        __syncthreads();
    }
    if (!pass) {
        if (threadIdx.x == 0) cnt[list * g.rows + y] = base;
        if (mod == 1) {
            for (int o = 32; o > 0; o >>= 1) inner += __shfl_down(inner, o, 64);
            if (lane == 0) wave_cnt[wv] = inner;
            __syncthreads();
            if (threadIdx.x == 0) icnt[((size_t)i * g.L + l) * g.rows + y] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        }
    }
}

inline unsigned blocks(size_t n) { return (unsigned)((n + kGenTile - 1) / kGenTile); }

}  // namespace

void lmk_gen_zbuffer(hipStream_t s, const float* xyz, int nv, const u32* idx, int ntri, const float* vp, int nviews, int W, int H,
                     float4* sv, u32* zbuf) {
    const size_t npx = (size_t)W * H * nviews;
    hipLaunchKernelGGL(k_gen_vertices, dim3(blocks((size_t)nv), (unsigned)nviews), dim3(kGenTile), 0, s, xyz, nv, vp, W, H, sv);
    hipLaunchKernelGGL(k_gen_zclear, dim3(blocks(npx)), dim3(kGenTile), 0, s, zbuf, npx);
    if (ntri > 0) hipLaunchKernelGGL(k_gen_raster, dim3(blocks((size_t)ntri), (unsigned)nviews), dim3(kGenTile), 0, s, sv, nv, idx, ntri, W, H, zbuf);
}

void lmk_gen_render(hipStream_t s, const float* xyz, int nv, const u32* idx, int ntri, const float* vp, int nviews, int W, int H,
                    float4* sv, u32* zbuf, u8* cov, u16* depth) {
    const size_t npx = (size_t)W * H * nviews;
    lmk_gen_zbuffer(s, xyz, nv, idx, ntri, vp, nviews, W, H, sv, zbuf);
    hipLaunchKernelGGL(k_gen_resolve, dim3(blocks(npx)), dim3(kGenTile), 0, s, zbuf, npx, cov, depth);
}

void lmk_gen_rotate(hipStream_t s, const u8* cov, const u16* dep, const int* img_view, const int* img_angle, const int* tabs, int nimg,
                    int W, int H, u8* rmask, u16* rdepth, u8* bgr_slot, u16* depth_slot, size_t slot_stride, u8* er) {
    const size_t npx = (size_t)W * H;
    hipLaunchKernelGGL(k_gen_rotate, dim3(blocks(npx), (unsigned)nimg), dim3(kGenTile), 0, s, cov, dep, img_view, img_angle, tabs, W, H,
                       rmask, rdepth, bgr_slot, depth_slot, slot_stride);
    if (er) hipLaunchKernelGGL(k_gen_erode, dim3(blocks(npx), (unsigned)nimg), dim3(kGenTile), 0, s, rmask, W, H, er);
}

void lmk_gen_candidates(hipStream_t s, int pass, const u8* er, const int* unmasked, int W, int H, int nimg, const LmGenGeom& g, u8* flags,
                        u16* hp, const u8* slot0, const u8* mag, size_t slot_stride, u32* cnt, u32* icnt, const u32* rowoff, LmGenCand* out) {
    if (pass == 0) {
        for (int l = 0; l < g.L; ++l) {
            const size_t px = (size_t)g.w[l] * g.h[l];
            hipLaunchKernelGGL(k_gen_flags, dim3(blocks(px), (unsigned)nimg), dim3(kGenTile), 0, s, er, unmasked, W, H, g, l, flags);
            if (g.M == 2)
                hipLaunchKernelGGL(k_gen_rowdist, dim3(blocks(px), (unsigned)nimg), dim3(kGenTile), 0, s, flags, slot0, slot_stride, g, l, hp);
        }
    }
    hipLaunchKernelGGL(k_gen_cands, dim3((unsigned)g.rows, (unsigned)(g.L * g.M), (unsigned)nimg), dim3(kGenTile), 0, s, pass, flags, hp,
                       slot0, mag, slot_stride, g, cnt, icnt, rowoff, out);
}
