// lm_k_preprocess.hip -- a3-a10 of the LINE-MOD match path for gfx950 (CDNA4, wave64): the kernels of lm_dev_color.h, lm_dev_depth.h and
// lm_dev_memories.h, the level-fused kernels that run several of their device functions in one grid (k_phase: few frames; k_bphase / k_bsplit:
// a lone lane of a batch), and lmk_preprocess_run, which launches the steps the host planner (lm_host.h plan_preprocess) lists.
// Every kernel takes the buffers of frame slot 0 plus the byte stride between slots, so a batch of resident frames is one launch per stage.
#include "lm_dev_color.h"
#include "lm_dev_depth.h"
#include "lm_dev_memories.h"
#include "lm_host.h"

namespace {

// ------------------------------------------------------------------------------------------------
// a3-a10 of few frames: the kernels of one dependency level in ONE launch, each on its own range of the block index
// (LmPhaseArgs in lm_kernels.h).  A single frame is 14 dependent launches of 3-12 us otherwise, each with its own
// dispatch and drain; here the independent ones overlap and the chain is five launches long.
// ------------------------------------------------------------------------------------------------
template <int PH, int T0>
__global__ __launch_bounds__(256) void k_phase(LmPhaseArgs a, LmPhaseGrid pg) {
    const u32 b = blockIdx.x, e0 = pg.nb[0], e1 = e0 + pg.nb[1], e2 = e1 + pg.nb[2];
    const size_t fs = a.slot_stride;
    const int w1 = a.w >> 1, h1 = a.h >> 1;
    const size_t a3_0 = ((size_t)a.w * a.h * 3 + 255) / 256 * 256, a3_1 = ((size_t)w1 * h1 * 3 + 255) / 256 * 256;   // qn behind S
    const float thr2 = a.weak_threshold * a.weak_threshold;
    if (PH == 1) {
        if (b < e0) d_cblur(b, a.bgr0, a.w, a.h, a.cs0, fs, fs, pg.g[0], a.nslots);
        else if (b < e1) d_dnormal(b - e0, a.depth, a.w, a.h, a.dist_thr, a.diff_thr, a.normal_lut, a.ds, fs, fs, pg.g[1], a.nslots);
        else d_pyrdown8(b - e1, a.bgr0, a.w, a.h, a.bgr1, w1, h1, fs, pg.g[2], a.nslots);
    } else if (PH == 2) {
        if (b < e0) d_dmedian<DM_ROWS>(b, a.ds, a.w, a.h, a.qd0, fs, fs, pg.g[0], a.nslots);
        else if (b < e1) d_cblur(b - e0, a.bgr1, w1, h1, a.cs1, fs, fs, pg.g[1], a.nslots);
        else d_corient(b - e1, a.cs0, a.w, a.h, thr2, a.cs0 + a3_0, nullptr, fs, fs, pg.g[2], a.nslots);
    } else if (PH == 3) {
        if (b < e0) d_cvote(b, a.cs0 + a3_0, a.w, a.h, a.qc0, fs, fs, pg.g[0], a.nslots);
        else if (b < e1) d_corient(b - e0, a.cs1, w1, h1, thr2, a.cs1 + a3_1, nullptr, fs, fs, pg.g[1], a.nslots);
        else if (b < e2) d_lm_fast<5, 128, 0, 1>(b - e1, a.qd0, a.w, a.w, a.h, a.resp_tab, a.lm_d0, 0u, fs, fs, pg.g[2], a.nslots);
        else d_lm_fast<8, 40, 1, 2>(b - e2, a.qd0, a.w, w1, h1, a.resp_tab, a.lm_d1, a.ori_stride1, fs, fs, pg.g[3], a.nslots, a.plane_ori1);
    } else {
        if (b < e0) d_cvote(b, a.cs1 + a3_1, w1, h1, a.qc1, fs, fs, pg.g[0], a.nslots);
        else if (T0 == 5) d_lm_fast<5, 128, 0, 1>(b - e0, a.qc0, a.w, a.w, a.h, a.resp_tab, a.lm_c0, 0u, fs, fs, pg.g[1], a.nslots);
        else d_lm_spread2(b - e0, a.qc0, a.w, a.w, a.h, a.lm_c0, fs, fs, pg.g[1], a.nslots);     // T0 == 2 (colour only)
    }
}

// ------------------------------------------------------------------------------------------------
// a3-a10 of a BATCH as four launches (r03: "horizontal fusion of the pyramid levels").  The batch kernels of one dependency
// level share ONE grid, each on its own range of the block index, the longest-running first: the level-1 kernels and the
// other short ones (a 320 x 240 level is 10 waves per frame: 960 waves for 1024 SIMDs when launched alone, each walking
// its strip serially) fill the chip's tail instead of holding a half-empty launch of their own, and a lane-step is 4 + 4
// dependent launches instead of 11 + 4.
//   1  depth normals          | blur(level 0)           | pyrDown(level 0 -> 1)
//   2  gradient + vote(0)     | median of the normals   | blur(level 1)
//   3  gradient + vote(1)     | colour spread memory(0) | depth spread memory(0) | depth response memories(1)
//   4  colour response memories(1)                                             (plain k_lm_fast launch)
// Same device functions, same results as the kernels launched one by one (LM_TUNE_BATCH_PHASES = 0).  Every part keeps
// its XCD affinity: the parts' block counts are multiples of 8 whenever the slot count is.
// SB / SG: rows per strip of the level-0 blur / gradient kernels (16, or 32 for tall images).
// ------------------------------------------------------------------------------------------------
template <int PH, int T0, int SB, int SG>
__global__ __launch_bounds__(256, 2) void k_bphase(LmPhaseArgs a, LmPhaseGrid pg) {
    const u32 b = blockIdx.x, e0 = pg.nb[0], e1 = e0 + pg.nb[1], e2 = e1 + pg.nb[2];
    const size_t fs = a.slot_stride;
    const int w1 = a.w >> 1, h1 = a.h >> 1, n = a.nslots;
    const float thr2 = a.weak_threshold * a.weak_threshold;
    const int ithr = thr2 >= 2147483648.f ? INT_MAX : (int)floorf(thr2);    // (float)m > thr2 <=> m > floor(thr2)
    if (PH == 1) {
        if (b < e0) d_dnormal(b, a.depth, a.w, a.h, a.dist_thr, a.diff_thr, a.normal_lut, a.ds, fs, fs, pg.g[0], n);
        else if (b < e1) d_cblur_sh<SB>(b - e0, a.bgr0, a.w, a.h, a.cs0, fs, fs, pg.g[1], n);
        else d_pyrdown16<PD_STRIP>(b - e1, a.bgr0, a.w, a.h, a.bgr1, w1, h1, fs, pg.g[2], n);
    } else if (PH == 2) {
        if (b < e0) d_cgrad<SG>(b, a.cs0, a.w, a.h, ithr, a.qc0, fs, fs, pg.g[0], n);
        else if (b < e1) d_dmedian<DM_ROWS_BATCH>(b - e0, a.ds, a.w, a.h, a.qd0, fs, fs, pg.g[1], n);
        else d_cblur_sh<16>(b - e1, a.bgr1, w1, h1, a.cs1, fs, fs, pg.g[2], n);
    } else {
        if (b < e0) d_cgrad<16>(b, a.cs1, w1, h1, ithr, a.qc1, fs, fs, pg.g[0], n);
        else if (b < e1) {
            if (T0 == 5) d_lm_spread5(b - e0, a.qc0, a.w, a.w, a.h, a.lm_c0, fs, fs, pg.g[1], n);
            else d_lm_spread2(b - e0, a.qc0, a.w, a.w, a.h, a.lm_c0, fs, fs, pg.g[1], n);
        }
        else if (b < e2) d_lm_spread5(b - e1, a.qd0, a.w, a.w, a.h, a.lm_d0, fs, fs, pg.g[2], n);
        else d_lm_fast<8, 40, 1, 2>(b - e2, a.qd0, a.w, w1, h1, a.resp_tab, a.lm_d1, a.ori_stride1, fs, fs, pg.g[3], n, a.plane_ori1);
    }
}

// The RGB-D form.  A fused kernel's waves all allocate the registers of its hungriest part: with the depth kernels
// (k_dnormal: 61 VGPRs, 8 waves per SIMD when launched alone) inside the grids of the blur / gradient kernels (204 / 238
// VGPRs, 2 waves per SIMD) the level-fused launches above LOSE (r03, config 2: pre-processing 4.82 -> 4.88 us per frame
// on one lane, 145 K -> 131 K detections/s with three lanes -- the fat waves also keep the other lanes' scan waves off
// the SIMDs).  So the RGB-D pyramid fuses only kernels of one register class:
//   light  0: depth normals | pyrDown                      heavy  1: gradient + vote(0) | blur(level 1)
//   light  2: colour spread memory(0) | depth spread memory(0) | depth response memories(1)
// between the plain launches of blur(level 0), median, gradient + vote(1) and the colour response memories(1): seven
// launches instead of eleven.
template <int PART, int SG>
__global__ __launch_bounds__(256, PART == 1 ? 2 : 1) void k_bsplit(LmPhaseArgs a, LmPhaseGrid pg) {
    const u32 b = blockIdx.x, e0 = pg.nb[0], e1 = e0 + pg.nb[1];
    const size_t fs = a.slot_stride;
    const int w1 = a.w >> 1, h1 = a.h >> 1, n = a.nslots;
    if (PART == 0) {
        if (b < e0) d_dnormal(b, a.depth, a.w, a.h, a.dist_thr, a.diff_thr, a.normal_lut, a.ds, fs, fs, pg.g[0], n);
        else d_pyrdown16<PD_STRIP>(b - e0, a.bgr0, a.w, a.h, a.bgr1, w1, h1, fs, pg.g[1], n);
    } else if (PART == 1) {
        const float thr2 = a.weak_threshold * a.weak_threshold;
        const int ithr = thr2 >= 2147483648.f ? INT_MAX : (int)floorf(thr2);
        if (b < e0) d_cgrad<SG>(b, a.cs0, a.w, a.h, ithr, a.qc0, fs, fs, pg.g[0], n);
        else d_cblur_sh<16>(b - e0, a.bgr1, w1, h1, a.cs1, fs, fs, pg.g[1], n);
    } else {
        if (b < e0) d_lm_spread5(b, a.qc0, a.w, a.w, a.h, a.lm_c0, fs, fs, pg.g[0], n);
        else if (b < e1) d_lm_spread5(b - e0, a.qd0, a.w, a.w, a.h, a.lm_d0, fs, fs, pg.g[1], n);
        else d_lm_fast<8, 40, 1, 2>(b - e1, a.qd0, a.w, w1, h1, a.resp_tab, a.lm_d1, a.ori_stride1, fs, fs, pg.g[2], n, a.plane_ori1);
    }
}

__global__ void k_nn_half(const u8* __restrict__ src0, int sp, u8* __restrict__ dst0, int dw, int dh,
                          size_t slot_stride) {
    const u8* src = slot_ptr(src0, slot_stride);
    u8* dst = slot_ptr(dst0, slot_stride);
    int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x < dw && y < dh) dst[(size_t)y * dw + x] = src[(size_t)(2 * y) * sp + 2 * x];
}

}  // namespace

// ================================================================================================
// execution: the steps of lm_host.h's planner (plan_preprocess and the single-stage planners) as launches.  Which kernel runs on which
// grid is decided there, from values alone; here a step's enumerator becomes its hipLaunchKernelGGL, with the pointers of LmPreArgs.
// ================================================================================================
size_t lmk_color_scratch_bytes(int w, int h) {
    // S u8 [h][3w] | qn u8 [h][w], each 256-B aligned (also the rank-code image of the depth passes)
    size_t px = (size_t)w * h;
    return (px * 3 + 255) / 256 * 256 + (px + 255) / 256 * 256;
}

void lmk_preprocess_run(hipStream_t s, const lmh::PrePlan& p, int from, int to, const LmPreArgs& a) {
    typedef lmh::PreKernel K;
    const size_t fs = a.slot_stride;
    const int n = a.nslots;
    const float thr2 = a.weak_threshold * a.weak_threshold;
    const int ithr = thr2 >= 2147483648.f ? INT_MAX : (int)floorf(thr2);    // (float)m > thr2 <=> m > floor(thr2)
    LmPhaseArgs pa{};       // the fused launches' view of the same buffers
    pa.bgr0 = a.bgr[0]; pa.bgr1 = a.bgr[1]; pa.depth = a.depth;
    pa.cs0 = a.cs[0]; pa.cs1 = a.cs[1]; pa.ds = a.ds;
    pa.qc0 = a.quant[0][0]; pa.qc1 = a.quant[1][0]; pa.qd0 = a.quant[0][1];
    pa.lm_c0 = a.lm[0][0]; pa.lm_c1 = a.lm[1][0]; pa.lm_d0 = a.lm[0][1]; pa.lm_d1 = a.lm[1][1];
    pa.w = a.w[0]; pa.h = a.h[0];
    pa.weak_threshold = a.weak_threshold; pa.dist_thr = a.dist_thr; pa.diff_thr = a.diff_thr;
    pa.normal_lut = a.normal_lut; pa.resp_tab = a.resp_tab; pa.ori_stride1 = a.ori_stride[1]; pa.plane_ori1 = a.planes;
    pa.slot_stride = fs; pa.nslots = n;
    for (int i = from; i < to; ++i) {
        const lmh::PreStep& st = p.step[i];
        const int l = st.level, m = st.modality, w = a.w[l], h = a.h[l];
        const int* g = st.pg.g;
        const dim3 grid(st.gx, st.gy, st.gz);
        u8* const S = a.cs[l];                                                  // the level's blurred image; behind it, its orientation labels
        const size_t qn_off = ((size_t)w * h * 3 + 255) / 256 * 256;
        // linear memories: the image read (src_shift: the finer level's depth image at (2y, 2x)), the memories written, the scanned level's planes
        const u8* const q = st.src_shift ? a.quant[l - 1][1] : a.quant[l][m];
        const int qpitch = st.src_shift ? a.w[l - 1] : w;
        const u32 planes = l == a.L - 1 && a.mode[l] == 2 ? a.planes : 0u;
#define LM_RUN(kern, ...) hipLaunchKernelGGL(kern, grid, dim3(256), st.lds, s, __VA_ARGS__)
#define LM_FAST(T, SEG)                                                                                                              \
        do {                                                                                                                        \
            const int md = a.mode[l];                                                                                               \
            if (st.src_shift) { if (md == 1) LM_FAST_(T, SEG, 1, 1); else if (md == 2) LM_FAST_(T, SEG, 1, 2); else LM_FAST_(T, SEG, 1, 0); }   \
            else              { if (md == 1) LM_FAST_(T, SEG, 0, 1); else if (md == 2) LM_FAST_(T, SEG, 0, 2); else LM_FAST_(T, SEG, 0, 0); }   \
        } while (0)
#define LM_FAST_(T, SEG, SH, MD) LM_RUN((k_lm_fast<T, SEG, SH, MD>), q, qpitch, w, h, a.resp_tab, a.lm[l][m], a.ori_stride[l], fs, fs, g[0], n, planes)
#define LM_CGL(A, B) LM_RUN((k_cgrad_levels<A, B>), a.cs[0], a.w[0], a.h[0], a.quant[0][0], g[0], a.cs[1], a.w[1], a.h[1], a.quant[1][0], g[1], ithr, fs, n)
#define LM_FUSED(...) LM_RUN((__VA_ARGS__), pa, st.pg)
        switch (st.k) {
            case K::Pyrdown: LM_RUN(k_pyrdown, a.bgr[l - 1], a.w[l - 1], a.h[l - 1], a.bgr[l], a.w[l - 1] / 2, a.h[l - 1] / 2, fs); break;
            case K::Pyrdown8: LM_RUN(k_pyrdown8, a.bgr[l - 1], a.w[l - 1], a.h[l - 1], a.bgr[l], a.w[l - 1] / 2, a.h[l - 1] / 2, fs, g[0], n); break;
            case K::Pyrdown16: LM_RUN(k_pyrdown16<PD_STRIP>, a.bgr[l - 1], a.w[l - 1], a.h[l - 1], a.bgr[l], a.w[l - 1] / 2, a.h[l - 1] / 2, fs, g[0], n); break;
            case K::NnHalf: LM_RUN(k_nn_half, a.quant[l - 1][1], a.w[l - 1], a.quant[l][1], w, h, fs); break;
            case K::BlurPyr16: LM_RUN(k_blur_pyr<CBS_STRIP>, a.bgr[0], w, h, S, a.bgr[1], fs, g[0], g[1], n, st.param); break;
            case K::BlurPyr32: LM_RUN(k_blur_pyr<32>, a.bgr[0], w, h, S, a.bgr[1], fs, g[0], g[1], n, st.param); break;
            case K::BlurPyr64: LM_RUN(k_blur_pyr<64>, a.bgr[0], w, h, S, a.bgr[1], fs, g[0], g[1], n, st.param); break;
            case K::BlurMxPyr: LM_RUN(k_blur_mx_pyr, a.bgr[0], w, h, S, a.bgr[1], fs, g[0], g[1], st.param, g[2], n); break;
            case K::Cblur: LM_RUN(k_cblur, a.bgr[l], w, h, S, fs, fs, g[0], n); break;
            case K::CblurSh16: LM_RUN(k_cblur_sh<CBS_STRIP>, a.bgr[l], w, h, S, fs, fs, g[0], n); break;
            case K::CblurSh32: LM_RUN(k_cblur_sh<32>, a.bgr[l], w, h, S, fs, fs, g[0], n); break;
            case K::CblurMx: LM_RUN(k_cblur_mx, a.bgr[l], w, h, S, fs, fs, g[0], g[1], st.param, n); break;
            case K::Corient: LM_RUN(k_corient, S, w, h, thr2, S + qn_off, a.mag[l], fs, fs, g[0], n); break;
            case K::Cvote: LM_RUN(k_cvote, S + qn_off, w, h, a.quant[l][0], fs, fs, g[0], n); break;
            case K::Cgrad8: LM_RUN(k_cgrad<8>, S, w, h, ithr, a.quant[l][0], fs, fs, g[0], n); break;
            case K::Cgrad16: LM_RUN(k_cgrad<CG_STRIP>, S, w, h, ithr, a.quant[l][0], fs, fs, g[0], n); break;
            case K::Cgrad32: LM_RUN(k_cgrad<32>, S, w, h, ithr, a.quant[l][0], fs, fs, g[0], n); break;
            case K::ColorQuantize: LM_RUN(k_color_quantize, a.bgr[l], w, h, thr2, a.quant[l][0], a.mag[l], fs); break;
            case K::CgradLevels32_16: LM_CGL(32, 16); break;
            case K::CgradLevels32_8: LM_CGL(32, 8); break;
            case K::CgradLevels16_16: LM_CGL(CG_STRIP, 16); break;
            case K::CgradLevels16_8: LM_CGL(CG_STRIP, 8); break;
            case K::CgradLevels8_8: LM_CGL(8, 8); break;
            case K::Dnormal: LM_RUN(k_dnormal, a.depth, w, h, a.dist_thr, a.diff_thr, a.normal_lut, a.ds, fs, fs, g[0], n); break;
            case K::Dmedian4: LM_RUN(k_dmedian<DM_ROWS>, a.ds, w, h, a.quant[0][1], fs, fs, g[0], n); break;
            case K::Dmedian16: LM_RUN(k_dmedian<DM_ROWS_BATCH>, a.ds, w, h, a.quant[0][1], fs, fs, g[0], n); break;
            case K::DepthQuantize: LM_RUN(k_depth_quantize, a.depth, w, h, a.dist_thr, a.diff_thr, a.normal_lut, a.quant[0][1], fs); break;
            case K::MaskRules: case K::MatchMasks: break;      // built from the slots: the detector launches them between its two calls
            case K::LmSpread2: LM_RUN(k_lm_spread2, q, qpitch, w, h, a.lm[l][m], fs, fs, g[0], n); break;
            case K::LmSpread5: LM_RUN(k_lm_spread5, q, qpitch, w, h, a.lm[l][m], fs, fs, g[0], n); break;
            case K::LmFast2_128: LM_FAST(2, 128); break;
            case K::LmFast4_64: LM_FAST(4, 64); break;
            case K::LmFast5_128: LM_FAST(5, 128); break;
            case K::LmFast8_40: LM_FAST(8, 40); break;
            case K::LmFast8_80: LM_FAST(8, 80); break;
            case K::LinearMemories:
                if (st.src_shift) { if (a.mode[l] == 1) LM_RUN((k_linear_memories<1, true>), q, qpitch, w, h, a.T[l], st.param, a.resp_tab, a.lm[l][m], a.ori_stride[l], fs, fs);
                                    else LM_RUN((k_linear_memories<1, false>), q, qpitch, w, h, a.T[l], st.param, a.resp_tab, a.lm[l][m], a.ori_stride[l], fs, fs); }
                else              { if (a.mode[l] == 1) LM_RUN((k_linear_memories<0, true>), q, qpitch, w, h, a.T[l], st.param, a.resp_tab, a.lm[l][m], a.ori_stride[l], fs, fs);
                                    else LM_RUN((k_linear_memories<0, false>), q, qpitch, w, h, a.T[l], st.param, a.resp_tab, a.lm[l][m], a.ori_stride[l], fs, fs); }
                break;
            case K::Phase1: LM_FUSED(k_phase<1, 5>); break;
            case K::Phase2: LM_FUSED(k_phase<2, 5>); break;
            case K::Phase3: LM_FUSED(k_phase<3, 5>); break;
            case K::Phase4_T5: LM_FUSED(k_phase<4, 5>); break;
            case K::Phase4_T2: LM_FUSED(k_phase<4, 2>); break;
            case K::Bsplit0: LM_FUSED(k_bsplit<0, 16>); break;
            case K::Bsplit1_16: LM_FUSED(k_bsplit<1, 16>); break;
            case K::Bsplit1_32: LM_FUSED(k_bsplit<1, 32>); break;
            case K::Bsplit2: LM_FUSED(k_bsplit<2, 16>); break;
            case K::Bphase1_T5_16: LM_FUSED(k_bphase<1, 5, 16, 16>); break;
            case K::Bphase2_T5_16: LM_FUSED(k_bphase<2, 5, 16, 16>); break;
            case K::Bphase3_T5_16: LM_FUSED(k_bphase<3, 5, 16, 16>); break;
            case K::Bphase1_T5_32: LM_FUSED(k_bphase<1, 5, 32, 32>); break;
            case K::Bphase2_T5_32: LM_FUSED(k_bphase<2, 5, 32, 32>); break;
            case K::Bphase3_T5_32: LM_FUSED(k_bphase<3, 5, 32, 32>); break;
            case K::Bphase1_T2_16: LM_FUSED(k_bphase<1, 2, 16, 16>); break;
            case K::Bphase2_T2_16: LM_FUSED(k_bphase<2, 2, 16, 16>); break;
            case K::Bphase3_T2_16: LM_FUSED(k_bphase<3, 2, 16, 16>); break;
            case K::Bphase1_T2_32: LM_FUSED(k_bphase<1, 2, 32, 32>); break;
            case K::Bphase2_T2_32: LM_FUSED(k_bphase<2, 2, 32, 32>); break;
            case K::Bphase3_T2_32: LM_FUSED(k_bphase<3, 2, 32, 32>); break;
            case K::Count: break;
        }
#undef LM_FUSED
#undef LM_CGL
#undef LM_FAST_
#undef LM_FAST
#undef LM_RUN
    }
}

void lmk_selftest_float_tail(hipStream_t s, unsigned long long* out2) {
    hipLaunchKernelGGL(k_selftest_float_tail, dim3(8192), dim3(256), 0, s, out2);
}
