// lm_detector_eval.hip -- host side of the pose-error evaluation (0.7): lm_pose_error_vsd, lm_pose_error_add and
// the stage hook lm_stage_vsd_counts.  Kernels: lm_k_eval.hip (and lm_k_gen.hip's rasteriser).
// Queries go in chunks of a fixed cap; the scratch is sized once per call for a full chunk.  Everything runs on the evaluation's own
// stream with *Async copies and memsets, one synchronisation per chunk (the read-back); no frame slot or lane is touched.
#include "lm_detector_impl.h"

namespace lmd {

struct EvalState {
    Stream stream;
    DevBuf<u8> buf;
};

void free_eval(lm_detector* d) { delete d->eval; d->eval = nullptr; }

static int ensure_eval(lm_detector* d) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if (d->eval) return LM_OK;
    std::unique_ptr<EvalState> s(new EvalState());
    const hipError_t e = s->stream.create(hipStreamNonBlocking);
    // published only once complete: a later call retries instead of running on a null stream
    if (e != hipSuccess) return fail(LM_ERR_HIP, std::string("evaluation stream: ") + hipGetErrorString(e));
    d->eval = s.release();
    return LM_OK;
}

static int grow(EvalState* s, size_t bytes) {
    if (bytes <= s->buf.size()) return LM_OK;
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(s->buf.grow(bytes));
    return LM_OK;
}

struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at = align_up(at + bytes, 256); return o; }
};

constexpr int kVsdChunk = 64;                          // queries per chunk (two renders each) ...
constexpr size_t kVsdChunkBytes = (size_t)512 << 20;   // ... fewer when their z-buffers and scenes would exceed this
constexpr int kAddChunk = 64;
constexpr int kMaxSide = 16384;

static void fill_result(const u32* c, lm_vsd_result* r) {
    r->rendered_gt = c[0]; r->rendered_est = c[1]; r->visible_gt = c[2]; r->visible_est = c[3];
    r->intersection = c[4]; r->combination = c[5]; r->within_tau = c[6];
    r->error = 1.f - (float)c[6] / (float)c[5];   // Benchmark.cpp: 0 / 0 (no pixel visible in either) gives NaN, kept
}

}  // namespace lmd

int lm_pose_error_vsd(lm_detector* d, const uint16_t* depth, int n_frames, int w, int h, const lm_vsd_query* q, int n, int delta, int tau,
                      lm_vsd_result* results) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (n < 0) return fail(LM_ERR_INVALID, "negative query count");
    if (n == 0) return LM_OK;
    if (!depth || !q || !results) return fail(LM_ERR_INVALID, "null argument");
    if (w < 1 || h < 1 || w > kMaxSide || h > kMaxSide || n_frames < 1) return fail(LM_ERR_INVALID, "bad frame size or frame count");
    int rc;
    if ((rc = ensure_eval(d))) return rc;
    int max_nv = 0;
    for (int k = 0; k < n; ++k) {
        if (q[k].frame < 0 || q[k].frame >= n_frames) return fail(LM_ERR_INVALID, "query " + std::to_string(k) + ": frame index out of range");
        const float* xyz; const u32* idx; int nv, ntri;
        if ((rc = render_mesh(d, q[k].mesh_idx, &xyz, &nv, &idx, &ntri))) return rc;
        max_nv = std::max(max_nv, nv);
    }
    EvalState* s = d->eval;
    const size_t npx = (size_t)w * h;
    const int C = (int)std::max<size_t>(1, std::min<size_t>(kVsdChunk, kVsdChunkBytes / (npx * 10)));
    Carve c;
    const size_t o_vp = c.take((size_t)2 * C * 16 * sizeof(float)), o_si = c.take((size_t)C * sizeof(int)),
                 o_sv = c.take((size_t)2 * C * max_nv * sizeof(float4)), o_z = c.take((size_t)2 * C * npx * 4), o_sc = c.take((size_t)C * npx * 2),
                 o_cnt = c.take((size_t)C * 8 * sizeof(u32));
    if ((rc = grow(s, c.at))) return rc;
    u8* b = s->buf;
    std::vector<float> vp((size_t)2 * C * 16);
    std::vector<int> sidx((size_t)C), frames;
    std::vector<u32> cnt((size_t)C * 8);
    for (int k0 = 0; k0 < n;) {
        // a chunk: up to C consecutive queries of one mesh; each distinct frame is copied once
        const int mesh_idx = q[k0].mesh_idx;
        int k1 = k0;
        frames.clear();
        while (k1 < n && k1 - k0 < C && q[k1].mesh_idx == mesh_idx) {
            const int f = q[k1].frame;
            int local = -1;
            for (size_t i = 0; i < frames.size(); ++i)
                if (frames[i] == f) { local = (int)i; break; }
            if (local < 0) {
                local = (int)frames.size();
                frames.push_back(f);
                HIP_TRY(hipMemcpyAsync(b + o_sc + (size_t)local * npx * 2, depth + (size_t)f * npx, npx * 2, hipMemcpyHostToDevice, s->stream));
            }
            sidx[(size_t)(k1 - k0)] = local;
            std::memcpy(&vp[(size_t)(k1 - k0) * 32], q[k1].view_proj_gt, 16 * sizeof(float));
            std::memcpy(&vp[(size_t)(k1 - k0) * 32 + 16], q[k1].view_proj_est, 16 * sizeof(float));
            ++k1;
        }
        const int nq = k1 - k0;
        const float* xyz; const u32* idx; int nv, ntri;
        if ((rc = render_mesh(d, mesh_idx, &xyz, &nv, &idx, &ntri))) return rc;
        HIP_TRY(hipMemcpyAsync(b + o_vp, vp.data(), (size_t)nq * 32 * sizeof(float), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(b + o_si, sidx.data(), (size_t)nq * sizeof(int), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemsetAsync(b + o_cnt, 0, (size_t)nq * 8 * sizeof(u32), s->stream));
        lmk_gen_zbuffer(s->stream, xyz, nv, idx, ntri, reinterpret_cast<const float*>(b + o_vp), 2 * nq, w, h, reinterpret_cast<float4*>(b + o_sv),
                        reinterpret_cast<u32*>(b + o_z));
        lmk_eval_vsd(s->stream, true, b + o_z, reinterpret_cast<const u16*>(b + o_sc), reinterpret_cast<const int*>(b + o_si), nq, npx, delta, tau,
                     reinterpret_cast<u32*>(b + o_cnt));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cnt.data(), b + o_cnt, (size_t)nq * 8 * sizeof(u32), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        for (int i = 0; i < nq; ++i) fill_result(&cnt[(size_t)i * 8], &results[k0 + i]);
        k0 = k1;
    }
    return LM_OK;
}

int lm_pose_error_add(lm_detector* d, int mesh_idx, int step, int symmetric, const lm_add_query* q, int n, float* mean_out, float* per_vertex_out) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (n < 0) return fail(LM_ERR_INVALID, "negative query count");
    if (step < 1) return fail(LM_ERR_INVALID, "step < 1");
    if (n == 0) return LM_OK;
    if (!q || !mean_out) return fail(LM_ERR_INVALID, "null argument");
    int rc;
    if ((rc = ensure_eval(d))) return rc;
    const float* xyz; const u32* idx; int nv, ntri;
    if ((rc = render_mesh(d, mesh_idx, &xyz, &nv, &idx, &ntri))) return rc;
    EvalState* s = d->eval;
    const int m = (int)(((size_t)nv + step - 1) / step);
    const int C = std::min(n, kAddChunk);
    const size_t nb = lmk_eval_add_parts(m), cm = (size_t)C * m;
    Carve c;
    const size_t o_q = c.take((size_t)C * 24 * sizeof(float)), o_gt = c.take(symmetric ? cm * sizeof(float4) : 0),
                 o_est = c.take(symmetric ? cm * sizeof(float4) : 0), o_min = c.take(symmetric ? cm * 4 : 0), o_dist = c.take(cm * 4),
                 o_part = c.take((size_t)C * nb * sizeof(double)), o_mean = c.take((size_t)C * 4);
    if ((rc = grow(s, c.at))) return rc;
    u8* b = s->buf;
    static_assert(sizeof(lm_add_query) == 24 * sizeof(float), "lm_add_query is 24 floats");
    for (int k0 = 0; k0 < n; k0 += C) {
        const int nq = std::min(C, n - k0);
        HIP_TRY(hipMemcpyAsync(b + o_q, q + k0, (size_t)nq * sizeof(lm_add_query), hipMemcpyHostToDevice, s->stream));
        lmk_eval_add(s->stream, xyz, step, m, reinterpret_cast<const float*>(b + o_q), nq, symmetric ? 1 : 0, reinterpret_cast<float4*>(b + o_gt),
                     reinterpret_cast<float4*>(b + o_est), reinterpret_cast<u32*>(b + o_min), reinterpret_cast<float*>(b + o_dist),
                     reinterpret_cast<double*>(b + o_part), reinterpret_cast<float*>(b + o_mean));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(mean_out + k0, b + o_mean, (size_t)nq * 4, hipMemcpyDeviceToHost, s->stream));
        if (per_vertex_out)
            HIP_TRY(hipMemcpyAsync(per_vertex_out + (size_t)k0 * m, b + o_dist, (size_t)nq * m * 4, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return LM_OK;
}

int lm_stage_vsd_counts(lm_detector* d, const uint16_t* gt_depth, const uint16_t* est_depth, const uint16_t* scene, int w, int h, int delta,
                        int tau, lm_vsd_result* out) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (!gt_depth || !est_depth || !scene || !out) return fail(LM_ERR_INVALID, "null argument");
    if (w < 1 || h < 1 || w > kMaxSide || h > kMaxSide) return fail(LM_ERR_INVALID, "bad image size");
    int rc;
    if ((rc = ensure_eval(d))) return rc;
    EvalState* s = d->eval;
    const size_t npx = (size_t)w * h;
    Carve c;
    const size_t o_r = c.take(npx * 4), o_sc = c.take(npx * 2), o_si = c.take(sizeof(int)), o_cnt = c.take(8 * sizeof(u32));
    if ((rc = grow(s, c.at))) return rc;
    u8* b = s->buf;
    const int zero = 0;
    u32 cnt[8];
    HIP_TRY(hipMemcpyAsync(b + o_r, gt_depth, npx * 2, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(b + o_r + npx * 2, est_depth, npx * 2, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(b + o_sc, scene, npx * 2, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(b + o_si, &zero, sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(b + o_cnt, 0, 8 * sizeof(u32), s->stream));
    lmk_eval_vsd(s->stream, false, b + o_r, reinterpret_cast<const u16*>(b + o_sc), reinterpret_cast<const int*>(b + o_si), 1, npx, delta, tau,
                 reinterpret_cast<u32*>(b + o_cnt));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cnt, b + o_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    fill_result(cnt, out);
    return LM_OK;
}
