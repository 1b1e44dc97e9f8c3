// lm_detector_icp.hip -- host side of the ICP pose refinement (0.5): resident model clouds per class, the
// refinement of a slot's frame (lm_icp_refine) and its stage hooks, and the best-pose check that follows it (0.8, lm_icp_verify*).
// Kernels: lm_k_icp.hip, lm_k_verify.hip (and lm_k_gen.hip's rasteriser).
// Per query: the scene cloud (5 launches), one read of its point count (the only host round trip of a query: it sizes the levels), then
// every round of every level that can iterate, enqueued at once for all poses of the query; one synchronisation at the end of the call.
#include "lm_detector_impl.h"

namespace lmd {

struct IcpModel { DevBuf<float> d; int n = 0; };

struct IcpState {
    Stream stream;
    std::vector<IcpModel> models;            // by class index
    DevBuf<u16> d_depth;                     // host-frame hooks: the frame's copy
    DevBuf<u8> d_buf;
    PinnedBuf<u32> h_counts;                 // pinned: the scene cloud's counts
};

void free_icp(lm_detector* d) { delete d->icp; d->icp = nullptr; }

static int ensure_icp(lm_detector* d) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if (d->icp) return LM_OK;
    std::unique_ptr<IcpState> s(new IcpState());
    hipError_t e = s->stream.create(hipStreamNonBlocking);
    if (e == hipSuccess) e = s->h_counts.alloc(4);
    // published only once complete: a later call retries instead of running on a null stream
    if (e != hipSuccess) return fail(LM_ERR_HIP, std::string("ICP stream / pinned counts: ") + hipGetErrorString(e));
    d->icp = s.release();
    return LM_OK;
}

static int grow(IcpState* s, size_t bytes) {
    if (bytes <= s->d_buf.size()) return LM_OK;
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(s->d_buf.grow(bytes));
    return LM_OK;
}

static int cv_round(double x) { return (int)std::nearbyint(x); }   // half to even under the default rounding mode, like cvRound

// The level schedule of registerModelToScene for a model of n rows and a scene of ns rows, coarsest level first.  fval_perc starts at
// 0, so a level iterates only while TolP = tolerance (level + 1)^2 <= 1 (the loop test !(fval_perc < 1 + TolP && fval_perc > 1 - TolP));
// a level whose clouds sample fewer than 6 rows cannot pair 6 points and stops at once.
static std::vector<LmIcpLevel> schedule(int n, int ns, const lm_icp_params& p) {
    std::vector<LmIcpLevel> out;
    for (int level = p.levels - 1; level >= 0; --level) {
        LmIcpLevel L{};
        L.level = level;
        const int num = std::max(cv_round((double)n / std::ldexp(1.0, level)), 1);
        L.s = std::max(cv_round((double)n / (double)num), 1);
        L.nL = n / L.s;
        L.ndL = ns / L.s;
        L.tolp = p.tolerance * (double)(level + 1) * (double)(level + 1);
        L.max_it = cv_round((double)p.iterations / (double)(level + 1));
        L.rounds = (L.tolp <= 1.0 && L.nL >= 6 && L.ndL >= 6) ? L.max_it : 0;
        out.push_back(L);
    }
    return out;
}

struct SceneLayout { size_t z, zsum, blockcnt, blockoff, counts, cloud, end; };
static SceneLayout scene_layout(size_t npx, size_t cap) {
    SceneLayout l{};
    const size_t nb = (npx + 255) / 256;
    size_t o = 0;
    l.z = o; o = align_up(o + npx * 4, 256);
    l.zsum = o; o = align_up(o + 8, 256);
    l.blockcnt = o; o = align_up(o + nb * 4, 256);
    l.blockoff = o; o = align_up(o + nb * 4, 256);
    l.counts = o; o = align_up(o + 16, 256);
    l.cloud = o; o = align_up(o + cap * 6 * sizeof(float), 256);
    l.end = o;
    return l;
}

static int check_params(const lm_icp_params* p) {
    if (!p || p->step < 1 || p->iterations < 0 || p->levels < 1 || p->levels > 30 || !(p->tolerance >= 0) || !(p->rejection_scale > 0) || p->max_points < 0)
        return fail(LM_ERR_INVALID, "bad ICP parameters");
    return LM_OK;
}

static int check_bbox(int x, int y, int w, int h, int W, int H) {
    if (w <= 0 || h <= 0) return fail(LM_ERR_INVALID, "empty bbox");
    if (x < 0 || y < 0 || x > W - w || y > H - h) return fail(LM_ERR_INVALID, "bbox outside the frame");
    return LM_OK;
}

// Scene cloud of one bbox into the scratch (base .. base + layout.end); *n = its rows (one synchronisation).
static int scene_cloud(lm_detector* d, const u16* depth, int W, int H, int x, int y, int bw, int bh, double fx, double fy, double cx, double cy,
                       int step, size_t cap, size_t base, int* n) {
    IcpState* s = d->icp;
    const size_t npx = (size_t)bw * bh;
    const SceneLayout l = scene_layout(npx, npx / step + 1);
    u8* b = s->d_buf + base;
    LmIcpSceneScratch sc{reinterpret_cast<u32*>(b + l.z), reinterpret_cast<unsigned long long*>(b + l.zsum), reinterpret_cast<u32*>(b + l.blockcnt),
                         reinterpret_cast<u32*>(b + l.blockoff), reinterpret_cast<u32*>(b + l.counts)};
    HIP_TRY(hipMemsetAsync(sc.zsum, 0, 8, s->stream));
    lmk_icp_scene(s->stream, depth, W, H, x, y, bw, bh, (float)fx, (float)fy, (float)cx, (float)cy, step, sc, reinterpret_cast<float*>(b + l.cloud));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->h_counts, sc.counts, 2 * sizeof(u32), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    *n = (int)s->h_counts[1];
    if ((size_t)*n > cap) return fail(LM_ERR_OVERFLOW, "scene cloud of " + std::to_string(*n) + " points exceeds the capacity of " + std::to_string(cap));
    return LM_OK;
}

// The refinement of every query against a W x H depth frame already on the device (on the ICP stream's order).
static int refine(lm_detector* d, const u16* depth, bool shifted_frame, const lm_icp_query* q, int nq, const lm_icp_params* p, double* poses) {
    int rc;
    IcpState* s = d->icp;
    const int W = d->cfg.width, H = d->cfg.height;
    if ((rc = check_params(p))) return rc;
    if (nq < 0 || (nq > 0 && (!q || !poses))) return fail(LM_ERR_INVALID, "bad argument");
    for (int k = 0; k < nq; ++k) {
        const lm_icp_query& e = q[k];
        if ((rc = check_bbox(e.x, e.y, e.width, e.height, W, H))) return rc;
        if (e.class_idx < 0 || e.class_idx >= (int)s->models.size() || !s->models[(size_t)e.class_idx].d)
            return fail(LM_ERR_INVALID, "class " + std::to_string(e.class_idx) + " has no ICP model (lm_icp_set_model)");
        if (e.first_pose < 0 || e.num_poses < 0) return fail(LM_ERR_INVALID, "bad pose range");
        if (!(e.fx > 0) || !(e.fy > 0)) return fail(LM_ERR_INVALID, "bad intrinsics");
    }
    int short_query = -1;
    for (int k = 0; k < nq; ++k) {
        const lm_icp_query& e = q[k];
        if (e.num_poses == 0) continue;
        const IcpModel& m = s->models[(size_t)e.class_idx];
        const size_t npx = (size_t)e.width * e.height;
        const size_t cap = p->max_points ? (size_t)p->max_points : std::min<size_t>(npx / (size_t)p->step, LM_ICP_DEFAULT_MAX_POINTS);
        const SceneLayout sl = scene_layout(npx, npx / p->step + 1);
        // ICP scratch behind the scene's, sized for the largest case of this query (the cloud's bound, cap rows)
        const size_t np = (size_t)e.num_poses, nm = (size_t)m.n, ns = std::max<size_t>(npx / p->step, 1);
        const size_t nch = (size_t)lmk_icp_nn_chunks((int)ns), nblk = (ns + 255) / 256;
        size_t o = sl.end;
        const size_t o_st = o;   o = align_up(o + np * sizeof(LmIcpPose), 256);
        const size_t o_src0 = o; o = align_up(o + np * nm * 6 * 8, 256);
        const size_t o_srcL = o; o = align_up(o + np * nm * 6 * 8, 256);
        const size_t o_part = o; o = align_up(o + np * nch * nm * sizeof(LmIcpNN), 256);
        const size_t o_nd = o;   o = align_up(o + np * nm * 4, 256);
        const size_t o_nidx = o; o = align_up(o + np * nm * 4, 256);
        const size_t o_keys = o; o = align_up(o + np * ns * 8, 256);
        const size_t o_acc = o;  o = align_up(o + np * nblk * 29 * 8, 256);
        const size_t o_out = o;  o = align_up(o + np * 16 * 8, 256);
        if ((rc = grow(s, o))) return rc;
        const double cx = shifted_frame ? 0.5 * W : e.cx, cy = shifted_frame ? 0.5 * H : e.cy;
        int n = 0;
        if ((rc = scene_cloud(d, depth, W, H, e.x, e.y, e.width, e.height, e.fx, e.fy, cx, cy, p->step, cap, 0, &n))) return rc;
        if (n < 6) { short_query = k; continue; }   // the poses stay as they are
        u8* b = s->d_buf;
        std::vector<LmIcpPose> st(np);
        for (size_t i = 0; i < np; ++i) {
            const double* P = poses + 16 * ((size_t)e.first_pose + i);
            for (int r = 0; r < 12; ++r) st[i].P[r] = P[r];
        }
        HIP_TRY(hipMemcpyAsync(b + o_st, st.data(), np * sizeof(LmIcpPose), hipMemcpyHostToDevice, s->stream));
        LmIcpScratch w{reinterpret_cast<LmIcpPose*>(b + o_st), reinterpret_cast<double*>(b + o_src0), reinterpret_cast<double*>(b + o_srcL),
                       reinterpret_cast<LmIcpNN*>(b + o_part), reinterpret_cast<float*>(b + o_nd), reinterpret_cast<int*>(b + o_nidx),
                       reinterpret_cast<unsigned long long*>(b + o_keys), reinterpret_cast<double*>(b + o_acc)};
        const std::vector<LmIcpLevel> levels = schedule(m.n, n, *p);
        lmk_icp_register(s->stream, m.d, m.n, reinterpret_cast<const float*>(b + sl.cloud), n, (int)np, levels.data(), (int)levels.size(),
                         p->rejection_scale, w, reinterpret_cast<double*>(b + o_out));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(poses + 16 * (size_t)e.first_pose, b + o_out, np * 16 * 8, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    if (short_query >= 0)
        return fail(LM_ERR_INVALID, "query " + std::to_string(short_query) + ": scene cloud of fewer than 6 points, its poses are left unchanged");
    return LM_OK;
}

// ---- the best-pose check (lm_icp_verify*): estimateBestMatch's meanDepthDifference, batched
constexpr int kVerifyChunk = 64;                          // queries per launch group ...
constexpr size_t kVerifyChunkBytes = (size_t)512 << 20;   // ... fewer when their z-buffers and scenes would exceed this
constexpr int kVerifyMaxSide = 16384;

struct VerifyRecord { u32 count, unused; unsigned long long sum; };
static_assert(sizeof(VerifyRecord) == 16, "the kernel's record is 16 bytes");

static void fill_verify(const VerifyRecord& c, lm_icp_verify_result* r) {
    r->count = c.count; r->reserved = 0; r->sum = c.sum;
    r->mean = c.count ? (double)c.sum / (double)c.count : 0.0;
}

// Queries order[0 .. m) of q at w x h, on the ICP stream.  host != null: query.frame indexes host frames of w * h pixels, each distinct
// frame of a chunk copied once; else the scene of a query is dev + query.frame * dev_stride (elements), already resident.
static int verify(lm_detector* d, const u16* host, const u16* dev, size_t dev_stride, int w, int h, const lm_icp_verify_query* q,
                  const std::vector<int>& order, int scene_min, lm_icp_verify_result* results) {
    int rc;
    IcpState* s = d->icp;
    int max_nv = 0;
    for (int k : order) {
        const float* xyz; const u32* idx; int nv, ntri;
        if ((rc = render_mesh(d, q[k].mesh_idx, &xyz, &nv, &idx, &ntri))) return rc;
        max_nv = std::max(max_nv, nv);
    }
    const size_t npx = (size_t)w * h, m = order.size();
    const size_t C = std::max<size_t>(1, std::min<size_t>({(size_t)kVerifyChunk, m, kVerifyChunkBytes / (npx * 6)}));
    size_t o = 0;
    const size_t o_vp = o;  o = align_up(o + C * 16 * sizeof(float), 256);
    const size_t o_si = o;  o = align_up(o + C * sizeof(int), 256);
    const size_t o_out = o; o = align_up(o + C * sizeof(VerifyRecord), 256);
    const size_t o_sv = o;  o = align_up(o + C * (size_t)max_nv * sizeof(float4), 256);
    const size_t o_z = o;   o = align_up(o + C * npx * 4, 256);
    const size_t o_sc = o;  o = align_up(o + (host ? C * npx * 2 : 0), 256);
    if ((rc = grow(s, o))) return rc;
    u8* b = s->d_buf;
    std::vector<float> vp(C * 16);
    std::vector<int> sidx(C), frames;
    std::vector<VerifyRecord> rec(C);
    for (size_t i0 = 0; i0 < m;) {
        // a chunk: up to C consecutive queries of one mesh
        const int mesh_idx = q[order[i0]].mesh_idx;
        size_t i1 = i0;
        frames.clear();
        while (i1 < m && i1 - i0 < C && q[order[i1]].mesh_idx == mesh_idx) {
            const lm_icp_verify_query& e = q[order[i1]];
            int local = e.frame;
            if (host) {
                local = -1;
                for (size_t i = 0; i < frames.size(); ++i)
                    if (frames[i] == e.frame) { local = (int)i; break; }
                if (local < 0) {
                    local = (int)frames.size();
                    frames.push_back(e.frame);
                    HIP_TRY(hipMemcpyAsync(b + o_sc + (size_t)local * npx * 2, host + (size_t)e.frame * npx, npx * 2, hipMemcpyHostToDevice, s->stream));
                }
            }
            sidx[i1 - i0] = local;
            std::memcpy(&vp[(i1 - i0) * 16], e.view_proj, 16 * sizeof(float));
            ++i1;
        }
        const int nq = (int)(i1 - i0);
        const float* xyz; const u32* idx; int nv, ntri;
        if ((rc = render_mesh(d, mesh_idx, &xyz, &nv, &idx, &ntri))) return rc;
        HIP_TRY(hipMemcpyAsync(b + o_vp, vp.data(), (size_t)nq * 16 * sizeof(float), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(b + o_si, sidx.data(), (size_t)nq * sizeof(int), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemsetAsync(b + o_out, 0, (size_t)nq * sizeof(VerifyRecord), s->stream));
        lmk_gen_zbuffer(s->stream, xyz, nv, idx, ntri, reinterpret_cast<const float*>(b + o_vp), nq, w, h, reinterpret_cast<float4*>(b + o_sv),
                        reinterpret_cast<u32*>(b + o_z));
        lmk_icp_verify(s->stream, true, b + o_z, host ? reinterpret_cast<const u16*>(b + o_sc) : dev, reinterpret_cast<const int*>(b + o_si),
                       host ? npx : dev_stride, nq, w, h, scene_min, reinterpret_cast<u32*>(b + o_out));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rec.data(), b + o_out, (size_t)nq * sizeof(VerifyRecord), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        for (int i = 0; i < nq; ++i) fill_verify(rec[(size_t)i], &results[order[i0 + (size_t)i]]);
        i0 = i1;
    }
    return LM_OK;
}

}  // namespace lmd

int lm_icp_set_model(lm_detector* d, int class_idx, const float* xyzn, int n, int step) {
    int rc;
    if ((rc = ensure_icp(d))) return rc;
    if (!xyzn || n <= 0 || step < 1 || class_idx < 0 || class_idx >= 4096)
        return fail(LM_ERR_INVALID, "bad argument");
    const int rows = n / step;
    if (rows < 6) return fail(LM_ERR_INVALID, "model cloud of fewer than 6 points");
    std::vector<float> h((size_t)rows * 6);
    for (int i = 0; i < rows; ++i) std::memcpy(&h[(size_t)i * 6], xyzn + (size_t)i * step * 6, 6 * sizeof(float));
    IcpState* s = d->icp;
    if ((size_t)class_idx >= s->models.size()) s->models.resize((size_t)class_idx + 1);
    IcpModel& m = s->models[(size_t)class_idx];
    HIP_TRY(hipStreamSynchronize(s->stream));
    m.n = 0;
    HIP_TRY(m.d.alloc(h.size()));
    HIP_TRY(hipMemcpy(m.d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    m.n = rows;
    return LM_OK;
}

int lm_icp_refine(lm_detector* d, int slot, const lm_icp_query* q, int nq, const lm_icp_params* p, double* poses) {
    int rc;
    if ((rc = ensure_icp(d))) return rc;
    if ((rc = check_slots(d, slot, 1))) return rc;
    if (d->cfg.num_modalities != 2) return fail(LM_ERR_INVALID, "the detector keeps no depth frame (colour-only): use lm_stage_icp_refine_host");
    Slot& sl = d->slots[(size_t)slot];
    if (!sl.has_frame) return fail(LM_ERR_INVALID, "no frame uploaded to slot");
    int expected = -1;
    if (!d->icp_slot.compare_exchange_strong(expected, slot)) return fail(LM_ERR_INVALID, "an ICP refinement is already in flight on this detector");
    // ordered after the slot's last upload on the copy streams (frames uploaded inline by lm_match have landed already)
    if (sl.up_seq > 0 && hipStreamWaitEvent(d->icp->stream, sl.ev_up, 0) != hipSuccess) {
        d->icp_slot.store(-1);
        return fail(LM_ERR_HIP, "hipStreamWaitEvent failed");
    }
    rc = refine(d, d->depth(slot), true, q, nq, p, poses);
    d->icp_slot.store(-1);
    return rc;
}

int lm_stage_icp_refine_host(lm_detector* d, const uint16_t* depth, const lm_icp_query* q, int nq, const lm_icp_params* p, double* poses) {
    int rc;
    if ((rc = ensure_icp(d))) return rc;
    if (!depth) return fail(LM_ERR_INVALID, "bad argument");
    IcpState* s = d->icp;
    const size_t bytes = (size_t)d->cfg.width * d->cfg.height * 2;
    if (bytes / 2 > s->d_depth.size()) {
        HIP_TRY(hipStreamSynchronize(s->stream));
        HIP_TRY(s->d_depth.grow(bytes / 2));
    }
    HIP_TRY(hipMemcpyAsync(s->d_depth, depth, bytes, hipMemcpyHostToDevice, s->stream));
    return refine(d, s->d_depth, false, q, nq, p, poses);
}

int lm_stage_icp_scene(lm_detector* d, const uint16_t* depth, int w, int h, const double* K, const int32_t* bbox, int step, float* out, size_t cap,
                       int* n_out) {
    int rc;
    if ((rc = ensure_icp(d))) return rc;
    if (!depth || !K || !bbox || !out || !n_out || w < 2 || h < 2 || step < 1) return fail(LM_ERR_INVALID, "bad argument");   // REFLECT_101 needs 2 pixels
    if ((rc = check_bbox(bbox[0], bbox[1], bbox[2], bbox[3], w, h))) return rc;
    IcpState* s = d->icp;
    const size_t npx = (size_t)bbox[2] * bbox[3];
    const SceneLayout l = scene_layout(npx, npx / step + 1);
    const size_t o_depth = align_up(l.end, 256), bytes = (size_t)w * h * 2;
    if ((rc = grow(s, o_depth + bytes))) return rc;
    u16* dd = reinterpret_cast<u16*>(s->d_buf + o_depth);
    HIP_TRY(hipMemcpyAsync(dd, depth, bytes, hipMemcpyHostToDevice, s->stream));
    int n = 0;
    rc = scene_cloud(d, dd, w, h, bbox[0], bbox[1], bbox[2], bbox[3], K[0], K[1], K[2], K[3], step, cap, 0, &n);
    *n_out = n;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, s->d_buf + l.cloud, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return LM_OK;
}

int lm_stage_icp_verify_host(lm_detector* d, const uint16_t* depth, int n_frames, int w, int h, const lm_icp_verify_query* q, int n, int scene_min,
                             lm_icp_verify_result* results) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (n < 0) return fail(LM_ERR_INVALID, "negative query count");
    if (n == 0) return LM_OK;
    if (!depth || !q || !results) return fail(LM_ERR_INVALID, "null argument");
    if (w < 1 || h < 1 || w > kVerifyMaxSide || h > kVerifyMaxSide || n_frames < 1) return fail(LM_ERR_INVALID, "bad frame size or frame count");
    int rc;
    if ((rc = ensure_icp(d))) return rc;
    std::vector<int> order((size_t)n);
    for (int k = 0; k < n; ++k) {
        if (q[k].frame < 0 || q[k].frame >= n_frames) return fail(LM_ERR_INVALID, "query " + std::to_string(k) + ": frame index out of range");
        order[(size_t)k] = k;
    }
    return verify(d, depth, nullptr, 0, w, h, q, order, scene_min, results);
}

int lm_icp_verify(lm_detector* d, const lm_icp_verify_query* q, int n, int scene_min, lm_icp_verify_result* results) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (n < 0) return fail(LM_ERR_INVALID, "negative query count");
    if (n == 0) return LM_OK;
    if (!q || !results) return fail(LM_ERR_INVALID, "null argument");
    int rc;
    if ((rc = ensure_icp(d))) return rc;
    if (d->cfg.num_modalities != 2) return fail(LM_ERR_INVALID, "the detector keeps no depth frame (colour-only): use lm_stage_icp_verify_host");
    std::vector<int> slots;   // distinct, in the order of their first query
    for (int k = 0; k < n; ++k) {
        if ((rc = check_slots(d, q[k].frame, 1))) return rc;
        if (!d->slots[(size_t)q[k].frame].has_frame) return fail(LM_ERR_INVALID, "query " + std::to_string(k) + ": no frame uploaded to slot");
        const float* xyz; const u32* idx; int nv, ntri;
        if ((rc = render_mesh(d, q[k].mesh_idx, &xyz, &nv, &idx, &ntri))) return rc;
        if (std::find(slots.begin(), slots.end(), q[k].frame) == slots.end()) slots.push_back(q[k].frame);
    }
    // slot by slot: the slot is claimed against uploads (as lm_icp_refine claims its one) while its queries run
    std::vector<int> order;
    for (int slot : slots) {
        order.clear();
        for (int k = 0; k < n; ++k)
            if (q[k].frame == slot) order.push_back(k);
        Slot& sl = d->slots[(size_t)slot];
        int expected = -1;
        if (!d->icp_slot.compare_exchange_strong(expected, slot)) return fail(LM_ERR_INVALID, "an ICP refinement is already in flight on this detector");
        // ordered after the slot's last upload on the copy streams (frames uploaded inline by lm_match have landed already)
        if (sl.up_seq > 0 && hipStreamWaitEvent(d->icp->stream, sl.ev_up, 0) != hipSuccess) {
            d->icp_slot.store(-1);
            return fail(LM_ERR_HIP, "hipStreamWaitEvent failed");
        }
        rc = verify(d, nullptr, d->depth(0), d->frame_stride / sizeof(u16), d->cfg.width, d->cfg.height, q, order, scene_min, results);
        d->icp_slot.store(-1);
        if (rc) return rc;
    }
    return LM_OK;
}

int lm_stage_icp_verify_counts(lm_detector* d, const uint16_t* render, const uint16_t* scene, int w, int h, int scene_min, lm_icp_verify_result* out) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (!render || !scene || !out) return fail(LM_ERR_INVALID, "null argument");
    if (w < 1 || h < 1 || w > kVerifyMaxSide || h > kVerifyMaxSide) return fail(LM_ERR_INVALID, "bad image size");
    int rc;
    if ((rc = ensure_icp(d))) return rc;
    IcpState* s = d->icp;
    const size_t npx = (size_t)w * h;
    const size_t o_r = 0, o_sc = align_up(npx * 2, 256), o_si = align_up(o_sc + npx * 2, 256), o_out = o_si + 256;
    if ((rc = grow(s, o_out + 256))) return rc;
    u8* b = s->d_buf;
    VerifyRecord rec;
    HIP_TRY(hipMemcpyAsync(b + o_r, render, npx * 2, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(b + o_sc, scene, npx * 2, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(b + o_si, 0, 512, s->stream));   // the scene index (0) and the record
    lmk_icp_verify(s->stream, false, b + o_r, reinterpret_cast<const u16*>(b + o_sc), reinterpret_cast<const int*>(b + o_si), npx, 1, w, h, scene_min,
                   reinterpret_cast<u32*>(b + o_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&rec, b + o_out, sizeof(rec), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    fill_verify(rec, out);
    return LM_OK;
}
