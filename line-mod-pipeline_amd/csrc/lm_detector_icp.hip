// lm_detector_icp.hip -- host side of the ICP pose refinement (0.5): resident model clouds per class, the
// refinement of a slot's frame (lm_icp_refine) and its stage hooks, and the best-pose check that follows it (0.8, lm_icp_verify*).
// Kernels: lm_k_icp.hip, lm_k_verify.hip (and lm_k_gen.hip's rasteriser).
// A refinement takes a list of queries, each against the frame of a slot of its own (lm_icp_refine_slots; lm_icp_refine and the host-frame
// hook are its one-frame case), and runs them in chunks (the plan: lm_host.h plan_icp_batch / plan_icp_levels).  Per
// chunk: the scene clouds of all its queries (5 launches), one read of their point counts (the only host round trip before the rounds: it
// sizes the levels), then every round of every level that can iterate for any query, enqueued at once for all poses of all live queries;
// one copy of the refined poses and one synchronisation at the end of the chunk.
#include "lm_detector_impl.h"

namespace lmd {

struct IcpModel { DevBuf<float> d; int n = 0; };

struct IcpState {
    Stream stream;
    std::vector<IcpModel> models;            // by class index
    DevBuf<u16> d_depth;                     // host-frame hooks: the frame's copy
    DevBuf<u8> d_buf;
    PinnedBuf<u8> h_pin;                     // pinned: a chunk's count pairs, then its refined poses
    int stats[3] = {0, 0, 0};                // the last refinement's chunks, kernel launches and host synchronisations (lm_stage_icp_batch_stats)
};

void free_icp(lm_detector* d) { delete d->icp; d->icp = nullptr; }

static int ensure_icp(lm_detector* d) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if (d->icp) return LM_OK;
    std::unique_ptr<IcpState> s(new IcpState());
    hipError_t e = s->stream.create(hipStreamNonBlocking);
    if (e == hipSuccess) e = s->h_pin.alloc(4096);
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

static int grow_pinned(IcpState* s, size_t bytes) {
    if (bytes <= s->h_pin.size()) return LM_OK;
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(s->h_pin.grow(bytes));
    return LM_OK;
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

// What a refinement refuses before it enqueues or claims anything
static int check_queries(lm_detector* d, const lm_icp_query* q, int nq, const lm_icp_params* p, const double* poses) {
    int rc;
    IcpState* s = d->icp;
    if ((rc = check_params(p))) return rc;
    if (nq < 0 || (nq > 0 && (!q || !poses))) return fail(LM_ERR_INVALID, "bad argument");
    for (int k = 0; k < nq; ++k) {
        const lm_icp_query& e = q[k];
        if ((rc = check_bbox(e.x, e.y, e.width, e.height, d->cfg.width, d->cfg.height))) return rc;
        if (e.class_idx < 0 || e.class_idx >= (int)s->models.size() || !s->models[(size_t)e.class_idx].d)
            return fail(LM_ERR_INVALID, "class " + std::to_string(e.class_idx) + " has no ICP model (lm_icp_set_model)");
        if (e.first_pose < 0 || e.num_poses < 0) return fail(LM_ERR_INVALID, "bad pose range");
        if (!(e.fx > 0) || !(e.fy > 0)) return fail(LM_ERR_INVALID, "bad intrinsics");
    }
    return LM_OK;
}

// The slots [lo, hi] an ICP call reads are claimed against uploads from other threads while it runs (refuse_checked_slots); one call at a time
static int claim_span(lm_detector* d, int lo, int hi) {
    long long expected = -1;
    if (!d->icp_span.compare_exchange_strong(expected, ((long long)lo << 32) | (long long)hi))
        return fail(LM_ERR_INVALID, "an ICP refinement is already in flight on this detector");
    return LM_OK;
}
static void release_span(lm_detector* d) { d->icp_span.store(-1); }

// The ICP stream waits for the last upload of every distinct slot on the copy streams (frames uploaded inline by lm_match have landed already)
static int wait_slot_uploads(lm_detector* d, std::vector<int> slots) {
    std::sort(slots.begin(), slots.end());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    for (int slot : slots) {
        Slot& sl = d->slots[(size_t)slot];
        if (sl.up_seq > 0 && hipStreamWaitEvent(d->icp->stream, sl.ev_up, 0) != hipSuccess) return fail(LM_ERR_HIP, "hipStreamWaitEvent failed");
    }
    return LM_OK;
}

// One chunk's scene clouds (phases a and b of DESIGN.md section 21): the records, five launches, one copy of all count pairs, one
// synchronisation.  rows[k] = the points of chunk query k.
static int scene_clouds(lm_detector* d, const lmh::IcpChunkPlan& c, const std::vector<LmIcpSceneRec>& recs, int W, int H, int step, LmIcpBatchArgs* args,
                        std::vector<int>* rows) {
    int rc;
    IcpState* s = d->icp;
    const size_t nq = c.q.size();
    if ((rc = grow(s, c.bytes)) || (rc = grow_pinned(s, nq * 2 * sizeof(u32)))) return rc;
    u8* b = s->d_buf;
    LmIcpBatchArgs a{};
    a.base = b;
    a.scene = reinterpret_cast<const LmIcpSceneRec*>(b + c.scene_recs);
    a.zsum = reinterpret_cast<unsigned long long*>(b + c.zsum);
    a.counts = reinterpret_cast<u32*>(b + c.counts);
    a.reg = reinterpret_cast<const LmIcpRegRec*>(b + c.reg_recs);
    a.lev = reinterpret_cast<const LmIcpLevel*>(b + c.levels);
    a.st = reinterpret_cast<LmIcpPose*>(b + c.st);
    a.out = reinterpret_cast<double*>(b + c.out);
    a.W = W; a.H = H; a.step = step; a.nlevels = c.nlevels;
    HIP_TRY(hipMemcpyAsync(b + c.scene_recs, recs.data(), nq * sizeof(LmIcpSceneRec), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(a.zsum, 0, nq * 8, s->stream));
    lmk_icp_scene(s->stream, c, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->h_pin, a.counts, nq * 2 * sizeof(u32), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->stats[1] += 5; s->stats[2] += 1;
    const u32* hc = reinterpret_cast<const u32*>(s->h_pin.get());
    rows->resize(nq);
    for (size_t k = 0; k < nq; ++k) (*rows)[k] = (int)hc[2 * k + 1];
    *args = a;
    return LM_OK;
}

static LmIcpSceneRec scene_rec(const lmh::IcpQueryPlan& e, const u16* depth, int x, int y, int bw, int bh, double fx, double fy, double cx, double cy) {
    LmIcpSceneRec r{};
    r.depth = depth;
    r.x0 = x; r.y0 = y; r.bw = bw; r.bh = bh; r.npx = e.npx; r.nb = e.nb;
    r.fx = (float)fx; r.fy = (float)fy; r.cx = (float)cx; r.cy = (float)cy;
    r.z = e.z; r.blockcnt = e.blockcnt; r.blockoff = e.blockoff; r.cloud = e.cloud;
    return r;
}

// The refinement of every query (checked by check_queries) against the W x H depth frame depth[k] of query k, already on the device in
// the ICP stream's order.  The queries run in chunks (lm_host.h plan_icp_batch); per chunk: the scene clouds of all its queries, one read
// of their counts (the only host round trip before the rounds: it sizes the levels), every round of every level of all poses of its live
// queries, one copy of the refined poses, one synchronisation.  status (may be null) receives every query's code; the return value is the
// first non-OK one.
static int refine(lm_detector* d, const u16* const* depth, bool shifted_frame, const lm_icp_query* q, int nq, const lm_icp_params* p, double* poses,
                  int32_t* status) {
    int rc;
    IcpState* s = d->icp;
    const int W = d->cfg.width, H = d->cfg.height;
    std::vector<lmh::IcpQueryIn> in((size_t)std::max(nq, 0));
    for (int k = 0; k < nq; ++k) {
        lmh::IcpQueryIn& e = in[(size_t)k];
        e.npx = q[k].width * q[k].height;
        e.nm = s->models[(size_t)q[k].class_idx].n;
        e.first_pose = q[k].first_pose; e.np = q[k].num_poses;
    }
    lmh::IcpBatchPlan plan;
    lmh::plan_icp_batch(in, p->step, p->levels, (size_t)d->icp_batch_mb << 20, plan);
    for (int k = 0; k < nq && status; ++k) status[k] = LM_OK;
    s->stats[0] = (int)plan.chunks.size(); s->stats[1] = s->stats[2] = 0;
    int bad = -1, bad_code = LM_OK;
    std::string bad_msg;
    std::vector<LmIcpSceneRec> srec;
    std::vector<LmIcpRegRec> rrec;
    std::vector<LmIcpPose> st;
    std::vector<int> rows;
    lmh::IcpLevelsPlan lp;
    for (const lmh::IcpChunkPlan& c : plan.chunks) {
        const size_t nqc = c.q.size();
        srec.resize(nqc);
        for (size_t k = 0; k < nqc; ++k) {
            const lm_icp_query& e = q[c.q[k].query];
            srec[k] = scene_rec(c.q[k], depth[c.q[k].query], e.x, e.y, e.width, e.height, e.fx, e.fy, shifted_frame ? 0.5 * W : e.cx,
                                shifted_frame ? 0.5 * H : e.cy);
        }
        LmIcpBatchArgs a;
        if ((rc = scene_clouds(d, c, srec, W, H, p->step, &a, &rows))) return rc;
        for (size_t k = 0; k < nqc; ++k) {
            const int qi = c.q[k].query, n = rows[k];
            const size_t npx = (size_t)c.q[k].npx;
            const size_t cap = p->max_points ? (size_t)p->max_points : std::min<size_t>(npx / (size_t)p->step, LM_ICP_DEFAULT_MAX_POINTS);
            int code = LM_OK;
            std::string msg;
            if ((size_t)n > cap) {
                code = LM_ERR_OVERFLOW;
                msg = "query " + std::to_string(qi) + ": scene cloud of " + std::to_string(n) + " points exceeds the capacity of " + std::to_string(cap) +
                      ", its poses are left unchanged";
            } else if (n < 6) {
                code = LM_ERR_INVALID;
                msg = "query " + std::to_string(qi) + ": scene cloud of fewer than 6 points, its poses are left unchanged";
            }
            if (code == LM_OK) continue;
            rows[k] = -1;
            if (status) status[qi] = code;
            if (bad < 0 || qi < bad) { bad = qi; bad_code = code; bad_msg = msg; }
        }
        lmh::plan_icp_levels(c, rows, p->iterations, p->levels, p->tolerance, lp);
        if (lp.np == 0) continue;
        rrec.assign(nqc, LmIcpRegRec{});
        st.assign((size_t)lp.np, LmIcpPose{});
        for (size_t k = 0; k < nqc; ++k) {
            const lmh::IcpQueryPlan& e = c.q[k];
            LmIcpRegRec& r = rrec[k];
            r.model = s->models[(size_t)q[e.query].class_idx].d;
            r.nm = e.nm; r.ns = std::max(rows[k], 0); r.nch_cap = e.nch_cap; r.nblk_cap = e.nblk_cap;
            r.cloud = e.cloud; r.src0 = e.src0; r.srcL = e.srcL; r.part = e.part; r.nd = e.nd; r.nidx = e.nidx; r.keys = e.keys; r.acc = e.acc;
            if (lp.pose0[k] < 0) continue;
            for (int i = 0; i < e.np; ++i) {
                LmIcpPose& t = st[(size_t)lp.pose0[k] + (size_t)i];
                const double* P = poses + 16 * ((size_t)q[e.query].first_pose + (size_t)i);
                for (int r12 = 0; r12 < 12; ++r12) t.P[r12] = P[r12];
                t.q = (int)k; t.li = i;
            }
        }
        u8* b = s->d_buf;
        if ((rc = grow_pinned(s, (size_t)lp.np * 16 * sizeof(double)))) return rc;
        a.rejection_scale = p->rejection_scale;
        HIP_TRY(hipMemcpyAsync(b + c.reg_recs, rrec.data(), nqc * sizeof(LmIcpRegRec), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(b + c.levels, lp.lev.data(), lp.lev.size() * sizeof(LmIcpLevel), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(b + c.st, st.data(), st.size() * sizeof(LmIcpPose), hipMemcpyHostToDevice, s->stream));
        lmk_icp_register(s->stream, lp, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(s->h_pin, a.out, (size_t)lp.np * 16 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->stats[2] += 1; s->stats[1] += 2;
        for (const lmh::IcpLevelLaunch& g : lp.level) s->stats[1] += g.rounds ? 1 + 5 * g.rounds : 0;
        const double* ho = reinterpret_cast<const double*>(s->h_pin.get());
        for (size_t k = 0; k < nqc; ++k)
            if (lp.pose0[k] >= 0)
                std::memcpy(poses + 16 * (size_t)q[c.q[k].query].first_pose, ho + 16 * (size_t)lp.pose0[k], (size_t)c.q[k].np * 16 * sizeof(double));
    }
    if (bad >= 0) return fail(bad_code, bad_msg);
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

int lm_icp_refine_slots(lm_detector* d, const int32_t* slots, const lm_icp_query* q, int nq, const lm_icp_params* p, double* poses, int32_t* status) {
    int rc;
    if ((rc = ensure_icp(d))) return rc;
    if (nq < 0 || (nq > 0 && (!slots || !q || !poses))) return fail(LM_ERR_INVALID, "bad argument");
    // (looked at first, claimed last: a call that is refused for another reason never holds the claim, not even for a moment)
    if (d->icp_span.load() >= 0) return fail(LM_ERR_INVALID, "an ICP refinement is already in flight on this detector");
    if (!keeps_depth(d)) return fail(LM_ERR_INVALID, "the detector keeps no depth frame (colour-only): use lm_stage_icp_refine_host");
    int lo = INT_MAX, hi = -1;
    for (int k = 0; k < nq; ++k) {
        if ((rc = check_slots(d, slots[k], 1))) return rc;
        if (!d->slots[(size_t)slots[k]].has_frame) return fail(LM_ERR_INVALID, "query " + std::to_string(k) + ": no frame uploaded to slot");
        if ((rc = slot_lacks_depth(d, slots[k]))) return rc;
        lo = std::min(lo, (int)slots[k]); hi = std::max(hi, (int)slots[k]);
    }
    if ((rc = check_queries(d, q, nq, p, poses))) return rc;
    if (nq == 0) return LM_OK;
    if ((rc = claim_span(d, lo, hi))) return rc;
    std::vector<const u16*> depth((size_t)nq);
    for (int k = 0; k < nq; ++k) depth[(size_t)k] = d->depth(slots[k]);
    if (!(rc = wait_slot_uploads(d, std::vector<int>(slots, slots + nq)))) rc = refine(d, depth.data(), true, q, nq, p, poses, status);
    release_span(d);
    return rc;
}

int lm_icp_refine(lm_detector* d, int slot, const lm_icp_query* q, int nq, const lm_icp_params* p, double* poses) {
    int rc;
    if ((rc = ensure_icp(d))) return rc;
    if ((rc = check_slots(d, slot, 1))) return rc;
    if (!keeps_depth(d)) return fail(LM_ERR_INVALID, "the detector keeps no depth frame (colour-only): use lm_stage_icp_refine_host");
    if (!d->slots[(size_t)slot].has_frame) return fail(LM_ERR_INVALID, "no frame uploaded to slot");
    if ((rc = slot_lacks_depth(d, slot))) return rc;
    if ((rc = check_queries(d, q, nq, p, poses))) return rc;
    if ((rc = claim_span(d, slot, slot))) return rc;
    const std::vector<const u16*> depth((size_t)std::max(nq, 1), d->depth(slot));
    if (!(rc = wait_slot_uploads(d, {slot}))) rc = refine(d, depth.data(), true, q, nq, p, poses, nullptr);
    release_span(d);
    return rc;
}

int lm_stage_icp_batch_stats(lm_detector* d, int32_t* out) {
    if (!d || !out) return fail(LM_ERR_INVALID, "null argument");
    for (int i = 0; i < 3; ++i) out[i] = d->icp ? d->icp->stats[i] : 0;
    return LM_OK;
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
    if ((rc = check_queries(d, q, nq, p, poses))) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_depth, depth, bytes, hipMemcpyHostToDevice, s->stream));
    const std::vector<const u16*> frames((size_t)std::max(nq, 1), s->d_depth.get());
    return refine(d, frames.data(), false, q, nq, p, poses, nullptr);
}

int lm_stage_icp_scene(lm_detector* d, const uint16_t* depth, int w, int h, const double* K, const int32_t* bbox, int step, float* out, size_t cap,
                       int* n_out) {
    int rc;
    if ((rc = ensure_icp(d))) return rc;
    if (!depth || !K || !bbox || !out || !n_out || w < 2 || h < 2 || step < 1) return fail(LM_ERR_INVALID, "bad argument");   // REFLECT_101 needs 2 pixels
    if ((rc = check_bbox(bbox[0], bbox[1], bbox[2], bbox[3], w, h))) return rc;
    IcpState* s = d->icp;
    // the one-query case of a refinement's scene phase (a query without poses to refine: one model row stands in)
    lmh::IcpBatchPlan plan;
    lmh::plan_icp_batch({lmh::IcpQueryIn{bbox[2] * bbox[3], 1, 0, 1}}, step, 1, ~(size_t)0, plan);
    const lmh::IcpChunkPlan& c = plan.chunks[0];
    const size_t o_depth = align_up(c.bytes, 256), bytes = (size_t)w * h * 2;
    if ((rc = grow(s, o_depth + bytes))) return rc;
    u16* dd = reinterpret_cast<u16*>(s->d_buf + o_depth);
    HIP_TRY(hipMemcpyAsync(dd, depth, bytes, hipMemcpyHostToDevice, s->stream));
    const std::vector<LmIcpSceneRec> rec(1, scene_rec(c.q[0], dd, bbox[0], bbox[1], bbox[2], bbox[3], K[0], K[1], K[2], K[3]));
    LmIcpBatchArgs a;
    std::vector<int> rows;
    if ((rc = scene_clouds(d, c, rec, w, h, step, &a, &rows))) return rc;
    const int n = rows[0];
    *n_out = n;
    if ((size_t)n > cap) return fail(LM_ERR_OVERFLOW, "scene cloud of " + std::to_string(n) + " points exceeds the capacity of " + std::to_string(cap));
    HIP_TRY(hipMemcpyAsync(out, s->d_buf + c.q[0].cloud, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost, s->stream));
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
    if (!keeps_depth(d)) return fail(LM_ERR_INVALID, "the detector keeps no depth frame (colour-only): use lm_stage_icp_verify_host");
    std::vector<int> slots((size_t)n), order((size_t)n);
    int lo = INT_MAX, hi = -1;
    for (int k = 0; k < n; ++k) {
        if ((rc = check_slots(d, q[k].frame, 1))) return rc;
        if (!d->slots[(size_t)q[k].frame].has_frame) return fail(LM_ERR_INVALID, "query " + std::to_string(k) + ": no frame uploaded to slot");
        if ((rc = slot_lacks_depth(d, q[k].frame))) return rc;
        const float* xyz; const u32* idx; int nv, ntri;
        if ((rc = render_mesh(d, q[k].mesh_idx, &xyz, &nv, &idx, &ntri))) return rc;
        slots[(size_t)k] = q[k].frame; order[(size_t)k] = k;
        lo = std::min(lo, (int)q[k].frame); hi = std::max(hi, (int)q[k].frame);
    }
    // the chunks run across the slots (a query names its scene): the span of slots is claimed against uploads, as lm_icp_refine_slots
    // claims its span, and the stream waits for every distinct slot's last upload first
    if ((rc = claim_span(d, lo, hi))) return rc;
    if (!(rc = wait_slot_uploads(d, slots)))
        rc = verify(d, nullptr, d->depth(0), d->frame_stride / sizeof(u16), d->cfg.width, d->cfg.height, q, order, scene_min, results);
    release_span(d);
    return rc;
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
