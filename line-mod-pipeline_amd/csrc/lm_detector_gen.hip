// lm_detector_gen.hip -- host side of template-bank generation on the GPU (0.6): resident render meshes,
// lm_add_templates_rendered and its stage hooks.  Kernels: lm_k_gen.hip.
// Per chunk of at most frame_slots images (view-major, angle-minor): render the chunk's views, rotate + erode into the slots, the existing
// quantisers over all the chunk's slots, the candidate counts (one read-back), the candidate lists (a second read-back), then the
// selection on up to 16 host threads and the bbox crops of the rotated depth.  Nothing else of a full frame comes back to the host.
#include "lm_detector_impl.h"

#include <thread>

namespace lmd {

struct GenMesh { DevBuf<float> xyz; DevBuf<u32> idx; int nv = 0, ntri = 0; };

struct GenState {
    GenMesh meshes[LM_MAX_RENDER_MESHES];
    DevBuf<u8> buf;
    DevBuf<LmGenCand> cand;
};

void free_gen(lm_detector* d) { delete d->gen; d->gen = nullptr; }

static GenState& gen(lm_detector* d) {
    if (!d->gen) d->gen = new GenState();
    return *d->gen;
}

static int grow_buf(lm_detector* d, size_t bytes) {
    GenState& s = gen(d);
    if (bytes <= s.buf.size()) return LM_OK;
    HIP_TRY(hipStreamSynchronize(d->lanes[0].stream));
    HIP_TRY(s.buf.grow(bytes));
    return LM_OK;
}

// warpAffine's inverse of getRotationMatrix2D(Point2f(w / 2, h / 2), angle, 1.0) and its fixed-point source coordinates, as
// TemplateGenerator.cpp's inverse_rotation / src_coord compute them (double on the host: the device only adds and shifts integers)
static void angle_table(int w, int h, float angleDegrees, int* tab) {
    double angle = angleDegrees * 3.14159265358979323846 / 180.0;
    double alpha = std::cos(angle), beta = std::sin(angle);
    double cx = (double)(w / 2), cy = (double)(h / 2);
    double M[6] = {alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy};
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
    double b1 = -M[0] * M[2] - M[1] * M[5], b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
    const int AB_BITS = 10, AB_SCALE = 1 << AB_BITS, round_delta = AB_SCALE / 32 / 2;
    for (int x = 0; x < w; ++x) {
        tab[x] = (int)std::lrint(M[0] * x * AB_SCALE);
        tab[w + x] = (int)std::lrint(M[3] * x * AB_SCALE);
    }
    for (int y = 0; y < h; ++y) {
        tab[2 * w + y] = (int)std::lrint((M[1] * y + M[2]) * AB_SCALE) + round_delta;
        tab[2 * w + h + y] = (int)std::lrint((M[4] * y + M[5]) * AB_SCALE) + round_delta;
    }
}

// sub-allocation of the generation buffer
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at = align_up(at + bytes, 256); return o; }
};

static int check_mesh(lm_detector* d, int mesh_idx) {
    if (mesh_idx < 0 || mesh_idx >= LM_MAX_RENDER_MESHES) return fail(LM_ERR_INVALID, "render mesh index out of range");
    if (!d->gen || !d->gen->meshes[mesh_idx].xyz) return fail(LM_ERR_INVALID, "no render mesh under this index (lm_set_render_mesh)");
    return LM_OK;
}

int render_mesh(lm_detector* d, int mesh_idx, const float** xyz, int* nv, const u32** idx, int* ntri) {
    int rc;
    if ((rc = check_mesh(d, mesh_idx))) return rc;
    const GenMesh& m = d->gen->meshes[mesh_idx];
    *xyz = m.xyz; *nv = m.nv; *idx = m.idx; *ntri = m.ntri;
    return LM_OK;
}

}  // namespace lmd

int lm_set_render_mesh(lm_detector* d, int mesh_idx, const float* xyz, int n_vertices, const uint32_t* indices, int n_indices) {
    if (d && any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (!d || !xyz || !indices) return fail(LM_ERR_INVALID, "null argument");
    if (mesh_idx < 0 || mesh_idx >= LM_MAX_RENDER_MESHES) return fail(LM_ERR_INVALID, "render mesh index out of range");
    if (n_vertices <= 0 || n_indices <= 0 || n_indices % 3 != 0) return fail(LM_ERR_INVALID, "a render mesh needs vertices and whole triangles");
    for (int i = 0; i < n_indices; ++i)
        if (indices[i] >= (uint32_t)n_vertices) return fail(LM_ERR_INVALID, "render mesh index beyond the vertices");
    for (int i = 0; i < 3 * n_vertices; ++i)
        if (!std::isfinite(xyz[i])) return fail(LM_ERR_INVALID, "render mesh vertex is not finite");
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    GenMesh& m = gen(d).meshes[mesh_idx];
    HIP_TRY(hipStreamSynchronize(d->lanes[0].stream));
    m = GenMesh();
    HIP_TRY(m.xyz.alloc((size_t)n_vertices * 3));
    HIP_TRY(m.idx.alloc((size_t)n_indices));
    HIP_TRY(hipMemcpy(m.xyz, xyz, (size_t)n_vertices * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m.idx, indices, (size_t)n_indices * sizeof(u32), hipMemcpyHostToDevice));
    m.nv = n_vertices; m.ntri = n_indices / 3;
    return LM_OK;
}

int lm_stage_render(lm_detector* d, int mesh_idx, const float* view_proj, int w, int h, uint8_t* coverage, uint16_t* depth) {
    if (d && any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (!d || !view_proj || !coverage || !depth || w < 1 || h < 1) return fail(LM_ERR_INVALID, "bad argument");
    int rc;
    if ((rc = check_mesh(d, mesh_idx))) return rc;
    if ((rc = ready_for_compute(d))) return rc;
    const GenMesh& m = d->gen->meshes[mesh_idx];
    const size_t npx = (size_t)w * h;
    Carve c;
    const size_t o_vp = c.take(16 * sizeof(float)), o_sv = c.take((size_t)m.nv * sizeof(float4)), o_z = c.take(npx * 4),
                 o_cov = c.take(npx), o_dep = c.take(npx * 2);
    if ((rc = grow_buf(d, c.at))) return rc;
    u8* b = d->gen->buf;
    HIP_TRY(hipMemcpyAsync(b + o_vp, view_proj, 16 * sizeof(float), hipMemcpyHostToDevice, d->lanes[0].stream));
    lmk_gen_render(d->lanes[0].stream, m.xyz, m.nv, m.idx, m.ntri, reinterpret_cast<float*>(b + o_vp), 1, w, h, reinterpret_cast<float4*>(b + o_sv),
                   reinterpret_cast<u32*>(b + o_z), b + o_cov, reinterpret_cast<u16*>(b + o_dep));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(coverage, b + o_cov, npx, hipMemcpyDeviceToHost, d->lanes[0].stream));
    HIP_TRY(hipMemcpyAsync(depth, b + o_dep, npx * 2, hipMemcpyDeviceToHost, d->lanes[0].stream));
    HIP_TRY(hipStreamSynchronize(d->lanes[0].stream));
    return LM_OK;
}

int lm_stage_rotate(lm_detector* d, const uint8_t* src8, const uint16_t* src16, int w, int h, float angle_deg, uint8_t* dst8, uint16_t* dst16) {
    if (d && any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (!d || !src8 || !src16 || !dst8 || !dst16 || w < 1 || h < 1) return fail(LM_ERR_INVALID, "bad argument");
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    const size_t npx = (size_t)w * h;
    std::vector<int> tab((size_t)(2 * w + 2 * h));
    angle_table(w, h, angle_deg, tab.data());
    Carve c;
    const size_t o_tab = c.take(tab.size() * 4), o_iv = c.take(8), o_s8 = c.take(npx), o_s16 = c.take(npx * 2), o_d8 = c.take(npx),
                 o_d16 = c.take(npx * 2), o_bgr = c.take(npx * 3);
    if ((rc = grow_buf(d, c.at))) return rc;
    u8* b = d->gen->buf;
    const int zero[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(b + o_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, d->lanes[0].stream));
    HIP_TRY(hipMemcpyAsync(b + o_iv, zero, 8, hipMemcpyHostToDevice, d->lanes[0].stream));
    HIP_TRY(hipMemcpyAsync(b + o_s8, src8, npx, hipMemcpyHostToDevice, d->lanes[0].stream));
    HIP_TRY(hipMemcpyAsync(b + o_s16, src16, npx * 2, hipMemcpyHostToDevice, d->lanes[0].stream));
    const int* iv = reinterpret_cast<const int*>(b + o_iv);
    lmk_gen_rotate(d->lanes[0].stream, b + o_s8, reinterpret_cast<u16*>(b + o_s16), iv, iv + 1, reinterpret_cast<int*>(b + o_tab), 1, w, h, b + o_d8,
                   reinterpret_cast<u16*>(b + o_d16), b + o_bgr, nullptr, 0, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst8, b + o_d8, npx, hipMemcpyDeviceToHost, d->lanes[0].stream));
    HIP_TRY(hipMemcpyAsync(dst16, b + o_d16, npx * 2, hipMemcpyDeviceToHost, d->lanes[0].stream));
    HIP_TRY(hipStreamSynchronize(d->lanes[0].stream));
    return LM_OK;
}

int lm_add_templates_rendered(lm_detector* d, const char* class_id, int mesh_idx, const float* view_proj, int n_views,
                              const float* angles_deg, int n_angles, int* template_ids_out, lm_rect* bboxes_out, uint16_t* crops_out,
                              size_t crop_capacity, size_t* crop_offsets_out) {
    if (d && any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (!d || !class_id || !view_proj || !angles_deg || !template_ids_out || !bboxes_out || !crop_offsets_out || (!crops_out && crop_capacity))
        return fail(LM_ERR_INVALID, "null argument");
    if (n_views <= 0 || n_angles <= 0) return fail(LM_ERR_INVALID, "no views or no angles");
    const int n_img = n_views * n_angles;
    for (int k = 0; k < n_img; ++k) { template_ids_out[k] = -1; bboxes_out[k] = lm_rect{0, 0, 0, 0}; crop_offsets_out[k] = 0; }
    crop_offsets_out[n_img] = 0;
    int rc;
    if ((rc = check_mesh(d, mesh_idx))) return rc;
    if ((rc = ready_for_compute(d))) return rc;
    const lm_config& cfg = d->cfg;
    const int W = cfg.width, H = cfg.height, M = cfg.num_modalities, L = cfg.pyramid_levels;
    const int C = std::min((int)d->slots.size(), n_img);
    if ((rc = refuse_checked_slots(d, 0, C))) return rc;
    for (int s = 0; s < C; ++s) {
        if ((rc = wait_slot_upload(d, d->slots[s]))) return rc;
        Slot& sl = d->slots[s];
        sl.has_frame = false; sl.prepared = false; sl.matched = false; sl.mask_ready = false; sl.match_mask_on[0] = sl.match_mask_on[1] = false;
    }
    const GenMesh& mesh = d->gen->meshes[mesh_idx];
    const size_t npx = (size_t)W * H;
    if (npx * sizeof(float) > d->frame_stride) return fail(LM_ERR_INVALID, "a slot is smaller than a level-0 magnitude image");
    LmGenGeom g;
    std::memset(&g, 0, sizeof(g));
    g.L = L; g.M = M; g.rows = H;
    g.min_mag = cfg.strong_threshold * cfg.strong_threshold;
    {
        size_t px = 0;
        int et = cfg.extract_threshold;
        for (int l = 0; l < L; ++l) {
            if (l > 0) et /= 2;
            g.w[l] = d->lw[l]; g.h[l] = d->lh[l]; g.et[l] = et;
            g.off[l] = px; px += align_up((size_t)d->lw[l] * d->lh[l], 256);
            g.q_off[l][0] = d->off_quant[l][0]; g.q_off[l][1] = M == 2 ? d->off_quant[l][1] : 0;
            g.mag_off[l] = (size_t)l * C * d->frame_stride;   // level l's magnitudes: their own region of C slot strides
        }
        g.img_px = px;
    }
    const size_t n_lists = (size_t)L * M, tab_n = (size_t)(2 * W + 2 * H);
    Carve c;
    const size_t o_vp = c.take((size_t)C * 16 * sizeof(float)), o_tab = c.take((size_t)n_angles * tab_n * 4), o_iv = c.take((size_t)C * 8),
                 o_sv = c.take((size_t)C * mesh.nv * sizeof(float4)), o_z = c.take((size_t)C * npx * 4), o_cov = c.take((size_t)C * npx),
                 o_dep = c.take((size_t)C * npx * 2), o_rm = c.take((size_t)C * npx), o_rd = c.take((size_t)C * npx * 2),
                 o_er = c.take((size_t)C * npx), o_fl = c.take((size_t)C * g.img_px), o_hp = c.take(M == 2 ? (size_t)C * 8 * g.img_px * 2 : 0),
                 o_mag = c.take((size_t)L * C * d->frame_stride), o_cnt = c.take((size_t)C * n_lists * H * 4),
                 o_icnt = c.take((size_t)C * L * H * 4), o_off = c.take((size_t)C * n_lists * H * 4);
    if ((rc = grow_buf(d, c.at))) return rc;
    GenState& gs = *d->gen;
    u8* b = gs.buf;
    {
        std::vector<int> tabs((size_t)n_angles * tab_n);
        for (int a = 0; a < n_angles; ++a) angle_table(W, H, angles_deg[a], &tabs[(size_t)a * tab_n]);
        HIP_TRY(hipMemcpy(b + o_tab, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
    }
    const int nf_color0 = cfg.num_features, nf_depth0 = cfg.depth_num_features;
    std::vector<u32> cnt((size_t)C * n_lists * H), icnt((size_t)C * L * H), rowoff(cnt.size());
    std::vector<LmGenCand> cands;
    std::vector<std::vector<u32>> list_base((size_t)C);
    struct Done { lmh::TemplatePyramid tp; lm_rect bb; bool ok = false; };
    std::vector<Done> done((size_t)C);
    std::vector<std::pair<lmh::TemplatePyramid, int>> accepted;   // (pyramid, image index), in the host generator's order
    std::vector<char> view_failed((size_t)n_views, 0);
    size_t crop_total = 0;
    bool any_failed = false;
    std::vector<int> iv((size_t)C * 2);
    for (int k0 = 0; k0 < n_img; k0 += C) {
        const int n = std::min(C, n_img - k0);
        const int v0 = k0 / n_angles, nv = (k0 + n - 1) / n_angles - v0 + 1;
        for (int i = 0; i < n; ++i) { iv[(size_t)i] = (k0 + i) / n_angles - v0; iv[(size_t)C + i] = (k0 + i) % n_angles; }
        HIP_TRY(hipMemcpyAsync(b + o_vp, view_proj + (size_t)v0 * 16, (size_t)nv * 16 * sizeof(float), hipMemcpyHostToDevice, d->lanes[0].stream));
        HIP_TRY(hipMemcpyAsync(b + o_iv, iv.data(), iv.size() * 4, hipMemcpyHostToDevice, d->lanes[0].stream));
        const int* d_view = reinterpret_cast<const int*>(b + o_iv);
        lmk_gen_render(d->lanes[0].stream, mesh.xyz, mesh.nv, mesh.idx, mesh.ntri, reinterpret_cast<float*>(b + o_vp), nv, W, H,
                       reinterpret_cast<float4*>(b + o_sv), reinterpret_cast<u32*>(b + o_z), b + o_cov, reinterpret_cast<u16*>(b + o_dep));
        lmk_gen_rotate(d->lanes[0].stream, b + o_cov, reinterpret_cast<u16*>(b + o_dep), d_view, d_view + C, reinterpret_cast<int*>(b + o_tab), n, W, H,
                       b + o_rm, reinterpret_cast<u16*>(b + o_rd), d->bgr(0, 0), M == 2 ? d->depth(0) : nullptr, d->frame_stride, b + o_er);
        // lm_add_template's quantisation, over the chunk's slots at once
        float* mag[LM_MAX_LEVELS] = {};
        for (int l = 0; l < L; ++l) mag[l] = reinterpret_cast<float*>(b + o_mag + g.mag_off[l]);
        enqueue_template_quantize(d, n, d->frame_stride, mag);
        lmk_gen_candidates(d->lanes[0].stream, 0, b + o_er, W, H, n, g, b + o_fl, reinterpret_cast<u16*>(b + o_hp), d->frame_arena,
                           b + o_mag, d->frame_stride, reinterpret_cast<u32*>(b + o_cnt), reinterpret_cast<u32*>(b + o_icnt), nullptr, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cnt.data(), b + o_cnt, (size_t)n * n_lists * H * 4, hipMemcpyDeviceToHost, d->lanes[0].stream));
        if (M == 2) HIP_TRY(hipMemcpyAsync(icnt.data(), b + o_icnt, (size_t)n * L * H * 4, hipMemcpyDeviceToHost, d->lanes[0].stream));
        HIP_TRY(hipStreamSynchronize(d->lanes[0].stream));
        // row offsets: lists image-major, level, modality; rows in order
        size_t total = 0;
        for (int i = 0; i < n; ++i) {
            list_base[(size_t)i].assign(n_lists + 1, 0);
            for (size_t li = 0; li < n_lists; ++li) {
                list_base[(size_t)i][li] = (u32)total;
                const int hl = d->lh[li / M];
                for (int y = 0; y < H; ++y) {
                    const size_t k = ((size_t)i * n_lists + li) * H + y;
                    rowoff[k] = (u32)total;
                    if (y < hl) total += cnt[k];
                }
            }
            list_base[(size_t)i][n_lists] = (u32)total;
        }
        if (total > 0xFFFFFFFFull) return fail(LM_ERR_OVERFLOW, "candidate lists of a chunk exceed 2^32");
        if (total > gs.cand.size()) HIP_TRY(gs.cand.grow(std::max<size_t>(total, 1 << 16)));
        cands.resize(total);
        if (total) {
            HIP_TRY(hipMemcpyAsync(b + o_off, rowoff.data(), (size_t)n * n_lists * H * 4, hipMemcpyHostToDevice, d->lanes[0].stream));
            lmk_gen_candidates(d->lanes[0].stream, 1, b + o_er, W, H, n, g, b + o_fl, reinterpret_cast<u16*>(b + o_hp), d->frame_arena,
                               b + o_mag, d->frame_stride, nullptr, nullptr, reinterpret_cast<u32*>(b + o_off), gs.cand);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(cands.data(), gs.cand, total * sizeof(LmGenCand), hipMemcpyDeviceToHost, d->lanes[0].stream));
            HIP_TRY(hipStreamSynchronize(d->lanes[0].stream));
        }
        // the selection of every image of the chunk (extract_pyramid's order: per level colour, then depth; the first failure decides)
        auto select = [&](int i) {
            Done& o = done[(size_t)i];
            o.ok = false;
            o.tp.assign((size_t)M * L, lmh::Template());
            int nf_color = nf_color0, nf_depth = nf_depth0;
            std::vector<lmh::Candidate> v;
            for (int l = 0; l < L; ++l) {
                if (l > 0) { nf_color /= 2; nf_depth /= 2; }
                for (int m = 0; m < M; ++m) {
                    const size_t li = (size_t)l * M + m;
                    const u32 lo = list_base[(size_t)i][li], hi = list_base[(size_t)i][li + 1];
                    v.resize(hi - lo);
                    int per_label[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    for (u32 k = lo; k < hi; ++k) {
                        const LmGenCand& gc = cands[k];
                        v[k - lo] = lmh::Candidate{{gc.x, gc.y, gc.label}, gc.score};
                        if (m == 1) ++per_label[gc.label];
                    }
                    lmh::Template& t = o.tp[li];
                    t.pyramid_level = l; t.width = t.height = -1;
                    bool ok;
                    if (m == 0) ok = lmh::select_color(v, (size_t)nf_color, t);
                    else {
                        float area = 0.f;
                        for (int y = 0; y < d->lh[l]; ++y) area += (float)icnt[((size_t)i * L + l) * H + y];
                        ok = lmh::select_depth(v, per_label, area, (size_t)nf_depth, t);
                    }
                    if (!ok) return;
                }
            }
            o.bb = lmh::crop_templates(o.tp);
            o.ok = true;
        };
        const int nthreads = std::min(16, n);
        if (nthreads <= 1) { for (int i = 0; i < n; ++i) select(i); }
        else {
            std::vector<std::thread> pool;
            std::atomic<int> next{0};
            for (int t = 0; t < nthreads; ++t)
                pool.emplace_back([&] { for (int i; (i = next.fetch_add(1)) < n;) select(i); });
            for (std::thread& t : pool) t.join();
        }
        // addTemplate's rule: a view stops at its first failing angle; the crops of the kept templates
        for (int i = 0; i < n; ++i) {
            const int k = k0 + i, v = k / n_angles;
            if (view_failed[(size_t)v]) continue;
            Done& o = done[(size_t)i];
            if (!o.ok) { view_failed[(size_t)v] = 1; any_failed = true; continue; }
            bboxes_out[k] = o.bb;
            const int x0 = std::max(o.bb.x, 0), y0 = std::max(o.bb.y, 0);
            const int x1 = (int)std::min<long long>((long long)o.bb.x + o.bb.width, W), y1 = (int)std::min<long long>((long long)o.bb.y + o.bb.height, H);
            const size_t cw = x1 > x0 ? (size_t)(x1 - x0) : 0, ch = y1 > y0 ? (size_t)(y1 - y0) : 0;
            crop_offsets_out[k] = crop_total;
            if (cw && ch && crop_total + cw * ch <= crop_capacity)
                HIP_TRY(hipMemcpy2DAsync(crops_out + crop_total, cw * 2, b + o_rd + ((size_t)i * npx + (size_t)y0 * W + x0) * 2, (size_t)W * 2,
                                         cw * 2, ch, hipMemcpyDeviceToHost, d->lanes[0].stream));
            crop_total += cw * ch;
            accepted.emplace_back(std::move(o.tp), k);
        }
        HIP_TRY(hipStreamSynchronize(d->lanes[0].stream));
    }
    crop_offsets_out[n_img] = crop_total;
    if (crop_total > crop_capacity) {
        for (int k = 0; k < n_img; ++k) template_ids_out[k] = -1;
        return fail(LM_ERR_OVERFLOW, "the bbox crops exceed crop_capacity (their total is in crop_offsets_out[n_views * n_angles])");
    }
    for (auto& a : accepted) template_ids_out[a.second] = d->bank.add_pyramid(class_id, std::move(a.first));
    if (!accepted.empty()) { d->bank_dirty = true; d->hulls_dirty = true; }
    if (any_failed) fail(LM_ERR_EXTRACT, "not enough features to build a template");
    return LM_OK;
}
