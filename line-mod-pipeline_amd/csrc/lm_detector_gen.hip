// lm_detector_gen.hip -- host side of template generation on the GPU: resident render meshes, lm_add_templates_rendered and its stage
// hooks (0.6), lm_add_templates_slots and lm_stage_select (0.11, section 15).  Kernels: lm_k_gen.hip, lm_k_select.hip.
// Per chunk of at most frame_slots images, the rendered generator (view-major, angle-minor) renders the chunk's views and rotates + erodes
// them into the slots; the slot learner gathers the chunk's object masks.  Both then share chunk_features: the existing quantisers over
// all the chunk's slots, the candidate counts (one read-back of the row counts), the candidate lists, the selection (k_select) and the
// read-back of the selected features; the crop to the bounding box runs on the host.  No image and no candidate list leaves the device.
#include "lm_detector_impl.h"

namespace lmd {

struct GenMesh { DevBuf<float> xyz; DevBuf<u32> idx; int nv = 0, ntri = 0; };

struct GenState {
    GenMesh meshes[LM_MAX_RENDER_MESHES];
    DevBuf<u8> buf;
    DevBuf<LmGenCand> cand;
    DevBuf<u32> skey, alive;      // k_select's scratch: a key word per candidate, the alive bitmap
    DevBuf<u8> sel;               // its lists, features and counts
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

// The chunk's geometry for up to C images: the levels' buffers, the slots' quantised images and the magnitude arena
static LmGenGeom chunk_geom(const lm_detector* d, int C) {
    const lm_config& cfg = d->cfg;
    const int M = cfg.num_modalities, L = cfg.pyramid_levels;
    LmGenGeom g;
    std::memset(&g, 0, sizeof(g));
    g.L = L; g.M = M; g.rows = cfg.height;
    g.min_mag = cfg.strong_threshold * cfg.strong_threshold;
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
    return g;
}

// chunk_features' share of the generation buffer
struct ChunkBufs { size_t o_um, o_fl, o_hp, o_mag, o_cnt, o_icnt, o_off; };
static ChunkBufs carve_chunk(const lm_detector* d, const LmGenGeom& g, int C, Carve& c) {
    const size_t n_lists = (size_t)g.L * g.M, H = (size_t)g.rows;
    ChunkBufs o;
    o.o_um = c.take((size_t)C * 4);
    o.o_fl = c.take((size_t)C * g.img_px);
    o.o_hp = c.take(g.M == 2 ? (size_t)C * 8 * g.img_px * 2 : 0);
    o.o_mag = c.take((size_t)g.L * C * d->frame_stride);
    o.o_cnt = c.take((size_t)C * n_lists * H * 4);
    o.o_icnt = c.take((size_t)C * g.L * H * 4);
    o.o_off = c.take((size_t)C * n_lists * H * 4);
    return o;
}

// k_select over `lists` (lo / n / want / distance / depth filled in; alive_lo is assigned here) of the first `total` candidates of
// gs.cand: feat[list][LM_MAX_FEATURES], nout[list].  Nothing enqueued reads the selection's own buffers on entry (they may grow
// here); lane 0's stream is idle on return.
static int run_select(lm_detector* d, std::vector<LmSelList>& lists, size_t total, std::vector<lm_feature>& feat, std::vector<int>& nout) {
    GenState& gs = gen(d);
    hipStream_t st = d->lanes[0].stream;
    const size_t nl = lists.size();
    feat.assign(nl * LM_MAX_FEATURES, lm_feature{0, 0, 0});
    nout.assign(nl, -1);
    if (!nl) return LM_OK;
    size_t words = 0;
    for (LmSelList& l : lists) { l.alive_lo = (u32)words; words += lmk_select_alive_words(l.n); }
    if (words > 0xFFFFFFFFull) return fail(LM_ERR_OVERFLOW, "candidate lists of a chunk exceed 2^32");
    Carve c;
    const size_t o_l = c.take(nl * sizeof(LmSelList)), o_f = c.take(nl * LM_MAX_FEATURES * sizeof(lm_feature)), o_n = c.take(nl * sizeof(int));
    HIP_TRY(gs.skey.grow(std::max<size_t>(total, 1)));
    HIP_TRY(gs.alive.grow(std::max<size_t>(words, 1)));
    HIP_TRY(gs.sel.grow(c.at));
    u8* s = gs.sel;
    HIP_TRY(hipMemcpyAsync(s + o_l, lists.data(), nl * sizeof(LmSelList), hipMemcpyHostToDevice, st));
    lmk_select(st, reinterpret_cast<const LmSelList*>(s + o_l), (int)nl, gs.cand, gs.skey, gs.alive, reinterpret_cast<lm_feature*>(s + o_f),
               reinterpret_cast<int*>(s + o_n));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(feat.data(), s + o_f, nl * LM_MAX_FEATURES * sizeof(lm_feature), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(nout.data(), s + o_n, nl * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LM_OK;
}

// pick_scattered's initial distance as select_color / select_depth (lm_extract.cpp) compute it
static float select_distance(int modality, size_t n, int want, float area) {
    if (want <= 0) return 0.f;
    return modality == 0 ? (float)(n / (size_t)want + 1) : sqrtf(area) / sqrtf((float)want) + 1.5f;
}

struct Done { lmh::TemplatePyramid tp; lm_rect bb; bool ok = false; };

// From level-0 masks to templates, for the images in slots [first_slot, first_slot + n): masks = n level-0 masks on the device, `pitch`
// bytes per row and pitch * height per image, used raw (rim: mask > its 3x3 minimum; interior: 5x5 minimum != 0); unmasked (may be
// null) = per image, non-zero: no mask.  lm_add_template's quantisation over the slots at once, the flags, row distances and candidate
// lists, the selection, and on the host extract_pyramid's order (per level colour, then depth; the first failing list decides) and the
// crop.  done[i].ok = false: the image has too few candidates somewhere.
static int chunk_features(lm_detector* d, const LmGenGeom& g, const ChunkBufs& o, const u8* masks, const int* unmasked, int pitch,
                          int first_slot, int n, std::vector<Done>& done) {
    GenState& gs = gen(d);
    u8* b = gs.buf;
    hipStream_t st = d->lanes[0].stream;
    const lm_config& cfg = d->cfg;
    const int H = cfg.height, M = g.M, L = g.L;
    const size_t n_lists = (size_t)L * M;
    const u8* slot0 = d->frame_arena + (size_t)first_slot * d->frame_stride;
    const int* d_um = nullptr;
    if (unmasked) {
        HIP_TRY(hipMemcpyAsync(b + o.o_um, unmasked, (size_t)n * 4, hipMemcpyHostToDevice, st));
        d_um = reinterpret_cast<const int*>(b + o.o_um);
    }
    float* mag[LM_MAX_LEVELS] = {};
    for (int l = 0; l < L; ++l) mag[l] = reinterpret_cast<float*>(b + o.o_mag + g.mag_off[l]);
    enqueue_template_quantize(d, first_slot, n, d->frame_stride, mag);
    lmk_gen_candidates(st, 0, masks, d_um, pitch, H, n, g, b + o.o_fl, reinterpret_cast<u16*>(b + o.o_hp), slot0, b + o.o_mag, d->frame_stride,
                       reinterpret_cast<u32*>(b + o.o_cnt), reinterpret_cast<u32*>(b + o.o_icnt), nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    std::vector<u32> cnt((size_t)n * n_lists * H), icnt((size_t)n * L * H), rowoff(cnt.size());
    HIP_TRY(hipMemcpyAsync(cnt.data(), b + o.o_cnt, cnt.size() * 4, hipMemcpyDeviceToHost, st));
    if (M == 2) HIP_TRY(hipMemcpyAsync(icnt.data(), b + o.o_icnt, icnt.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // row offsets: lists image-major, level, modality; rows in order.  The selection's lists with them: want halves per level
    // (pyrDown: num_features /= 2), the depth area is the interior's pixel count (the whole level without a mask)
    std::vector<LmSelList> lists((size_t)n * n_lists);
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        int nf[2] = {cfg.num_features, cfg.depth_num_features};
        for (size_t li = 0; li < n_lists; ++li) {
            const int l = (int)(li / M), m = (int)(li % M), hl = d->lh[l];
            if (l > 0 && m == 0) { nf[0] /= 2; nf[1] /= 2; }
            const size_t lo = total;
            for (int y = 0; y < H; ++y) {
                const size_t k = ((size_t)i * n_lists + li) * H + y;
                rowoff[k] = (u32)total;
                if (y < hl) total += cnt[k];
            }
            float area = 0.f;
            if (m == 1) {
                if (unmasked && unmasked[i]) area = (float)((size_t)d->lw[l] * hl);
                else for (int y = 0; y < hl; ++y) area += (float)icnt[((size_t)i * L + l) * H + y];
            }
            LmSelList& s = lists[(size_t)i * n_lists + li];
            s.lo = (u32)lo; s.n = (u32)(total - lo); s.want = nf[m]; s.depth = m;
            s.distance = select_distance(m, total - lo, nf[m], area);
            s.alive_lo = 0;
        }
    }
    if (total > 0xFFFFFFFFull) return fail(LM_ERR_OVERFLOW, "candidate lists of a chunk exceed 2^32");
    if (total > gs.cand.size()) HIP_TRY(gs.cand.grow(std::max<size_t>(total, 1 << 16)));
    if (total) {
        HIP_TRY(hipMemcpyAsync(b + o.o_off, rowoff.data(), rowoff.size() * 4, hipMemcpyHostToDevice, st));
        lmk_gen_candidates(st, 1, masks, d_um, pitch, H, n, g, b + o.o_fl, reinterpret_cast<u16*>(b + o.o_hp), slot0, b + o.o_mag,
                           d->frame_stride, nullptr, nullptr, reinterpret_cast<u32*>(b + o.o_off), gs.cand);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));      // (rowoff is read by the launch; run_select may grow its buffers)
    }
    std::vector<lm_feature> feat;
    std::vector<int> nout;
    int rc;
    if ((rc = run_select(d, lists, total, feat, nout))) return rc;
    done.assign((size_t)n, Done());
    for (int i = 0; i < n; ++i) {
        Done& dn = done[(size_t)i];
        dn.tp.assign(n_lists, lmh::Template());
        bool ok = true;
        for (size_t li = 0; li < n_lists && ok; ++li) {
            const size_t k = (size_t)i * n_lists + li;
            lmh::Template& t = dn.tp[li];
            t.pyramid_level = (int)(li / M); t.width = t.height = -1;
            if (nout[k] < 0) { ok = false; break; }
            t.features.assign(feat.begin() + (ptrdiff_t)(k * LM_MAX_FEATURES), feat.begin() + (ptrdiff_t)(k * LM_MAX_FEATURES + (size_t)nout[k]));
        }
        if (!ok) continue;
        dn.bb = lmh::crop_templates(dn.tp);
        dn.ok = true;
    }
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
    const int W = cfg.width, H = cfg.height, M = cfg.num_modalities;
    const int C = std::min((int)d->slots.size(), n_img);
    if ((rc = refuse_checked_slots(d, 0, C))) return rc;
    for (int s = 0; s < C; ++s) {
        if ((rc = wait_slot_upload(d, d->slots[s]))) return rc;
        Slot& sl = d->slots[s];
        sl.has_frame = false; sl.has_depth = false; sl.prepared = false; sl.matched = false; sl.mask_ready = false; sl.match_mask_on[0] = sl.match_mask_on[1] = false;
    }
    const GenMesh& mesh = d->gen->meshes[mesh_idx];
    const size_t npx = (size_t)W * H;
    if (npx * sizeof(float) > d->frame_stride) return fail(LM_ERR_INVALID, "a slot is smaller than a level-0 magnitude image");
    const LmGenGeom g = chunk_geom(d, C);
    const size_t tab_n = (size_t)(2 * W + 2 * H);
    Carve c;
    const size_t o_vp = c.take((size_t)C * 16 * sizeof(float)), o_tab = c.take((size_t)n_angles * tab_n * 4), o_iv = c.take((size_t)C * 8),
                 o_sv = c.take((size_t)C * mesh.nv * sizeof(float4)), o_z = c.take((size_t)C * npx * 4), o_cov = c.take((size_t)C * npx),
                 o_dep = c.take((size_t)C * npx * 2), o_rm = c.take((size_t)C * npx), o_rd = c.take((size_t)C * npx * 2),
                 o_er = c.take((size_t)C * npx);
    const ChunkBufs cb = carve_chunk(d, g, C, c);
    if ((rc = grow_buf(d, c.at))) return rc;
    GenState& gs = *d->gen;
    u8* b = gs.buf;
    {
        std::vector<int> tabs((size_t)n_angles * tab_n);
        for (int a = 0; a < n_angles; ++a) angle_table(W, H, angles_deg[a], &tabs[(size_t)a * tab_n]);
        HIP_TRY(hipMemcpy(b + o_tab, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
    }
    std::vector<Done> done;
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
        if ((rc = chunk_features(d, g, cb, b + o_er, nullptr, W, 0, n, done))) return rc;
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

// ---- learning from resident frames (0.11)
int lm_add_templates_slots(lm_detector* d, const char* class_id, int first_slot, int n_slots, const lm_object_mask* masks,
                           int* template_ids_out, lm_rect* bboxes_out) {
    if (d && any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (!d || !class_id || !template_ids_out || !bboxes_out) return fail(LM_ERR_INVALID, "null argument");
    if (n_slots <= 0) return fail(LM_ERR_INVALID, "no slots");
    for (int k = 0; k < n_slots; ++k) { template_ids_out[k] = -1; bboxes_out[k] = lm_rect{0, 0, 0, 0}; }
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    for (int k = 0; k < n_slots; ++k)
        if (!d->slots[first_slot + k].has_frame) return fail(LM_ERR_INVALID, "no frame uploaded to slot");
    if ((rc = refuse_checked_slots(d, first_slot, n_slots))) return rc;
    const lm_config& cfg = d->cfg;
    const int W = cfg.width, H = cfg.height;
    // the object masks: a rule is checked as lm_set_mask_rule checks it (its modalities do not matter here)
    std::vector<LmRule> rules((size_t)n_slots);
    std::vector<int> unmasked((size_t)n_slots, 1);
    bool any_hsv = false;
    for (int k = 0; masks && k < n_slots; ++k) {
        const lm_object_mask& m = masks[k];
        if (m.data) {
            if (m.row_stride != 0 && m.row_stride < W) return fail(LM_ERR_INVALID, "object mask: a row stride below the width");
            if (m.on_device != 0 && m.on_device != 1) return fail(LM_ERR_INVALID, "object mask: on_device must be 0 or 1");
            unmasked[(size_t)k] = 0;
        } else if (m.rule) {
            lm_mask_rule r = *m.rule;
            r.modalities = 1;
            if ((rc = check_mask_rule(d, &r, &rules[(size_t)k]))) return rc;
            // a depth gate reads the slot's depth plane (keeps_depth(d): check_mask_rule); the frame must have come with its depth image
            if (rules[(size_t)k].use_depth && (rc = slot_lacks_depth(d, first_slot + k))) return rc;
            any_hsv |= rules[(size_t)k].use_hsv != 0;
            unmasked[(size_t)k] = 0;
        }
    }
    if ((size_t)W * H * sizeof(float) > d->frame_stride) return fail(LM_ERR_INVALID, "a slot is smaller than a level-0 magnitude image");
    if (any_hsv && (rc = ensure_hsv_div(d))) return rc;
    for (int k = 0; k < n_slots; ++k)
        if ((rc = wait_slot_upload(d, d->slots[first_slot + k]))) return rc;
    const LmGenGeom g = chunk_geom(d, n_slots);
    const size_t pitch = d->match_mask_pitch, plane = pitch * (size_t)H;
    Carve c;
    const size_t o_er = c.take((size_t)n_slots * plane);
    const ChunkBufs cb = carve_chunk(d, g, n_slots, c);
    if ((rc = grow_buf(d, c.at))) return rc;
    u8* b = d->gen->buf;
    hipStream_t st = d->lanes[0].stream;
    // the frames stay, what a3-a10 made of them does not: the template quantisation overwrites the slots' quantised images
    for (int k = 0; k < n_slots; ++k) d->slots[first_slot + k].prepared = false;
    // gather the masks into the chunk's level-0 mask buffer: a copy from the host, a copy on the device, or k_mask_rule on the slot's frame
    LmRuleArgs a{};
    a.bgr = d->bgr(0, 0); a.depth = keeps_depth(d) ? d->depth(0) : nullptr; a.slot_stride = d->frame_stride;      // ("is there a depth plane": the rule's gate, not a modality)
    a.divtab = d->d_hsv_div; a.w = W; a.h = H; a.mask_pitch = (u32)pitch;
    for (int k = 0; masks && k < n_slots; ++k) {
        const lm_object_mask& m = masks[k];
        u8* dst = b + o_er + (size_t)k * plane;
        if (m.data)
            HIP_TRY(hipMemcpy2DAsync(dst, pitch, m.data, m.row_stride ? (size_t)m.row_stride : (size_t)W, (size_t)W, (size_t)H,
                                     m.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        else if (m.rule) {
            a.n = 1; a.rule[0] = rules[(size_t)k]; a.slot[0] = (u16)(first_slot + k); a.kind[0] = 0; a.plane[0] = dst;
            lmk_mask_rule(st, a);
        }
    }
    HIP_TRY(hipGetLastError());
    std::vector<Done> done;
    if ((rc = chunk_features(d, g, cb, b + o_er, unmasked.data(), (int)pitch, first_slot, n_slots, done))) return rc;
    bool any_failed = false, any_added = false;
    for (int k = 0; k < n_slots; ++k) {
        Done& dn = done[(size_t)k];
        if (!dn.ok) { any_failed = true; continue; }
        bboxes_out[k] = dn.bb;
        template_ids_out[k] = d->bank.add_pyramid(class_id, std::move(dn.tp));
        any_added = true;
    }
    if (any_added) { d->bank_dirty = true; d->hulls_dirty = true; }
    if (any_failed) fail(LM_ERR_EXTRACT, "not enough features to build a template");
    return LM_OK;
}

int lm_stage_select(lm_detector* d, int modality, int n_lists, const int32_t* list_offsets, const int16_t* xy, const int32_t* labels,
                    const float* scores, const int32_t* want, const float* area, lm_feature* features_out, int32_t* n_out) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if (any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (!list_offsets || !want || !features_out || !n_out || (modality != 0 && modality != 1) || n_lists <= 0 || (modality == 1 && !area))
        return fail(LM_ERR_INVALID, "bad argument");
    if (list_offsets[0] != 0) return fail(LM_ERR_INVALID, "list_offsets must start at 0");
    for (int i = 0; i < n_lists; ++i) {
        if (list_offsets[i + 1] < list_offsets[i]) return fail(LM_ERR_INVALID, "list_offsets must not decrease");
        if (want[i] < 1 || want[i] > LM_MAX_FEATURES) return fail(LM_ERR_INVALID, "want must be in 1..63");
        if (modality == 1 && !(area[i] >= 0.f)) return fail(LM_ERR_INVALID, "area must not be negative");
    }
    const size_t total = (size_t)list_offsets[n_lists];
    if (total && (!xy || !labels || !scores)) return fail(LM_ERR_INVALID, "null candidate arrays");
    std::vector<LmGenCand> cands(total);
    for (size_t k = 0; k < total; ++k) {
        if (labels[k] < 0 || labels[k] > 7) return fail(LM_ERR_INVALID, "label out of range (0 .. 7)");
        if (!(scores[k] >= 0.f) || !std::isfinite(scores[k])) return fail(LM_ERR_INVALID, "scores must be finite and not negative");
        cands[k] = LmGenCand{xy[2 * k], xy[2 * k + 1], labels[k], scores[k]};
    }
    std::vector<LmSelList> lists((size_t)n_lists);
    for (int i = 0; i < n_lists; ++i) {
        LmSelList& s = lists[(size_t)i];
        s.lo = (u32)list_offsets[i]; s.n = (u32)(list_offsets[i + 1] - list_offsets[i]); s.want = want[i]; s.depth = modality;
        s.distance = select_distance(modality, s.n, want[i], modality == 1 ? area[i] : 0.f);
        s.alive_lo = 0;
    }
    GenState& gs = gen(d);
    hipStream_t st = d->lanes[0].stream;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(gs.cand.grow(std::max<size_t>(total, 1)));
    if (total) HIP_TRY(hipMemcpyAsync(gs.cand, cands.data(), total * sizeof(LmGenCand), hipMemcpyHostToDevice, st));
    std::vector<lm_feature> feat;
    std::vector<int> nout;
    if ((rc = run_select(d, lists, total, feat, nout))) return rc;
    for (int i = 0; i < n_lists; ++i) {
        n_out[i] = nout[(size_t)i];
        for (int k = 0; k < nout[(size_t)i]; ++k) features_out[(size_t)i * LM_MAX_FEATURES + k] = feat[(size_t)i * LM_MAX_FEATURES + k];
    }
    return LM_OK;
}
