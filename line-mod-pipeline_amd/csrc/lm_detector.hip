// lm_detector.hip -- host side of liblinemod_hip.so: the C ABI of include/linemod_hip.h, the
// template bank (host copy + device upload), resident frame slots and the per-batch launch sequence.
//
// Mirrors cv::linemod::Detector as the reference uses it (/root/reference/src/HighLevelLinemod.cpp:
// 33-34,41-42 ctor; :93 addTemplate; :152 match; :115,181 getTemplates; :55,60,65 class queries).
// There is no CPU fallback: every compute entry point needs a HIP device and fails with
// LM_ERR_NO_DEVICE otherwise.
#include "lm_detector_impl.h"
#include "lm_median_counts.h"

namespace lmd {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

bool any_lane_busy(const lm_detector* d) {
    for (const lm_detector::Lane& ln : d->lanes) if (ln.busy) return true;
    return false;
}

// the device bank goes: every list of it, and the work items built for it
void free_device_bank(lm_detector* d) {
    for (auto* b : {&d->d_item_t, &d->d_item_chunk, &d->d_scan_off, &d->d_off1, &d->d_offn, &d->d_offs3, &d->d_offl, &d->d_offsl, &d->d_litem}) b->reset();
    for (auto* b : {&d->d_scan_P, &d->d_scan_n, &d->d_t_global, &d->d_t_class}) b->reset();
    d->items1.clear();
    for (int l = 0; l < LM_MAX_LEVELS; ++l) { d->d_ref_meta[l].reset(); d->d_ref_feat[l].reset(); }
}

// A failure on the way returns with dev_ready false and whatever exists so far owned by its member (the detector's destructor frees it);
// the next call starts again at the top, and every alloc / create below releases what the failed attempt left in its member first.
int ensure_device(lm_detector* d) {
    if (d->dev_ready) {
        HIP_TRY(hipSetDevice(d->cfg.device));
        return LM_OK;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(LM_ERR_NO_DEVICE, "no HIP device available: liblinemod_hip has no CPU fallback");
    if (d->cfg.device < 0 || d->cfg.device >= ndev) return fail(LM_ERR_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(d->cfg.device));
    d->dev_begun = true;
    d->scanl_lds = lmk_scanl_raise_lds();      // (per device: a detector on another device raises it there)
    const lm_config& c = d->cfg;
    const int M = c.num_modalities, L = c.pyramid_levels, S = c.frame_slots;
    // ---- frame arena layout
    size_t off = 0;
    // level-0 colour and depth back to back (no padding between them): a host frame laid out the same way is ONE copy
    d->off_bgr[0] = off; off += (size_t)c.width * c.height * 3;
    d->off_depth = off; off += align_up((size_t)c.width * c.height * 2, 256);
    off = align_up(off, 256);
    for (int l = 1; l < L; ++l) { d->off_bgr[l] = off; off += align_up((size_t)d->lw[l] * d->lh[l] * 3, 256); }
    for (int l = 0; l < L; ++l)
        for (int m = 0; m < M; ++m) { d->off_quant[l][m] = off; off += align_up((size_t)d->lw[l] * d->lh[l], 256); }
    for (int l = 0; l < L; ++l) { d->off_lm[l] = off; off += align_up(d->geom[l].arena_bytes, 256); }
    d->off_cscratch = off; off += align_up(lmk_color_scratch_bytes(c.width, c.height), 256);
    d->off_cscratch1 = off; off += align_up(lmk_color_scratch_bytes(d->lw[L > 1 ? 1 : 0], d->lh[L > 1 ? 1 : 0]), 256);
    d->off_dscratch = off; off += align_up((size_t)c.width * c.height, 256);
    d->cmask_wpr = (c.width + 31) / 32;
    d->off_cmask = off; off += align_up((size_t)d->cmask_wpr * c.height * 4, 256);
    d->match_mask_pitch = align_up((size_t)c.width, 64);
    d->frame_stride = align_up(off, 4096);
    HIP_TRY(d->frame_arena.alloc(d->frame_stride * S));
    HIP_TRY(hipMemset(d->frame_arena, 0, d->frame_stride * S));  // linear-memory pads / zero blocks stay zero forever
    // ---- aux arena layout
    off = 0;
    d->off_hdr = off; off += 256;
    d->off_cand = off; off += align_up((size_t)d->max_cand * sizeof(LmCand), 256);
    d->off_keys = off; off += align_up((size_t)d->max_match * 16, 256);
    d->off_out = off; off += align_up((size_t)LM_SORT_CAP * sizeof(LmOutMatch), 256);
    d->aux_stride = align_up(off, 4096);
    HIP_TRY(d->aux_arena.alloc(d->aux_stride * S));
    HIP_TRY(hipMemset(d->aux_arena, 0, d->aux_stride * S));      // counters start at zero; k_sort_unique re-arms them
    d->host_stride = align_up(sizeof(LmHostBlock), 256);
    HIP_TRY(d->host_blocks.alloc(d->host_stride * S, hipHostMallocMapped));
    std::memset(d->host_blocks, 0, d->host_stride * S);
    lm_detector::Lane& l0 = d->lanes[0];
    HIP_TRY(l0.d_raw_thr.alloc(128));
    HIP_TRY(l0.h_raw_thr.alloc(128));
    d->plan_stride_cap = std::max(S / 8, 1) + 8;    // pieces per XCD list: nslots / 8 + 8 (k_refine_plan)
    const size_t plan_words = 24 * (size_t)d->plan_stride_cap + 16;
    HIP_TRY(d->d_plan.alloc(LM_NLANES * plan_words));
    for (int l = 0; l < LM_NLANES; ++l) d->lanes[l].plan = d->d_plan + (size_t)l * plan_words;
    HIP_TRY(l0.stream.create(hipStreamNonBlocking));
    // lane 1's stream right behind lane 0's: the runtime deals streams to its hardware queues in creation order, and
    // two lanes that land on one queue run strictly one after the other (measured r02: 87 K instead of 102 K det/s)
    for (int l = 1; l < LM_NLANES; ++l) HIP_TRY(d->lanes[l].stream.create(hipStreamNonBlocking));
    for (int k = 0; k < LM_NCOPY; ++k) {
        HIP_TRY(d->copy_stream[k].create(hipStreamNonBlocking));
        d->up_seq_next[k] = 1; d->up_seq_done[k] = 0;
    }
    for (Event& ev : l0.ev) HIP_TRY(ev.create());
    l0.created = true;      // (lanes 1..3 get their events and tables on first use: ensure_lane)
    d->slots = std::vector<Slot>((size_t)S);
    for (Slot& s : d->slots) {
        HIP_TRY(s.ev_up.create(hipEventDisableTiming));
        HIP_TRY(s.ev_bgr.create(hipEventDisableTiming));
    }
    // pinned staging for pageable sources is allocated on a slot's first staged upload (ensure_staging): a
    // streaming server that hands over pinned frames (lm_upload_frame_pinned) never needs it
    HIP_TRY(d->d_resp_tab.alloc(256 + 256 / sizeof(u64)));   // + the miss masks of the 256 spread bytes (d_lm_fast's planes)
    HIP_TRY(d->d_scan_stat.alloc(4096));
    HIP_TRY(hipMemset(d->d_scan_stat, 0, 4096 * sizeof(unsigned long long)));
    HIP_TRY(d->d_sim_lut.alloc(256 / sizeof(u32)));
    HIP_TRY(d->d_normal_lut.alloc(2 * 8000 + 16));    // the table, then its labels as rank codes (LMK_NORMAL_CODE_OFFSET) + a zero entry for indices outside the table
    HIP_TRY(hipDeviceSynchronize());
    if (const char* ev = getenv("LM_REFINE_STAT")) {
        if (atoi(ev) > 0 && d->d_refine_stat.alloc(8) == hipSuccess)
            (void)hipMemset(d->d_refine_stat, 0, 8 * sizeof(unsigned long long));
    }
    d->dev_ready = true;
    d->luts_dirty = true;
    d->bank_dirty = true; d->hulls_dirty = true;
    return LM_OK;
}

int ensure_luts(lm_detector* d) {
    if (!d->luts_dirty) return LM_OK;
    u64 tab[256 + 32];
    u8* miss = reinterpret_cast<u8*>(tab + 256);       // bit o of miss[v]: orientation o's response to the spread byte v is below 4
    int below4 = 0;                                    // the largest response below 4 the table can give
    for (int v = 0; v < 256; ++v) {
        u64 e = 0;
        miss[v] = 0;
        for (int o = 0; o < 8; ++o) {
            u8 r = std::max(d->sim_lut[32 * o + (v & 15)], d->sim_lut[32 * o + 16 + (v >> 4)]);
            e |= (u64)r << (8 * o);
            if (r < 4) { miss[v] |= (u8)(1u << o); below4 = std::max(below4, (int)r); }
        }
        tab[v] = e;
    }
    d->miss_delta = 4 - below4;                        // what a missed feature costs at least (k_scan1's bound): 1 with upstream's table (responses 0 .. 4)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(d->d_resp_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->d_sim_lut, d->sim_lut, 256, hipMemcpyHostToDevice));
    {
        // k_dnormal writes the label's RANK CODE (lm_dev_depth.h, a5 streaming form): looked up directly from a second table
        u8 both[2 * 8000 + 16] = {};                      // [LMK_NORMAL_CODE_OFFSET + 8000 ..] = 0: the code of an index outside the table
        std::memcpy(both, d->normal_lut, 8000);
        for (int i = 0; i < 8000; ++i) {
            const u8 v = d->normal_lut[i];
            const unsigned rank = v ? (unsigned)__builtin_ffs((int)v) : 0u;        // 0 for none, 1 + label otherwise
            both[LMK_NORMAL_CODE_OFFSET + i] = (u8)lm_mc_rank_code(rank);   // 4 rank, 29 for rank 8: lm_median_counts.h
        }
        HIP_TRY(hipMemcpy(d->d_normal_lut, both, sizeof(both), hipMemcpyHostToDevice));
    }
    d->luts_dirty = false;
    return LM_OK;
}

int ensure_bank(lm_detector* d) {
    if (!d->bank_dirty) return LM_OK;
    HIP_TRY(hipDeviceSynchronize());
    free_device_bank(d);
    std::string err;
    if (!lmh::build_device_bank(d->bank, d->cfg, d->geom, d->hb, d->scan_list_order, err)) return fail(LM_ERR_INVALID, err);
    HIP_TRY(upload_vec(d->d_item_t, d->hb.item_t));
    HIP_TRY(upload_vec(d->d_item_chunk, d->hb.item_chunk));
    HIP_TRY(upload_vec(d->d_scan_off, d->hb.scan_off));
    HIP_TRY(upload_vec(d->d_scan_P, d->hb.scan_P));
    HIP_TRY(upload_vec(d->d_scan_n, d->hb.scan_n));
    if (d->hb.fpad1) {
        HIP_TRY(upload_vec(d->d_off1, d->hb.off1));
        HIP_TRY(upload_vec(d->d_offn, d->hb.offn));
        HIP_TRY(upload_vec(d->d_offs3, d->hb.offs3));
    }
    if (d->hb.lds_ok) {
        HIP_TRY(upload_vec(d->d_offl, d->hb.offl));
        HIP_TRY(upload_vec(d->d_offsl, d->hb.offsl));
        HIP_TRY(upload_vec(d->d_litem, d->hb.lrec));      // (the lane items with their templates' records: 16 bytes each)
    }
    HIP_TRY(upload_vec(d->d_t_global, d->hb.t_global));
    HIP_TRY(upload_vec(d->d_t_class, d->hb.t_class));
    for (int l = 0; l + 1 < d->cfg.pyramid_levels; ++l) {
        HIP_TRY(upload_vec(d->d_ref_meta[l], d->hb.ref_meta[l]));
        HIP_TRY(upload_vec(d->d_ref_feat[l], d->hb.ref_feat[l]));
    }
    d->bank_dirty = false;
    return LM_OK;
}

int check_slots(lm_detector* d, int first, int n) {
    if (first < 0 || n < 0 || first + n > (int)d->slots.size()) return fail(LM_ERR_INVALID, "slot out of range");
    return LM_OK;
}

// upstream's NORMAL_LUT holds 0 or one-hot bytes; the streaming depth kernels rely on it (counting median)
bool normal_lut_onehot(lm_detector* d) {
    if (d->lut_onehot < 0) {
        d->lut_onehot = 1;
        for (int i = 0; i < 8000; ++i) { const u8 v = d->normal_lut[i]; if (v & (v - 1)) { d->lut_onehot = 0; break; } }
    }
    return d->lut_onehot != 0;
}

// an upload must not overwrite a frame that a colour check / depth-count call in flight is reading on the colour-check stream
int refuse_checked_slots(const lm_detector* d, int first, int n) {
    if (d->cc_inflight && d->cc_pending && first <= d->cc_hi && d->cc_lo < first + n) return fail(LM_ERR_INVALID, "slot is read by a colour check in flight: call lm_color_check_end first");
    if (d->dc_inflight && d->dc_pending && first <= d->dc_hi && d->dc_lo < first + n) return fail(LM_ERR_INVALID, "slot is read by depth counts in flight: call lm_depth_counts_end first");
    if (d->ds_inflight && d->ds_pending && first <= d->ds_hi && d->ds_lo < first + n) return fail(LM_ERR_INVALID, "slot is read by a depth selection in flight: call lm_depth_select_end first");
    const long long icp_span = d->icp_span.load();
    if (icp_span >= 0 && first <= (int)(icp_span & 0xFFFFFFFF) && (int)(icp_span >> 32) < first + n)
        return fail(LM_ERR_INVALID, "slot is read by an ICP refinement in flight");
    const long long export_span = d->export_span.load();
    if (export_span >= 0 && first <= (int)(export_span & 0xFFFFFFFF) && (int)(export_span >> 32) < first + n)
        return fail(LM_ERR_INVALID, "slot is read by an export in flight");
    return LM_OK;
}

// what the planner (lm_host.h plan_layout / plan_scan) looks at for a call on lane ln
lmh::ScanInputs scan_inputs(const lm_detector* d, const lm_detector::Lane& ln) {
    const LmLevelGeom& g = d->geom[d->cfg.pyramid_levels - 1];
    lmh::ScanInputs in;
    in.form = d->scan_form; in.M = d->cfg.num_modalities;
    in.nibble = g.nibble != 0; in.planes = g.plane_ori != 0; in.lds_fits = lmh::lds_image_fits(g, in.M);
    in.bank_built = !d->bank_dirty;
    in.scanl_bank = d->hb.lds_ok && d->d_litem; in.scanl_device = d->scanl_lds;
    in.fpad1 = d->hb.fpad1; in.items1_by_L = d->hb.items1_by_L; in.items4 = (long long)d->hb.item_t.size();
    in.frame_stride = d->frame_stride; in.arena_bytes = g.arena_bytes;
    in.threshold = ln.raw_thr_for; in.scan1_min_threshold = d->scan1_min_threshold;
    in.scanl_min_slots = d->scanl_min_slots; in.scanl_R = d->scanl_R;
    return in;
}

// How many 640 x 480 frames one frame of this detector counts as in the few-frame / batch kernel selection (at least 1).
int slot_weight(const lm_detector* d) {
    const long px = (long)d->lw[0] * d->lh[0];
    const int w = d->work_weight_by_pixels ? (int)(px / (640L * 480L)) : 1;
    return w < 1 ? 1 : w;
}

bool any_match_mask(const lm_detector* d, int first, int n) {
    for (int i = first; i < first + n; ++i)
        if (d->slots[i].match_mask_on[0] || d->slots[i].match_mask_on[1] || d->slots[i].rule_on) return true;
    return false;
}

// A bound of the HSV range as cv::inRange means it for 8-bit channels: rounded to the nearest integer (ties to even), and clamped to [-1, 256]
// first -- beyond 8 bits a bound means "no limit" (or "nothing"), while (int) of lrint(1e12) keeps the low 32 bits, a negative number.
int hsv_bound(double b) { return (int)std::lrint(std::min(256.0, std::max(-1.0, b))); }

// cv::cvtColor's 8-bit RGB2HSV tables: sdiv_table[i] = round((255 << 12) / i), hdiv_table180[i] = round((180 << 12) / (6 i)), for the
// colour check's k_hsv_mask and the mask rules' HSV gate.  Uploaded once, on lane 0's stream, and waited for.
int ensure_hsv_div(lm_detector* d) {
    if (d->d_hsv_div) return LM_OK;
    std::vector<int> tab(512, 0);
    for (int i = 1; i < 256; ++i) {
        tab[(size_t)i] = (int)std::lrint((255 << 12) / (1.0 * i));
        tab[256 + (size_t)i] = (int)std::lrint((180 << 12) / (6.0 * i));
    }
    DevBuf<int> p;
    HIP_TRY(p.alloc(tab.size()));
    hipStream_t st = d->lanes[0].stream;
    if (hipMemcpyAsync(p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(LM_ERR_HIP, "upload of the HSV division tables failed");
    d->d_hsv_div = std::move(p);
    return LM_OK;
}

int slot_lacks_depth(const lm_detector* d, int slot) {
    if (d->slots[(size_t)slot].has_depth) return LM_OK;
    return fail(LM_ERR_INVALID, "the frame in slot " + std::to_string(slot) + " came without a depth image");
}

// A ruled slot whose rule has a depth gate needs its frame's depth image: refused before anything is enqueued.  depth_coming: the call
// itself brings the depth image of the one slot it names (the host-frame matches).
int refuse_depthless_rules(const lm_detector* d, int first, int n, bool depth_coming) {
    if (!depth_optional(d)) return LM_OK;      // (an RGB-D frame always has its depth image; without a depth plane no rule has a depth gate)
    for (int i = first; i < first + n; ++i) {
        const Slot& s = d->slots[(size_t)i];
        if (s.rule_on && s.rule.use_depth && !depth_coming)
            if (int rc = slot_lacks_depth(d, i)) return rc;
    }
    return LM_OK;
}

// The contract of lm_mask_rule (include/linemod_hip.h); *out = the rule as k_mask_rule takes it.
int check_mask_rule(const lm_detector* d, const lm_mask_rule* r, LmRule* out) {
    const lm_config& c = d->cfg;
    if (r->modalities <= 0 || r->modalities >= (1 << c.num_modalities))
        return fail(LM_ERR_INVALID, "mask rule: modalities must name at least one modality the detector has (bit 0 colour, bit 1 depth)");
    if (r->use_depth && !keeps_depth(d))
        return fail(LM_ERR_INVALID, "mask rule: a depth gate needs the depth frame, which a colour-only detector does not keep on the device");
    if (r->use_depth && (r->zmin < 0 || r->zmax > 65535 || r->zmin > r->zmax))
        return fail(LM_ERR_INVALID, "mask rule: depth gate needs 0 <= zmin <= zmax <= 65535");
    if (r->grow < 0 || r->grow > LM_RULE_MAX_GROW) return fail(LM_ERR_INVALID, "mask rule: grow out of range (0 .. 16)");
    const lm_rect& q = r->rect;
    const bool no_rect = q.width == 0 && q.height == 0;
    if (!no_rect && (q.x < 0 || q.y < 0 || q.width <= 0 || q.height <= 0 || q.x > c.width - q.width || q.y > c.height - q.height))
        return fail(LM_ERR_INVALID, "mask rule: the rectangle must lie inside the frame");
    if (!lmk_mask_rule_fits(c.width)) return fail(LM_ERR_INVALID, "mask rule: frame too wide for the rule kernel");
    LmRule o{};
    o.use_depth = r->use_depth != 0; o.keep_invalid = r->keep_invalid != 0; o.use_hsv = r->use_hsv != 0;
    o.zmin = r->zmin; o.zmax = r->zmax; o.grow = r->grow;
    for (int k = 0; k < 3; ++k) { o.hsv.lo[k] = hsv_bound(r->lower[k]); o.hsv.hi[k] = hsv_bound(r->upper[k]); }
    o.rx = no_rect ? 0 : q.x; o.ry = no_rect ? 0 : q.y; o.rw = no_rect ? c.width : q.width; o.rh = no_rect ? c.height : q.height;
    *out = o;
    return LM_OK;
}

// k_mask_rule over the ruled slots of [first, first + n): their rule planes from the frames they hold.  One launch per LM_MASK_SLOTS
// slots or LM_RULE_KINDS different rules (a rule set on a slot range is one kind).
void enqueue_mask_rules(lm_detector* d, lm_detector::Lane& ln, int first, int n) {
    const lm_config& c = d->cfg;
    LmRuleArgs a{};
    a.bgr = d->bgr(0, 0); a.depth = keeps_depth(d) ? d->depth(0) : nullptr; a.slot_stride = d->frame_stride;
    a.divtab = d->d_hsv_div; a.w = c.width; a.h = c.height; a.mask_pitch = (u32)d->match_mask_pitch;
    int kinds = 0;
    for (int i = first; i < first + n; ++i) {
        const Slot& s = d->slots[i];
        if (!s.rule_on) continue;
        int k = 0;
        while (k < kinds && std::memcmp(&a.rule[k], &s.rule_dev, sizeof(LmRule)) != 0) ++k;
        if (k == LM_RULE_KINDS) { lmk_mask_rule(ln.stream, a); a.n = 0; kinds = 0; k = 0; }
        if (k == kinds) a.rule[kinds++] = s.rule_dev;
        a.slot[a.n] = (u16)i; a.kind[a.n] = (u8)k; a.plane[a.n] = s.d_rule_mask;
        if (++a.n == LM_MASK_SLOTS) { lmk_mask_rule(ln.stream, a); a.n = 0; kinds = 0; }
    }
    lmk_mask_rule(ln.stream, a);
}

static_assert(LM_MAX_LEVELS <= LM_MASK_LEVELS, "LmMaskArgs holds LM_MASK_LEVELS levels");
// k_match_mask over the masked slots of [first, first + n), after the last quantiser: colour quant[l][0] at every level, depth quant[0][1]
// only -- the depth levels above read quant[0][1] at (2y, 2x) (the level-1 memories and enqueue_depth_pyramid's k_nn_half for
// L > 2), the NN rule the mask pyramid follows too (mask_l = mask0[y << l][x << l]), so masking quant[0][1] once is exact at every level.
void enqueue_match_masks(lm_detector* d, lm_detector::Lane& ln, int first, int n) {
    const lm_config& c = d->cfg;
    LmMaskArgs a{};
    a.frame = d->frame_arena; a.slot_stride = d->frame_stride;
    a.levels = c.pyramid_levels; a.mask_pitch = (u32)d->match_mask_pitch;
    a.vec_rows = 1;
    for (int l = 0; l < c.pyramid_levels; ++l) {
        for (int m = 0; m < c.num_modalities; ++m) a.off_quant[l][m] = (u32)d->off_quant[l][m];
        a.w[l] = (u32)d->lw[l];
        a.vec_begin[l + 1] = a.vec_begin[l] + (u32)((size_t)d->lw[l] * d->lh[l] / 16);   // (w * h % 16 == 0 at every level: lm_create)
        if (d->lw[l] % 16) a.vec_rows = 0;
    }
    a.vec_depth = a.vec_begin[1];
    for (int i = first; i < first + n; ++i) {
        const Slot& s = d->slots[i];
        if (!s.match_mask_on[0] && !(c.num_modalities == 2 && s.match_mask_on[1])) continue;
        a.slot[a.n] = (u16)i;
        a.cmask[a.n] = s.match_mask_on[0] ? s.d_match_mask : nullptr;
        a.dmask[a.n] = (c.num_modalities == 2 && s.match_mask_on[1]) ? s.d_match_mask + d->match_mask_pitch * c.height : nullptr;
        if (++a.n == LM_MASK_SLOTS) { lmk_match_mask(ln.stream, a); a.n = 0; }
    }
    if (a.n) lmk_match_mask(ln.stream, a);
    // second pass: the rule planes of the ruled slots (one plane for the modalities the rule names); a slot with both ends up
    // with the AND of the two masks
    a.n = 0;
    for (int i = first; i < first + n; ++i) {
        const Slot& s = d->slots[i];
        if (!s.rule_on) continue;
        a.slot[a.n] = (u16)i;
        a.cmask[a.n] = (s.rule.modalities & 1) ? s.d_rule_mask : nullptr;
        a.dmask[a.n] = (c.num_modalities == 2 && (s.rule.modalities & 2)) ? s.d_rule_mask : nullptr;
        if (++a.n == LM_MASK_SLOTS) { lmk_match_mask(ln.stream, a); a.n = 0; }
    }
    if (a.n) lmk_match_mask(ln.stream, a);
}

// What the pre-processing planner (lm_host.h) looks at for the frames in slots [first, first + n), slot_stride bytes apart: shapes, the
// levels' memory modes, the low address bits of the buffers and ONE snapshot of the process-wide LM_TUNE_* knobs.  The call-specific
// fields (weight, masks, lanes, planes) stay at their defaults: a single stage's.
lmh::PreInputs pre_inputs(lm_detector* d, int first, int n, size_t slot_stride) {
    const lm_config& c = d->cfg;
    const auto low = [](const void* p) { return (u32)((uintptr_t)p & 15); };
    lmh::PreInputs in;
    in.M = c.num_modalities; in.L = c.pyramid_levels; in.n = n;
    for (int l = 0; l < in.L; ++l) {
        const LmLevelGeom& g = d->geom[l];
        lmh::PreLevel& v = in.lv[l];
        v.w = g.w; v.h = g.h; v.T = g.T; v.mode = g.spread_only ? 1 : g.nibble ? 2 : 0;
        v.a_bgr = low(d->bgr(first, l)); v.a_cs = low(d->cscratch(first, l));
        for (int m = 0; m < in.M; ++m) { v.a_quant[m] = low(d->quant(first, l, m)); v.a_lm[m] = low(d->lm(first, l) + (size_t)m * g.mod_stride); }
    }
    in.lut_onehot = in.M == 2 ? normal_lut_onehot(d) : true;
    in.ori_stride = d->geom[in.L - 1].ori_stride;
    in.a_depth = in.M == 2 ? low(d->depth(first)) : 0u; in.a_ds = low(d->dscratch(first));
    in.a_stride = (u32)(slot_stride & 15);
    in.knobs = lmh::pre_knobs();
    return in;
}

// ... and the same slots' buffers for lmk_preprocess_run; mag: the levels' gradient magnitudes, or null
LmPreArgs pre_args(lm_detector* d, int first, int n, size_t slot_stride, float* const* mag) {
    const lm_config& c = d->cfg;
    LmPreArgs a{};
    a.L = c.pyramid_levels;
    for (int l = 0; l < a.L; ++l) {
        const LmLevelGeom& g = d->geom[l];
        a.w[l] = g.w; a.h[l] = g.h; a.T[l] = g.T; a.mode[l] = g.spread_only ? 1 : g.nibble ? 2 : 0; a.ori_stride[l] = g.ori_stride;
        a.bgr[l] = d->bgr(first, l); a.cs[l] = d->cscratch(first, l); a.mag[l] = mag ? mag[l] : nullptr;
        for (int m = 0; m < c.num_modalities; ++m) { a.quant[l][m] = d->quant(first, l, m); a.lm[l][m] = d->lm(first, l) + (size_t)m * g.mod_stride; }
    }
    a.depth = c.num_modalities == 2 ? d->depth(first) : nullptr; a.ds = d->dscratch(first);
    a.weak_threshold = c.weak_threshold; a.dist_thr = c.distance_threshold; a.diff_thr = c.difference_threshold;
    a.normal_lut = d->d_normal_lut; a.resp_tab = d->d_resp_tab;
    a.slot_stride = slot_stride; a.nslots = n;
    return a;
}

// quant[l][1] for l >= 1: DepthNormalPyramid::pyrDown = NN half-size copy of the quantised image
void enqueue_depth_pyramid(lm_detector* d, lm_detector::Lane& ln, int first, int n) {
    const lmh::PreInputs in = pre_inputs(d, first, n, d->frame_stride);
    lmh::PrePlan plan;
    for (int l = 1; l < in.L; ++l) lmh::plan_nn_half(in, l, plan);
    lmk_preprocess_run(ln.stream, plan, 0, plan.n, pre_args(d, first, n, d->frame_stride, nullptr));
}

// lm_add_template's quantisation of the images in slots [first, first + n) (the generators: a chunk's slots at once): every level's colour image with
// its gradient magnitudes (mag[l]: level l of the first slot), the depth normals and their NN pyramid.  One stage after the other, each planned
// on its own at weight 1 -- the generator's chunks of large frames included, as before the planner.
void enqueue_template_quantize(lm_detector* d, int first, int n, size_t slot_stride, float* const* mag) {
    lmh::PreInputs in = pre_inputs(d, first, n, slot_stride);
    in.want_mag = true;
    lmh::PrePlan plan;
    for (int l = 0; l < in.L; ++l) {
        if (l > 0) lmh::plan_pyrdown(in, l, plan);
        lmh::plan_color_quantize(in, l, false, plan);
    }
    if (in.M == 2) lmh::plan_depth_quantize(in, plan);
    lmk_preprocess_run(d->lanes[0].stream, plan, 0, plan.n, pre_args(d, first, n, slot_stride, mag));
    if (in.M == 2) enqueue_depth_pyramid(d, d->lanes[0], first, n);
}

// a3-a10 on the frames resident in slots [first, first + n): fill the planner's inputs, plan, note the layout, execute.
void enqueue_preprocess(lm_detector* d, lm_detector::Lane& ln, int first, int n) {
    const int L = d->cfg.pyramid_levels;
    const lmh::Layout layout = lmh::plan_layout(scan_inputs(d, ln), n);
    for (int i = 0; i < n; ++i) d->slots[first + i].layout = layout;
    lmh::PreInputs in = pre_inputs(d, first, n, d->frame_stride);
    in.weight = slot_weight(d);
    in.masked = any_match_mask(d, first, n);
    for (int o = 0; o < LM_NLANES; ++o) in.others_busy |= (&d->lanes[o] != &ln && d->lanes[o].busy);
    in.phase_max_slots = d->phase_max_slots; in.batch_phases = d->batch_phases;
    // the scanned level's plane stride when the planes are written; bit 31: d_lm_fast writes the spread byte instead of the response memories
    in.planes = layout == lmh::Layout::Responses ? 0u : d->geom[L - 1].plane_ori | (layout == lmh::Layout::SpreadAndPlanes ? 0x80000000u : 0u);
    lmh::PrePlan plan;
    lmh::plan_preprocess(in, plan);
    LmPreArgs a = pre_args(d, first, n, d->frame_stride, nullptr);
    a.planes = in.planes;
    int next = 0;
    if (plan.mask_step >= 0) {      // Detector::match's masks, between the last quantiser and the first reader of the quantised images
        lmk_preprocess_run(ln.stream, plan, 0, plan.mask_step, a);
        enqueue_mask_rules(d, ln, first, n);      // (the caller's upload wait is on the stream already: the rules read the new frames)
        enqueue_match_masks(d, ln, first, n);
        next = plan.mask_step + 2;
    }
    lmk_preprocess_run(ln.stream, plan, next, plan.n, a);
}

void fill_raw_thr(int* tab, float threshold) {
    // A.7: int(2n + (t/100)*2n + 0.5f) in float arithmetic (file is built with -ffp-contract=off)
    for (int n = 0; n < 128; ++n) tab[n] = static_cast<int>(2 * n + (threshold / 100.f) * (2 * n) + 0.5f);
}

int item_range(lm_detector* d, int class_idx, ItemRange* r) {
    const int nc = (int)d->bank.classes.size();
    if (class_idx >= nc || class_idx < -1) return fail(LM_ERR_INVALID, "class index out of range");
    if (class_idx < 0) { r->lo = 0; r->n = (int)d->hb.item_t.size(); r->t_lo = 0; r->t_hi = (int)d->hb.t_global.size(); }
    else {
        r->lo = d->hb.class_item_lo[class_idx]; r->n = d->hb.class_item_hi[class_idx] - r->lo;
        r->t_lo = d->hb.class_t_lo[class_idx]; r->t_hi = d->hb.class_t_hi[class_idx];
    }
    return LM_OK;
}

// Detector::match(..., class_ids): the work-item ranges of a LIST of classes (HighLevelLinemod.cpp:145,152).  {-1} or an
// empty list = every class (upstream: an empty class_ids vector).  Duplicates are dropped (upstream would emit the
// class twice and std::unique would remove the copies again); ranges of neighbouring classes are merged, so the usual
// "all classes of the bank" list is ONE scan launch.  `classes` comes back normalised (sorted, unique).
int item_ranges(lm_detector* d, std::vector<int>& classes, std::vector<ItemRange>& out) {
    const int nc = (int)d->bank.classes.size();
    out.clear();
    for (int c : classes) if (c < -1 || c >= nc) return fail(LM_ERR_INVALID, "class index out of range");
    std::sort(classes.begin(), classes.end());
    classes.erase(std::unique(classes.begin(), classes.end()), classes.end());
    if (classes.empty() || classes[0] < 0) {
        if (classes.size() > 1) return fail(LM_ERR_INVALID, "class index -1 (all classes) cannot be combined with others");
        classes.assign(1, -1);
        out.push_back(ItemRange{0, (int)d->hb.item_t.size(), 0, (int)d->hb.t_global.size()});
        return LM_OK;
    }
    for (int c : classes) {
        const int lo = d->hb.class_item_lo[c], hi = d->hb.class_item_hi[c];
        if (!out.empty() && out.back().lo + out.back().n == lo && out.back().t_hi == d->hb.class_t_lo[c]) { out.back().n += hi - lo; out.back().t_hi = d->hb.class_t_hi[c]; }
        else out.push_back(ItemRange{lo, hi - lo, d->hb.class_t_lo[c], d->hb.class_t_hi[c]});
    }
    return LM_OK;
}

// the work items of k_scan1 for L1 lanes per frame, built and uploaded on first use
int ensure_items1(lm_detector* d, int L1, const lm_detector::Items1** out) {
    for (const auto& it : d->items1) if (it.L == L1) { *out = &it; return LM_OK; }
    std::vector<u32> t, c;
    lm_detector::Items1 it;
    it.L = L1;
    lmh::build_items1(d->hb, L1, t, c, it.begin);
    HIP_TRY(upload_vec(it.d_t, t));
    HIP_TRY(upload_vec(it.d_chunk, c));
    d->items1.push_back(std::move(it));
    *out = &d->items1.back();
    return LM_OK;
}

// the layouts slots [first, first + n) hold (lmh::layout_bit)
static unsigned slot_layouts(const lm_detector* d, int first, int n) {
    unsigned held = 0;
    for (int i = first; i < first + n; ++i) held |= lmh::layout_bit(d->slots[i].layout);
    return held;
}

static int refuse_scan(lmh::ScanPlan::Kind k) {
    if (k == lmh::ScanPlan::Mixed)
        return fail(LM_ERR_INVALID, "the slots were prepared by calls of different scan forms (some keep only the spread byte of the scanned level): match them apart or upload again");
    // (no work items -- allocation failure, no lane count fits: k_scan4 would read garbage in slots without response memories)
    return fail(LM_ERR_HIP, "the slots keep only the spread byte of the scanned level and the bit-plane scan could not be set up for them: upload the frames again");
}

// The lane's survivor queue (k_scan1), allocated on the lane's first bit-plane scan; false: there is none (the waves take their
// survivors' exact sums themselves).
static bool ensure_surv_queue(lm_detector* d, lm_detector::Lane& ln) {
    DevBuf<unsigned long long>& q = ln.d_surv;
    if (!q) {
        if (q.alloc(16 + (size_t)d->surv_cap) != hipSuccess) (void)hipGetLastError();
        // (on the lane's OWN stream: the lanes' streams are non-blocking, a hipMemset on the null stream is not ordered against them -- it could land after the
        // lane's first k_scan1 had started counting its survivors, and k_scan1_exact then summed fewer than were queued: the rare lost match of a lane's FIRST
        // bit-plane scan, tests/test_gpu_fullsize.py::test_config3_batch_bit_plane_scan_at_stated_size, about once in ten runs of the suite)
        else if (hipMemsetAsync(q, 0, 16 * sizeof(unsigned long long), ln.stream) != hipSuccess) { q.reset(); (void)hipGetLastError(); }
        ln.surv_set = 0;
    }
    return q != nullptr;
}

// what the planner (lm_host.h plan_match) looks at for slots [first, first + nslots) over the items of r, but for the resources of k_scan1
static lmh::MatchInputs match_inputs(const lm_detector* d, const lm_detector::Lane& ln, int first, ItemRange r, int nslots, int variant) {
    const int L = d->cfg.pyramid_levels;
    const LmLevelGeom& g = d->geom[L - 1];
    lmh::MatchInputs in;
    in.scan = scan_inputs(d, ln);
    in.layouts = slot_layouts(d, first, nslots); in.nslots = nslots;
    in.n_items = r.n;
    in.n_litems = d->hb.lds_ok ? d->hb.lbegin[(size_t)r.t_hi] - d->hb.lbegin[(size_t)r.t_lo] : 0;
    in.T = g.T; in.wh = g.wh; in.ori_stride = g.ori_stride; in.nibble = g.nibble != 0;
    in.M = d->cfg.num_modalities; in.L = L;
    for (int l = 0; l < L; ++l) in.level_W[l] = d->geom[l].W;
    in.miss_delta = d->miss_delta;
    in.have_plan = ln.plan != nullptr; in.plan_stride_cap = d->plan_stride_cap;
    in.variant = variant;
    in.sort_split_mode = d->sort_split_mode; in.sort_long_score = d->sort_long_score;
    return in;
}

// Plans a11-a15 of slots [first, first + nslots) over the items of r (after making sure of what a k_scan1 launch needs: its work items, the
// lane's queue) and binds the scan's pointers.  variant: the launch's scan variant.
int make_scan_args(lm_detector* d, lm_detector::Lane& ln, int first, ItemRange r, int nslots, int variant, lmh::MatchPlan* plan, LmScanArgs* out) {
    const int L = d->cfg.pyramid_levels;
    const LmLevelGeom& g = d->geom[L - 1];
    lmh::MatchInputs in = match_inputs(d, ln, first, r, nslots, variant);
    const lm_detector::Items1* it = nullptr;
    if (const int L1 = lmh::match_scan1_lanes(in))
        if (ensure_items1(d, L1, &it) == LM_OK) {
            in.items1_L = L1; in.n_items1 = it->begin[(size_t)r.t_hi] - it->begin[(size_t)r.t_lo];
            in.have_queue = ensure_surv_queue(d, ln);
        }
    lmh::MatchPlan& p = *plan;
    lmh::plan_match(in, p);
    if (p.kind == lmh::ScanPlan::Mixed || p.kind == lmh::ScanPlan::NoBitPlaneForm) return refuse_scan(p.kind);
    LmScanArgs& a = *out;
    a = LmScanArgs();       // (what a form does not read stays null / 0)
    a.lm = d->lm(first, L - 1); a.lm_slot_stride = d->frame_stride;
    a.item_t = d->d_item_t; a.item_chunk = d->d_item_chunk; a.item_lo = r.lo; a.n_items = p.n_items;
    a.nibble = g.nibble; a.M = d->cfg.num_modalities; a.fpad = d->hb.fpad; a.W = g.W; a.T = g.T;
    a.scan_off = d->d_scan_off; a.scan_P = d->d_scan_P; a.scan_n = d->d_scan_n;
    a.raw_thr_by_n = ln.d_raw_thr;
    a.hdr = reinterpret_cast<LmDevHeader*>(d->aux(first, d->off_hdr));
    a.cand = reinterpret_cast<LmCand*>(d->aux(first, d->off_cand));
    a.aux_slot_stride = d->aux_stride; a.cand_cap = d->max_cand;
    a.stat = d->scan_stats ? d->d_scan_stat : nullptr;
    // the plan's numbers
    a.wgs_per_slot = p.wgs_per_slot; a.nslots = nslots;
    a.L1 = p.L1; a.G1 = p.G1; a.L1_rcp16 = p.L1_rcp16; a.delta_rcp16 = p.delta_rcp16; a.no_exact = p.no_exact; a.exact_spread = p.exact_spread ? 1 : 0;
    a.R = p.R; a.pb = p.pb; a.planes_off = p.planes_off; a.tbl_bytes = p.tbl_bytes; a.queue_cap = p.queue_cap; a.dbg = p.dbg;
    // the bit-plane forms' lists
    if (p.kind != lmh::ScanPlan::Scan4) { a.fpad1 = d->hb.fpad1; a.offs3 = d->d_offs3; a.resp_tab = d->d_resp_tab; }
    if (p.kind == lmh::ScanPlan::ScanL) {
        a.lds_form = 1;
        a.offl = d->d_offl; a.offsl = d->d_offsl; a.litem = d->d_litem; a.litem_lo = d->hb.lbegin[(size_t)r.t_lo]; a.n_litems = in.n_litems;
        a.mod_stride = g.mod_stride; a.plane_ori = g.plane_ori;
    } else if (p.kind == lmh::ScanPlan::Scan1) {
        a.off1 = d->d_off1; a.offn = d->d_offn;
        a.item_t = it->d_t; a.item_chunk = it->d_chunk; a.item_lo = it->begin[(size_t)r.t_lo];
        a.surv = p.queue ? ln.d_surv : nullptr; a.surv_cap = d->surv_cap; a.surv_set = ln.surv_set;
    }
    return LM_OK;
}

// the scan steps of the plan with these arguments; where the plan says so the lane's next bit-plane scan takes the other set of queue counters
// (this launch's k_scan1_exact has zeroed it, or a reset in front of the launch has zeroed both)
void launch_scan(lm_detector::Lane& ln, const lmh::MatchPlan& plan, LmScanArgs& a) {
    lmk_scan_run(ln.stream, plan, a, ln.d_surv);
    if (!plan.flip_surv_set) return;
    ln.surv_set ^= 1;
    a.surv_set = ln.surv_set;
}

// the arguments of the plan's launches that work at `level`
static LmRefineArgs make_refine_args(lm_detector* d, const lm_detector::Lane& ln, int first, int n, int level, float threshold, const lmh::MatchPlan& p) {
    LmRefineArgs a;
    a.lm = d->lm(first, level); a.lm_slot_stride = d->frame_stride;
    a.g = d->geom[level];
    a.M = d->cfg.num_modalities;
    a.meta = d->d_ref_meta[level]; a.feats = d->d_ref_feat[level];
    a.sim_lut = d->d_sim_lut;
    a.hdr = reinterpret_cast<LmDevHeader*>(d->aux(first, d->off_hdr));
    a.cand = reinterpret_cast<LmCand*>(d->aux(first, d->off_cand));
    a.keys = reinterpret_cast<u64*>(d->aux(first, d->off_keys));
    a.aux_slot_stride = d->aux_stride;
    a.cand_cap = d->max_cand; a.match_cap = d->max_match;
    a.threshold = threshold;
    a.t_global = d->d_t_global; a.t_class = d->d_t_class;
    a.plan = p.refine_plan ? ln.plan : nullptr; a.plan_cap = p.plan_cap;
    a.blocks_per_slot = p.blocks_per_slot; a.nslots = n;
    a.stat = d->d_refine_stat;
    return a;
}

static LmSortArgs make_sort_args(lm_detector* d, int first, const lmh::MatchPlan& p) {
    LmSortArgs a;
    a.hdr = reinterpret_cast<LmDevHeader*>(d->aux(first, d->off_hdr));
    a.keys = reinterpret_cast<u64*>(d->aux(first, d->off_keys));
    a.out = reinterpret_cast<LmOutMatch*>(d->aux(first, d->off_out));
    a.split = p.split;
    a.aux_slot_stride = d->aux_stride;
    a.host = d->host_block(first);
    a.host_slot_stride = d->host_stride;
    a.cand_cap = d->max_cand; a.match_cap = d->max_match;
    return a;
}

int enqueue_threshold(lm_detector::Lane& ln, float threshold) {
    if (!(threshold >= 0.0f)) return fail(LM_ERR_INVALID, "threshold must be >= 0");
    if (ln.raw_thr_for != threshold) {
        HIP_TRY(hipStreamSynchronize(ln.stream));  // the pinned table may still feed an earlier copy
        fill_raw_thr(ln.h_raw_thr, threshold);
        HIP_TRY(hipMemcpyAsync(ln.d_raw_thr, ln.h_raw_thr, 128 * sizeof(int), hipMemcpyHostToDevice, ln.stream));
        ln.raw_thr_for = threshold;
    }
    return LM_OK;
}

// a11-a15 on prepared linear memories; the sort kernel publishes the results to host-mapped memory.
int enqueue_match_stages(lm_detector* d, lm_detector::Lane& ln, int first, int n, float threshold, const std::vector<ItemRange>& ranges, bool timed) {
    const int L = d->cfg.pyramid_levels;
    if (lmh::layouts_mixed(slot_layouts(d, first, n))) return refuse_scan(lmh::ScanPlan::Mixed);      // (whatever the ranges)
    if (timed) HIP_TRY(hipEventRecord(ln.ev[1], ln.stream));
    // one plan and one scan launch per run of neighbouring classes; the launches append to the same candidate lists.  The stages behind the
    // scan are the same in every range's plan: the last one's run
    lmh::MatchPlan mp;
    bool planned = false;
    for (const ItemRange& r : ranges)
        if (r.n > 0) {
            LmScanArgs sa;
            if (int rc = make_scan_args(d, ln, first, r, n, d->scan_variant, &mp, &sa)) return rc;
            launch_scan(ln, mp, sa);
            planned = true;
            d->cnt_scan_launches += 1; d->cnt_scan1_launches += (sa.L1 || sa.lds_form) ? 1 : 0; d->last_scan1_lanes = scan_form_code(sa);
        }
    if (!planned) lmh::plan_match(match_inputs(d, ln, first, ItemRange{0, 0, 0, 0}, n, d->scan_variant), mp);      // (no class of the list has a template here)
    if (timed) HIP_TRY(hipEventRecord(ln.ev[2], ln.stream));
    LmRefineArgs ra[LM_MAX_LEVELS];
    for (int l = 0; l < std::max(L - 1, 1); ++l) ra[l] = make_refine_args(d, ln, first, n, l, threshold, mp);
    const LmSortArgs so = make_sort_args(d, first, mp);
    lmk_refine_run(ln.stream, mp, mp.scan_end, mp.refine_end, ra, so, ln.plan);
    d->cnt_refine_launches += L - 1;
    if (timed) HIP_TRY(hipEventRecord(ln.ev[3], ln.stream));
    lmk_refine_run(ln.stream, mp, mp.refine_end, mp.n, ra, so, ln.plan);
    d->cnt_sort_launches += 1;
    if (timed) HIP_TRY(hipEventRecord(ln.ev[4], ln.stream));
    HIP_TRY(hipGetLastError());
    return LM_OK;
}

// The lane's stream waits for the copy-stream uploads of the slots it is about to read.
int enqueue_upload_wait(lm_detector* d, lm_detector::Lane& ln, int first, int n) {
    int rc;
    unsigned long long seqs[LM_NCOPY];
    if ((rc = wait_uploads(d, ln.stream, first, n, seqs))) return rc;
    for (int k = 0; k < LM_NCOPY; ++k) if (seqs[k] > ln.waited_seq[k]) ln.waited_seq[k] = seqs[k];
    return LM_OK;
}

// `classes` is normalised in place (item_ranges).  prepared: the slots' a3-a10 results are current (checked by the
// caller): a11-a15 only.
int enqueue_match(lm_detector* d, lm_detector::Lane& ln, int first, int n, float threshold, std::vector<int>& classes, bool timed,
                  bool prepared) {
    std::vector<ItemRange> ranges;
    int rc;
    if (!prepared && (rc = refuse_depthless_rules(d, first, n))) return rc;
    if ((rc = item_ranges(d, classes, ranges))) return rc;
    if ((rc = enqueue_threshold(ln, threshold))) return rc;
    if ((rc = enqueue_upload_wait(d, ln, first, n))) return rc;
    if (timed) HIP_TRY(hipEventRecord(ln.ev[0], ln.stream));
    if (!prepared) {
        enqueue_preprocess(d, ln, first, n);
        d->cnt_preprocess_frames += n;
        for (int i = 0; i < n; ++i) d->slots[first + i].prepared = true;
    }
    return enqueue_match_stages(d, ln, first, n, threshold, ranges, timed);
}
int enqueue_match(lm_detector* d, lm_detector::Lane& ln, int first, int n, float threshold, int class_idx, bool timed) {
    std::vector<int> classes(1, class_idx);
    return enqueue_match(d, ln, first, n, threshold, classes, timed);
}

inline bool key_less(const u64* a, const u64* b) { return a[0] < b[0] || (a[0] == b[0] && a[1] < b[1]); }

// Delivers the sorted unique matches of one slot (the stream has been synchronised).
int collect_slot(lm_detector* d, int slot, lm_match_t* out, size_t cap, size_t* n_out) {
    const LmHostBlock* hb = d->host_block(slot);
    const LmHeader h = hb->hdr;
    if (h.cand_count > d->max_cand)
        return fail(LM_ERR_OVERFLOW, "scan produced " + std::to_string(h.cand_count) + " candidates, capacity " +
                                         std::to_string(d->max_cand) + " (raise lm_config.max_candidates)");
    if (h.match_count > d->max_match)
        return fail(LM_ERR_OVERFLOW, "refinement produced " + std::to_string(h.match_count) + " matches, capacity " +
                                         std::to_string(d->max_match) + " (raise lm_config.max_matches)");
    note_sort_length(d, h.match_count);
    size_t n = 0;
    if (h.sorted_on_device) {
        n = h.out_count;
        size_t ncopy = std::min(n, cap);
        size_t inl = std::min<size_t>(ncopy, LM_INLINE_MATCHES);
        if (out && inl) std::memcpy(out, hb->rec, inl * sizeof(lm_match_t));
        if (out && ncopy > inl)
            HIP_TRY(hipMemcpy(out + inl, reinterpret_cast<lm_match_t*>(d->aux(slot, d->off_out)) + inl,
                              (ncopy - inl) * sizeof(lm_match_t), hipMemcpyDeviceToHost));
    } else {
        // more than LM_SORT_CAP matches: sort + unique the keys on the host (same total order)
        std::vector<u64> keys((size_t)h.match_count * 2);
        if (h.match_count)
            HIP_TRY(hipMemcpy(keys.data(), d->aux(slot, d->off_keys), keys.size() * sizeof(u64), hipMemcpyDeviceToHost));
        std::vector<u32> idx(h.match_count);
        for (u32 i = 0; i < h.match_count; ++i) idx[i] = i;
        std::sort(idx.begin(), idx.end(), [&](u32 a, u32 b) { return key_less(&keys[2 * (size_t)a], &keys[2 * (size_t)b]); });
        const u64* prev = nullptr;
        for (u32 i : idx) {
            const u64* k = &keys[2 * (size_t)i];
            if (prev && prev[1] == k[1] && (prev[0] >> 32) == (k[0] >> 32)) { prev = k; continue; }
            prev = k;
            if (out && n < cap) {
                lm_match_t m;
                u32 sb = ~(u32)(k[0] >> 32);
                std::memcpy(&m.similarity, &sb, 4);
                m.template_id = (int)(u32)k[0];
                m.class_idx = (int)(k[1] >> 48);
                m.y = (int)((k[1] >> 24) & 0xFFFFFFu) - 0x800000;
                m.x = (int)(k[1] & 0xFFFFFFu) - 0x800000;
                out[n] = m;
            }
            ++n;
        }
    }
    if (n_out) *n_out = n;
    if (n > cap && out) return fail(LM_ERR_OVERFLOW, "output buffer too small for " + std::to_string(n) + " matches");
    return LM_OK;
}

int ready_for_compute(lm_detector* d) {
    int rc;
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if ((rc = ensure_device(d))) return rc;
    if ((rc = ensure_luts(d))) return rc;
    return LM_OK;
}

int ensure_scratch(lm_detector* d, size_t bytes) {
    if (bytes <= d->d_scratch.size()) return LM_OK;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(d->d_scratch.grow(bytes));
    return LM_OK;
}

// ---- lanes: LM_NLANES HIP streams, each with its own events, threshold table and upload tickets -------
// Lane 0's events and tables are created with the device state (ensure_device), those of lanes 1..3 on the lane's first use.  After a
// failure on the way `created` stays false and the next call creates everything again, each create releasing what its member holds.
int ensure_lane(lm_detector* d, int l) {
    lm_detector::Lane& ln = d->lanes[l];
    if (ln.created) return LM_OK;
    if (!ln.stream) HIP_TRY(ln.stream.create(hipStreamNonBlocking));
    for (Event& e : ln.ev) HIP_TRY(e.create());
    HIP_TRY(ln.d_raw_thr.alloc(128));
    HIP_TRY(ln.h_raw_thr.alloc(128));
    ln.raw_thr_for = -1.0f;
    ln.created = true;
    return LM_OK;
}

void account_profile(lm_detector* d, const lm_detector::Lane& ln, int n, const std::vector<int>& classes, bool gathered) {
    for (int k = 0; k < 4; ++k) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ln.ev[k], ln.ev[k + 1]) == hipSuccess) d->prof_us[k] += (double)ms * 1000.0;
    }
    if (gathered) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ln.ev[4], ln.ev[5]) == hipSuccess) { d->prof_exch_us += (double)ms * 1000.0; d->prof_exch_launches += 1; }
    }
    double b = 0;
    for (int c : classes) {
        if (c < 0) for (double v : d->hb.class_alg_bytes) b += v;
        else if (c < (int)d->hb.class_alg_bytes.size()) b += d->hb.class_alg_bytes[c];
    }
    d->prof_scan_bytes += b * n;
    d->prof_launches += 1;
    d->prof_frames += n;
}

// Waits for everything enqueued on the lane's stream.  LM_FLAG_BLOCKING_SYNC: sleep on an event created with
// hipEventBlockingSync instead of spinning in hipStreamSynchronize (for hosts with fewer CPUs than busy processes).
int wait_stream(lm_detector* d, lm_detector::Lane& ln) {
    if (d->cfg.flags & LM_FLAG_BLOCKING_SYNC) {
        Event& ev = ln.blocking_ev;
        if (!ev) HIP_TRY(ev.create(hipEventBlockingSync | hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, ln.stream));
        HIP_TRY(hipEventSynchronize(ev));
    } else {
        HIP_TRY(hipStreamSynchronize(ln.stream));
    }
    // everything this stream was told to wait for has landed
    for (int k = 0; k < LM_NCOPY; ++k) if (ln.waited_seq[k] > d->up_seq_done[k]) d->up_seq_done[k] = ln.waited_seq[k];
    return LM_OK;
}

// lm_match_end's wait (r05).  hipStreamSynchronize on a stream whose work is long done still enqueues a marker and waits for it, and
// HIP streams share a few hardware queues: the marker lands behind the event-record barriers of a COPY stream on the same queue,
// which wait for the NEXT batch's H2D copies -- measured in the streamed PoseDetection (profiles/r05_e2e_timeline.txt): the lane's
// kernels had finished 4.6 ms earlier, the sync still took 0.43-0.52 ms = the next batch's upload.  An event recorded right behind the
// lane's last command when it was enqueued has no such false dependency.
int wait_lane_done(lm_detector* d, lm_detector::Lane& ln) {
    HIP_TRY(hipEventSynchronize(ln.ev_done));
    for (int k = 0; k < LM_NCOPY; ++k) if (ln.waited_seq[k] > d->up_seq_done[k]) d->up_seq_done[k] = ln.waited_seq[k];
    return LM_OK;
}

int run_match(lm_detector* d, lm_detector::Lane& ln, int first, int n, float threshold, std::vector<int> classes, bool prepared = false) {
    if (any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    for (int i = 0; i < n; ++i) {
        if (!d->slots[first + i].has_frame) return fail(LM_ERR_INVALID, "no frame uploaded to slot " + std::to_string(first + i));
        if (prepared && !d->slots[first + i].prepared)
            return fail(LM_ERR_INVALID, "slot " + std::to_string(first + i) + " holds no current a3-a10 results: run lm_prepare_slot or a match on it first");
    }
    int rc;
    if ((rc = enqueue_match(d, ln, first, n, threshold, classes, d->profiling, prepared))) return rc;
    if ((rc = wait_stream(d, ln))) return rc;
    if (d->profiling) account_profile(d, ln, n, classes);   // HIP events on the launch stream bracket every stage
    for (int i = 0; i < n; ++i) d->slots[first + i].matched = true;
    return LM_OK;
}
int run_match(lm_detector* d, lm_detector::Lane& ln, int first, int n, float threshold, int class_idx) {
    return run_match(d, ln, first, n, threshold, std::vector<int>(1, class_idx));
}

}  // namespace lmd

// (the three states are defined in their own files; everything else is a member that releases itself)
lm_detector::~lm_detector() { free_icp(this); free_gen(this); free_eval(this); }

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* lm_last_error(void) { return g_err.c_str(); }
const char* lm_version(void) { return "linemod_hip 0.13 (gfx950; 0.13 = the 0.12 ABI plus the depth registration, lm_set_registration and lm_ingest_frames_registered, and additively the lens rectification at ingest, lm_set_rectification and lm_ingest_frames_rectified; 0.13 additive: raw Bayer ingest formats; 0.13 additive: high-bit raw ingest formats and the raw pipeline; 0.13 additive: the area-averaged reduction at ingest, lm_set_reduction and lm_ingest_frames_reduced; 0.13 additive: rectification and reduction in one ingest pass, lm_ingest_frames_rectified_reduced and lm_stage_rectify_reduce; 0.13 additive: LM_FLAG_KEEP_DEPTH and lm_keeps_depth, a depth frame beside a colour-only detector; 0.13 additive: the depth check's sorted order statistic on the GPU, lm_depth_select_begin and lm_depth_select_end; 0.13 additive: the ICP refinement batched across slots, lm_icp_refine_slots; 0.12 = the 0.11 ABI plus the YUV and grey ingest formats; 0.11 = the 0.10 ABI plus lm_add_templates_slots; 0.10 = the 0.9 ABI plus lm_ingest_*; 0.9 = the 0.8 ABI plus the mask rules, lm_set_mask_rule; 0.8 = the 0.7 ABI plus lm_icp_verify*; 0.7 = the 0.6 ABI plus lm_pose_error_*; 0.6 = the 0.5 ABI plus template generation; 0.5 = the 0.4 ABI plus lm_icp_*)"; }

void lm_default_config(lm_config* c, int color_only, int width, int height) {
    std::memset(c, 0, sizeof(*c));
    c->width = width; c->height = height;
    c->num_modalities = color_only ? 1 : 2;
    c->pyramid_levels = 2;
    c->T[0] = color_only ? 2 : 5;
    c->T[1] = 8;
    c->weak_threshold = 10.0f; c->num_features = 63; c->strong_threshold = 55.0f;
    c->distance_threshold = 2000; c->difference_threshold = 50; c->depth_num_features = 63; c->extract_threshold = 2;
    c->device = 0; c->shard_rank = 0; c->shard_size = 1;
    c->max_candidates = 0; c->max_matches = 0; c->frame_slots = 0;
}

int lm_create(const lm_config* cfg, lm_detector** out) {
    if (!cfg || !out) return fail(LM_ERR_INVALID, "null argument");
    *out = nullptr;
    lm_config c = *cfg;
    if (c.num_modalities < 1 || c.num_modalities > 2) return fail(LM_ERR_INVALID, "num_modalities must be 1 or 2");
    if (c.pyramid_levels < 1 || c.pyramid_levels > LM_MAX_LEVELS) return fail(LM_ERR_INVALID, "pyramid_levels out of range");
    if (c.width <= 0 || c.height <= 0) return fail(LM_ERR_INVALID, "bad frame size");
    if (c.shard_size < 1 || c.shard_rank < 0 || c.shard_rank >= c.shard_size) return fail(LM_ERR_INVALID, "bad shard rank/size");
    if (c.max_candidates <= 0) c.max_candidates = 1 << 18;
    if (c.max_matches <= 0) c.max_matches = 1 << 18;
    if (c.frame_slots <= 0) c.frame_slots = 8;
    if (c.frame_slots > 1024) return fail(LM_ERR_INVALID, "frame_slots out of range");
    {
        std::string why;   // negative / non-finite thresholds would select kernel paths that were never meant to see them
        if (!lmh::check_modality_params(c, why)) return fail(LM_ERR_INVALID, why);
    }
    lm_detector* d = new lm_detector();
    d->cfg = c;
    d->max_cand = (u32)c.max_candidates;
    d->max_match = (u32)c.max_matches;
    int w = c.width, h = c.height;
    for (int l = 0; l < c.pyramid_levels; ++l) {
        if (l > 0) { w /= 2; h /= 2; }
        int T = c.T[l];
        // CV_Assert(rows % T == 0 && cols % T == 0) in linearize, (rows*cols) % 16 == 0 in computeResponseMaps
        if (T <= 0 || w <= 0 || h <= 0 || w % T || h % T || ((long long)w * h) % 16) {
            delete d;
            return fail(LM_ERR_INVALID, "frame size violates cols%T==0, rows%T==0, (rows*cols)%16==0 at level " + std::to_string(l));
        }
        d->lw[l] = w; d->lh[l] = h;
        LmLevelGeom& g = d->geom[l];
        g.w = w; g.h = h; g.T = T; g.W = w / T; g.H = h / T;
        g.wh = (u32)g.W * (u32)g.H;
        // pad: one full linear memory (a scan may start W*H-1 bytes into the last memory and read
        // template_positions <= W*H bytes) + the 16-row patch of the refinement + vector-load slack
        size_t pad = align_up((size_t)g.wh + 16 * (size_t)g.W + 2 * LM_SCAN_CHUNK + 64, 256);
        // the lowest level is scanned (8 response memories per modality); the levels above it are only
        // refined at and keep one spread linear memory per modality (1/8 of the bytes)
        g.spread_only = (l + 1 < c.pyramid_levels) ? 1 : 0;
        // responses are <= 4: the scanned level packs two positions per byte when the linearize fast path applies
        g.nibble = (!g.spread_only && !(c.flags & LM_FLAG_BYTE_RESPONSES) && lmh::nibble_supported(w, T)) ? 1 : 0;
        size_t ori = align_up(((size_t)T * T * g.wh) >> g.nibble, 256) + pad;
        // r05: next to the nibble memories one miss BIT per position and orientation (k_scan1); a scan may start wh - 1 bits into the last
        // plane's last memory and its 64 lanes read 128 bits each
        size_t plane = g.nibble ? align_up(((size_t)T * T * g.wh + 7) / 8 + ((size_t)g.wh + 64 * 128) / 8 + 64, 256) : 0;
        if (g.nibble && (size_t)c.num_modalities * (8 * ori + 8 * plane) + pad > 0x1FFFFFFFull) plane = 0;     // bit offsets are 32-bit
        size_t mod = g.spread_only ? ori : 8 * ori + 8 * plane;
        size_t arena = (size_t)c.num_modalities * mod + pad;
        if (arena > (g.spread_only ? 0x1FFFFFFFull : g.nibble ? 0x7FFFFFFFull : 0xFFFFFFFFull)) { delete d; return fail(LM_ERR_INVALID, "frame too large for the arena offset encoding"); }
        g.ori_stride = (u32)ori;
        g.plane_ori = (u32)plane;
        g.mod_stride = (u32)mod;
        g.zero_off = (u32)((size_t)c.num_modalities * g.mod_stride);
        g.arena_bytes = (u32)arena;
    }
    lmh::default_similarity_lut(d->sim_lut);
    lmh::default_normal_lut(d->normal_lut);
    if (const char* ev = getenv("LM_SCANL_R")) d->scanl_R = std::max(1, atoi(ev));       // (experiments: read once, clamped by lmh::plan_scan)
    *out = d;
    return LM_OK;
}


void lm_destroy(lm_detector* d) {
    if (!d) return;
    if (d->dev_begun) {      // (a detector that never reached its device owns nothing there, and does not start the runtime to say so)
        hipSetDevice(d->cfg.device);
        hipDeviceSynchronize();
        if (d->d_refine_stat) {
            unsigned long long h[8] = {};
            if (hipMemcpy(h, d->d_refine_stat, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess)
                fprintf(stderr, "LM_REFINE_STAT: refined alone %llu, in pairs %llu | pair candidates pruned %llu (both of a pair: %llu pairs) | single candidates pruned %llu | dropped by the final test %llu\n",
                        h[0], h[1], h[2], h[3], h[4], h[5]);
        }
    }
    delete d;      // every member releases what it owns, in reverse order of declaration (lm_detector_impl.h)
}

int lm_set_similarity_lut(lm_detector* d, const uint8_t lut[256]) {
    if (d && any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (!d || !lut) return fail(LM_ERR_INVALID, "null argument");
    for (int i = 0; i < 256; ++i) if (lut[i] > 4) return fail(LM_ERR_INVALID, "similarity LUT entries must be <= 4 (63*4 must fit a byte)");
    // an empty spread value must score 0: reads past a linear memory land in zero padding (upstream: undefined)
    for (int o = 0; o < 8; ++o) if (lut[32 * o] || lut[32 * o + 16]) return fail(LM_ERR_INVALID, "similarity LUT must map an empty nibble to 0");
    std::memcpy(d->sim_lut, lut, 256); d->luts_dirty = true;
    for (Slot& sl : d->slots) sl.prepared = false;
    return LM_OK;
}
int lm_set_normal_lut(lm_detector* d, const uint8_t lut[8000]) {
    if (d && any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (!d || !lut) return fail(LM_ERR_INVALID, "null argument");
    std::memcpy(d->normal_lut, lut, 8000); d->luts_dirty = true; d->lut_onehot = -1; d->normal_lut_substitute = false;
    for (Slot& sl : d->slots) sl.prepared = false;
    return LM_OK;
}
int lm_get_similarity_lut(const lm_detector* d, uint8_t lut[256]) { if (!d || !lut) return fail(LM_ERR_INVALID, "null argument"); std::memcpy(lut, d->sim_lut, 256); return LM_OK; }
int lm_normal_lut_is_substitute(const lm_detector* d) { return (d && d->normal_lut_substitute) ? 1 : 0; }
int lm_get_normal_lut(const lm_detector* d, uint8_t lut[8000]) { if (!d || !lut) return fail(LM_ERR_INVALID, "null argument"); std::memcpy(lut, d->normal_lut, 8000); return LM_OK; }

int lm_num_classes(const lm_detector* d) { return d ? (int)d->bank.classes.size() : -1; }
int lm_num_templates(const lm_detector* d) {
    if (!d) return -1;
    int n = 0;
    for (const auto& c : d->bank.classes) n += (int)c.pyramids.size();
    return n;
}
int lm_class_num_templates(const lm_detector* d, int ci) {
    if (!d || ci < 0 || ci >= (int)d->bank.classes.size()) return -1;
    return (int)d->bank.classes[ci].pyramids.size();
}
const char* lm_class_id(const lm_detector* d, int ci) {
    if (!d || ci < 0 || ci >= (int)d->bank.classes.size()) return nullptr;
    return d->bank.classes[ci].id.c_str();
}
int lm_find_class(const lm_detector* d, const char* id) { return (d && id) ? d->bank.find(id) : -1; }
int lm_get_T(const lm_detector* d, int level) { return (d && level >= 0 && level < d->cfg.pyramid_levels) ? d->cfg.T[level] : -1; }
int lm_num_modalities(const lm_detector* d) { return d ? d->cfg.num_modalities : -1; }
int lm_keeps_depth(const lm_detector* d) { return d ? (keeps_depth(d) ? 1 : 0) : -1; }
int lm_pyramid_levels(const lm_detector* d) { return d ? d->cfg.pyramid_levels : -1; }

int lm_add_class(lm_detector* d, const char* class_id, int n_templates, const lm_template_desc* descs,
                 const lm_feature* features, int* class_idx_out) {
    if (d && any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (!d || !class_id || n_templates < 0 || (n_templates && (!descs || !features))) return fail(LM_ERR_INVALID, "null argument");
    std::string err;
    int ci = d->bank.add_class(class_id, n_templates, descs, features, d->cfg.pyramid_levels, d->cfg.num_modalities, err);
    if (ci < 0) return fail(LM_ERR_INVALID, err);
    if (class_idx_out) *class_idx_out = ci;
    d->bank_dirty = true; d->hulls_dirty = true;
    return LM_OK;
}

int lm_add_template(lm_detector* d, const char* class_id, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth,
                    size_t depth_stride, const uint8_t* mask, size_t mask_stride, int* template_id_out, lm_rect* bbox_out) {
    if (d && any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (template_id_out) *template_id_out = -1;
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if (!class_id) return fail(LM_ERR_INVALID, "null class id");
    const lm_config& c = d->cfg;
    const int M = c.num_modalities, L = c.pyramid_levels;
    hipStream_t st = d->lanes[0].stream;
    if ((rc = upload_frame(d, 0, bgr, bgr_stride, depth, depth_stride, inline_on(st)))) return rc;
    d->slots[0].has_frame = false; d->slots[0].has_depth = false;  // slot 0 now holds a template image, not a scene frame
    d->slots[0].prepared = false;
    // quantise every level on the GPU, keeping the gradient magnitude this time
    size_t mag_off[LM_MAX_LEVELS], total = 0;
    for (int l = 0; l < L; ++l) { mag_off[l] = total; total += align_up((size_t)d->lw[l] * d->lh[l] * sizeof(float), 256); }
    if ((rc = ensure_scratch(d, total))) return rc;
    u8* scratch = static_cast<u8*>(d->d_scratch);
    float* mag[LM_MAX_LEVELS] = {};
    for (int l = 0; l < L; ++l) mag[l] = reinterpret_cast<float*>(scratch + mag_off[l]);
    enqueue_template_quantize(d, 0, 1, 0, mag);
    std::vector<lmh::ExtractLevel> lv(L);
    for (int l = 0; l < L; ++l) {
        size_t px = (size_t)d->lw[l] * d->lh[l];
        lv[l].w = d->lw[l]; lv[l].h = d->lh[l];
        lv[l].color_q.resize(px); lv[l].color_mag.resize(px);
        HIP_TRY(hipMemcpyAsync(lv[l].color_q.data(), d->quant(0, l, 0), px, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(lv[l].color_mag.data(), scratch + mag_off[l], px * sizeof(float), hipMemcpyDeviceToHost, st));
        if (M == 2) {
            lv[l].depth_q.resize(px);
            HIP_TRY(hipMemcpyAsync(lv[l].depth_q.data(), d->quant(0, l, 1), px, hipMemcpyDeviceToHost, st));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
    if (mask) {  // mask pyramid: resize(..., INTER_NEAREST) per level
        if (mask_stride == 0) mask_stride = (size_t)c.width;
        lv[0].mask.resize((size_t)c.width * c.height);
        for (int y = 0; y < c.height; ++y) std::memcpy(&lv[0].mask[(size_t)y * c.width], mask + y * mask_stride, (size_t)c.width);
        for (int l = 1; l < L; ++l) {
            lv[l].mask.resize((size_t)lv[l].w * lv[l].h);
            for (int y = 0; y < lv[l].h; ++y)
                for (int x = 0; x < lv[l].w; ++x) lv[l].mask[(size_t)y * lv[l].w + x] = lv[l - 1].mask[(size_t)(2 * y) * lv[l - 1].w + 2 * x];
        }
    }
    lmh::TemplatePyramid tp;
    if (!lmh::extract_pyramid(lv, c, tp)) return fail(LM_ERR_EXTRACT, "not enough features to build a template");
    lm_rect bb = lmh::crop_templates(tp);
    if (bbox_out) *bbox_out = bb;
    int tid = d->bank.add_pyramid(class_id, std::move(tp));
    if (template_id_out) *template_id_out = tid;
    d->bank_dirty = true; d->hulls_dirty = true;
    return LM_OK;
}

int lm_get_template(const lm_detector* d, int ci, int tid, int level, int modality, int* width, int* height,
                    lm_feature* features, int* num_features) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (ci < 0 || ci >= (int)d->bank.classes.size()) return fail(LM_ERR_INVALID, "class index out of range");
    const auto& c = d->bank.classes[ci];
    if (tid < 0 || tid >= (int)c.pyramids.size()) return fail(LM_ERR_INVALID, "template id out of range");
    if (level < 0 || level >= d->cfg.pyramid_levels || modality < 0 || modality >= d->cfg.num_modalities)
        return fail(LM_ERR_INVALID, "level/modality out of range");
    const lmh::Template& t = c.pyramids[tid][level * d->cfg.num_modalities + modality];
    if (width) *width = t.width;
    if (height) *height = t.height;
    if (num_features) *num_features = (int)t.features.size();
    if (features && !t.features.empty()) std::memcpy(features, t.features.data(), t.features.size() * sizeof(lm_feature));
    return LM_OK;
}

int lm_set_tuning(lm_detector* d, int key, int value) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    switch (key) {
        // the pre-processing kernels' knobs are process-wide (lmh::set_pre_knob validates and stores them)
        case LM_TUNE_CBLUR_VARIANT: case LM_TUNE_CGRAD_VARIANT: case LM_TUNE_PYRDOWN_VARIANT: case LM_TUNE_BLUR_PYR: case LM_TUNE_BLUR_STRIP:
        case LM_TUNE_DMEDIAN_VARIANT: case LM_TUNE_CGRAD_LEVELS:
            if (!lmh::set_pre_knob(key, value)) break;
            return LM_OK;
        case LM_TUNE_PHASE_MAX_SLOTS: if (value < 0) break; d->phase_max_slots = value; return LM_OK;
        case LM_TUNE_COPY_STREAMS: if (value < 1 || value > LM_NCOPY) break; d->n_copy_streams = value; return LM_OK;
        case LM_TUNE_BATCH_PHASES: if (value < 0 || value > 2) break; d->batch_phases = value; return LM_OK;
        case LM_TUNE_WORK_WEIGHT: if (value < 0 || value > 1) break; d->work_weight_by_pixels = value; return LM_OK;
        case LM_TUNE_SORT_SPLIT: if (value < 0 || value > 2) break; d->sort_split_mode = value; return LM_OK;
        case LM_TUNE_SCAN_LIST_ORDER: if (value < 0 || value > 3) break; d->scan_list_order = value; d->bank_dirty = true; return LM_OK;
        case LM_TUNE_SCAN_FORM:
            if (value < 0 || value > 3) break;
            if (any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
            d->scan_form = value;
            for (Slot& sl : d->slots) sl.prepared = false;          // (prepared slots may lack the miss planes the new form reads)
            return LM_OK;
        case LM_TUNE_RECTIFY_REDUCE_GRID: if (value < 0 || value > 1) break; d->rectify_reduce_grid = value; return LM_OK;
        case LM_TUNE_ICP_BATCH_MB: if (value < 1 || value > 4096) break; d->icp_batch_mb = value; return LM_OK;
        case LM_TUNE_SCAN1_MIN_THRESHOLD: if (value < 0 || value > 100) break; d->scan1_min_threshold = (float)value; return LM_OK;
        case LM_TUNE_SURVIVOR_QUEUE:
            if (value < 64 || value > (1 << 24)) break;
            if (d->dev_ready) {       // no lane is busy (checked above); the queues' re-arming stores ran inside the matches that have ended
                HIP_TRY(hipSetDevice(d->cfg.device));
                HIP_TRY(hipDeviceSynchronize());
                for (lm_detector::Lane& ln : d->lanes) { ln.d_surv.reset(); ln.surv_set = 0; }
            }
            d->surv_cap = ((u32)value + 7u) & ~7u;
            return LM_OK;
        default: return fail(LM_ERR_INVALID, "unknown tuning key");
    }
    return fail(LM_ERR_INVALID, "tuning value out of range");
}

int lm_match_slot(lm_detector* d, int slot, float threshold, int class_idx, lm_match_t* out, size_t cap, size_t* n_out) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, slot, 1))) return rc;
    if ((rc = ensure_bank(d))) return rc;
    if ((rc = run_match(d, d->lanes[0], slot, 1, threshold, class_idx))) return rc;
    return collect_slot(d, slot, out, cap, n_out);
}

static int match_host_frame(lm_detector* d, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                            float threshold, std::vector<int> classes, lm_match_t* out, size_t cap, size_t* n_out,
                            const uint8_t* color_mask = nullptr, size_t color_mask_stride = 0, const uint8_t* depth_mask = nullptr,
                            size_t depth_mask_stride = 0) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = ensure_bank(d))) return rc;
    if (any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    lm_detector::Lane& l0 = d->lanes[0];       // a host frame names no lane: the detector's own
    const bool depth_used = keeps_depth(d) && depth;      // (the depth image goes into slot 0: it is a modality, or the detector keeps it)
    if (depth_optional(d) && (rc = refuse_depthless_rules(d, 0, 1, depth_used))) return rc;
    if (color_mask || depth_mask) {
        if (depth_mask && d->cfg.num_modalities < 2) return fail(LM_ERR_INVALID, "depth mask given to a colour-only detector");
        // the masks' copies go inline too, from slot 0's own staging buffer; whatever fails, nothing of this call stays in flight
        if ((rc = upload_frame(d, 0, bgr, bgr_stride, depth, depth_stride, inline_on(l0.stream))) ||
            (color_mask && (rc = upload_match_mask(d, 0, 0, color_mask, color_mask_stride, l0.stream))) ||
            (depth_mask && (rc = upload_match_mask(d, 0, 1, depth_mask, depth_mask_stride, l0.stream))) ||
            (rc = run_match(d, l0, 0, 1, threshold, std::move(classes)))) {
            (void)hipStreamSynchronize(l0.stream);
            return rc;
        }
        return collect_slot(d, 0, out, cap, n_out);
    }
    // the copies go inline on the compute stream, in order with the kernels (r02 measured the copy-stream forms -- one stream with split
    // events, pieces over all copy streams -- slower for one frame: 133 -> 167 us; they were deleted in r05).  Frames that already live
    // in pinned host memory (lm_host_alloc, hipHostMalloc, hipHostRegister) skip the staging copy
    const size_t hh = (size_t)d->cfg.height;
    const bool pinned = bgr && is_pinned_host(bgr, (bgr_stride ? bgr_stride : (size_t)d->cfg.width * 3) * hh) &&
                        (depth_used ? is_pinned_host(depth, (depth_stride ? depth_stride : (size_t)d->cfg.width * 2) * hh) : d->cfg.num_modalities < 2);
    if ((rc = upload_frame(d, 0, bgr, bgr_stride, depth, depth_stride, inline_on(l0.stream, pinned)))) return rc;
    if ((rc = run_match(d, l0, 0, 1, threshold, std::move(classes)))) return rc;
    return collect_slot(d, 0, out, cap, n_out);
}

int lm_match(lm_detector* d, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
             float threshold, int class_idx, lm_match_t* out, size_t cap, size_t* n_out) {
    return match_host_frame(d, bgr, bgr_stride, depth, depth_stride, threshold, std::vector<int>(1, class_idx), out, cap, n_out);
}

int lm_match_masked(lm_detector* d, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                    const uint8_t* color_mask, size_t color_mask_stride, const uint8_t* depth_mask, size_t depth_mask_stride,
                    float threshold, int class_idx, lm_match_t* out, size_t cap, size_t* n_out) {
    return match_host_frame(d, bgr, bgr_stride, depth, depth_stride, threshold, std::vector<int>(1, class_idx), out, cap, n_out,
                            color_mask, color_mask_stride, depth_mask, depth_mask_stride);
}

int lm_set_mask_rule(lm_detector* d, int first_slot, int n_slots, const lm_mask_rule* rule) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    LmRule dev{};
    if (rule && (rc = check_mask_rule(d, rule, &dev))) return rc;
    if ((rc = claim_slots(d, first_slot, n_slots))) return rc;
    if (rule && rule->use_hsv && (rc = ensure_hsv_div(d))) return rc;
    const size_t plane = d->match_mask_pitch * (size_t)d->cfg.height;
    if (rule)
        for (int i = first_slot; i < first_slot + n_slots; ++i)     // (k_mask_rule writes every byte of the plane: nothing to clear)
            if (!d->slots[i].d_rule_mask) HIP_TRY(d->slots[i].d_rule_mask.alloc(plane));
    for (int i = first_slot; i < first_slot + n_slots; ++i) {
        Slot& s = d->slots[i];
        s.rule_on = rule != nullptr;
        if (rule) { s.rule = *rule; s.rule_dev = dev; }
        s.prepared = false; s.matched = false;      // (the slot's last lists belong to the old rule: lm_match_collect refuses them)
    }
    return LM_OK;
}

int lm_get_mask_rule(const lm_detector* d, int slot, lm_mask_rule* out, int* is_set) {
    if (!d || !is_set) return fail(LM_ERR_INVALID, "null argument");
    if (slot < 0 || slot >= d->cfg.frame_slots) return fail(LM_ERR_INVALID, "slot out of range");
    const bool on = (size_t)slot < d->slots.size() && d->slots[(size_t)slot].rule_on;     // (no device yet: no rule was set)
    *is_set = on ? 1 : 0;
    if (on && out) *out = d->slots[(size_t)slot].rule;
    return LM_OK;
}

int lm_match_classes(lm_detector* d, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                     float threshold, const int32_t* class_idxs, int n_classes, lm_match_t* out, size_t cap, size_t* n_out) {
    if (n_classes < 0 || (n_classes && !class_idxs)) return fail(LM_ERR_INVALID, "bad class list");
    return match_host_frame(d, bgr, bgr_stride, depth, depth_stride, threshold, std::vector<int>(class_idxs, class_idxs + n_classes), out, cap, n_out);
}

// the lists of slots [first, first + n), one after the other; the first error wins, every count is delivered
static int collect_range(lm_detector* d, int first, int n, lm_match_t* out, size_t cap_per_frame, int32_t* counts) {
    int first_err = LM_OK;
    std::string first_msg;
    for (int i = 0; i < n; ++i) {
        size_t k = 0;
        int rc = collect_slot(d, first + i, out ? out + (size_t)i * cap_per_frame : nullptr, cap_per_frame, &k);
        if (counts) counts[i] = (int32_t)k;
        if (rc && !first_err) { first_err = rc; first_msg = g_err; }
    }
    if (first_err) return fail(first_err, first_msg);
    return LM_OK;
}

int lm_match_batch(lm_detector* d, int n_slots, float threshold, int class_idx, lm_match_t* out, size_t cap_per_frame,
                   int32_t* counts) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = ensure_bank(d))) return rc;
    if ((rc = check_slots(d, 0, n_slots))) return rc;
    if (n_slots == 0) return LM_OK;
    if ((rc = run_match(d, d->lanes[0], 0, n_slots, threshold, class_idx))) return rc;
    return collect_range(d, 0, n_slots, out, cap_per_frame, counts);
}

// Detector::match(sources, threshold, matches, class_ids) with upstream's class LIST: a3-a10 once per frame, one
// scan launch per run of neighbouring classes, one refinement, one sort; the lists hold the matches of all the named
// classes in the total order (HighLevelLinemod.cpp:145,152).
int lm_match_batch_classes(lm_detector* d, int first_slot, int n_slots, float threshold, const int32_t* class_idxs, int n_classes,
                           lm_match_t* out, size_t cap_per_frame, int32_t* counts) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = ensure_bank(d))) return rc;
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    if (n_classes < 0 || (n_classes && !class_idxs)) return fail(LM_ERR_INVALID, "bad class list");
    if (n_slots == 0) return LM_OK;
    if ((rc = run_match(d, d->lanes[0], first_slot, n_slots, threshold, std::vector<int>(class_idxs, class_idxs + n_classes)))) return rc;
    return collect_range(d, first_slot, n_slots, out, cap_per_frame, counts);
}

// a11-a15 only, on slots whose a3-a10 results are current (a match or lm_prepare_slot has run on the frame the slot
// holds, no upload and no LUT change since): the reference's per-class detect calls on ONE camera frame
// (PoseDetection.cpp:45-66 per class name) pay the pre-processing once.
int lm_match_prepared(lm_detector* d, int first_slot, int n_slots, float threshold, const int32_t* class_idxs, int n_classes,
                      lm_match_t* out, size_t cap_per_frame, int32_t* counts) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = ensure_bank(d))) return rc;
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    if (n_classes < 0 || (n_classes && !class_idxs)) return fail(LM_ERR_INVALID, "bad class list");
    if (n_slots == 0) return LM_OK;
    if ((rc = run_match(d, d->lanes[0], first_slot, n_slots, threshold, std::vector<int>(class_idxs, class_idxs + n_classes), true))) return rc;
    return collect_range(d, first_slot, n_slots, out, cap_per_frame, counts);
}

int lm_synchronize(lm_detector* d) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return LM_OK;
}


static int begin_lane(lm_detector* d, int lane, int first_slot, int n_slots, float threshold, std::vector<int> classes, bool gathered) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if (lane < 0 || lane >= LM_NLANES) return fail(LM_ERR_INVALID, "lane out of range (0 .. 3)");
    if (gathered && !d->lanes[0].comm) return fail(LM_ERR_INVALID, "no communicator: call lm_comm_init first");
    if ((rc = ensure_bank(d))) return rc;
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    if (n_slots <= 0) return fail(LM_ERR_INVALID, "no slots");
    lm_detector::Lane& ln = d->lanes[lane];
    if (ln.busy) return fail(LM_ERR_INVALID, "lane is busy: call lm_match_end first");
    if (lane_holds_slots(d, first_slot, n_slots))      // (this lane is idle: a lane that holds them is another one)
        return fail(LM_ERR_INVALID, "slot range overlaps the range another lane is working on");
    for (int i = 0; i < n_slots; ++i)
        if (!d->slots[first_slot + i].has_frame) return fail(LM_ERR_INVALID, "no frame uploaded to slot " + std::to_string(first_slot + i));
    if ((rc = ensure_lane(d, lane))) return rc;
    if ((rc = enqueue_match(d, ln, first_slot, n_slots, threshold, classes, d->profiling))) return rc;
    if (gathered && (rc = enqueue_gather(d, ln, first_slot, n_slots))) return rc;
    if (!ln.ev_done && ln.ev_done.create(((d->cfg.flags & LM_FLAG_BLOCKING_SYNC) ? hipEventBlockingSync : 0) | hipEventDisableTiming) != hipSuccess)
        rc = fail(LM_ERR_HIP, "creating the lane's completion event failed");
    if (!rc && hipEventRecord(ln.ev_done, ln.stream) != hipSuccess) rc = fail(LM_ERR_HIP, "hipEventRecord failed");
    if (rc) {
        (void)hipStreamSynchronize(ln.stream);      // what was enqueued must not outlive the failed call
        return rc;
    }
    ln.busy = true; ln.first = first_slot; ln.n = n_slots; ln.classes = classes; ln.timed = d->profiling;
    ln.gather.active = gathered;
    return LM_OK;
}

int lm_match_begin(lm_detector* d, int lane, int first_slot, int n_slots, float threshold, int class_idx) {
    return begin_lane(d, lane, first_slot, n_slots, threshold, std::vector<int>(1, class_idx), false);
}

int lm_match_begin_classes(lm_detector* d, int lane, int first_slot, int n_slots, float threshold, const int32_t* class_idxs,
                           int n_classes) {
    if (n_classes < 0 || (n_classes && !class_idxs)) return fail(LM_ERR_INVALID, "bad class list");
    return begin_lane(d, lane, first_slot, n_slots, threshold, std::vector<int>(class_idxs, class_idxs + n_classes), false);
}

int lm_match_begin_gathered(lm_detector* d, int lane, int first_slot, int n_slots, float threshold, int class_idx) {
    return begin_lane(d, lane, first_slot, n_slots, threshold, std::vector<int>(1, class_idx), true);
}

int lm_match_end(lm_detector* d, int lane, lm_match_t* out, size_t cap_per_frame, int32_t* counts) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (lane < 0 || lane >= LM_NLANES) return fail(LM_ERR_INVALID, "lane out of range (0 .. 3)");
    lm_detector::Lane& ln = d->lanes[lane];
    if (!ln.busy) return fail(LM_ERR_INVALID, "lane has no match in flight");
    if (ln.gather.active) return fail(LM_ERR_INVALID, "the lane's match was begun with lm_match_begin_gathered: collect it with lm_match_end_gathered");
    HIP_TRY(hipSetDevice(d->cfg.device));
    const int wrc = wait_lane_done(d, ln);
    if (!wrc && ln.timed) account_profile(d, ln, ln.n, ln.classes);
    ln.busy = false;
    if (wrc) return wrc;
    for (int i = 0; i < ln.n; ++i) d->slots[ln.first + i].matched = true;
    return collect_range(d, ln.first, ln.n, out, cap_per_frame, counts);
}

// The lists of the last completed match on slots [first_slot, first_slot + n_slots) once more (they stay in the slots' result blocks
// until the next upload or match): what a caller does after LM_ERR_OVERFLOW told it the capacity it needs -- no second pass over the GPU.
int lm_match_collect(lm_detector* d, int first_slot, int n_slots, lm_match_t* out, size_t cap_per_frame, int32_t* counts) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    if (lane_holds_slots(d, first_slot, n_slots)) return fail(LM_ERR_INVALID, "slot belongs to a match in flight");
    for (int i = 0; i < n_slots; ++i)
        if (!d->slots[first_slot + i].matched) return fail(LM_ERR_INVALID, "slot " + std::to_string(first_slot + i) + " holds no completed match");
    return collect_range(d, first_slot, n_slots, out, cap_per_frame, counts);
}

}  // extern "C"
