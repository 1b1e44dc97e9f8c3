// lm_detector_ingest.hip -- frames whose source already lies in device memory in the producer's format, into the resident slots: one stage's
// launch under one upload ticket.  The five lm_ingest_frames* are ingest_frames with a route: the stage the images go through -- k_ingest
// (lm_ingest_frames), k_rectify (lm_ingest_frames_rectified, lm_set_rectification), k_reduce (lm_ingest_frames_reduced, lm_set_reduction:
// host state alone) or k_rectify_reduce (lm_ingest_frames_rectified_reduced: the map in front of the box) in its
// place -- and whether the raw depth image is registered onto the colour camera behind it (lm_ingest_frames_registered, the rectified
// routes' depth_route; lm_k_register.hip, lm_set_registration).  One geometry function (geometry_of), one argument struct filled in one
// place (fill_ingest_args, launch_stage), one body for the stages' hooks (stage_hook); beside them the setters, the raw pipeline of the raw
// colour formats (lm_set_raw_processing: host state and its device copy, read by the *_raw kernels) and lm_stage_register_depth.  It is an
// upload and follows lm_detector_upload.hip's rule: check the arguments (the descriptors: lm_ingest_check.h, host code of its own), claim
// the slots, only then touch a slot or the device, end with the ticket.
#include "lm_detector_impl.h"

namespace lmd {

// What a call does with a frame's images: the stage they go through -- k_ingest, or k_rectify / k_reduce / k_rectify_reduce in its place --
// and whether `depth` holds the RAW depth images, to be registered onto the colour camera behind that stage (which then takes the colour
// images alone).  "No depth this call" is not the route's: lmc::check_depth_call.
enum Stage { PLAIN, RECTIFY, REDUCE, RECTIFY_REDUCE };
struct Route { Stage stage; bool reg; };
static bool mapped(Stage s) { return s == RECTIFY || s == RECTIFY_REDUCE; }
static bool boxed(Stage s) { return s == REDUCE || s == RECTIFY_REDUCE; }

static int ensure_ingest(lm_detector* d) {
    if (!d->h_ingest) HIP_TRY(d->h_ingest.alloc(d->slots.size()));
    if (!d->d_ingest) HIP_TRY(d->d_ingest.alloc(d->slots.size()));
    if (!d->ev_ingest_src) HIP_TRY(d->ev_ingest_src.create(hipEventDisableTiming));
    return LM_OK;
}

// A host table (the registration's rays, the rectification's map) on the device, if the device does not hold it yet
template <class T>
static int ensure_table(const std::vector<T>& host, DevBuf<T>& dev, bool& dirty) {
    if (!dirty) return LM_OK;
    HIP_TRY(hipDeviceSynchronize());        // (nothing in flight reads the table that is replaced)
    HIP_TRY(dev.alloc(host.size()));
    HIP_TRY(hipMemcpy(dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    dirty = false;
    return LM_OK;
}

static int check(const lmc::Geometry& g, const lm_image_desc& im, int i, const lm_ingest_opts& o, LmIngestImage* out, int* matrix) {
    const std::string refusal = lmc::check_image(g, im, i, o, out, matrix);
    return refusal.empty() ? LM_OK : fail(LM_ERR_INVALID, refusal);
}

static void fill_register_args(const lm_detector* d, LmRegisterArgs* a) {
    const lm_registration_desc& r = d->reg;
    for (int k = 0; k < 9; ++k) a->rig.r[k] = r.rotation[k];
    for (int k = 0; k < 3; ++k) a->rig.t[k] = r.translation[k];
    const lm_camera& cc = r.colour;
    a->rig.fx = cc.fx; a->rig.fy = cc.fy; a->rig.cx = cc.cx; a->rig.cy = cc.cy;
    a->rig.k1 = cc.k1; a->rig.k2 = cc.k2; a->rig.p1 = cc.p1; a->rig.p2 = cc.p2; a->rig.k3 = cc.k3;
    a->splat_x = r.splat_x; a->splat_y = r.splat_y;
    a->dw = r.depth.width; a->dh = r.depth.height;
    a->rays = d->d_reg_rays;
}

static lmx::Ratio ratio_of(const lm_reduction_desc& r, int bit) {
    return (r.apply & bit) ? lmx::Ratio{r.num_x, r.den_x, r.num_y, r.den_y} : lmx::Ratio{1, 1, 1, 1};
}

// The geometry an image of a stage is checked against: an ingest's (a window) or a stage hook's (whole: the image itself)
static lmc::Geometry geometry_of(const lm_detector* d, Stage stage, lmc::Role role, bool whole) {
    switch (stage) {
    case RECTIFY: return lmc::rectified(d->cfg, d->rect, role, whole);
    case REDUCE: return lmc::reduced(d->cfg, d->red, role, whole);
    case RECTIFY_REDUCE: return lmc::rectified_reduced(d->cfg, d->rect, d->red, role, whole);
    default: return lmc::plain(d->cfg, role);
    }
}

// What every stage's kernels are told: the table, the frames, their size and families, the planes (null: not written).  After the raw
// pipeline's ensure_table, where a frame needs it.
static LmIngestArgs fill_ingest_args(const lm_detector* d, const LmIngestDesc* table, int first, int n, int w, int h, const int (&n_family)[LM_INGEST_FAMILIES], u8* out_bgr,
                                     u8* out_depth, size_t out_stride) {
    LmIngestArgs a = LmIngestArgs();
    a.table = table; a.first = first; a.n = n; a.w = w; a.h = h;
    for (int f = 0; f < LM_INGEST_FAMILIES; ++f) a.n_family[f] = n_family[f];
    a.raw = n_family[LM_INGEST_FAMILY_RAW] > 0 ? d->d_raw.get() : nullptr;
    a.out_bgr = out_bgr; a.out_depth = out_depth; a.out_stride = out_stride;
    return a;
}

// A stage's own arguments -- the map and both cameras' sizes, the ratios and the depth rule, the grid order -- and its launch
static void launch_stage(const lm_detector* d, hipStream_t st, Stage stage, LmIngestArgs a) {
    if (mapped(stage)) {
        a.map = d->d_rect_map;
        a.mw = d->rect.ideal.width; a.mh = d->rect.ideal.height; a.sw = d->rect.source.width; a.sh = d->rect.source.height;
    }
    if (boxed(stage)) {
        a.colour = ratio_of(d->red, LM_REDUCE_COLOUR); a.depth = ratio_of(d->red, LM_REDUCE_DEPTH); a.depth_rule = d->red.depth_rule;
    }
    a.frame_fast = d->rectify_reduce_grid;
    switch (stage) {
    case RECTIFY: lmk_rectify(st, a); break;
    case REDUCE: lmk_reduce(st, a); break;
    case RECTIFY_REDUCE: lmk_rectify_reduce(st, a); break;
    default: lmk_ingest(st, a); break;
    }
}

// The five lm_ingest_frames*.  The colour images go through the route's stage, and so do the depth images unless they are the RAW ones
// (route.reg): then the stage's kernels take the colour images alone and the depth planes are k_register_resolve's, behind them on the
// same stream and under the same ticket -- with RECTIFY / RECTIFY_REDUCE beside it the raw depth image lands on the slot's camera directly.
// REDUCE / RECTIFY_REDUCE: each image with the reduction's ratio or, its apply bit clear, with 1 / 1 (the plain / the rectified rule
// alone).  Everything else of the call is the same.
static int ingest_frames(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth, const lm_ingest_opts* opts,
                         void* producer_stream, Route route) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    const lm_config& c = d->cfg;
    const Stage stage = route.stage;
    const bool reg = route.reg;
    bool takes_depth = false;
    const std::string depth_refusal = lmc::check_depth_call(c, reg, depth != nullptr, &takes_depth);
    const bool reads_depth = takes_depth || reg;        // the call reads `depth` and writes the slots' depth planes
    if (mapped(stage) && !d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    if (!depth_refusal.empty()) return fail(LM_ERR_INVALID, depth_refusal);
    if (reg && !d->reg_on) return fail(LM_ERR_INVALID, "no registration set: lm_set_registration first");
    if (!colour || (lmc::depth_required(c, reg) && !depth) || n_slots <= 0) return fail(LM_ERR_INVALID, "bad argument");
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    if (c.width % 16) return fail(LM_ERR_INVALID, "lm_ingest_frames needs a frame width that is a multiple of 16");
    if (mapped(stage) && reg) {
        // the colour image's geometry in this route: the ideal one, or the reduced ideal one where the reduction applies to the colour image
        const bool red = stage == RECTIFY_REDUCE && (d->red.apply & LM_REDUCE_COLOUR);
        const lmx::Ratio q = red ? ratio_of(d->red, LM_REDUCE_COLOUR) : lmx::Ratio{1, 1, 1, 1};
        const int gw = lmx::reduced_size(d->rect.ideal.width, q.num_x, q.den_x), gh = lmx::reduced_size(d->rect.ideal.height, q.num_y, q.den_y);
        if (d->reg.colour.width != gw || d->reg.colour.height != gh)
            return fail(LM_ERR_INVALID, "rectification: the registration's colour camera (" + std::to_string(d->reg.colour.width) + " x " + std::to_string(d->reg.colour.height) +
                        ") is not the " + (red ? "reduced ideal geometry (" : "ideal camera (") + std::to_string(gw) + " x " + std::to_string(gh) + ")");
    }
    const lmc::Geometry gc = geometry_of(d, stage, lmc::COLOUR, false);
    const lmc::Geometry gd = reg ? lmc::raw_depth(c, d->reg, false) : geometry_of(d, stage, lmc::DEPTH, false);
    // the descriptors, checked into a table of the call's own: the detector's pinned table is written only once the slots are claimed and
    // their earlier uploads have landed
    static thread_local std::vector<LmIngestDesc> table;
    table.resize((size_t)n_slots);
    int n_family[LM_INGEST_FAMILIES] = {0, 0, 0, 0, 0};     // frames per lm_ingest_family of their colour image
    for (int i = 0; i < n_slots; ++i) {
        LmIngestDesc& e = table[(size_t)i];
        e = LmIngestDesc();
        lm_ingest_opts o = opts ? opts[i] : lm_ingest_opts{0, 0, 0};
        o.flip_x = o.flip_x != 0;
        o.shift_x = lmh::clamp_shift(o.shift_x, c.width); o.shift_y = lmh::clamp_shift(o.shift_y, c.height);     // (beyond: an all-zero frame either way)
        e.flip_x = o.flip_x; e.shift_x = o.shift_x; e.shift_y = o.shift_y;
        if ((rc = check(gc, colour[i], i, o, &e.colour, &e.matrix))) return rc;
        if (d->raw_on) lmc::process_bayer8(&e.colour);
        if (reads_depth && (rc = check(gd, depth[i], i, o, &e.depth, nullptr))) return rc;
        ++n_family[lm_ingest_family(e.colour.kind)];
    }
    if ((rc = claim_slots(d, first_slot, n_slots))) return rc;
    for (int i = 0; i < n_slots; ++i) if ((rc = wait_slot_upload(d, d->slots[first_slot + i]))) return rc;
    if ((rc = ensure_ingest(d))) return rc;
    std::memcpy(d->h_ingest + first_slot, table.data(), (size_t)n_slots * sizeof(LmIngestDesc));
    const int cs = (first_slot / n_slots) % d->n_copy_streams;   // as lm_upload_frames_pinned: consecutive runs take turns on the copy streams
    hipStream_t st = d->copy_stream[cs];
    const size_t z_words = (size_t)n_slots * (size_t)c.width * (size_t)c.height;
    if (mapped(stage) && (rc = ensure_table(d->rect_map, d->d_rect_map, d->rect_map_dirty))) return rc;
    if (n_family[LM_INGEST_FAMILY_RAW] > 0 && (rc = ensure_table(d->raw, d->d_raw, d->raw_dirty))) return rc;
    if (reg) {
        if ((rc = ensure_table(d->reg_rays, d->d_reg_rays, d->reg_rays_dirty))) return rc;
        if (d->d_reg_z[cs].size() < z_words) {
            HIP_TRY(hipStreamSynchronize(st));      // the stream's earlier calls are done with the buffer that is released
            HIP_TRY(d->d_reg_z[cs].grow(z_words));
        }
    }
    if (producer_stream) {
        HIP_TRY(hipEventRecord(d->ev_ingest_src, static_cast<hipStream_t>(producer_stream)));
        HIP_TRY(hipStreamWaitEvent(st, d->ev_ingest_src, 0));
    }
    HIP_TRY(hipMemcpyAsync(d->d_ingest + first_slot, d->h_ingest + first_slot, (size_t)n_slots * sizeof(LmIngestDesc), hipMemcpyHostToDevice, st));
    // (the stage's kernels write the depth planes too, unless the registration does)
    launch_stage(d, st, stage, fill_ingest_args(d, d->d_ingest, first_slot, n_slots, c.width, c.height, n_family, d->frame_arena + d->off_bgr[0],
                                                takes_depth && !reg ? d->frame_arena + d->off_depth : nullptr, d->frame_stride));
    HIP_TRY(hipGetLastError());
    if (reg) {
        LmRegisterArgs r;
        fill_register_args(d, &r);
        r.table = d->d_ingest; r.first = first_slot; r.n = n_slots; r.w = c.width; r.h = c.height;
        r.zbuf = d->d_reg_z[cs]; r.out = d->frame_arena + d->off_depth; r.out_stride = d->frame_stride;
        HIP_TRY(hipMemsetAsync(r.zbuf, 0xFF, z_words * sizeof(u32), st));      // re-armed on the ingest's own stream, behind the last call's resolve
        lmk_register(st, r);
        HIP_TRY(hipGetLastError());
    }
    return issue_run_ticket(d, first_slot, n_slots, cs, false, reads_depth);      // one ticket for the whole launch
}

// The one descriptor of a stage hook on the device, landed (`e` is the caller's local)
static int put_desc(hipStream_t st, const LmIngestDesc& e, DevBuf<LmIngestDesc>& d_e) {
    HIP_TRY(d_e.alloc(1));
    HIP_TRY(hipMemcpyAsync(d_e, &e, sizeof(e), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LM_OK;
}

// The stage hooks' shared body: one whole image of each kind given through the stage alone (no window, no mirror, no shift), back to the
// host.  A pair (image, output) may be absent, not half of one.  Each image has an output size of its own -- the ideal camera's, its
// own reduced size, the reduced ideal one -- and so a launch of its own.
static int stage_hook(lm_detector* d, Stage stage, const lm_image_desc* colour, const lm_image_desc* depth, uint8_t* bgr_out_host, uint16_t* depth_out_host) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    const bool do_c = colour && bgr_out_host, do_d = depth && depth_out_host;
    if ((!do_c && !do_d) || (colour != nullptr) != (bgr_out_host != nullptr) || (depth != nullptr) != (depth_out_host != nullptr))
        return fail(LM_ERR_INVALID, "bad argument");
    if (mapped(stage) && !d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    LmIngestDesc e = LmIngestDesc();
    const lm_ingest_opts o = {0, 0, 0};
    if (do_c && (rc = check(geometry_of(d, stage, lmc::COLOUR, true), *colour, 0, o, &e.colour, &e.matrix))) return rc;
    if (do_c && d->raw_on) lmc::process_bayer8(&e.colour);
    if (do_d && (rc = check(geometry_of(d, stage, lmc::DEPTH, true), *depth, 0, o, &e.depth, nullptr))) return rc;
    if (mapped(stage) && (rc = ensure_table(d->rect_map, d->d_rect_map, d->rect_map_dirty))) return rc;
    int n_family[LM_INGEST_FAMILIES] = {0, 0, 0, 0, 0};
    n_family[lm_ingest_family(e.colour.kind)] = 1;      // (the kernel that owns the entry; a depth-only call: the RGB family's)
    if (n_family[LM_INGEST_FAMILY_RAW] && (rc = ensure_table(d->raw, d->d_raw, d->raw_dirty))) return rc;
    hipStream_t st = d->copy_stream[0];
    DevBuf<LmIngestDesc> d_e;
    if ((rc = put_desc(st, e, d_e))) return rc;
    for (int depth_turn = 0; depth_turn < 2; ++depth_turn) {
        const lm_image_desc* im = depth_turn ? depth : colour;
        if (!(depth_turn ? do_d : do_c)) continue;
        const lmx::Ratio q = boxed(stage) ? ratio_of(d->red, depth_turn ? LM_REDUCE_DEPTH : LM_REDUCE_COLOUR) : lmx::Ratio{1, 1, 1, 1};
        const int w = lmx::reduced_size(mapped(stage) ? d->rect.ideal.width : im->width, q.num_x, q.den_x);
        const int h = lmx::reduced_size(mapped(stage) ? d->rect.ideal.height : im->height, q.num_y, q.den_y);
        const size_t bytes = (size_t)w * (size_t)h * (depth_turn ? sizeof(u16) : 3);
        if (!bytes) continue;
        DevBuf<u8> d_out;
        HIP_TRY(d_out.alloc(bytes));
        launch_stage(d, st, stage, fill_ingest_args(d, d_e, 0, 1, w, h, n_family, depth_turn ? nullptr : d_out.get(), depth_turn ? d_out.get() : nullptr, 0));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(depth_turn ? (void*)depth_out_host : (void*)bgr_out_host, d_out, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));      // (d_out is released at the end of the turn)
    }
    return LM_OK;
}

static bool camera_finite(const lm_camera& k) {
    for (float v : {k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, k.k3}) if (!std::isfinite(v)) return false;
    return true;
}

// What both setters ask of their two cameras.  finite_words: the setter's own sentence; others_finite: its numbers outside the cameras.
static int check_cameras(const std::string& prefix, const char* finite_words, bool others_finite, const lm_camera& a, const lm_camera& b) {
    if (!(camera_finite(a) && camera_finite(b) && others_finite)) return fail(LM_ERR_INVALID, prefix + finite_words);
    if (!(a.fx > 0.0f && a.fy > 0.0f && b.fx > 0.0f && b.fy > 0.0f)) return fail(LM_ERR_INVALID, prefix + "fx and fy of both cameras must be positive");
    for (int v : {a.width, a.height, b.width, b.height})
        if (v < 1 || v > 16384) return fail(LM_ERR_INVALID, prefix + "width and height of both cameras must lie in 1 .. 16384");
    return LM_OK;
}

// Before a setter swaps its host table: no lane in flight, and no ingest on a copy stream that may still read the table that is replaced
static int quiesce_for_set(lm_detector* d, const char* prefix) {
    if (any_lane_busy(d)) return fail(LM_ERR_INVALID, std::string(prefix) + "a lane has a match in flight: call lm_match_end first");
    if (!d->dev_ready) return LM_OK;
    if (int rc = ensure_device(d)) return rc;
    return lm_upload_wait(d, -1);
}

}  // namespace lmd

extern "C" {

int lm_ingest_frames(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth, const lm_ingest_opts* opts,
                     void* producer_stream) {
    return ingest_frames(d, first_slot, n_slots, colour, depth, opts, producer_stream, {PLAIN, false});
}

int lm_ingest_frames_registered(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth_raw,
                                const lm_ingest_opts* opts, void* producer_stream) {
    return ingest_frames(d, first_slot, n_slots, colour, depth_raw, opts, producer_stream, {PLAIN, true});
}

int lm_ingest_frames_rectified(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                               const lm_ingest_opts* opts, int depth_route, void* producer_stream) {
    if (depth_route != LM_RECTIFY_DEPTH_ALIGNED && depth_route != LM_RECTIFY_DEPTH_REGISTERED) {
        int rc;
        if ((rc = ready_for_compute(d))) return rc;
        return fail(LM_ERR_INVALID, "rectification: unknown depth_route " + std::to_string(depth_route));
    }
    return ingest_frames(d, first_slot, n_slots, colour, depth, opts, producer_stream,
                         {RECTIFY, depth_route == LM_RECTIFY_DEPTH_REGISTERED});
}

int lm_ingest_frames_reduced(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                             const lm_ingest_opts* opts, void* producer_stream) {
    // (host state: refused with or without a device)
    if (d && !d->red_on) return fail(LM_ERR_INVALID, "reduction: no reduction set: lm_set_reduction first");
    return ingest_frames(d, first_slot, n_slots, colour, depth, opts, producer_stream, {REDUCE, false});
}

int lm_ingest_frames_rectified_reduced(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                                       const lm_ingest_opts* opts, int depth_route, void* producer_stream) {
    // (host state: refused with or without a device)
    if (d && !d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    if (d && !d->red_on) return fail(LM_ERR_INVALID, "reduction: no reduction set: lm_set_reduction first");
    if (d && depth_route != LM_RECTIFY_DEPTH_ALIGNED && depth_route != LM_RECTIFY_DEPTH_REGISTERED)
        return fail(LM_ERR_INVALID, "rectification: unknown depth_route " + std::to_string(depth_route));
    return ingest_frames(d, first_slot, n_slots, colour, depth, opts, producer_stream,
                         {RECTIFY_REDUCE, depth_route == LM_RECTIFY_DEPTH_REGISTERED});
}

int lm_ingest_release(lm_detector* d, int first_slot, int n_slots, void* stream) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if (n_slots <= 0) return fail(LM_ERR_INVALID, "bad argument");
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    return wait_uploads(d, static_cast<hipStream_t>(stream), first_slot, n_slots, nullptr);
}

int lm_set_registration(lm_detector* d, const lm_registration_desc* desc) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    std::vector<float> rays;
    int rc;
    if (desc) {
        const lm_camera &dc = desc->depth, &cc = desc->colour;
        bool ok = true;
        for (float v : desc->rotation) ok = ok && std::isfinite(v);
        for (float v : desc->translation) ok = ok && std::isfinite(v);
        if ((rc = check_cameras("registration: ", "every number must be finite", ok, dc, cc))) return rc;
        if (desc->splat_x < 0 || desc->splat_x > 3 || desc->splat_y < 0 || desc->splat_y > 3) return fail(LM_ERR_INVALID, "registration: splat_x and splat_y must lie in 0 .. 3");
        const size_t n = 2 * (size_t)dc.width * (size_t)dc.height;
        if (desc->rays) {
            for (size_t k = 0; k < n; ++k) if (!std::isfinite(desc->rays[k])) return fail(LM_ERR_INVALID, "registration: every ray must be finite");
            rays.assign(desc->rays, desc->rays + n);
        } else {
            rays.resize(n);
            lmr::build_rays(dc.fx, dc.fy, dc.cx, dc.cy, dc.k1, dc.k2, dc.p1, dc.p2, dc.k3, dc.width, dc.height, rays.data());
            for (size_t k = 0; k < n; ++k) if (!std::isfinite(rays[k])) return fail(LM_ERR_INVALID, "registration: the depth camera's distortion has no finite inverse at some pixel");
        }
    }
    if ((rc = quiesce_for_set(d, ""))) return rc;
    d->reg_on = desc != nullptr;
    d->reg = desc ? *desc : lm_registration_desc{};
    d->reg.rays = nullptr;
    d->reg_rays = std::move(rays);
    d->reg_rays_dirty = d->reg_on;
    return LM_OK;
}

int lm_get_registration_rays(lm_detector* d, float* out) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (!d->reg_on) return fail(LM_ERR_INVALID, "no registration set: lm_set_registration first");
    if (!out) return fail(LM_ERR_INVALID, "bad argument");
    std::memcpy(out, d->reg_rays.data(), d->reg_rays.size() * sizeof(float));
    return LM_OK;
}

int lm_stage_register_depth(lm_detector* d, const lm_image_desc* depth_raw, uint16_t* out_host) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if (!depth_raw || !out_host) return fail(LM_ERR_INVALID, "bad argument");
    if (!d->reg_on) return fail(LM_ERR_INVALID, "no registration set: lm_set_registration first");
    LmIngestDesc e = LmIngestDesc();
    if ((rc = check(lmc::raw_depth(d->cfg, d->reg, true), *depth_raw, 0, lm_ingest_opts{0, 0, 0}, &e.depth, nullptr))) return rc;
    if ((rc = ensure_table(d->reg_rays, d->d_reg_rays, d->reg_rays_dirty))) return rc;
    const int w = d->reg.colour.width, h = d->reg.colour.height;
    const size_t n = (size_t)w * (size_t)h;
    hipStream_t st = d->copy_stream[0];
    DevBuf<LmIngestDesc> d_e; DevBuf<u32> d_z; DevBuf<u16> d_out;
    HIP_TRY(d_z.alloc(n));
    HIP_TRY(d_out.alloc(n));
    if ((rc = put_desc(st, e, d_e))) return rc;
    LmRegisterArgs r;
    fill_register_args(d, &r);
    r.table = d_e; r.first = 0; r.n = 1; r.w = w; r.h = h;
    r.zbuf = d_z; r.out = reinterpret_cast<u8*>(d_out.get()); r.out_stride = 0;
    HIP_TRY(hipMemsetAsync(r.zbuf, 0xFF, n * sizeof(u32), st));
    lmk_register(st, r);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, d_out, n * sizeof(u16), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LM_OK;
}

int lm_set_rectification(lm_detector* d, const lm_rectification_desc* desc) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    std::vector<int32_t> map;
    int rc;
    if (desc) {
        const lm_camera &sc = desc->source, &ic = desc->ideal;
        if ((rc = check_cameras("rectification: ", "every camera number must be finite", true, sc, ic))) return rc;
        for (float v : {ic.k1, ic.k2, ic.p1, ic.p2, ic.k3})
            if (v != 0.0f) return fail(LM_ERR_INVALID, "rectification: the ideal camera's coefficients must be 0");
        const lmq::Cam s = {sc.fx, sc.fy, sc.cx, sc.cy, sc.k1, sc.k2, sc.p1, sc.p2, sc.k3, sc.width, sc.height};
        const lmq::Cam t = {ic.fx, ic.fy, ic.cx, ic.cy, 0.0, 0.0, 0.0, 0.0, 0.0, ic.width, ic.height};
        map.resize(2 * (size_t)ic.width * (size_t)ic.height);
        lmq::build_map(s, t, desc->map, map.data());
    }
    if ((rc = quiesce_for_set(d, "rectification: "))) return rc;
    d->rect_on = desc != nullptr;
    d->rect = desc ? *desc : lm_rectification_desc{};
    d->rect.map = nullptr;
    d->rect_map = std::move(map);
    d->rect_map_dirty = d->rect_on;
    return LM_OK;
}

int lm_get_rectification_map(lm_detector* d, int32_t* out) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (!d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    if (!out) return fail(LM_ERR_INVALID, "bad argument");
    std::memcpy(out, d->rect_map.data(), d->rect_map.size() * sizeof(int32_t));
    return LM_OK;
}

int lm_set_raw_processing(lm_detector* d, const lm_raw_processing* p) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (p) {
        if (p->black < 0 || p->black > 65535) return fail(LM_ERR_INVALID, "raw processing: black " + std::to_string(p->black) + " lies outside 0 .. 65535");
        for (int c = 0; c < 3; ++c)
            if (p->gain[c] > 65535u) return fail(LM_ERR_INVALID, "raw processing: gain " + std::to_string(p->gain[c]) + " lies above 65535");
        for (int k = 0; k < 9; ++k)
            if (p->ccm[k] < -8192 || p->ccm[k] > 8192) return fail(LM_ERR_INVALID, "raw processing: matrix entry " + std::to_string(p->ccm[k]) + " lies outside -8192 .. 8192");
    }
    if (int rc = quiesce_for_set(d, "raw processing: ")) return rc;
    d->raw_on = p != nullptr;
    d->raw[0] = p ? *p : raw_identity();
    d->raw_dirty = true;
    return LM_OK;
}

int lm_get_raw_processing(lm_detector* d, lm_raw_processing* out) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (!out) return fail(LM_ERR_INVALID, "bad argument");
    *out = d->raw[0];
    return LM_OK;
}

int lm_stage_rectify(lm_detector* d, const lm_image_desc* colour, const lm_image_desc* depth, uint8_t* bgr_out_host, uint16_t* depth_out_host) {
    return stage_hook(d, RECTIFY, colour, depth, bgr_out_host, depth_out_host);
}

int lm_set_reduction(lm_detector* d, const lm_reduction_desc* desc) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    lm_reduction_desc r = {};
    if (desc) {
        const std::string refusal = lmc::check_reduction(*desc, &r);
        if (!refusal.empty()) return fail(LM_ERR_INVALID, refusal);
    }
    if (int rc = quiesce_for_set(d, "reduction: ")) return rc;
    d->red_on = desc != nullptr;
    d->red = r;
    return LM_OK;
}

int lm_get_reduction(lm_detector* d, lm_reduction_desc* out, int* is_set) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    if (!out || !is_set) return fail(LM_ERR_INVALID, "bad argument");
    *out = d->red;
    *is_set = d->red_on ? 1 : 0;
    return LM_OK;
}

int lm_reduced_camera(const lm_camera* source, const lm_reduction_desc* reduction, int crop_x, int crop_y, int w, int h, lm_camera* out) {
    if (!source || !reduction || !out) return fail(LM_ERR_INVALID, "bad argument");
    lm_reduction_desc r = {};
    const std::string refusal = lmc::check_reduction(*reduction, &r);
    if (!refusal.empty()) return fail(LM_ERR_INVALID, refusal);
    *out = *source;
    out->fx = (float)((double)source->fx * r.den_x / r.num_x);
    out->fy = (float)((double)source->fy * r.den_y / r.num_y);
    out->cx = (float)(((double)source->cx + 0.5) * r.den_x / r.num_x - 0.5 - crop_x);
    out->cy = (float)(((double)source->cy + 0.5) * r.den_y / r.num_y - 0.5 - crop_y);
    out->width = w; out->height = h;
    return LM_OK;
}

int lm_stage_reduce(lm_detector* d, const lm_image_desc* colour, const lm_image_desc* depth, uint8_t* bgr_out_host, uint16_t* depth_out_host) {
    if (d && !d->red_on) return fail(LM_ERR_INVALID, "reduction: no reduction set: lm_set_reduction first");
    return stage_hook(d, REDUCE, colour, depth, bgr_out_host, depth_out_host);
}

int lm_stage_rectify_reduce(lm_detector* d, const lm_image_desc* colour, const lm_image_desc* depth, uint8_t* bgr_out_host, uint16_t* depth_out_host) {
    if (d && !d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    if (d && !d->red_on) return fail(LM_ERR_INVALID, "reduction: no reduction set: lm_set_reduction first");
    return stage_hook(d, RECTIFY_REDUCE, colour, depth, bgr_out_host, depth_out_host);
}

}  // extern "C"
