// lm_detector_ingest.hip -- frames whose source already lies in device memory in the producer's format, into the resident slots: one k_ingest
// launch under one upload ticket (lm_ingest_frames), the raw depth image registered onto the colour camera behind it (lm_ingest_frames_registered,
// lm_k_register.hip, lm_set_registration), k_rectify in k_ingest's place (lm_ingest_frames_rectified, lm_k_rectify.hip, lm_set_rectification),
// the raw pipeline of the raw colour formats (lm_set_raw_processing: host state and its device copy, read by k_ingest_raw / k_rectify_raw)
// the area-averaged reduction in k_ingest's place (lm_ingest_frames_reduced, lm_k_reduce.hip, lm_set_reduction: host state alone)
// both in one pass (lm_ingest_frames_rectified_reduced, lm_k_rectify_reduce.hip: the map in front of the box)
// and the four stage hooks.  It is an upload and follows lm_detector_upload.hip's rule: check the arguments (the descriptors: lm_ingest_check.h,
// host code of its own), claim the slots, only then touch a slot or the device, end with the ticket.
#include "lm_detector_impl.h"

namespace lmd {

// What a call does with a frame's colour image and with its depth image (NONE: the detector keeps no depth frame, or
// a colour-only detector that keeps one was handed no depth descriptors: lmc::check_depth_call).
struct Route {
    enum Colour { C_INGEST, C_RECTIFY, C_REDUCE, C_RECTIFY_REDUCE } colour;
    enum Depth { D_NONE, D_INGEST, D_RECTIFY, D_REGISTER, D_REDUCE, D_RECTIFY_REDUCE } depth;
};

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

static void fill_rectify_args(const lm_detector* d, LmRectifyArgs* a) {
    a->map = d->d_rect_map;
    a->mw = d->rect.ideal.width; a->mh = d->rect.ideal.height; a->sw = d->rect.source.width; a->sh = d->rect.source.height;
}

static lmx::Ratio ratio_of(const lm_reduction_desc& r, int bit) {
    return (r.apply & bit) ? lmx::Ratio{r.num_x, r.den_x, r.num_y, r.den_y} : lmx::Ratio{1, 1, 1, 1};
}

// k_rectify_reduce's arguments but the table, the planes and the frame's size: the map, both cameras' sizes, the ratios, the grid order
static void fill_rectify_reduce_args(const lm_detector* d, LmRectifyReduceArgs* q) {
    q->map = d->d_rect_map;
    q->mw = d->rect.ideal.width; q->mh = d->rect.ideal.height; q->sw = d->rect.source.width; q->sh = d->rect.source.height;
    q->colour = ratio_of(d->red, LM_REDUCE_COLOUR); q->depth = ratio_of(d->red, LM_REDUCE_DEPTH); q->depth_rule = d->red.depth_rule;
    q->frame_fast = d->rectify_reduce_grid;
}

// The four lm_ingest_frames*.  D_REGISTER: `depth` holds the RAW depth images; the first kernel then takes the colour images alone and the
// depth planes are k_register_resolve's, behind it on the same stream and under the same ticket.  C_RECTIFY: the colour images, and the
// depth images of D_RECTIFY, go through k_rectify in k_ingest's place; C_REDUCE / D_REDUCE: both go through k_reduce, each with the
// reduction's ratio or, its apply bit clear, with 1 / 1 (the plain rule).  C_RECTIFY_REDUCE / D_RECTIFY_REDUCE: both go through
// k_rectify_reduce, the rectifier's map in front of the reduction's box, each with the reduction's ratio or with 1 / 1 (the rectified
// rule alone); with D_REGISTER beside it the raw depth image lands on the slot's camera directly.  Everything else of the call is the same.
static int ingest_frames(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth, const lm_ingest_opts* opts,
                         void* producer_stream, Route route) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    const lm_config& c = d->cfg;
    const bool rectify = route.colour == Route::C_RECTIFY, reg = route.depth == Route::D_REGISTER, reduce = route.colour == Route::C_REDUCE;
    bool takes_depth = false;
    const std::string depth_refusal = lmc::check_depth_call(c, reg, depth != nullptr, &takes_depth);
    if (!takes_depth && !reg) route.depth = Route::D_NONE;
    const bool both = route.colour == Route::C_RECTIFY_REDUCE;
    if (rectify && !d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    if (!depth_refusal.empty()) return fail(LM_ERR_INVALID, depth_refusal);
    if (reg && !d->reg_on) return fail(LM_ERR_INVALID, "no registration set: lm_set_registration first");
    if (!colour || (lmc::depth_required(c, reg) && !depth) || n_slots <= 0) return fail(LM_ERR_INVALID, "bad argument");
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    if (c.width % 16) return fail(LM_ERR_INVALID, "lm_ingest_frames needs a frame width that is a multiple of 16");
    if (rectify && reg && (d->reg.colour.width != d->rect.ideal.width || d->reg.colour.height != d->rect.ideal.height))
        return fail(LM_ERR_INVALID, "rectification: the registration's colour camera (" + std::to_string(d->reg.colour.width) + " x " + std::to_string(d->reg.colour.height) +
                    ") is not the ideal camera (" + std::to_string(d->rect.ideal.width) + " x " + std::to_string(d->rect.ideal.height) + ")");
    if (both && reg) {
        // the colour image's geometry in this route: the reduced ideal one, or the ideal one while the reduction leaves the colour image alone
        const lmx::Ratio q = ratio_of(d->red, LM_REDUCE_COLOUR);
        const int gw = lmx::reduced_size(d->rect.ideal.width, q.num_x, q.den_x), gh = lmx::reduced_size(d->rect.ideal.height, q.num_y, q.den_y);
        if (d->reg.colour.width != gw || d->reg.colour.height != gh)
            return fail(LM_ERR_INVALID, "rectification: the registration's colour camera (" + std::to_string(d->reg.colour.width) + " x " + std::to_string(d->reg.colour.height) +
                        ") is not the " + ((d->red.apply & LM_REDUCE_COLOUR) ? "reduced ideal geometry (" : "ideal camera (") + std::to_string(gw) + " x " + std::to_string(gh) + ")");
    }
    const lmc::Geometry gc = both ? lmc::rectified_reduced(c, d->rect, d->red, lmc::COLOUR, false) : rectify ? lmc::rectified(c, d->rect, lmc::COLOUR, false) : reduce ? lmc::reduced(c, d->red, lmc::COLOUR, false) : lmc::plain(c, lmc::COLOUR);
    const lmc::Geometry gd = reg ? lmc::raw_depth(c, d->reg, false) : both ? lmc::rectified_reduced(c, d->rect, d->red, lmc::DEPTH, false) : reduce ? lmc::reduced(c, d->red, lmc::DEPTH, false)
                           : route.depth == Route::D_RECTIFY ? lmc::rectified(c, d->rect, lmc::DEPTH, false) : lmc::plain(c, lmc::DEPTH);
    // the descriptors, checked into a table of the call's own: the detector's pinned table is written only once the slots are claimed and
    // their earlier uploads have landed
    static thread_local std::vector<LmIngestDesc> table;
    table.resize((size_t)n_slots);
    int n_family[4] = {0, 0, 0, 0};     // frames per lm_ingest_family of their colour image: k_ingest's, k_ingest_yuv's, k_ingest_bayer's, k_ingest_raw's
    for (int i = 0; i < n_slots; ++i) {
        LmIngestDesc& e = table[(size_t)i];
        e = LmIngestDesc();
        lm_ingest_opts o = opts ? opts[i] : lm_ingest_opts{0, 0, 0};
        o.flip_x = o.flip_x != 0;
        o.shift_x = lmh::clamp_shift(o.shift_x, c.width); o.shift_y = lmh::clamp_shift(o.shift_y, c.height);     // (beyond: an all-zero frame either way)
        e.flip_x = o.flip_x; e.shift_x = o.shift_x; e.shift_y = o.shift_y;
        if ((rc = check(gc, colour[i], i, o, &e.colour, &e.matrix))) return rc;
        if (d->raw_on) lmc::process_bayer8(&e.colour);
        if (route.depth != Route::D_NONE && (rc = check(gd, depth[i], i, o, &e.depth, nullptr))) return rc;
        ++n_family[lm_ingest_family(e.colour.kind)];
    }
    if ((rc = claim_slots(d, first_slot, n_slots))) return rc;
    for (int i = 0; i < n_slots; ++i) if ((rc = wait_slot_upload(d, d->slots[first_slot + i]))) return rc;
    if ((rc = ensure_ingest(d))) return rc;
    std::memcpy(d->h_ingest + first_slot, table.data(), (size_t)n_slots * sizeof(LmIngestDesc));
    const int cs = (first_slot / n_slots) % d->n_copy_streams;   // as lm_upload_frames_pinned: consecutive runs take turns on the copy streams
    hipStream_t st = d->copy_stream[cs];
    const size_t z_words = (size_t)n_slots * (size_t)c.width * (size_t)c.height;
    if ((rectify || both) && (rc = ensure_table(d->rect_map, d->d_rect_map, d->rect_map_dirty))) return rc;
    const int n_raw = n_family[LM_INGEST_FAMILY_RAW];
    if (n_raw > 0 && (rc = ensure_table(d->raw, d->d_raw, d->raw_dirty))) return rc;
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
    LmIngestArgs a;
    a.table = d->d_ingest; a.frame = d->frame_arena; a.slot_stride = d->frame_stride; a.off_bgr = d->off_bgr[0]; a.off_depth = d->off_depth;
    a.first = first_slot; a.n = n_slots; a.w = c.width; a.h = c.height;
    a.rgbd = route.depth == Route::D_INGEST || route.depth == Route::D_RECTIFY || route.depth == Route::D_REDUCE || route.depth == Route::D_RECTIFY_REDUCE ? 1 : 0;      // (the first kernel writes the depth planes too)
    a.n_rgb = n_family[LM_INGEST_FAMILY_RGB]; a.n_yuv = n_family[LM_INGEST_FAMILY_YUV]; a.n_bayer = n_family[LM_INGEST_FAMILY_BAYER];
    a.n_raw = n_raw; a.raw = n_raw > 0 ? d->d_raw.get() : nullptr;
    if (rectify) {
        LmRectifyArgs q;
        fill_rectify_args(d, &q);
        q.table = d->d_ingest; q.first = first_slot; q.n = n_slots; q.n_rgb = a.n_rgb; q.n_yuv = a.n_yuv; q.n_bayer = a.n_bayer; q.n_raw = a.n_raw; q.raw = a.raw; q.w = c.width; q.h = c.height;
        q.out_bgr = d->frame_arena + d->off_bgr[0]; q.out_depth = a.rgbd ? d->frame_arena + d->off_depth : nullptr; q.out_stride = d->frame_stride;
        lmk_rectify(st, q);
    } else if (reduce) {
        LmReduceArgs q = LmReduceArgs();
        q.table = d->d_ingest; q.first = first_slot; q.n = n_slots; q.n_rgb = a.n_rgb; q.n_conv = a.n_yuv + a.n_bayer + a.n_raw; q.raw = a.raw; q.w = c.width; q.h = c.height;
        q.out_bgr = d->frame_arena + d->off_bgr[0]; q.out_depth = a.rgbd ? d->frame_arena + d->off_depth : nullptr; q.out_stride = d->frame_stride;
        q.colour = ratio_of(d->red, LM_REDUCE_COLOUR); q.depth = ratio_of(d->red, LM_REDUCE_DEPTH); q.depth_rule = d->red.depth_rule;
        lmk_reduce(st, q);
    } else if (both) {
        LmRectifyReduceArgs q = LmRectifyReduceArgs();
        fill_rectify_reduce_args(d, &q);
        q.table = d->d_ingest; q.first = first_slot; q.n = n_slots; q.n_rgb = a.n_rgb; q.n_yuv = a.n_yuv; q.n_bayer = a.n_bayer; q.n_raw = a.n_raw; q.raw = a.raw; q.w = c.width; q.h = c.height;
        q.out_bgr = d->frame_arena + d->off_bgr[0]; q.out_depth = a.rgbd ? d->frame_arena + d->off_depth : nullptr; q.out_stride = d->frame_stride;
        lmk_rectify_reduce(st, q);
    } else lmk_ingest(st, a);
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
    return issue_run_ticket(d, first_slot, n_slots, cs, false, route.depth != Route::D_NONE);      // one ticket for the whole launch
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

// The one descriptor of a stage hook on the device, landed (`e` is the caller's local)
static int put_desc(hipStream_t st, const LmIngestDesc& e, DevBuf<LmIngestDesc>& d_e) {
    HIP_TRY(d_e.alloc(1));
    HIP_TRY(hipMemcpyAsync(d_e, &e, sizeof(e), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LM_OK;
}

}  // namespace lmd

extern "C" {

int lm_ingest_frames(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth, const lm_ingest_opts* opts,
                     void* producer_stream) {
    return ingest_frames(d, first_slot, n_slots, colour, depth, opts, producer_stream, {Route::C_INGEST, Route::D_INGEST});
}

int lm_ingest_frames_registered(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth_raw,
                                const lm_ingest_opts* opts, void* producer_stream) {
    return ingest_frames(d, first_slot, n_slots, colour, depth_raw, opts, producer_stream, {Route::C_INGEST, Route::D_REGISTER});
}

int lm_ingest_frames_rectified(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                               const lm_ingest_opts* opts, int depth_route, void* producer_stream) {
    if (depth_route != LM_RECTIFY_DEPTH_ALIGNED && depth_route != LM_RECTIFY_DEPTH_REGISTERED) {
        int rc;
        if ((rc = ready_for_compute(d))) return rc;
        return fail(LM_ERR_INVALID, "rectification: unknown depth_route " + std::to_string(depth_route));
    }
    return ingest_frames(d, first_slot, n_slots, colour, depth, opts, producer_stream,
                         {Route::C_RECTIFY, depth_route == LM_RECTIFY_DEPTH_REGISTERED ? Route::D_REGISTER : Route::D_RECTIFY});
}

int lm_ingest_frames_reduced(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                             const lm_ingest_opts* opts, void* producer_stream) {
    // (host state: refused with or without a device)
    if (d && !d->red_on) return fail(LM_ERR_INVALID, "reduction: no reduction set: lm_set_reduction first");
    return ingest_frames(d, first_slot, n_slots, colour, depth, opts, producer_stream, {Route::C_REDUCE, Route::D_REDUCE});
}

int lm_ingest_frames_rectified_reduced(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                                       const lm_ingest_opts* opts, int depth_route, void* producer_stream) {
    // (host state: refused with or without a device)
    if (d && !d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    if (d && !d->red_on) return fail(LM_ERR_INVALID, "reduction: no reduction set: lm_set_reduction first");
    if (d && depth_route != LM_RECTIFY_DEPTH_ALIGNED && depth_route != LM_RECTIFY_DEPTH_REGISTERED)
        return fail(LM_ERR_INVALID, "rectification: unknown depth_route " + std::to_string(depth_route));
    return ingest_frames(d, first_slot, n_slots, colour, depth, opts, producer_stream,
                         {Route::C_RECTIFY_REDUCE, depth_route == LM_RECTIFY_DEPTH_REGISTERED ? Route::D_REGISTER : Route::D_RECTIFY_REDUCE});
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
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    const bool do_c = colour && bgr_out_host, do_d = depth && depth_out_host;
    if ((!do_c && !do_d) || (colour != nullptr) != (bgr_out_host != nullptr) || (depth != nullptr) != (depth_out_host != nullptr))
        return fail(LM_ERR_INVALID, "bad argument");
    if (!d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    LmIngestDesc e = LmIngestDesc();
    const lm_ingest_opts o = {0, 0, 0};
    if (do_c && (rc = check(lmc::rectified(d->cfg, d->rect, lmc::COLOUR, true), *colour, 0, o, &e.colour, &e.matrix))) return rc;
    if (do_c && d->raw_on) lmc::process_bayer8(&e.colour);
    if (do_d && (rc = check(lmc::rectified(d->cfg, d->rect, lmc::DEPTH, true), *depth, 0, o, &e.depth, nullptr))) return rc;
    if ((rc = ensure_table(d->rect_map, d->d_rect_map, d->rect_map_dirty))) return rc;
    const int w = d->rect.ideal.width, h = d->rect.ideal.height;
    const size_t n = (size_t)w * (size_t)h;
    hipStream_t st = d->copy_stream[0];
    DevBuf<LmIngestDesc> d_e; DevBuf<u8> d_bgr; DevBuf<u16> d_depth;
    if (do_c) HIP_TRY(d_bgr.alloc(n * 3));
    if (do_d) HIP_TRY(d_depth.alloc(n));
    if ((rc = put_desc(st, e, d_e))) return rc;
    LmRectifyArgs q;
    fill_rectify_args(d, &q);
    const int family = do_c ? lm_ingest_family(e.colour.kind) : LM_INGEST_FAMILY_RGB;      // (a depth-only call is k_rectify's)
    q.table = d_e; q.first = 0; q.n = 1; q.w = w; q.h = h;
    q.n_rgb = family == LM_INGEST_FAMILY_RGB; q.n_yuv = family == LM_INGEST_FAMILY_YUV; q.n_bayer = family == LM_INGEST_FAMILY_BAYER;
    q.n_raw = family == LM_INGEST_FAMILY_RAW; q.raw = nullptr;
    if (q.n_raw) {
        if ((rc = ensure_table(d->raw, d->d_raw, d->raw_dirty))) return rc;
        q.raw = d->d_raw.get();
    }
    q.out_bgr = do_c ? d_bgr.get() : nullptr; q.out_depth = do_d ? reinterpret_cast<u8*>(d_depth.get()) : nullptr; q.out_stride = 0;
    lmk_rectify(st, q);
    HIP_TRY(hipGetLastError());
    if (do_c) HIP_TRY(hipMemcpyAsync(bgr_out_host, d_bgr, n * 3, hipMemcpyDeviceToHost, st));
    if (do_d) HIP_TRY(hipMemcpyAsync(depth_out_host, d_depth, n * sizeof(u16), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LM_OK;
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
    int rc;
    if (d && !d->red_on) return fail(LM_ERR_INVALID, "reduction: no reduction set: lm_set_reduction first");
    if ((rc = ready_for_compute(d))) return rc;
    const bool do_c = colour && bgr_out_host, do_d = depth && depth_out_host;
    if ((!do_c && !do_d) || (colour != nullptr) != (bgr_out_host != nullptr) || (depth != nullptr) != (depth_out_host != nullptr))
        return fail(LM_ERR_INVALID, "bad argument");
    LmIngestDesc e = LmIngestDesc();
    const lm_ingest_opts o = {0, 0, 0};
    if (do_c && (rc = check(lmc::reduced(d->cfg, d->red, lmc::COLOUR, true), *colour, 0, o, &e.colour, &e.matrix))) return rc;
    if (do_c && d->raw_on) lmc::process_bayer8(&e.colour);
    if (do_d && (rc = check(lmc::reduced(d->cfg, d->red, lmc::DEPTH, true), *depth, 0, o, &e.depth, nullptr))) return rc;
    const lmx::Ratio qc = ratio_of(d->red, LM_REDUCE_COLOUR), qd = ratio_of(d->red, LM_REDUCE_DEPTH);
    const int cw = do_c ? lmx::reduced_size(colour->width, qc.num_x, qc.den_x) : 0, ch = do_c ? lmx::reduced_size(colour->height, qc.num_y, qc.den_y) : 0;
    const int dw = do_d ? lmx::reduced_size(depth->width, qd.num_x, qd.den_x) : 0, dh = do_d ? lmx::reduced_size(depth->height, qd.num_y, qd.den_y) : 0;
    hipStream_t st = d->copy_stream[0];
    DevBuf<LmIngestDesc> d_e; DevBuf<u8> d_bgr; DevBuf<u16> d_depth;
    const size_t nc = (size_t)cw * (size_t)ch, nd = (size_t)dw * (size_t)dh;
    if (nc) HIP_TRY(d_bgr.alloc(nc * 3));
    if (nd) HIP_TRY(d_depth.alloc(nd));
    if ((rc = put_desc(st, e, d_e))) return rc;
    // the two images have sizes of their own: one launch each
    LmReduceArgs q = LmReduceArgs();
    q.table = d_e; q.first = 0; q.n = 1; q.out_stride = 0; q.colour = qc; q.depth = qd; q.depth_rule = d->red.depth_rule;
    if (nc) {
        const int family = lm_ingest_family(e.colour.kind);
        q.n_rgb = family == LM_INGEST_FAMILY_RGB; q.n_conv = !q.n_rgb;
        if (family == LM_INGEST_FAMILY_RAW) {
            if ((rc = ensure_table(d->raw, d->d_raw, d->raw_dirty))) return rc;
            q.raw = d->d_raw.get();
        }
        q.w = cw; q.h = ch; q.out_bgr = d_bgr.get(); q.out_depth = nullptr;
        lmk_reduce(st, q);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(bgr_out_host, d_bgr, nc * 3, hipMemcpyDeviceToHost, st));
    }
    if (nd) {
        const int family = lm_ingest_family(e.colour.kind);         // (the kernel that owns the entry; a depth-only call: k_reduce)
        q.n_rgb = family == LM_INGEST_FAMILY_RGB; q.n_conv = !q.n_rgb;
        q.w = dw; q.h = dh; q.out_bgr = nullptr; q.out_depth = reinterpret_cast<u8*>(d_depth.get());
        lmk_reduce(st, q);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(depth_out_host, d_depth, nd * sizeof(u16), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return LM_OK;
}

int lm_stage_rectify_reduce(lm_detector* d, const lm_image_desc* colour, const lm_image_desc* depth, uint8_t* bgr_out_host, uint16_t* depth_out_host) {
    int rc;
    if (d && !d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    if (d && !d->red_on) return fail(LM_ERR_INVALID, "reduction: no reduction set: lm_set_reduction first");
    if ((rc = ready_for_compute(d))) return rc;
    const bool do_c = colour && bgr_out_host, do_d = depth && depth_out_host;
    if ((!do_c && !do_d) || (colour != nullptr) != (bgr_out_host != nullptr) || (depth != nullptr) != (depth_out_host != nullptr))
        return fail(LM_ERR_INVALID, "bad argument");
    LmIngestDesc e = LmIngestDesc();
    const lm_ingest_opts o = {0, 0, 0};
    if (do_c && (rc = check(lmc::rectified_reduced(d->cfg, d->rect, d->red, lmc::COLOUR, true), *colour, 0, o, &e.colour, &e.matrix))) return rc;
    if (do_c && d->raw_on) lmc::process_bayer8(&e.colour);
    if (do_d && (rc = check(lmc::rectified_reduced(d->cfg, d->rect, d->red, lmc::DEPTH, true), *depth, 0, o, &e.depth, nullptr))) return rc;
    if ((rc = ensure_table(d->rect_map, d->d_rect_map, d->rect_map_dirty))) return rc;
    LmRectifyReduceArgs q = LmRectifyReduceArgs();
    fill_rectify_reduce_args(d, &q);
    const int cw = do_c ? lmx::reduced_size(q.mw, q.colour.num_x, q.colour.den_x) : 0, ch = do_c ? lmx::reduced_size(q.mh, q.colour.num_y, q.colour.den_y) : 0;
    const int dw = do_d ? lmx::reduced_size(q.mw, q.depth.num_x, q.depth.den_x) : 0, dh = do_d ? lmx::reduced_size(q.mh, q.depth.num_y, q.depth.den_y) : 0;
    hipStream_t st = d->copy_stream[0];
    DevBuf<LmIngestDesc> d_e; DevBuf<u8> d_bgr; DevBuf<u16> d_depth;
    const size_t nc = (size_t)cw * (size_t)ch, nd = (size_t)dw * (size_t)dh;
    if (nc) HIP_TRY(d_bgr.alloc(nc * 3));
    if (nd) HIP_TRY(d_depth.alloc(nd));
    if ((rc = put_desc(st, e, d_e))) return rc;
    const int family = do_c ? lm_ingest_family(e.colour.kind) : LM_INGEST_FAMILY_RGB;      // (the kernel that owns the entry; a depth-only call: k_rectify_reduce)
    q.table = d_e; q.first = 0; q.n = 1; q.out_stride = 0;
    q.n_rgb = family == LM_INGEST_FAMILY_RGB; q.n_yuv = family == LM_INGEST_FAMILY_YUV; q.n_bayer = family == LM_INGEST_FAMILY_BAYER;
    q.n_raw = family == LM_INGEST_FAMILY_RAW;
    if (q.n_raw) {
        if ((rc = ensure_table(d->raw, d->d_raw, d->raw_dirty))) return rc;
        q.raw = d->d_raw.get();
    }
    // the two images have reduced sizes of their own: one launch each
    if (nc) {
        q.w = cw; q.h = ch; q.out_bgr = d_bgr.get(); q.out_depth = nullptr;
        lmk_rectify_reduce(st, q);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(bgr_out_host, d_bgr, nc * 3, hipMemcpyDeviceToHost, st));
    }
    if (nd) {
        q.w = dw; q.h = dh; q.out_bgr = nullptr; q.out_depth = reinterpret_cast<u8*>(d_depth.get());
        lmk_rectify_reduce(st, q);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(depth_out_host, d_depth, nd * sizeof(u16), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return LM_OK;
}

}  // extern "C"
