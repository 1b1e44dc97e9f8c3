// lm_detector_export.hip -- the slots' colour frames out again, with primitives drawn, in the consumer's format, into DEVICE memory the
// caller owns (lm_export_frames): the mirror image of lm_detector_ingest.hip.  One k_export launch per call on the
// export's own stream, behind the slots' upload tickets; synchronous.  It only READS the slots: a match in flight on them is no
// obstacle, but an upload from another thread is -- the call claims its slot span against uploads the way an ICP refinement does
// (export_span, refuse_checked_slots) and releases it on every path out.  Check the arguments (lm_export_check.h, host code of its own),
// plan the tile lists (lmh::plan_export), only then claim, enqueue and wait.
#include "lm_detector_impl.h"

namespace lmd {

static int ensure_export(lm_detector* d) {
    if (!d->ex_stream) HIP_TRY(d->ex_stream.create(hipStreamNonBlocking));
    return LM_OK;
}

static int claim_export_span(lm_detector* d, int lo, int hi) {
    long long expected = -1;
    if (!d->export_span.compare_exchange_strong(expected, ((long long)lo << 32) | (long long)hi))
        return fail(LM_ERR_INVALID, "an export is already in flight on this detector");
    return LM_OK;
}

// Where the call's four tables lie in its one block (every table 16-byte aligned)
struct ExportBlock { size_t images, recs, tile_off, idx, bytes; };
static ExportBlock export_block(int n, const lmh::ExportPlan& p) {
    ExportBlock b;
    b.images = 0;
    b.recs = align_up((size_t)n * sizeof(LmExportImage), 16);
    b.tile_off = b.recs + p.recs.size() * sizeof(lmw::Rec);
    b.idx = align_up(b.tile_off + p.tile_off.size() * sizeof(u32), 16);
    b.bytes = align_up(b.idx + p.idx.size() * sizeof(u32), 16);
    return b;
}

// behind the claim: the tables up in one copy, the launch, the wait
static int run_export(lm_detector* d, int first_slot, int n_slots, const std::vector<LmExportImage>& images, const lmh::ExportPlan& plan) {
    int rc;
    if ((rc = ensure_export(d))) return rc;
    hipStream_t st = d->ex_stream;
    for (int i = 0; i < n_slots; ++i) {
        Slot& sl = d->slots[(size_t)(first_slot + i)];
        if (sl.up_seq > 0) HIP_TRY(hipStreamWaitEvent(st, sl.ev_up, 0));
    }
    const ExportBlock b = export_block(n_slots, plan);
    if (b.bytes > d->ex_host.size()) HIP_TRY(d->ex_host.grow(b.bytes));       // (the last export has returned: nothing reads either block)
    if (b.bytes > d->ex_dev.size()) HIP_TRY(d->ex_dev.grow(b.bytes));
    u8* h = d->ex_host;
    std::memcpy(h + b.images, images.data(), images.size() * sizeof(LmExportImage));
    if (!plan.recs.empty()) std::memcpy(h + b.recs, plan.recs.data(), plan.recs.size() * sizeof(lmw::Rec));
    std::memcpy(h + b.tile_off, plan.tile_off.data(), plan.tile_off.size() * sizeof(u32));
    if (!plan.idx.empty()) std::memcpy(h + b.idx, plan.idx.data(), plan.idx.size() * sizeof(u32));
    HIP_TRY(hipMemcpyAsync(d->ex_dev, h, b.bytes, hipMemcpyHostToDevice, st));
    const u8* dv = d->ex_dev;
    LmExportArgs a;
    a.frame = d->frame_arena; a.slot_stride = d->frame_stride; a.off_bgr = d->off_bgr[0];
    a.first = first_slot; a.n = n_slots; a.w = d->cfg.width; a.h = d->cfg.height;
    a.tiles_x = plan.tiles_x; a.tiles_y = plan.tiles_y;
    a.n_float = 0;
    for (const LmExportImage& e : images) a.n_float += e.es != 0;
    a.n_plain = n_slots - a.n_float;
    a.images = reinterpret_cast<const LmExportImage*>(dv + b.images);
    a.recs = reinterpret_cast<const lmw::Rec*>(dv + b.recs);
    a.tile_off = reinterpret_cast<const u32*>(dv + b.tile_off);
    a.idx = reinterpret_cast<const u32*>(dv + b.idx);
    lmk_export(st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return LM_OK;
}

}  // namespace lmd

extern "C" {

int lm_export_frames(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* dst, const lm_ingest_opts* undo, const lm_draw_prim* prims,
                     size_t n_prims) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    std::string refusal = lmc::check_export_counts(!dst, n_slots, !prims, n_prims);
    if (!refusal.empty()) return fail(LM_ERR_INVALID, refusal);
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    for (int i = 0; i < n_slots; ++i)
        if (!d->slots[(size_t)(first_slot + i)].has_frame) return fail(LM_ERR_INVALID, "export: frame " + std::to_string(i) + ": no frame uploaded to slot");
    const int W = d->cfg.width, H = d->cfg.height;
    if (!(refusal = lmc::check_export_frame(W, H)).empty()) return fail(LM_ERR_INVALID, refusal);
    // (looked at first, claimed last: a call that is refused for another reason never holds the claim, not even for a moment)
    if (d->export_span.load() >= 0) return fail(LM_ERR_INVALID, "an export is already in flight on this detector");
    // the call's own tables: the detector's blocks are written only behind the claim
    static thread_local std::vector<LmExportImage> images;
    static thread_local std::vector<lmh::ExportUndo> opts;
    static thread_local lmh::ExportPlan plan;
    images.resize((size_t)n_slots); opts.resize((size_t)n_slots);
    for (int i = 0; i < n_slots; ++i) {
        LmExportImage& e = images[(size_t)i];
        if (!(refusal = lmc::check_export_image(W, H, dst[i], i, &e)).empty()) return fail(LM_ERR_INVALID, refusal);
        lmh::ExportUndo& o = opts[(size_t)i];
        o = {0, 0, 0};
        if (undo) o = {undo[i].flip_x != 0, lmh::clamp_shift(undo[i].shift_x, W), lmh::clamp_shift(undo[i].shift_y, H)};     // (beyond: an all-zero image either way)
        e.flip_x = o.flip_x; e.shift_x = o.shift_x; e.shift_y = o.shift_y;
    }
    if (!(refusal = lmc::check_export_overlap(W, H, images.data(), n_slots)).empty()) return fail(LM_ERR_INVALID, refusal);
    for (size_t k = 0; k < n_prims; ++k)
        if (!(refusal = lmc::check_export_prim(prims[k], k, n_slots)).empty()) return fail(LM_ERR_INVALID, refusal);
    if (!lmh::plan_export(W, H, n_slots, opts.data(), prims, n_prims, lmh::EXPORT_MAX_ENTRIES, plan))
        return fail(LM_ERR_OVERFLOW, "export: the tile-binning table needs " + std::to_string(plan.entries) + " entries, more than " +
                    std::to_string(lmh::EXPORT_MAX_ENTRIES) + ": split the primitive list over several calls");
    if ((rc = claim_export_span(d, first_slot, first_slot + n_slots - 1))) return rc;
    rc = run_export(d, first_slot, n_slots, images, plan);
    d->export_span.store(-1);
    return rc;
}

}  // extern "C"
