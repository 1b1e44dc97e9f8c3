// lm_detector_upload.hip -- frames, match masks and staged rows on their way into the resident slots: pinned staging, the copy streams'
// upload tickets, the copy routines and the lm_upload_* / lm_stage_* / lm_host_* / lm_device_* entry points.  An entry point checks its
// arguments, then claims the slots (claim_slots); only then does it touch a slot (frame_replaced) or the device, and it ends with the
// ticket (issue_ticket, issue_run_ticket).  Frames whose source already lies in device memory: lm_detector_ingest.hip, under the same rule.
#include "lm_detector_impl.h"

namespace lmd {

bool lane_holds_slots(const lm_detector* d, int first, int n) {
    for (const lm_detector::Lane& ln : d->lanes)
        if (ln.busy && first < ln.first + ln.n && ln.first < first + n) return true;
    return false;
}

int claim_slots(const lm_detector* d, int first, int n) {
    if (lane_holds_slots(d, first, n)) return fail(LM_ERR_INVALID, "slot belongs to a match in flight");
    return refuse_checked_slots(d, first, n);
}

void frame_replaced(Slot& s) {
    s.prepared = false; s.matched = false; s.mask_ready = false; s.staging_open = false;
    s.match_mask_on[0] = s.match_mask_on[1] = false;
    s.has_depth = false;        // (until the call that replaces the frame says what it brought)
}

// The slot's copies on `st` (copy stream cs) are enqueued: ev_up behind them, and the ticket -- the stream's next one, or `seq` where
// several slots share the ticket of one transfer (issue_run_ticket).
static int issue_ticket(Slot& s, int cs, hipStream_t st, unsigned long long seq) {
    HIP_TRY(hipEventRecord(s.ev_up, st));
    s.up_stream = cs; s.up_seq = seq;
    return LM_OK;
}
static unsigned long long draw_ticket(lm_detector* d, int cs) { return d->up_seq_next[cs]++; }
int issue_ticket(lm_detector* d, Slot& s, int cs, hipStream_t st) { return issue_ticket(s, cs, st, draw_ticket(d, cs)); }

// One transfer or launch on copy stream cs has filled slots [first, first + n): they share one ticket and hold a new frame.  ev_bgr: also
// recorded per slot (the transfer carried the colour image of an RGB-D frame).  has_depth: the frames came with their depth images.
int issue_run_ticket(lm_detector* d, int first, int n, int cs, bool ev_bgr, bool has_depth) {
    hipStream_t st = d->copy_stream[cs];
    const unsigned long long seq = draw_ticket(d, cs);
    for (int i = first; i < first + n; ++i) {
        Slot& s = d->slots[i];
        if (ev_bgr) HIP_TRY(hipEventRecord(s.ev_bgr, st));
        if (int rc = issue_ticket(s, cs, st, seq)) return rc;
        frame_replaced(s);
        s.has_frame = true; s.has_depth = has_depth;
    }
    return LM_OK;
}

// A frame's host images as an entry point was handed them: both present (depth: RGB-D detectors; optional on a colour-only detector
// that keeps depth, ignored on one that keeps none), stride 0 = dense rows.
int check_frame_source(const lm_detector* d, const uint8_t* bgr, size_t* bgr_stride, const uint16_t* depth, size_t* depth_stride) {
    const lm_config& c = d->cfg;
    if (!bgr) return fail(LM_ERR_INVALID, "sources.size() != modalities.size(): colour image missing");
    if (c.num_modalities == 2 && !depth) return fail(LM_ERR_INVALID, "sources.size() != modalities.size(): depth image missing");
    if (*bgr_stride == 0) *bgr_stride = (size_t)c.width * 3;
    if (*depth_stride == 0) *depth_stride = (size_t)c.width * 2;
    if (*bgr_stride < (size_t)c.width * 3 || *depth_stride < (size_t)c.width * 2) return fail(LM_ERR_INVALID, "stride smaller than a row");
    return LM_OK;
}

static int ensure_staging(lm_detector* d, Slot& s) {
    const lm_config& c = d->cfg;
    if (!s.h_bgr) HIP_TRY(s.h_bgr.alloc((size_t)c.width * c.height * 3));
    if (!s.h_depth && keeps_depth(d))
        HIP_TRY(s.h_depth.alloc((size_t)c.width * c.height));
    return LM_OK;
}

// Host waits until the slot's last copy-stream upload has landed (its staging buffer / the caller's pinned
// source may then be reused).  A stream's copies complete in ticket order, so this also retires its older tickets.
int wait_slot_upload(lm_detector* d, Slot& s) {
    if (s.up_seq > d->up_seq_done[s.up_stream]) {
        HIP_TRY(hipEventSynchronize(s.ev_up));
        d->up_seq_done[s.up_stream] = s.up_seq;
    }
    return LM_OK;
}

// Makes `stream` wait for the uploads of slots [first, first + n): per copy stream one hipStreamWaitEvent on the
// newest ticket among them (each copy stream is in order).  seqs[k]: that ticket (0: nothing pending on stream k).
int wait_uploads(lm_detector* d, hipStream_t stream, int first, int n, unsigned long long* seqs) {
    unsigned long long best[LM_NCOPY] = {};
    int bi[LM_NCOPY];
    for (int k = 0; k < LM_NCOPY; ++k) bi[k] = -1;
    for (int i = first; i < first + n; ++i) {
        const Slot& s = d->slots[i];
        if (s.up_seq > d->up_seq_done[s.up_stream] && s.up_seq > best[s.up_stream]) { best[s.up_stream] = s.up_seq; bi[s.up_stream] = i; }
    }
    for (int k = 0; k < LM_NCOPY; ++k) {
        if (bi[k] >= 0) HIP_TRY(hipStreamWaitEvent(stream, d->slots[bi[k]].ev_up, 0));
        if (seqs) seqs[k] = best[k];
    }
    return LM_OK;
}

// rows x row_bytes from a strided host image to dense device memory.  Pageable source: rows are packed into the
// slot's pinned staging buffer in `chunks` pieces, each followed by its own async copy, so the host memcpy of
// piece k + 1 overlaps the DMA of piece k.  pinned: the source goes straight to the DMA engine.
static int copy_image(hipStream_t st, u8* dst, u8* staging, const u8* src, size_t stride, size_t row_bytes, int rows,
                      bool pinned, int chunks) {
    if (pinned) {
        if (stride == row_bytes) HIP_TRY(hipMemcpyAsync(dst, src, row_bytes * rows, hipMemcpyHostToDevice, st));
        else HIP_TRY(hipMemcpy2DAsync(dst, row_bytes, src, stride, row_bytes, rows, hipMemcpyHostToDevice, st));
        return LM_OK;
    }
    if (chunks < 1) chunks = 1;
    for (int k = 0; k < chunks; ++k) {
        const int r0 = (int)((long long)rows * k / chunks), r1 = (int)((long long)rows * (k + 1) / chunks);
        if (r1 <= r0) continue;
        if (stride == row_bytes) lmh::copy_stream(staging + (size_t)r0 * row_bytes, src + (size_t)r0 * stride, (size_t)(r1 - r0) * row_bytes);
        else for (int y = r0; y < r1; ++y) lmh::copy_stream(staging + (size_t)y * row_bytes, src + (size_t)y * stride, row_bytes);
        lmh::copy_stream_fence();
        HIP_TRY(hipMemcpyAsync(dst + (size_t)r0 * row_bytes, staging + (size_t)r0 * row_bytes, (size_t)(r1 - r0) * row_bytes,
                               hipMemcpyHostToDevice, st));
    }
    return LM_OK;
}

// The translated image of a pageable source: shifted while the staging buffer is filled (lmh::stage_rows_shifted), then one copy.
static int copy_image_shifted(hipStream_t st, u8* dst, u8* staging, const u8* src, size_t stride, int w, int h, int px, int ox, int oy) {
    lmh::stage_rows_shifted(staging, src, stride, w, h, px, ox, oy, 0, h);
    HIP_TRY(hipMemcpyAsync(dst, staging, (size_t)w * px * (size_t)h, hipMemcpyHostToDevice, st));
    return LM_OK;
}

// The translated image from PINNED host memory: the DMA engine copies the overlapping rectangle row by row (hipMemcpy2DAsync) behind
// a memset of the destination -- no staging copy, no host pass over the pixels at all.
static int copy_image_shifted_pinned(hipStream_t st, u8* dst, const u8* src, size_t stride, int w, int h, int px, int ox, int oy) {
    const size_t row_bytes = (size_t)w * px;
    const lmh::ShiftRect q = lmh::shift_rect(w, h, ox, oy);
    HIP_TRY(hipMemsetAsync(dst, 0, row_bytes * (size_t)h, st));
    if (q.x1 <= q.x0 || q.y1 <= q.y0) return LM_OK;
    if (stride == row_bytes) {
        // Dense rows: a rectangle copy whose rows start at odd byte offsets runs at a TENTH of the link rate (measured r05,
        // tools/time_shifted_upload.py: 1 148 instead of 115 us per 1280 x 960 RGB-D frame for a shift of 7 pixels).  The rows are contiguous on
        // both sides, so ONE linear copy displaced by ox pixels shifts every row at once; what it wraps from a row's end into the next row's
        // start (or the other way round) is cleared again by a device-side 2-D memset of |ox| columns.
        const size_t rows = (size_t)(q.y1 - q.y0), shift_bytes = (size_t)std::abs(ox) * px;
        const u8* s0 = src + (size_t)(q.y0 - oy) * stride;
        u8* d0 = dst + (size_t)q.y0 * row_bytes;
        if (ox > 0) HIP_TRY(hipMemcpyAsync(d0 + shift_bytes, s0, rows * row_bytes - shift_bytes, hipMemcpyHostToDevice, st));
        else HIP_TRY(hipMemcpyAsync(d0, s0 + shift_bytes, rows * row_bytes - shift_bytes, hipMemcpyHostToDevice, st));
        if (ox != 0) HIP_TRY(hipMemset2DAsync(ox > 0 ? d0 : d0 + row_bytes - shift_bytes, row_bytes, 0, shift_bytes, rows, st));
        return LM_OK;
    }
    HIP_TRY(hipMemcpy2DAsync(dst + (size_t)q.y0 * row_bytes + (size_t)q.x0 * px, row_bytes, src + (size_t)(q.y0 - oy) * stride + (size_t)(q.x0 - ox) * px, stride,
                             (size_t)(q.x1 - q.x0) * px, (size_t)(q.y1 - q.y0), hipMemcpyHostToDevice, st));
    return LM_OK;
}

// One plane of a frame (px bytes per pixel) -> dst: as it is, translated on its way through the staging buffer, or translated by the DMA engine
static int copy_plane(lm_detector* d, hipStream_t st, u8* dst, u8* staging, const u8* src, size_t stride, int px, const UploadOpts& o) {
    const lm_config& c = d->cfg;
    if (o.shift_x == 0 && o.shift_y == 0) return copy_image(st, dst, staging, src, stride, (size_t)c.width * px, c.height, o.pinned, d->stage_chunks);
    if (o.pinned) return copy_image_shifted_pinned(st, dst, src, stride, c.width, c.height, px, o.shift_x, o.shift_y);
    return copy_image_shifted(st, dst, staging, src, stride, c.width, c.height, px, o.shift_x, o.shift_y);
}

// Frame -> slot.  o.inline_stream == nullptr: the copies go to the copy stream and the slot gets an upload ticket
// (consumers call wait_uploads); otherwise they are issued on `inline_stream` itself, in order with the kernels
// the caller enqueues behind them (single-frame calls: no cross-stream dependency on the latency path).
int upload_frame(lm_detector* d, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride, UploadOpts o) {
    const lm_config& c = d->cfg;
    Slot& s = d->slots[slot];
    int rc;
    if ((rc = check_frame_source(d, bgr, &bgr_stride, depth, &depth_stride))) return rc;
    if ((rc = claim_slots(d, slot, 1))) return rc;
    frame_replaced(s);
    o.shift_x = lmh::clamp_shift(o.shift_x, c.width); o.shift_y = lmh::clamp_shift(o.shift_y, c.height);     // (beyond: an all-zero frame either way)
    // the slot's previous upload may still be reading the staging buffer (and must land before this one anyway)
    if ((rc = wait_slot_upload(d, s))) return rc;
    if (!o.pinned && (rc = ensure_staging(d, s))) return rc;
    const int cs = slot % d->n_copy_streams;
    const bool ticket = !o.inline_stream, rgbd = keeps_depth(d) && depth != nullptr;      // (the call carries a depth image)
    hipStream_t st = ticket ? d->copy_stream[cs] : o.inline_stream;
    const size_t bgr_bytes = (size_t)c.width * c.height * 3;
    if (o.pinned && o.shift_x == 0 && o.shift_y == 0 && rgbd && bgr_stride == (size_t)c.width * 3 && depth_stride == (size_t)c.width * 2 &&
        reinterpret_cast<const u8*>(depth) == bgr + bgr_bytes) {
        // [colour | depth] contiguous on the host, as in the frame arena: one DMA transfer
        HIP_TRY(hipMemcpyAsync(d->bgr(slot, 0), bgr, bgr_bytes + (size_t)c.width * c.height * 2, hipMemcpyHostToDevice, st));
        if (ticket) HIP_TRY(hipEventRecord(s.ev_bgr, st));
    } else {
        if ((rc = copy_plane(d, st, d->bgr(slot, 0), s.h_bgr, bgr, bgr_stride, 3, o))) return rc;
        if (ticket && rgbd) HIP_TRY(hipEventRecord(s.ev_bgr, st));
        if (rgbd && (rc = copy_plane(d, st, reinterpret_cast<u8*>(d->depth(slot)), reinterpret_cast<u8*>(s.h_depth.get()), reinterpret_cast<const u8*>(depth),
                                     depth_stride, 2, o))) return rc;
    }
    if (ticket && (rc = issue_ticket(d, s, cs, st))) return rc;
    s.has_frame = true; s.has_depth = rgbd;
    return LM_OK;
}

// Detector::match's mask of one modality (-1: the same mask for every modality) -> slot; mask == nullptr clears it.  The ordering of
// Slot::d_match_mask: see lm_detector_impl.h.  inline_stream == nullptr: the copy rides the copy stream of the slot's last upload under a
// new ticket (a later ticket on the SAME stream also covers the frame's copies); otherwise it is issued on `inline_stream`.
int upload_match_mask(lm_detector* d, int slot, int modality, const uint8_t* mask, size_t stride, hipStream_t inline_stream) {
    const lm_config& c = d->cfg;
    const int M = c.num_modalities;
    Slot& s = d->slots[slot];
    if (modality < -1 || modality >= M) return fail(LM_ERR_INVALID, "mask modality out of range (-1 = all, 0 = colour, 1 = depth)");
    if (mask && stride == 0) stride = (size_t)c.width;
    if (mask && stride < (size_t)c.width) return fail(LM_ERR_INVALID, "mask stride smaller than a row");
    int rc;
    if ((rc = claim_slots(d, slot, 1))) return rc;
    const int m0 = modality < 0 ? 0 : modality, m1 = modality < 0 ? M : modality + 1;
    if (mask && !s.has_frame) return fail(LM_ERR_INVALID, "no frame uploaded to slot " + std::to_string(slot) + " (a frame upload clears the slot's masks: upload the frame first)");
    s.prepared = false; s.matched = false;      // (the slot's last lists belong to the old mask: lm_match_collect refuses them)
    if (!mask) {
        for (int m = m0; m < m1; ++m) s.match_mask_on[m] = false;
        return LM_OK;
    }
    if ((rc = wait_slot_upload(d, s))) return rc;       // the slot's last upload (an earlier mask's too) has left h_match_mask
    const size_t pitch = d->match_mask_pitch, plane = pitch * (size_t)c.height;
    if (!s.d_match_mask) HIP_TRY(s.d_match_mask.alloc(plane * M));
    if (!s.h_match_mask) {
        HIP_TRY(s.h_match_mask.alloc(plane * M));
        std::memset(s.h_match_mask, 0, plane * M);
    }
    const int cs = s.up_seq ? s.up_stream : slot % d->n_copy_streams;
    hipStream_t st = inline_stream ? inline_stream : d->copy_stream[cs];
    for (int m = m0; m < m1; ++m) {
        u8* h = s.h_match_mask + plane * m;
        for (int y = 0; y < c.height; ++y) std::memcpy(h + (size_t)y * pitch, mask + (size_t)y * stride, (size_t)c.width);
        HIP_TRY(hipMemcpyAsync(s.d_match_mask + plane * m, h, plane, hipMemcpyHostToDevice, st));
    }
    if (!inline_stream && (rc = issue_ticket(d, s, cs, st))) return rc;
    for (int m = m0; m < m1; ++m) s.match_mask_on[m] = true;
    return LM_OK;
}

struct PinnedBlock { const u8* p; size_t bytes; };
static std::mutex g_pinned_mu;
static std::vector<PinnedBlock> g_pinned;      // blocks handed out by lm_host_alloc

// [p, p + bytes) inside a block from lm_host_alloc?  (A table of our own: asking the runtime about a pageable pointer,
// hipPointerGetAttributes, costs 10-20 us per call -- measured -- on the path this is meant to shorten.)
bool is_pinned_host(const void* p, size_t bytes) {
    std::lock_guard<std::mutex> g(g_pinned_mu);
    for (const PinnedBlock& b : g_pinned)
        if (reinterpret_cast<const u8*>(p) >= b.p && reinterpret_cast<const u8*>(p) + bytes <= b.p + b.bytes) return true;
    return false;
}

// the single-frame uploads of the ABI
static int upload_entry(lm_detector* d, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                        bool pinned, int shift_x, int shift_y) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, slot, 1))) return rc;
    UploadOpts o;
    o.pinned = pinned; o.shift_x = shift_x; o.shift_y = shift_y;
    return upload_frame(d, slot, bgr, bgr_stride, depth, depth_stride, o);
}

}  // namespace lmd

extern "C" {

int lm_read_frame(lm_detector* d, int slot, uint8_t* bgr_out, uint16_t* depth_out) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, slot, 1))) return rc;
    const lm_config& c = d->cfg;
    Slot& s = d->slots[slot];
    if (!s.has_frame) return fail(LM_ERR_INVALID, "no frame uploaded to slot " + std::to_string(slot));
    if (depth_out && !keeps_depth(d)) return fail(LM_ERR_INVALID, "a colour-only detector holds no depth frame");
    if (depth_out && (rc = slot_lacks_depth(d, slot))) return rc;
    if ((rc = wait_slot_upload(d, s))) return rc;
    if (bgr_out) HIP_TRY(hipMemcpy(bgr_out, d->bgr(slot, 0), (size_t)c.width * c.height * 3, hipMemcpyDeviceToHost));
    if (depth_out) HIP_TRY(hipMemcpy(depth_out, d->depth(slot), (size_t)c.width * c.height * 2, hipMemcpyDeviceToHost));
    return LM_OK;
}

int lm_device_alloc(size_t bytes, void** out) {
    if (!out || !bytes) return fail(LM_ERR_INVALID, "bad argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(LM_ERR_NO_DEVICE, "no HIP device available: liblinemod_hip has no CPU fallback");
    DevBuf<u8> b;
    HIP_TRY(b.alloc(bytes));
    *out = b.release();      // the caller's from here on (lm_device_free), and counted live until then
    return LM_OK;
}

void lm_device_free(void* p) {
    DevBuf<u8>(static_cast<u8*>(p)).reset();
}

int lm_device_copy(void* dst, const void* src, size_t bytes, int kind) {
    if (!dst || !src || kind < 0 || kind > 2) return fail(LM_ERR_INVALID, "bad argument");
    if (!bytes) return LM_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(LM_ERR_NO_DEVICE, "no HIP device available: liblinemod_hip has no CPU fallback");
    HIP_TRY(hipMemcpy(dst, src, bytes, kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return LM_OK;
}


int lm_upload_frame(lm_detector* d, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride) {
    return upload_entry(d, slot, bgr, bgr_stride, depth, depth_stride, false, 0, 0);
}
int lm_upload_frame_shifted(lm_detector* d, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                            int shift_x, int shift_y) {
    return upload_entry(d, slot, bgr, bgr_stride, depth, depth_stride, false, shift_x, shift_y);
}
int lm_upload_frame_pinned(lm_detector* d, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride) {
    return upload_entry(d, slot, bgr, bgr_stride, depth, depth_stride, true, 0, 0);
}
int lm_upload_frame_pinned_shifted(lm_detector* d, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                                   int shift_x, int shift_y) {
    return upload_entry(d, slot, bgr, bgr_stride, depth, depth_stride, true, shift_x, shift_y);
}

int lm_upload_frames_pinned(lm_detector* d, int first_slot, int n_slots, const uint8_t* frames, size_t frame_stride) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    if (!frames || n_slots <= 0) return fail(LM_ERR_INVALID, "bad argument");
    const lm_config& c = d->cfg;
    const size_t fb = (size_t)c.width * c.height * (keeps_depth(d) ? 5 : 3);
    if (frame_stride == 0) frame_stride = fb;
    if (frame_stride < fb) return fail(LM_ERR_INVALID, "frame stride smaller than a frame");
    if ((rc = claim_slots(d, first_slot, n_slots))) return rc;
    for (int i = 0; i < n_slots; ++i) if ((rc = wait_slot_upload(d, d->slots[first_slot + i]))) return rc;
    // one strided transfer: row i = host frame i ([colour | depth] dense), destination pitch = the arena's slot stride
    const int cs = (first_slot / n_slots) % d->n_copy_streams;   // consecutive runs of n_slots slots take turns on the copy streams
    hipStream_t st = d->copy_stream[cs];
    HIP_TRY(hipMemcpy2DAsync(d->bgr(first_slot, 0), d->frame_stride, frames, frame_stride, fb, (size_t)n_slots, hipMemcpyHostToDevice, st));
    return issue_run_ticket(d, first_slot, n_slots, cs, keeps_depth(d), keeps_depth(d));      // one ticket for the whole transfer
}

// ---- staged uploads (r05): the staging copy of a pageable frame split from the transfer, so that a host thread pool fills the
// pinned staging buffers of a batch (row ranges in parallel) while the thread that owns the detector does something else:
//     lm_stage_reserve(first, n)                       owner thread: the slots' earlier uploads have landed, staging exists
//     lm_stage_rows(slot, ..., row0, row1)  x many     ANY thread, disjoint row ranges: host memory only, no HIP call
//     lm_upload_staged(slot)                           owner thread: the H2D copies + the slot's upload ticket
int lm_stage_reserve(lm_detector* d, int first_slot, int n_slots) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    if ((rc = claim_slots(d, first_slot, n_slots))) return rc;
    for (int i = 0; i < n_slots; ++i) {
        Slot& s = d->slots[first_slot + i];
        if ((rc = wait_slot_upload(d, s))) return rc;
        if ((rc = ensure_staging(d, s))) return rc;
        s.staging_open = true; s.staged.clear();
    }
    return LM_OK;
}

int lm_stage_rows(lm_detector* d, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                  int shift_x, int shift_y, int row0, int row1) {
    if (!d || !d->dev_ready) return fail(LM_ERR_INVALID, "lm_stage_reserve first");
    if (slot < 0 || slot >= (int)d->slots.size()) return fail(LM_ERR_INVALID, "slot out of range");
    const lm_config& c = d->cfg;
    Slot& s = d->slots[slot];
    if (!s.staging_open || !s.h_bgr) return fail(LM_ERR_INVALID, "lm_stage_reserve first");
    if (int rc = check_frame_source(d, bgr, &bgr_stride, depth, &depth_stride)) return rc;
    if (row0 < 0 || row1 > c.height || row0 > row1) return fail(LM_ERR_INVALID, "row range outside the frame");
    const int ox = lmh::clamp_shift(shift_x, c.width), oy = lmh::clamp_shift(shift_y, c.height);
    lmh::stage_rows_shifted(s.h_bgr, bgr, bgr_stride, c.width, c.height, 3, ox, oy, row0, row1);
    if (keeps_depth(d) && depth)
        lmh::stage_rows_shifted(reinterpret_cast<u8*>(s.h_depth.get()), reinterpret_cast<const u8*>(depth), depth_stride, c.width, c.height, 2, ox, oy, row0, row1);
    s.staged.add(depth ? StagedBits::WITH_DEPTH : StagedBits::WITHOUT_DEPTH);
    return LM_OK;
}

int lm_upload_staged(lm_detector* d, int slot) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, slot, 1))) return rc;
    Slot& s = d->slots[slot];
    if (!s.staging_open) return fail(LM_ERR_INVALID, "lm_stage_reserve first");
    if ((rc = claim_slots(d, slot, 1))) return rc;
    const lm_config& c = d->cfg;
    // the depth image is optional on a colour-only detector that keeps depth, but for the slot as a whole: rows staged with a depth image
    // beside rows staged without one would send up a plane that is partly the staging buffer's old bytes
    const int staged = s.staged.get();
    if (depth_optional(d) && staged == (StagedBits::WITH_DEPTH | StagedBits::WITHOUT_DEPTH))
        return fail(LM_ERR_INVALID, "the lm_stage_rows calls of slot " + std::to_string(slot) + " brought a depth image for some rows and none for others");
    const int cs = slot % d->n_copy_streams;
    hipStream_t st = d->copy_stream[cs];
    const bool with_depth = c.num_modalities == 2 || (depth_optional(d) && (staged & StagedBits::WITH_DEPTH));
    frame_replaced(s);
    HIP_TRY(hipMemcpyAsync(d->bgr(slot, 0), s.h_bgr, (size_t)c.width * c.height * 3, hipMemcpyHostToDevice, st));
    if (with_depth) {
        HIP_TRY(hipEventRecord(s.ev_bgr, st));
        HIP_TRY(hipMemcpyAsync(d->depth(slot), s.h_depth, (size_t)c.width * c.height * 2, hipMemcpyHostToDevice, st));
    }
    if ((rc = issue_ticket(d, s, cs, st))) return rc;
    s.has_frame = true; s.has_depth = with_depth;
    return LM_OK;
}

int lm_upload_wait(lm_detector* d, int slot) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if (slot < 0) {
        for (int k = 0; k < LM_NCOPY; ++k) {
            HIP_TRY(hipStreamSynchronize(d->copy_stream[k]));
            d->up_seq_done[k] = d->up_seq_next[k] - 1;
        }
        return LM_OK;
    }
    if ((rc = check_slots(d, slot, 1))) return rc;
    return wait_slot_upload(d, d->slots[slot]);
}

int lm_host_alloc(size_t bytes, void** out) {
    if (!out || !bytes) return fail(LM_ERR_INVALID, "bad argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(LM_ERR_NO_DEVICE, "no HIP device available: pinned host memory needs the HIP runtime");
    PinnedBuf<u8> b;
    HIP_TRY(b.alloc(bytes));
    *out = b.release();      // the caller's from here on (lm_host_free), and counted live until then
    {
        std::lock_guard<std::mutex> g(g_pinned_mu);
        g_pinned.push_back({reinterpret_cast<const u8*>(*out), bytes});
    }
    return LM_OK;
}

void lm_host_free(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_pinned_mu);
        for (size_t i = 0; i < g_pinned.size(); ++i)
            if (g_pinned[i].p == p) { g_pinned.erase(g_pinned.begin() + (long)i); break; }
    }
    PinnedBuf<u8>(static_cast<u8*>(p)).reset();
}

int lm_set_stage_chunks(lm_detector* d, int chunks) {
    if (!d || chunks < 1 || chunks > 64) return fail(LM_ERR_INVALID, "bad argument");
    d->stage_chunks = chunks;
    return LM_OK;
}

int lm_upload_match_mask(lm_detector* d, int slot, int modality, const uint8_t* mask, size_t stride) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, slot, 1))) return rc;
    return upload_match_mask(d, slot, modality, mask, stride);
}

}  // extern "C"
