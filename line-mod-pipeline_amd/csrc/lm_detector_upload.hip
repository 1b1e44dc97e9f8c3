// lm_detector_upload.hip -- frames, match masks and staged rows on their way into the resident slots: pinned staging, the copy streams'
// upload tickets, the copy routines and the lm_upload_* / lm_stage_* / lm_host_* entry points, and frames whose source already lies in
// device memory in the producer's format (lm_ingest_*: one k_ingest launch under one ticket; lm_ingest_frames_registered: the raw depth
// image registered onto the colour camera behind it, lm_k_register.hip, and lm_set_registration; lm_ingest_frames_rectified: k_rectify in
// k_ingest's place, lm_k_rectify.hip, and lm_set_rectification).  An entry point checks its arguments, then
// claims the slots (claim_slots); only then does it touch a slot (frame_replaced) or the device, and it ends with the ticket (issue_ticket).
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
}

// The slot's copies on `st` (copy stream cs) are enqueued: ev_up behind them, and the ticket -- the stream's next one, or `seq` where
// several slots share the ticket of one transfer (lm_upload_frames_pinned).
int issue_ticket(Slot& s, int cs, hipStream_t st, unsigned long long seq) {
    HIP_TRY(hipEventRecord(s.ev_up, st));
    s.up_stream = cs; s.up_seq = seq;
    return LM_OK;
}
static unsigned long long draw_ticket(lm_detector* d, int cs) { return d->up_seq_next[cs]++; }
int issue_ticket(lm_detector* d, Slot& s, int cs, hipStream_t st) { return issue_ticket(s, cs, st, draw_ticket(d, cs)); }

// A frame's host images as an entry point was handed them: both present (depth: RGB-D detectors), stride 0 = dense rows.
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
    if (!s.h_depth && c.num_modalities == 2)
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
    const bool ticket = !o.inline_stream, rgbd = c.num_modalities == 2;
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
    s.has_frame = true;
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

// ---- lm_ingest_frames: what the caller handed over, checked and turned into what k_ingest reads
static const char* pix_name(int f) {
    static const char* const names[] = {"LM_PIX_BGR8", "LM_PIX_RGB8", "LM_PIX_BGRA8", "LM_PIX_RGBA8", "LM_PIX_BGR8_PLANAR", "LM_PIX_RGB8_PLANAR",
                                        "LM_PIX_DEPTH_U16", "LM_PIX_DEPTH_F32", "LM_PIX_GRAY8", "LM_PIX_NV12", "LM_PIX_NV21", "LM_PIX_YUY2",
                                        "LM_PIX_UYVY"};
    return names[f];
}

// One image of frame i -> out (*matrix: the coefficient row of a YUV colour image).  o: the frame's options, shifts already clamped.
static int check_ingest_image(const lm_config& c, const lm_image_desc& im, bool is_depth, int i, const lm_ingest_opts& o, LmIngestImage* out, int* matrix) {
    const std::string who = std::string(is_depth ? "depth" : "colour") + " image of frame " + std::to_string(i) + ": ";
    // the matrix and range flags belong to the YUV formats alone; with any other bit set, or on another format, the value names no format
    const int flags = im.format >= 0 ? im.format & (LM_PIX_YUV_BT709 | LM_PIX_YUV_FULL) : 0, format = im.format - flags;
    if (format < LM_PIX_BGR8 || format > LM_PIX_UYVY || (flags && format < LM_PIX_NV12))
        return fail(LM_ERR_INVALID, who + "unknown pixel format " + std::to_string(im.format));
    const bool depth_format = format == LM_PIX_DEPTH_U16 || format == LM_PIX_DEPTH_F32;
    if (depth_format != is_depth) return fail(LM_ERR_INVALID, who + pix_name(format) + (depth_format ? " is a depth format" : " is a colour format"));
    if (!im.data) return fail(LM_ERR_INVALID, who + "null data pointer");
    if (im.crop_x < 0 || im.crop_y < 0 || im.width < 0 || im.height < 0 || (long long)im.crop_x + c.width > im.width ||
        (long long)im.crop_y + c.height > im.height)
        return fail(LM_ERR_INVALID, who + "0 <= roi.x && roi.x + roi.width <= m.cols && 0 <= roi.y && roi.y + roi.height <= m.rows failed: window " +
                    std::to_string(c.width) + " x " + std::to_string(c.height) + " at (" + std::to_string(im.crop_x) + ", " + std::to_string(im.crop_y) +
                    ") in a " + std::to_string(im.width) + " x " + std::to_string(im.height) + " source");
    int kind, bpp;
    switch (format) {
    case LM_PIX_BGR8: case LM_PIX_RGB8: kind = LM_INGEST_PX3; bpp = 3; break;
    case LM_PIX_BGRA8: case LM_PIX_RGBA8: kind = LM_INGEST_PX4; bpp = 4; break;
    case LM_PIX_BGR8_PLANAR: case LM_PIX_RGB8_PLANAR: kind = LM_INGEST_PLANAR; bpp = 1; break;
    case LM_PIX_DEPTH_U16: kind = LM_INGEST_U16; bpp = 2; break;
    case LM_PIX_DEPTH_F32: kind = LM_INGEST_F32; bpp = 4; break;
    case LM_PIX_GRAY8: kind = LM_INGEST_GRAY8; bpp = 1; break;
    case LM_PIX_NV12: kind = LM_INGEST_NV12; bpp = 1; break;
    case LM_PIX_NV21: kind = LM_INGEST_NV21; bpp = 1; break;
    case LM_PIX_YUY2: kind = LM_INGEST_YUY2; bpp = 2; break;
    default: kind = LM_INGEST_UYVY; bpp = 2; break;
    }
    // a chroma sample covers two columns (and, 4:2:0, two rows): a source with half a pair at its edge has no chroma there
    const bool nv = kind == LM_INGEST_NV12 || kind == LM_INGEST_NV21, yuv422 = kind == LM_INGEST_YUY2 || kind == LM_INGEST_UYVY;
    if (nv && (im.width % 2 || im.height % 2))
        return fail(LM_ERR_INVALID, who + "width and height of a " + pix_name(format) + " source must be even");
    if (yuv422 && im.width % 2) return fail(LM_ERR_INVALID, who + "width of a " + pix_name(format) + " source must be even");
    const bool planes = kind == LM_INGEST_PLANAR || nv;
    if (im.row_stride < (long long)c.width * bpp) return fail(LM_ERR_INVALID, who + "row_stride smaller than a window row");
    if (planes && im.plane_stride <= 0) return fail(LM_ERR_INVALID, who + "plane_stride must be positive");
    if (is_depth) {
        const int al = kind == LM_INGEST_U16 ? 2 : 4;
        if (reinterpret_cast<uintptr_t>(im.data) % al || im.row_stride % al)
            return fail(LM_ERR_INVALID, who + "data and row_stride of a " + (al == 2 ? "u16" : "f32") + " source must be multiples of " + std::to_string(al));
        if (kind == LM_INGEST_F32 && !(std::isfinite(im.scale) && im.scale > 0.0f)) return fail(LM_ERR_INVALID, who + "scale must be finite and positive");
    }
    out->data = static_cast<const u8*>(im.data);
    out->row_stride = im.row_stride; out->plane_stride = planes ? im.plane_stride : 0;
    out->crop_x = im.crop_x; out->crop_y = im.crop_y;
    out->kind = kind; out->swap_rb = format == LM_PIX_RGB8 || format == LM_PIX_RGBA8 || format == LM_PIX_RGB8_PLANAR;
    out->scale = im.scale;
    if (matrix) *matrix = flags >> 8;
    // the fast path: every lane's span starts on a 16-byte boundary (lmi::spans_aligned).  A lane's first source column is
    // crop_x + x0 - shift_x, or crop_x + W - 16 - x0 + shift_x when mirrored, x0 a multiple of 16.
    const long long col0 = (long long)im.crop_x + (o.flip_x ? c.width - 16 + o.shift_x : -o.shift_x);
    out->aligned = lmi::spans_aligned(reinterpret_cast<uintptr_t>(im.data), im.row_stride, out->plane_stride, col0, bpp);
    return LM_OK;
}

static int ensure_ingest(lm_detector* d) {
    if (!d->h_ingest) HIP_TRY(d->h_ingest.alloc(d->slots.size()));
    if (!d->d_ingest) HIP_TRY(d->d_ingest.alloc(d->slots.size()));
    if (!d->ev_ingest_src) HIP_TRY(d->ev_ingest_src.create(hipEventDisableTiming));
    return LM_OK;
}

// ---- lm_ingest_frames_registered: the raw depth image of frame i, checked against the registration -> out (what k_register_scatter reads:
// crop_x, crop_y place the window in the COLOUR geometry)
static int check_raw_depth(const lm_detector* d, const lm_image_desc& im, int i, bool whole, LmIngestImage* out) {
    const lm_config& c = d->cfg;
    const lm_camera &dc = d->reg.depth, &cc = d->reg.colour;
    const std::string who = "raw depth image of frame " + std::to_string(i) + ": ";
    const int flags = im.format >= 0 ? im.format & (LM_PIX_YUV_BT709 | LM_PIX_YUV_FULL) : 0, format = im.format - flags;
    if (format < LM_PIX_BGR8 || format > LM_PIX_UYVY || (flags && format < LM_PIX_NV12))
        return fail(LM_ERR_INVALID, who + "unknown pixel format " + std::to_string(im.format));
    if (format != LM_PIX_DEPTH_U16 && format != LM_PIX_DEPTH_F32) return fail(LM_ERR_INVALID, who + pix_name(format) + " is a colour format");
    if (!im.data) return fail(LM_ERR_INVALID, who + "null data pointer");
    if (im.width != dc.width || im.height != dc.height)
        return fail(LM_ERR_INVALID, who + "a " + std::to_string(im.width) + " x " + std::to_string(im.height) + " image is not the registration's depth camera (" +
                    std::to_string(dc.width) + " x " + std::to_string(dc.height) + ")");
    if (!whole && (im.crop_x < 0 || im.crop_y < 0 || (long long)im.crop_x + c.width > cc.width || (long long)im.crop_y + c.height > cc.height))
        return fail(LM_ERR_INVALID, who + "window " + std::to_string(c.width) + " x " + std::to_string(c.height) + " at (" + std::to_string(im.crop_x) + ", " +
                    std::to_string(im.crop_y) + ") lies outside the " + std::to_string(cc.width) + " x " + std::to_string(cc.height) + " colour geometry");
    const bool f32 = format == LM_PIX_DEPTH_F32;
    const int al = f32 ? 4 : 2;
    if (im.row_stride < (long long)dc.width * al) return fail(LM_ERR_INVALID, who + "row_stride smaller than a raw row");
    if (reinterpret_cast<uintptr_t>(im.data) % al || im.row_stride % al)
        return fail(LM_ERR_INVALID, who + "data and row_stride of a " + (f32 ? "f32" : "u16") + " source must be multiples of " + std::to_string(al));
    if (f32 && !(std::isfinite(im.scale) && im.scale > 0.0f)) return fail(LM_ERR_INVALID, who + "scale must be finite and positive");
    *out = LmIngestImage();
    out->data = static_cast<const u8*>(im.data);
    out->row_stride = im.row_stride;
    out->crop_x = whole ? 0 : im.crop_x; out->crop_y = whole ? 0 : im.crop_y;
    out->kind = f32 ? LM_INGEST_F32 : LM_INGEST_U16;
    out->scale = im.scale;
    return LM_OK;
}

// the ray table on the device
static int ensure_registration(lm_detector* d) {
    if (!d->reg_rays_dirty) return LM_OK;
    HIP_TRY(hipDeviceSynchronize());        // (nothing in flight reads the table that is replaced)
    HIP_TRY(d->d_reg_rays.alloc(d->reg_rays.size()));
    HIP_TRY(hipMemcpy(d->d_reg_rays, d->reg_rays.data(), d->reg_rays.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    d->reg_rays_dirty = false;
    return LM_OK;
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

// ---- lm_ingest_frames_rectified: one source image of frame i, checked against the rectification -> out (what k_rectify reads: crop_x,
// crop_y place the window in the IDEAL geometry; `aligned`: a 4-byte pixel may be read as one dword).  whole: the stage hook, no window.
static int check_rect_image(const lm_detector* d, const lm_image_desc& im, bool is_depth, int i, bool whole, LmIngestImage* out, int* matrix) {
    const lm_config& c = d->cfg;
    const lm_camera &sc = d->rect.source, &ic = d->rect.ideal;
    const std::string who = std::string(is_depth ? "depth" : "colour") + " image of frame " + std::to_string(i) + ": ";
    const int flags = im.format >= 0 ? im.format & (LM_PIX_YUV_BT709 | LM_PIX_YUV_FULL) : 0, format = im.format - flags;
    if (format < LM_PIX_BGR8 || format > LM_PIX_UYVY || (flags && format < LM_PIX_NV12))
        return fail(LM_ERR_INVALID, who + "unknown pixel format " + std::to_string(im.format));
    const bool depth_format = format == LM_PIX_DEPTH_U16 || format == LM_PIX_DEPTH_F32;
    if (depth_format != is_depth) return fail(LM_ERR_INVALID, who + pix_name(format) + (depth_format ? " is a depth format" : " is a colour format"));
    if (!im.data) return fail(LM_ERR_INVALID, who + "null data pointer");
    if (im.width != sc.width || im.height != sc.height)
        return fail(LM_ERR_INVALID, "rectification: " + who + "a " + std::to_string(im.width) + " x " + std::to_string(im.height) + " image is not the source camera (" +
                    std::to_string(sc.width) + " x " + std::to_string(sc.height) + ")");
    if (!whole && (im.crop_x < 0 || im.crop_y < 0 || (long long)im.crop_x + c.width > ic.width || (long long)im.crop_y + c.height > ic.height))
        return fail(LM_ERR_INVALID, "rectification: " + who + "window " + std::to_string(c.width) + " x " + std::to_string(c.height) + " at (" + std::to_string(im.crop_x) +
                    ", " + std::to_string(im.crop_y) + ") lies outside the " + std::to_string(ic.width) + " x " + std::to_string(ic.height) + " ideal geometry");
    int kind, bpp;
    switch (format) {
    case LM_PIX_BGR8: case LM_PIX_RGB8: kind = LM_INGEST_PX3; bpp = 3; break;
    case LM_PIX_BGRA8: case LM_PIX_RGBA8: kind = LM_INGEST_PX4; bpp = 4; break;
    case LM_PIX_BGR8_PLANAR: case LM_PIX_RGB8_PLANAR: kind = LM_INGEST_PLANAR; bpp = 1; break;
    case LM_PIX_DEPTH_U16: kind = LM_INGEST_U16; bpp = 2; break;
    case LM_PIX_DEPTH_F32: kind = LM_INGEST_F32; bpp = 4; break;
    case LM_PIX_GRAY8: kind = LM_INGEST_GRAY8; bpp = 1; break;
    case LM_PIX_NV12: kind = LM_INGEST_NV12; bpp = 1; break;
    case LM_PIX_NV21: kind = LM_INGEST_NV21; bpp = 1; break;
    case LM_PIX_YUY2: kind = LM_INGEST_YUY2; bpp = 2; break;
    default: kind = LM_INGEST_UYVY; bpp = 2; break;
    }
    const bool nv = kind == LM_INGEST_NV12 || kind == LM_INGEST_NV21, yuv422 = kind == LM_INGEST_YUY2 || kind == LM_INGEST_UYVY;
    if (nv && (im.width % 2 || im.height % 2))
        return fail(LM_ERR_INVALID, who + "width and height of a " + pix_name(format) + " source must be even");
    if (yuv422 && im.width % 2) return fail(LM_ERR_INVALID, who + "width of a " + pix_name(format) + " source must be even");
    const bool planes = kind == LM_INGEST_PLANAR || nv;
    if (im.row_stride < (long long)sc.width * bpp) return fail(LM_ERR_INVALID, "rectification: " + who + "row_stride smaller than a source row");
    if (planes && im.plane_stride <= 0) return fail(LM_ERR_INVALID, who + "plane_stride must be positive");
    if (is_depth) {
        const int al = kind == LM_INGEST_U16 ? 2 : 4;
        if (reinterpret_cast<uintptr_t>(im.data) % al || im.row_stride % al)
            return fail(LM_ERR_INVALID, who + "data and row_stride of a " + (al == 2 ? "u16" : "f32") + " source must be multiples of " + std::to_string(al));
        if (kind == LM_INGEST_F32 && !(std::isfinite(im.scale) && im.scale > 0.0f)) return fail(LM_ERR_INVALID, who + "scale must be finite and positive");
    }
    *out = LmIngestImage();
    out->data = static_cast<const u8*>(im.data);
    out->row_stride = im.row_stride; out->plane_stride = planes ? im.plane_stride : 0;
    out->crop_x = whole ? 0 : im.crop_x; out->crop_y = whole ? 0 : im.crop_y;
    out->kind = kind; out->swap_rb = format == LM_PIX_RGB8 || format == LM_PIX_RGBA8 || format == LM_PIX_RGB8_PLANAR;
    out->scale = im.scale;
    out->aligned = kind == LM_INGEST_PX4 && reinterpret_cast<uintptr_t>(im.data) % 4 == 0 && im.row_stride % 4 == 0;
    if (matrix) *matrix = flags >> 8;
    return LM_OK;
}

// the map on the device
static int ensure_rectification(lm_detector* d) {
    if (!d->rect_map_dirty) return LM_OK;
    HIP_TRY(hipDeviceSynchronize());        // (nothing in flight reads the map that is replaced)
    HIP_TRY(d->d_rect_map.alloc(d->rect_map.size()));
    HIP_TRY(hipMemcpy(d->d_rect_map, d->rect_map.data(), d->rect_map.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    d->rect_map_dirty = false;
    return LM_OK;
}

static void fill_rectify_args(const lm_detector* d, LmRectifyArgs* a) {
    a->map = d->d_rect_map;
    a->mw = d->rect.ideal.width; a->mh = d->rect.ideal.height; a->sw = d->rect.source.width; a->sh = d->rect.source.height;
}

// lm_ingest_frames and lm_ingest_frames_registered (registered: `depth` holds the RAW depth images; k_ingest then takes the colour images
// alone and the depth planes are k_register_resolve's, behind it on the same stream and under the same ticket)
static int ingest_frames(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth, const lm_ingest_opts* opts,
                         void* producer_stream, bool registered, bool rectified = false) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    const lm_config& c = d->cfg;
    const bool rgbd = c.num_modalities == 2;
    // (rectified: lm_ingest_frames_rectified -- the colour images, and the depth images unless `registered`, go through k_rectify in
    // k_ingest's place; everything else of the call is the same)
    if (rectified && !d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    if (registered && !rgbd) return fail(LM_ERR_INVALID, "lm_ingest_frames_registered needs an RGB-D detector: a colour-only detector holds no depth frame");
    if (registered && !d->reg_on) return fail(LM_ERR_INVALID, "no registration set: lm_set_registration first");
    if (!colour || (rgbd && !depth) || n_slots <= 0) return fail(LM_ERR_INVALID, "bad argument");
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    if (c.width % 16) return fail(LM_ERR_INVALID, "lm_ingest_frames needs a frame width that is a multiple of 16");
    if (rectified && registered && (d->reg.colour.width != d->rect.ideal.width || d->reg.colour.height != d->rect.ideal.height))
        return fail(LM_ERR_INVALID, "rectification: the registration's colour camera (" + std::to_string(d->reg.colour.width) + " x " + std::to_string(d->reg.colour.height) +
                    ") is not the ideal camera (" + std::to_string(d->rect.ideal.width) + " x " + std::to_string(d->rect.ideal.height) + ")");
    // the descriptors, checked into a table of the call's own: the detector's pinned table is written only once the slots are claimed and
    // their earlier uploads have landed
    static thread_local std::vector<LmIngestDesc> table;
    table.resize((size_t)n_slots);
    int n_yuv = 0;      // frames whose colour image is grey or YUV: k_ingest_yuv's
    for (int i = 0; i < n_slots; ++i) {
        LmIngestDesc& e = table[(size_t)i];
        e = LmIngestDesc();
        lm_ingest_opts o = opts ? opts[i] : lm_ingest_opts{0, 0, 0};
        o.flip_x = o.flip_x != 0;
        o.shift_x = lmh::clamp_shift(o.shift_x, c.width); o.shift_y = lmh::clamp_shift(o.shift_y, c.height);     // (beyond: an all-zero frame either way)
        e.flip_x = o.flip_x; e.shift_x = o.shift_x; e.shift_y = o.shift_y;
        if (rectified) { if ((rc = check_rect_image(d, colour[i], false, i, false, &e.colour, &e.matrix))) return rc; }
        else if ((rc = check_ingest_image(c, colour[i], false, i, o, &e.colour, &e.matrix))) return rc;
        if (registered) { if ((rc = check_raw_depth(d, depth[i], i, false, &e.depth))) return rc; }
        else if (rgbd && rectified) { if ((rc = check_rect_image(d, depth[i], true, i, false, &e.depth, nullptr))) return rc; }
        else if (rgbd && (rc = check_ingest_image(c, depth[i], true, i, o, &e.depth, nullptr))) return rc;
        if (e.colour.kind >= LM_INGEST_GRAY8) ++n_yuv;
    }
    if ((rc = claim_slots(d, first_slot, n_slots))) return rc;
    for (int i = 0; i < n_slots; ++i) if ((rc = wait_slot_upload(d, d->slots[first_slot + i]))) return rc;
    if ((rc = ensure_ingest(d))) return rc;
    std::memcpy(d->h_ingest + first_slot, table.data(), (size_t)n_slots * sizeof(LmIngestDesc));
    const int cs = (first_slot / n_slots) % d->n_copy_streams;   // as lm_upload_frames_pinned: consecutive runs take turns on the copy streams
    hipStream_t st = d->copy_stream[cs];
    const size_t z_words = (size_t)n_slots * (size_t)c.width * (size_t)c.height;
    if (rectified && (rc = ensure_rectification(d))) return rc;
    if (registered) {
        if ((rc = ensure_registration(d))) return rc;
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
    a.first = first_slot; a.n = n_slots; a.w = c.width; a.h = c.height; a.rgbd = rgbd && !registered ? 1 : 0;
    a.n_rgb = n_slots - n_yuv; a.n_yuv = n_yuv;
    if (rectified) {
        LmRectifyArgs q;
        fill_rectify_args(d, &q);
        q.table = d->d_ingest; q.first = first_slot; q.n = n_slots; q.n_rgb = a.n_rgb; q.n_yuv = a.n_yuv; q.w = c.width; q.h = c.height;
        q.out_bgr = d->frame_arena + d->off_bgr[0]; q.out_depth = a.rgbd ? d->frame_arena + d->off_depth : nullptr; q.out_stride = d->frame_stride;
        lmk_rectify(st, q);
    } else lmk_ingest(st, a);
    HIP_TRY(hipGetLastError());
    if (registered) {
        LmRegisterArgs r;
        fill_register_args(d, &r);
        r.table = d->d_ingest; r.first = first_slot; r.n = n_slots; r.w = c.width; r.h = c.height;
        r.zbuf = d->d_reg_z[cs]; r.out = d->frame_arena + d->off_depth; r.out_stride = d->frame_stride;
        HIP_TRY(hipMemsetAsync(r.zbuf, 0xFF, z_words * sizeof(u32), st));      // re-armed on the ingest's own stream, behind the last call's resolve
        lmk_register(st, r);
        HIP_TRY(hipGetLastError());
    }
    const unsigned long long seq = draw_ticket(d, cs);      // one ticket for the whole launch
    for (int i = 0; i < n_slots; ++i) {
        Slot& s = d->slots[first_slot + i];
        if ((rc = issue_ticket(s, cs, st, seq))) return rc;
        frame_replaced(s);
        s.has_frame = true;
    }
    return LM_OK;
}

static bool camera_finite(const lm_camera& k) {
    for (float v : {k.fx, k.fy, k.cx, k.cy, k.k1, k.k2, k.p1, k.p2, k.k3}) if (!std::isfinite(v)) return false;
    return true;
}

}  // namespace lmd

extern "C" {

int lm_ingest_frames(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth, const lm_ingest_opts* opts,
                     void* producer_stream) {
    return ingest_frames(d, first_slot, n_slots, colour, depth, opts, producer_stream, false);
}

int lm_ingest_frames_registered(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth_raw,
                                const lm_ingest_opts* opts, void* producer_stream) {
    return ingest_frames(d, first_slot, n_slots, colour, depth_raw, opts, producer_stream, true);
}

int lm_set_registration(lm_detector* d, const lm_registration_desc* desc) {
    if (!d) return fail(LM_ERR_INVALID, "null detector");
    std::vector<float> rays;
    if (desc) {
        const lm_camera &dc = desc->depth, &cc = desc->colour;
        bool ok = camera_finite(dc) && camera_finite(cc);
        for (float v : desc->rotation) ok = ok && std::isfinite(v);
        for (float v : desc->translation) ok = ok && std::isfinite(v);
        if (!ok) return fail(LM_ERR_INVALID, "registration: every number must be finite");
        if (!(dc.fx > 0.0f && dc.fy > 0.0f && cc.fx > 0.0f && cc.fy > 0.0f)) return fail(LM_ERR_INVALID, "registration: fx and fy of both cameras must be positive");
        for (int v : {dc.width, dc.height, cc.width, cc.height})
            if (v < 1 || v > 16384) return fail(LM_ERR_INVALID, "registration: width and height of both cameras must lie in 1 .. 16384");
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
    if (any_lane_busy(d)) return fail(LM_ERR_INVALID, "a lane has a match in flight: call lm_match_end first");
    if (d->dev_ready) {     // an ingest on a copy stream may still read the registration that is replaced
        int rc;
        if ((rc = ensure_device(d))) return rc;
        if ((rc = lm_upload_wait(d, -1))) return rc;
    }
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
    if ((rc = check_raw_depth(d, *depth_raw, 0, true, &e.depth))) return rc;
    if ((rc = ensure_registration(d))) return rc;
    const int w = d->reg.colour.width, h = d->reg.colour.height;
    const size_t n = (size_t)w * (size_t)h;
    DevBuf<LmIngestDesc> d_e;
    DevBuf<u32> d_z;
    DevBuf<u16> d_out;
    HIP_TRY(d_e.alloc(1));
    HIP_TRY(d_z.alloc(n));
    HIP_TRY(d_out.alloc(n));
    hipStream_t st = d->copy_stream[0];
    HIP_TRY(hipMemcpyAsync(d_e, &e, sizeof(e), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      // (`e` is a local)
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
    if (desc) {
        const lm_camera &sc = desc->source, &ic = desc->ideal;
        if (!(camera_finite(sc) && camera_finite(ic))) return fail(LM_ERR_INVALID, "rectification: every camera number must be finite");
        if (!(sc.fx > 0.0f && sc.fy > 0.0f && ic.fx > 0.0f && ic.fy > 0.0f)) return fail(LM_ERR_INVALID, "rectification: fx and fy of both cameras must be positive");
        for (int v : {sc.width, sc.height, ic.width, ic.height})
            if (v < 1 || v > 16384) return fail(LM_ERR_INVALID, "rectification: width and height of both cameras must lie in 1 .. 16384");
        for (float v : {ic.k1, ic.k2, ic.p1, ic.p2, ic.k3})
            if (v != 0.0f) return fail(LM_ERR_INVALID, "rectification: the ideal camera's coefficients must be 0");
        const lmq::Cam s = {sc.fx, sc.fy, sc.cx, sc.cy, sc.k1, sc.k2, sc.p1, sc.p2, sc.k3, sc.width, sc.height};
        const lmq::Cam t = {ic.fx, ic.fy, ic.cx, ic.cy, 0.0, 0.0, 0.0, 0.0, 0.0, ic.width, ic.height};
        map.resize(2 * (size_t)ic.width * (size_t)ic.height);
        lmq::build_map(s, t, desc->map, map.data());
    }
    if (any_lane_busy(d)) return fail(LM_ERR_INVALID, "rectification: a lane has a match in flight: call lm_match_end first");
    if (d->dev_ready) {     // an ingest on a copy stream may still read the map that is replaced
        int rc;
        if ((rc = ensure_device(d))) return rc;
        if ((rc = lm_upload_wait(d, -1))) return rc;
    }
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

int lm_ingest_frames_rectified(lm_detector* d, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                               const lm_ingest_opts* opts, int depth_route, void* producer_stream) {
    if (depth_route != LM_RECTIFY_DEPTH_ALIGNED && depth_route != LM_RECTIFY_DEPTH_REGISTERED) {
        int rc;
        if ((rc = ready_for_compute(d))) return rc;
        return fail(LM_ERR_INVALID, "rectification: unknown depth_route " + std::to_string(depth_route));
    }
    return ingest_frames(d, first_slot, n_slots, colour, depth, opts, producer_stream, depth_route == LM_RECTIFY_DEPTH_REGISTERED, true);
}

int lm_stage_rectify(lm_detector* d, const lm_image_desc* colour, const lm_image_desc* depth, uint8_t* bgr_out_host, uint16_t* depth_out_host) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    const bool do_c = colour && bgr_out_host, do_d = depth && depth_out_host;
    if ((!do_c && !do_d) || (colour != nullptr) != (bgr_out_host != nullptr) || (depth != nullptr) != (depth_out_host != nullptr))
        return fail(LM_ERR_INVALID, "bad argument");
    if (!d->rect_on) return fail(LM_ERR_INVALID, "rectification: no rectification set: lm_set_rectification first");
    LmIngestDesc e = LmIngestDesc();
    if (do_c && (rc = check_rect_image(d, *colour, false, 0, true, &e.colour, &e.matrix))) return rc;
    if (do_d && (rc = check_rect_image(d, *depth, true, 0, true, &e.depth, nullptr))) return rc;
    if ((rc = ensure_rectification(d))) return rc;
    const int w = d->rect.ideal.width, h = d->rect.ideal.height;
    const size_t n = (size_t)w * (size_t)h;
    DevBuf<LmIngestDesc> d_e;
    DevBuf<u8> d_bgr;
    DevBuf<u16> d_depth;
    HIP_TRY(d_e.alloc(1));
    if (do_c) HIP_TRY(d_bgr.alloc(n * 3));
    if (do_d) HIP_TRY(d_depth.alloc(n));
    hipStream_t st = d->copy_stream[0];
    HIP_TRY(hipMemcpyAsync(d_e, &e, sizeof(e), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      // (`e` is a local)
    LmRectifyArgs q;
    fill_rectify_args(d, &q);
    const bool yuv = do_c && e.colour.kind >= LM_INGEST_GRAY8;
    q.table = d_e; q.first = 0; q.n = 1; q.n_rgb = yuv ? 0 : 1; q.n_yuv = yuv ? 1 : 0; q.w = w; q.h = h;
    q.out_bgr = do_c ? d_bgr.get() : nullptr; q.out_depth = do_d ? reinterpret_cast<u8*>(d_depth.get()) : nullptr; q.out_stride = 0;
    lmk_rectify(st, q);
    HIP_TRY(hipGetLastError());
    if (do_c) HIP_TRY(hipMemcpyAsync(bgr_out_host, d_bgr, n * 3, hipMemcpyDeviceToHost, st));
    if (do_d) HIP_TRY(hipMemcpyAsync(depth_out_host, d_depth, n * sizeof(u16), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LM_OK;
}

int lm_ingest_release(lm_detector* d, int first_slot, int n_slots, void* stream) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if (n_slots <= 0) return fail(LM_ERR_INVALID, "bad argument");
    if ((rc = check_slots(d, first_slot, n_slots))) return rc;
    return wait_uploads(d, static_cast<hipStream_t>(stream), first_slot, n_slots, nullptr);
}

int lm_read_frame(lm_detector* d, int slot, uint8_t* bgr_out, uint16_t* depth_out) {
    int rc;
    if ((rc = ready_for_compute(d))) return rc;
    if ((rc = check_slots(d, slot, 1))) return rc;
    const lm_config& c = d->cfg;
    Slot& s = d->slots[slot];
    if (!s.has_frame) return fail(LM_ERR_INVALID, "no frame uploaded to slot " + std::to_string(slot));
    if (depth_out && c.num_modalities < 2) return fail(LM_ERR_INVALID, "a colour-only detector holds no depth frame");
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
    const size_t fb = (size_t)c.width * c.height * (c.num_modalities == 2 ? 5 : 3);
    if (frame_stride == 0) frame_stride = fb;
    if (frame_stride < fb) return fail(LM_ERR_INVALID, "frame stride smaller than a frame");
    if ((rc = claim_slots(d, first_slot, n_slots))) return rc;
    for (int i = 0; i < n_slots; ++i) if ((rc = wait_slot_upload(d, d->slots[first_slot + i]))) return rc;
    // one strided transfer: row i = host frame i ([colour | depth] dense), destination pitch = the arena's slot stride
    const int cs = (first_slot / n_slots) % d->n_copy_streams;   // consecutive runs of n_slots slots take turns on the copy streams
    hipStream_t st = d->copy_stream[cs];
    HIP_TRY(hipMemcpy2DAsync(d->bgr(first_slot, 0), d->frame_stride, frames, frame_stride, fb, (size_t)n_slots, hipMemcpyHostToDevice, st));
    const unsigned long long seq = draw_ticket(d, cs);      // one ticket for the whole transfer
    for (int i = 0; i < n_slots; ++i) {
        Slot& s = d->slots[first_slot + i];
        if (c.num_modalities == 2) HIP_TRY(hipEventRecord(s.ev_bgr, st));
        if ((rc = issue_ticket(s, cs, st, seq))) return rc;
        frame_replaced(s);
        s.has_frame = true;
    }
    return LM_OK;
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
        s.staging_open = true;
    }
    return LM_OK;
}

int lm_stage_rows(lm_detector* d, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                  int shift_x, int shift_y, int row0, int row1) {
    if (!d || !d->dev_ready) return fail(LM_ERR_INVALID, "lm_stage_reserve first");
    if (slot < 0 || slot >= (int)d->slots.size()) return fail(LM_ERR_INVALID, "slot out of range");
    const lm_config& c = d->cfg;
    const Slot& s = d->slots[slot];
    if (!s.staging_open || !s.h_bgr) return fail(LM_ERR_INVALID, "lm_stage_reserve first");
    if (int rc = check_frame_source(d, bgr, &bgr_stride, depth, &depth_stride)) return rc;
    if (row0 < 0 || row1 > c.height || row0 > row1) return fail(LM_ERR_INVALID, "row range outside the frame");
    const int ox = lmh::clamp_shift(shift_x, c.width), oy = lmh::clamp_shift(shift_y, c.height);
    lmh::stage_rows_shifted(s.h_bgr, bgr, bgr_stride, c.width, c.height, 3, ox, oy, row0, row1);
    if (c.num_modalities == 2)
        lmh::stage_rows_shifted(reinterpret_cast<u8*>(s.h_depth.get()), reinterpret_cast<const u8*>(depth), depth_stride, c.width, c.height, 2, ox, oy, row0, row1);
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
    const int cs = slot % d->n_copy_streams;
    hipStream_t st = d->copy_stream[cs];
    frame_replaced(s);
    HIP_TRY(hipMemcpyAsync(d->bgr(slot, 0), s.h_bgr, (size_t)c.width * c.height * 3, hipMemcpyHostToDevice, st));
    if (c.num_modalities == 2) {
        HIP_TRY(hipEventRecord(s.ev_bgr, st));
        HIP_TRY(hipMemcpyAsync(d->depth(slot), s.h_depth, (size_t)c.width * c.height * 2, hipMemcpyHostToDevice, st));
    }
    if ((rc = issue_ticket(d, s, cs, st))) return rc;
    s.has_frame = true;
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
