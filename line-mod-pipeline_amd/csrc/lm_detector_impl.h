// lm_detector_impl.h -- what the sources of the detector's host side share: the detector's state (struct lm_detector, the opaque handle of
// include/linemod_hip.h), a frame slot's bookkeeping, the error channel of the C ABI and the internal functions one source calls in another.
//   lm_detector.hip         device state, bank upload, the per-batch launch sequence (a3-a15), lanes, create / templates / match.  Which kernels a3-a15
//                           launch, on which grids, is planned in lm_host.cpp (plan_preprocess; plan_layout / plan_scan / plan_match: host code,
//                           testable without a GPU); enqueue_preprocess and make_scan_args fill the planners' inputs, make sure of the resources a
//                           plan needs, bind the pointers and hand the plans to the executors (lm_k_preprocess.hip lmk_preprocess_run,
//                           lm_k_scan.hip lmk_scan_run, lm_k_refine.hip lmk_refine_run); the detector applies a plan's one side effect on host
//                           state itself (launch_scan: the lane's survivor counter set)
//   lm_detector_upload.hip  frames and masks into the slots from host memory: staging, copy streams and their tickets, lm_upload_* / lm_stage_* /
//                           lm_host_* / lm_read_frame / lm_device_*
//   lm_detector_ingest.hip  device-resident sources into the slots: lm_ingest_* through k_ingest; the depth registration (lm_set_registration,
//                           lm_ingest_frames_registered, lm_stage_register_depth); the lens rectification (lm_set_rectification,
//                           lm_ingest_frames_rectified, lm_stage_rectify); the area-averaged reduction (lm_set_reduction,
//                           lm_ingest_frames_reduced, lm_stage_reduce); both in one pass (lm_ingest_frames_rectified_reduced,
//                           lm_stage_rectify_reduce).  The descriptor check is host code of its own, testable without a
//                           GPU: lm_ingest_check.h / .cpp
//   lm_detector_export.hip  the slots' colour frames out again, primitives drawn, into device memory of the caller's: lm_export_frames through
//                           k_export.  The checks are host code of their own (lm_export_check.h / .cpp), the tile lists lm_host.cpp's plan_export
//   lm_detector_post.hip    f1: colour check (hulls, HSV masks) and the depth check's counts on the GPU
//   lm_detector_gather.hip  8e: RCCL communicator, the gathered match, the host side of the exchange (plans, merges)
//   lm_detector_io.hip      f2: bank / YAML persistence
//   lm_detector_debug.hip   stage hooks, timing calls, counters and statistics
//   lm_own.h                the four owners of HIP resources (DevBuf, PinnedBuf, Stream, Event): every device buffer, pinned buffer, stream and event
//                           of the structs below, of IcpState / GenState / EvalState and of the functions' temporaries is a member or a local of
//                           one of these types, created through it and released by its destructor.  No source of the detector calls a HIP
//                           create / free function; lm_destroy waits for the device and deletes the detector
// Internal names live in namespace lmd (external linkage between these sources, nothing of it is part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <memory>
#include <mutex>
#include <atomic>

#include "../../include/linemod_hip.h"
#include "lm_common.h"
#include "lm_extract.h"
#include <thread>

#include "lm_host.h"
#include "lm_yaml.h"
#include "lm_kernels.h"
#include "lm_comm.h"
#include "lm_own.h"

namespace lmd {

extern thread_local std::string g_err;           // what lm_last_error() returns on this thread (defined in lm_detector.hip)
int fail(int code, const std::string& msg);   // sets lm_last_error() of the calling thread and returns `code`

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(LM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the raw pipeline that changes nothing: black 0, gains 1024, the matrix 1024 * I, tone[i] = i >> 4 (include/linemod_hip.h)
inline lm_raw_processing raw_identity() {
    lm_raw_processing p = {};
    for (int c = 0; c < 3; ++c) { p.gain[c] = 1024u; p.ccm[4 * c] = 1024; }
    for (int i = 0; i < 4096; ++i) p.tone[i] = (uint8_t)(i >> 4);
    return p;
}

#define LM_NCOPY 4
#define LM_NLANES 4      // lanes per detector (lm_match_begin / lm_match_end): HIP streams whose stages overlap

// What the lm_stage_rows calls of a slot brought (Slot::staged).  lm_stage_rows is the one entry point that runs on ANY thread, several at once
// for one slot (a pool fills disjoint row ranges), so a plain bool of the owner thread would be a data race: the calls OR their bit in,
// relaxed (the owner reads it in lm_upload_staged, behind whatever joined the pool's tasks).  Copyable, because a Slot lives in a vector.
struct StagedBits {
    enum { WITH_DEPTH = 1, WITHOUT_DEPTH = 2 };
    std::atomic<int> v{0};
    StagedBits() = default;
    StagedBits(const StagedBits& o) : v(o.v.load(std::memory_order_relaxed)) {}
    StagedBits& operator=(const StagedBits& o) { v.store(o.v.load(std::memory_order_relaxed), std::memory_order_relaxed); return *this; }
    void clear() { v.store(0, std::memory_order_relaxed); }
    void add(int bit) { v.fetch_or(bit, std::memory_order_relaxed); }
    int get() const { return v.load(std::memory_order_relaxed); }
};

struct Slot {
    PinnedBuf<u8> h_bgr;     // pinned upload staging
    PinnedBuf<u16> h_depth;
    bool has_frame = false;
    // The frame the slot holds came WITH a depth image: the slot's depth plane is that frame's.  Meaningful while
    // has_frame; always true then on an RGB-D detector, always false on a colour-only one without LM_FLAG_KEEP_DEPTH.
    //   writers: every upload and ingest form, on the owner thread, where it sets has_frame (upload_frame, lm_upload_staged,
    //            issue_run_ticket): true iff the call brought depth; a call that brings none leaves the plane's bytes alone.  The
    //            template calls that void has_frame (lm_add_template, lm_add_templates_rendered) clear it with it.
    //   readers: the depth consumers, before they enqueue or claim anything (slot_lacks_depth): lm_depth_counts_begin,
    //            lm_depth_select_begin, lm_icp_refine, lm_icp_refine_slots, lm_icp_verify, lm_read_frame's depth_out, and a match or
    //            lm_prepare_slot on a ruled slot whose rule has a depth gate (refuse_depthless_rules).
    bool has_depth = false;
    StagedBits staged;               // between lm_stage_reserve and lm_upload_staged: lm_stage_rows calls came with / without a depth image
    lmh::Layout layout = lmh::Layout::Responses;   // what the last pre-processing of the frame wrote for the scanned level (lmh::plan_layout)
    bool prepared = false;   // a3-a10 have run on the frame the slot holds with the LUTs / thresholds now in force (lm_match_prepared)
    // Uploads run on the detector's copy stream: ev_up is recorded behind the slot's H2D copies, up_seq is the
    // upload's ticket (0 = never uploaded through the copy stream).  Copies complete in ticket order.
    Event ev_up;
    Event ev_bgr;                    // recorded behind the colour image alone (RGB-D: the depth copy follows it)
    unsigned long long up_seq = 0;
    int up_stream = 0;               // which copy stream carried the upload (tickets are per stream)
    bool mask_ready = false;         // the slot's colour bit mask holds inRange(HSV(frame), mask_lo, mask_hi) of the frame the slot holds (lm_color_mask_prepare)
    int mask_lane = -1;              // ... written on that lane's stream (its mask_done event orders a later colour check behind the launch)
    int mask_lo[3] = {0, 0, 0}, mask_hi[3] = {0, 0, 0};
    bool staging_open = false;       // lm_stage_reserve has run: lm_stage_rows may fill the staging buffers, lm_upload_staged sends them
    bool matched = false;            // a match on the frame the slot holds has completed: its lists are still in the slot's result block (lm_match_collect)
    // Detector::match's per-modality masks (lm_upload_match_mask; NOT the colour check's mask_* above): [modality][height][match_mask_pitch]
    // bytes, allocated on the slot's first mask upload.  They belong to the frame the slot holds: every frame upload clears match_mask_on.
    //   writer: lm_upload_match_mask -- a copy from h_match_mask (pinned, the masks' own staging) on the copy stream of the slot's last
    //           upload, under a new upload ticket (up_seq / ev_up): every lane's wait_uploads orders its k_match_mask behind it; the
    //           single-frame lm_match_masked copies on the compute stream itself, in order with the kernels.
    //   reader: k_match_mask (enqueue_preprocess), on the stream of the match that pre-processes the slot.  A mask upload to a slot a lane
    //           in flight, a colour check or depth counts reads is refused; the next upload waits for the ticket before h_match_mask is refilled.
    DevBuf<u8> d_match_mask;
    PinnedBuf<u8> h_match_mask;
    bool match_mask_on[2] = {false, false};
    // The slot's mask rule (lm_set_mask_rule) and its plane, [height][match_mask_pitch] bytes, allocated when the slot's first rule is
    // set.  The rule belongs to the SLOT, not to the frame: uploads leave it alone, and every pre-processing fills the plane again.
    //   writer: k_mask_rule (enqueue_preprocess), on the stream of the match that pre-processes the slot, behind that stream's wait
    //           for the frame's upload.
    //   reader: k_match_mask's second pass (enqueue_match_masks), behind it on the same stream.  Nothing else touches the plane, and
    //           a slot belongs to one lane at a time, so the plane needs no event.  Setting or clearing the rule of a slot that a
    //           lane in flight, a colour check or depth counts reads is refused; the rule itself is host state.
    DevBuf<u8> d_rule_mask;
    bool rule_on = false;
    lm_mask_rule rule = {};          // as it was set (lm_get_mask_rule)
    LmRule rule_dev = {};            // what k_mask_rule takes: bounds rounded, the rectangle made explicit
};

struct IcpState;   // lm_detector_icp.hip
struct GenState;   // lm_detector_gen.hip
struct EvalState;  // lm_detector_eval.hip

}  // namespace lmd
using namespace lmd;

struct lm_detector {
    ~lm_detector();               // lm_detector.hip
    lm_config cfg;
    LmLevelGeom geom[LM_MAX_LEVELS];
    int lw[LM_MAX_LEVELS], lh[LM_MAX_LEVELS];
    u8 sim_lut[256];
    u8 normal_lut[8000];
    int lut_onehot = -1;          // cached: every NORMAL_LUT entry is 0 or one-hot (-1 = not evaluated)
    bool normal_lut_substitute = true;   // the built-in table (NOT OpenCV's normal_lut.i) is active: lm_set_normal_lut clears it
    lmh::Bank bank;

    // ---- device state
    bool dev_ready = false;
    bool dev_begun = false;       // ensure_device has selected the device: lm_destroy waits for it before the members below release
    // ---- multi-GPU exchange: a lane's gather buffers
    struct Gather {
        DevBuf<int> d_cnt; DevBuf<LmOutMatch> d_rec;                // this rank's packed lists (k_pack_lists)
        DevBuf<int> d_all_cnt; DevBuf<LmOutMatch> d_all_rec;        // all ranks', rank-major
        PinnedBuf<int> h_all_cnt; PinnedBuf<LmOutMatch> h_all_rec;  // pinned host copies
        bool active = false;                                        // the lane's match in flight ends with a gather
        u32 cap_lane = 0;
    };
    // A lane owns everything that belongs to one of the LM_NLANES streams whose matches overlap, lane 0 included: lanes[0] is the lane of
    // the calls that name none (lm_match*, the stage hooks and timing calls, template generation, lm_comm_max).  The functions that
    // enqueue or wait for a lane are handed the Lane; the detector keeps no notion of a "current" lane.
    struct Lane {
        Stream stream;                   // all four are created in ensure_device (creation order matters, see there).  Declared first: the
                                         // lane's other members, its communicator among them, are destroyed before the stream they work on
        Event ev[6];   // [0..4] stage boundaries, [5] behind the exchange
        DevBuf<int> d_raw_thr;
        PinnedBuf<int> h_raw_thr;
        float raw_thr_for = -1.0f;       // the threshold the lane's tables hold: two lanes with different thresholds do not re-upload each other's
        bool created = false, busy = false, timed = false;   // created: events and threshold tables exist (lane 0: ensure_device, 1..3: ensure_lane)
        Event ev_done;                   // recorded behind the last command of the lane's match in flight (lm_match_end waits for IT, see wait_lane_done)
        Event blocking_ev;                  // LM_FLAG_BLOCKING_SYNC: what wait_stream sleeps on
        Event mask_done;                    // behind the mask launch of lm_color_mask_prepare on the lane: a colour check that reuses the masks waits for it
        int first = 0, n = 0;
        std::vector<int> classes;                       // class list of the match in flight ({-1} = all classes)
        unsigned long long waited_seq[LM_NCOPY] = {};   // newest upload ticket per copy stream this lane's stream waits for
        DevBuf<unsigned long long> d_surv;              // k_scan1's survivor queue, allocated on the lane's first bit-plane scan
        int surv_set = 0;                               // which of the queue's two counter sets the lane's next scan launch uses (the other is zeroed behind it)
        u32* plan = nullptr;                            // the lane's slice of d_plan (k_refine_plan output)
        Gather gather;
        std::unique_ptr<LmComm> comm;                   // one communicator per lane: the lanes' collectives never wait for each other.  Declared last:
                                                        // it is destroyed first, before the gather buffers and the stream its collectives ran on
    };
    Lane lanes[LM_NLANES];
    // H2D copies of lm_upload_frame* go through their own stream so that the frames of step k + 1 travel while
    // the lanes compute step k; a lane's stream waits (hipStreamWaitEvent) for the newest upload among its slots.
    // LM_NCOPY copy streams (slot -> stream round-robin): one in-order stream moved 0.6-0.9 MB copies at 25.6 GB/s
    // (per-copy set-up of the DMA engine), several streams keep several engines busy.
    Stream copy_stream[LM_NCOPY];
    unsigned long long up_seq_next[LM_NCOPY], up_seq_done[LM_NCOPY];   // per stream: next ticket / newest ticket known landed
    int n_copy_streams = LM_NCOPY;
    int stage_chunks = 1;                                  // pageable source: pieces of the staging memcpy (each piece is its own
                                                           // async copy; measured: every extra hipMemcpyAsync costs more than the overlap wins)
    std::vector<Slot> slots;
    // lm_ingest_frames (device-resident sources, k_ingest): the descriptor table, one LmIngestDesc per SLOT, pinned (h_ingest) and on the
    // device (d_ingest), both allocated by the first ingest; ev_ingest_src is the event recorded on a caller's producer stream.
    //   h_ingest[slot]  writer: lm_ingest_frames on the owner thread, AFTER wait_slot_upload(slot) -- the slot's previous upload, an
    //                   earlier ingest's table copy included, has landed (every upload waits its slot's ticket out before it draws a
    //                   new one, so a slot's ticket always covers the last reader of its entry).
    //                   reader: the hipMemcpyAsync h_ingest -> d_ingest of entries [first, first + n) on the call's copy stream.
    //   d_ingest[slot]  writer: that copy.  reader: k_ingest, behind it on the same copy stream; the slot's ticket (ev_up) is recorded
    //                   behind the kernel, so the entry is rewritten only behind the same wait_slot_upload.
    //   the sources     writer: the caller (its producer stream).  reader: k_ingest.  Edge in: hipEventRecord(ev_ingest_src, producer) +
    //                   hipStreamWaitEvent(copy stream) in front of the table copy (no producer stream: the caller's word that they
    //                   are complete).  Edge out: the ticket -- lm_upload_wait on the host, lm_ingest_release on a stream.  The event
    //                   is re-recorded by the next call: a stream's wait holds the record it was enqueued behind.
    //   bgr(slot, 0), depth(slot)   writer: k_ingest on the copy stream.  readers: the lanes' a3-a10, k_mask_rule, the colour check, the
    //                   depth counts, the ICP -- each behind wait_uploads / the ticket, exactly as behind an H2D copy; a slot one of
    //                   them holds is refused by claim_slots before anything is enqueued.
    PinnedBuf<LmIngestDesc> h_ingest;
    DevBuf<LmIngestDesc> d_ingest;
    Event ev_ingest_src;
    // lm_set_registration (raw depth onto the colour camera, lm_k_register.hip).  reg / reg_rays are host state, set
    // while no lane is in flight and after every copy stream has drained; reg_rays_dirty: d_reg_rays does not hold reg_rays yet.
    //   d_reg_rays      writer: ensure_table (lm_ingest_frames_registered / lm_stage_register_depth on the owner thread), a
    //                   synchronous copy behind hipDeviceSynchronize, only when dirty.  readers: k_register_scatter on a copy stream.
    //   d_reg_z[cs]     the z-buffer of copy stream cs, n * width * height u32 for the largest call so far on that stream.  writer:
    //                   the memset to the sentinel and k_register_scatter; reader: k_register_resolve -- all three on copy stream cs
    //                   and on no other stream, in that order, in every call: a call re-arms the buffer behind the previous call's
    //                   resolve.  It grows behind hipStreamSynchronize(copy stream cs).
    bool reg_on = false, reg_rays_dirty = false;
    lm_registration_desc reg = {};      // (reg.rays is not kept: the table is reg_rays)
    std::vector<float> reg_rays;
    DevBuf<float> d_reg_rays;
    DevBuf<u32> d_reg_z[LM_NCOPY];
    // lm_set_rectification (lens rectification at ingest, lm_k_rectify.hip).  rect / rect_map are host state, set while
    // no lane is in flight and after every copy stream has drained; rect_map_dirty: d_rect_map does not hold rect_map yet.
    //   d_rect_map      writer: ensure_table (lm_ingest_frames_rectified / lm_stage_rectify on the owner thread), a synchronous
    //                   copy behind hipDeviceSynchronize, only when dirty.  readers: k_rectify* / k_rectify_reduce* on a copy stream.
    bool rect_on = false, rect_map_dirty = false;
    lm_rectification_desc rect = {};    // (rect.map is not kept: the table is rect_map)
    std::vector<int32_t> rect_map;      // (qx, qy) per ideal pixel
    DevBuf<int32_t> d_rect_map;
    // lm_set_raw_processing (the raw pipeline of the raw colour formats, lm_ingest_raw.h).  raw holds ONE element, the
    // pipeline in force (the identity while raw_on is false); host state, set while no lane is in flight and after every copy stream has
    // drained; raw_dirty: d_raw does not hold it yet.  raw_on: a pipeline is set -- the 8-bit Bayer formats go through it too.
    //   d_raw           writer: ensure_table (the first ingest or stage call with a raw frame, on the owner thread), a synchronous copy
    //                   behind hipDeviceSynchronize, only when dirty.  readers: k_ingest_raw / k_rectify_raw on a copy stream.
    bool raw_on = false, raw_dirty = true;
    std::vector<lm_raw_processing> raw = std::vector<lm_raw_processing>(1, lmd::raw_identity());
    DevBuf<lm_raw_processing> d_raw;
    // lm_set_reduction (area-averaged reduction at ingest, lm_k_reduce.hip): host state alone, in lowest terms, set
    // while no lane is in flight and after every copy stream has drained.  It travels in the kernel's arguments: no device table.
    bool red_on = false;
    lm_reduction_desc red = {};
    // LM_TUNE_RECTIFY_REDUCE_GRID: the grid order of k_rectify_reduce (lm_k_rectify_reduce.hip; DESIGN.md section 19 has both measured)
    int rectify_reduce_grid = 0;
    // frame arena: [slot][bgr[l] | depth | quant[l][m] | lm[l]]
    DevBuf<u8> frame_arena;
    size_t frame_stride = 0;
    size_t off_bgr[LM_MAX_LEVELS] = {}, off_depth = 0, off_quant[LM_MAX_LEVELS][2] = {}, off_lm[LM_MAX_LEVELS] = {};
    // colour-quantisation scratch S | qn: one region for level 0, one (sized for level 1) shared by the levels above,
    // and the rank-code image of the depth passes -- disjoint, so independent kernels of one dependency level may run in one launch (k_phase)
    size_t off_cscratch = 0, off_cscratch1 = 0, off_dscratch = 0;
    // ---- f1 colour check on the GPU: hulls of every template, HSV division tables, per-slot colour bit mask
    bool hulls_dirty = true;
    DevBuf<u32> d_hull_class_base, d_hull_off; DevBuf<int16_t> d_hull_xy;
    DevBuf<int> d_hsv_div;
    size_t off_cmask = 0; int cmask_wpr = 0;
    size_t match_mask_pitch = 0;        // row pitch of Slot::d_match_mask / h_match_mask (the width rounded up to 64 bytes)
    // r05: the colour check has its own (high-priority) stream and buffers, so that it runs beside the lanes: the post-processing of
    // batch k overlaps the match of batch k + 1 (HighLevelLineMOD::detectTemplatesBatchBegin / End)
    Stream cc_stream;
    DevBuf<u8> cc_dev; PinnedBuf<u8> cc_host; size_t cc_cap = 0;          // room for cc_cap matches: records | slot index | two counts
    size_t cc_pending = 0; bool cc_inflight = false;                      // lm_color_check_begin_slots enqueued a check of cc_pending matches
    DevBuf<u8> dc_dev; PinnedBuf<u8> dc_host; size_t dc_cap = 0;          // r06, lm_depth_counts_begin: room for dc_cap queries | two counts each
    size_t dc_pending = 0; bool dc_inflight = false;
    DevBuf<u8> ds_dev; PinnedBuf<u8> ds_host; size_t ds_cap = 0;          // lm_depth_select_begin: room for ds_cap queries | one value each
    size_t ds_pending = 0; bool ds_inflight = false; int ds_lo = 0, ds_hi = -1;
    int cc_lo = 0, cc_hi = -1, dc_lo = 0, dc_hi = -1;                   // slots a colour check / depth counts in flight read: no upload goes there
    // ICP refinement (lm_detector_icp.hip): resident model clouds, its stream and scratch; icp_span = the slots [lo, hi] an ICP call in
    // flight reads, lo << 32 | hi (-1: none; a single-slot call claims a span of one), refused to uploads like the slots of a colour check
    // in flight.  icp_batch_mb (LM_TUNE_ICP_BATCH_MB): the scratch budget of a chunk of queries
    lmd::IcpState* icp = nullptr;    // (these three are defined in their own files, which also delete them: free_icp / free_gen / free_eval, called by ~lm_detector)
    lmd::GenState* gen = nullptr;    // template-bank generation (lm_detector_gen.hip): resident render meshes and the chunk buffers
    lmd::EvalState* eval = nullptr;  // pose-error evaluation (lm_detector_eval.hip): its stream and scratch
    std::atomic<long long> icp_span{-1};
    int icp_batch_mb = 512;
    // lm_export_frames (lm_detector_export.hip): its stream, and one block for the call's tables -- the frames'
    // LmExportImage, the primitive records, the tile offsets and the index list -- pinned (ex_host) and on the device (ex_dev), sent in one
    // copy.  export_span = the slots [lo, hi] the export in flight reads, as icp_span: refused to uploads from other threads
    // (refuse_checked_slots), one call at a time; only the call that holds the span touches the three members.
    Stream ex_stream;
    PinnedBuf<u8> ex_host;
    DevBuf<u8> ex_dev;
    std::atomic<long long> export_span{-1};
    Event ds_done;                                                        // behind the depth selection's last copy
    Event cc_done, dc_done;                                               // behind the colour check's / the depth counts' last copy: their `end` waits for the event, not the stream
    int comm_recs_per_frame = 0;
    DevBuf<double> d_red;      // small device buffer of lm_comm_max / lm_comm_barrier
    int batch_phases = 2;            // calls of 16+ frames run a3-a10 as launches of level-fused batch kernels (lm_host.cpp plan_batch_phases):
                                     // 0 never, 1 always, 2 (default) when no other lane has work in flight -- measured r03: alone on the
                                     // chip the fused launches win (config 2: 4.81 -> 4.66, config 3: 8.54 -> 8.06 us per frame), beside two
                                     // other lanes the separate launches interleave better (config 2: 145 K against 140 K detections/s)
    int scan_list_order = 3;         // LM_TUNE_SCAN_LIST_ORDER (lm_host.h build_device_bank)
    int sort_split_mode = 2;         // device sort: 0 one workgroup per frame (r03), 1 always the split form (chunk workgroups + merge launch),
                                     // 2 (default) the split form while the recently collected lists were longer than LM_SORT_CHUNK keys
    int sort_long_score = 0;         // see note_sort_length
    int work_weight_by_pixels = 1;   // r04: the selection below counts a frame as level-0 pixels / (640 x 480) frames (LM_TUNE_WORK_WEIGHT = 0: by frame count, r03)
    int phase_max_slots = 15;        // calls of up to this many frames run a3-a10 as one launch per dependency level (LmPhaseArgs)
    // aux arena: [slot][LmDevHeader | cand | keys | out]
    DevBuf<u8> aux_arena;
    size_t aux_stride = 0;
    size_t off_hdr = 0, off_cand = 0, off_keys = 0, off_out = 0;
    // host-mapped result blocks
    PinnedBuf<u8> host_blocks;
    size_t host_stride = 0;
    DevBuf<u32> d_plan;           // k_refine_plan output, one per lane (Lane::plan): [8][cap] slots + [8] lengths + [8][cap + 1] running sums + [8][cap] first entries
    int plan_stride_cap = 0;
    DevBuf<u64> d_resp_tab;       // 256 responses, then (32 more words) the miss masks of the 256 spread bytes
    int miss_delta = 1;           // 4 - the largest response below 4 of the similarity table (ensure_luts; upstream's table: a neighbouring orientation scores 3)
    DevBuf<u32> d_sim_lut;
    DevBuf<u8> d_normal_lut;
    bool luts_dirty = true;
    // ---- device bank
    bool bank_dirty = true;
    lmh::DeviceBankHost hb;
    DevBuf<u32> d_item_t, d_item_chunk;
    DevBuf<u32> d_scan_off; DevBuf<int> d_scan_P, d_scan_n;
    DevBuf<int> d_t_global, d_t_class;
    // bit-plane scan (k_scan1): the concatenated offset lists, and the work items of the lane counts used so far
    DevBuf<u32> d_off1, d_offn;
    struct Items1 { int L = 0; DevBuf<u32> d_t, d_chunk; std::vector<int> begin; };
    std::vector<Items1> items1;
    int scan_form = 0;               // LM_TUNE_SCAN_FORM: 0 = by cost (default), 1 = always the nibble scan k_scan4, 2 = the bit-plane scan k_scan1 whenever the level has planes,
                                     //    3 = the bit-plane scan with the planes in LDS (k_scanl) wherever a frame's planes fit (k_scan1 where they do not)
    float scan1_min_threshold = 50.0f;   // below this similarity threshold the miss bound keeps too many positions alive: k_scan4 (LM_TUNE_SCAN1_MIN_THRESHOLD)
    long long cnt_scan1_launches = 0; int last_scan1_lanes = 0;
    DevBuf<u32> d_offs3;             // [nt][fpad1] orientation << 29 | spread-memory offset of the bit-plane scan's features
    // r06, the bit-plane scan with a frame's planes in LDS (k_scanl; hb.lds_ok): the lists in the LDS image's layout and the lane items
    DevBuf<u32> d_offl, d_offsl, d_litem;
    DevBuf<unsigned long long> d_refine_stat;        // LM_REFINE_STAT=1: k_refine's counting experiment (printed by lm_destroy)
    int scanl_min_slots = 24;        // by cost (LM_TUNE_SCAN_FORM 0) from this many frames per call (measured: 16 frames 35.5 us against k_scan4's 35.3, 32 frames 43.4 against 57.5)
    int scanl_R = 0;                 // LM_SCANL_R at lm_create (experiments: k_scanl's shares per frame; 0 = unset)
    bool scanl_lds = false;          // the device took k_scanl's dynamic-LDS size (ensure_device): without it k_scanl is never planned
    u32 surv_cap = 1u << 20;         // entries of a lane's survivor queue (Lane::d_surv)
    DevBuf<LmRefMeta> d_ref_meta[LM_MAX_LEVELS];
    DevBuf<LmRefFeat> d_ref_feat[LM_MAX_LEVELS];
    // scratch for stage hooks
    DevBuf<u8> d_scratch;            // (ensure_scratch; its size() is the bytes it holds)
    u32 max_cand = 0, max_match = 0;
    int scan_variant = 0;
    bool scan_stats = false;                        // lm_set_scan_stats: the scan counts the features it loads
    DevBuf<unsigned long long> d_scan_stat;         // [1024][4]: features loaded per wave, features of an exhaustive scan, lane-loads issued
    // live profile of lm_match* (lm_set_profiling): per-stage HIP-event time, scan launches and bytes
    bool profiling = false;
    double prof_us[4] = {0, 0, 0, 0};
    double prof_scan_bytes = 0;
    long long prof_launches = 0, prof_frames = 0;
    long long prof_exch_fallbacks = 0;                           // lane-steps that needed the sized second exchange
    double prof_exch_us = 0; long long prof_exch_launches = 0;   // pack + 2 x all-gather + D2H of the gathered path (ev[4] -> ev[5])
    long long cnt_preprocess_frames = 0, cnt_scan_launches = 0, cnt_refine_launches = 0, cnt_sort_launches = 0;   // lm_get_stage_counts

    u8* bgr(int slot, int l) const { return frame_arena + (size_t)slot * frame_stride + off_bgr[l]; }
    u16* depth(int slot) const { return reinterpret_cast<u16*>(frame_arena + (size_t)slot * frame_stride + off_depth); }
    u8* quant(int slot, int l, int m) const { return frame_arena + (size_t)slot * frame_stride + off_quant[l][m]; }
    u8* lm(int slot, int l) const { return frame_arena + (size_t)slot * frame_stride + off_lm[l]; }
    u8* cscratch(int slot, int l = 0) const { return frame_arena + (size_t)slot * frame_stride + (l == 0 ? off_cscratch : off_cscratch1); }
    u8* dscratch(int slot) const { return frame_arena + (size_t)slot * frame_stride + off_dscratch; }
    u8* aux(int slot, size_t off) const { return aux_arena + (size_t)slot * aux_stride + off; }
    LmHostBlock* host_block(int slot) const { return reinterpret_cast<LmHostBlock*>(host_blocks + (size_t)slot * host_stride); }
};

namespace lmd {

struct ItemRange { int lo, n; int t_lo, t_hi; };   // items of the nibble / byte scan, and the bank-local templates they belong to


// The device sort's split form pays for lists longer than one chunk, and a launch lasts as long as its longest list: the score says
// whether any of the last 4096 collected frames had such a list.
inline void note_sort_length(lm_detector* d, u32 match_count) {
    const int is_long = match_count > LM_SORT_CHUNK && match_count <= LM_SORT_CAP;
    d->sort_long_score = is_long ? 4096 : std::max(d->sort_long_score - 1, 0);
}

// "Is there a depth plane": an RGB-D detector, or a colour-only one created with LM_FLAG_KEEP_DEPTH.  NOT "is depth a modality"
// (cfg.num_modalities == 2: quantised planes, linear memories, the depth masks, bit 1 of a rule's modalities, extraction, YAML, the bank).
inline bool keeps_depth(const lm_detector* d) { return lmc::keeps_depth(d->cfg); }
// the detector keeps depth, but the depth image of a frame is optional (the colour-only detector with the flag)
inline bool depth_optional(const lm_detector* d) { return d->cfg.num_modalities < 2 && keeps_depth(d); }

// defined in lm_detector.hip
int slot_lacks_depth(const lm_detector* d, int slot);              // LM_OK, or LM_ERR_INVALID naming the slot: its frame came without a depth image
int refuse_depthless_rules(const lm_detector* d, int first, int n, bool depth_coming = false);   // ... for the ruled slots of the range whose rule has a depth gate
bool any_lane_busy(const lm_detector* d);
int ensure_device(lm_detector* d);
int ensure_luts(lm_detector* d);
int ensure_bank(lm_detector* d);
int check_slots(lm_detector* d, int first, int n);
int refuse_checked_slots(const lm_detector* d, int first, int n);   // LM_ERR_INVALID: a colour check, depth counts, an ICP refinement or an export in flight reads one of the slots
bool normal_lut_onehot(lm_detector* d);
void enqueue_depth_pyramid(lm_detector* d, lm_detector::Lane& ln, int first, int n);
void enqueue_template_quantize(lm_detector* d, int first, int n, size_t slot_stride, float* const* mag);   // lm_add_template's a3-a5 over slots [first, first + n), keeping the magnitudes
void enqueue_preprocess(lm_detector* d, lm_detector::Lane& ln, int first, int n);
bool any_match_mask(const lm_detector* d, int first, int n);
int ensure_hsv_div(lm_detector* d);
int hsv_bound(double b);
int check_mask_rule(const lm_detector* d, const lm_mask_rule* rule, LmRule* out);
int item_range(lm_detector* d, int class_idx, ItemRange* r);
int make_scan_args(lm_detector* d, lm_detector::Lane& ln, int first, ItemRange r, int nslots, int variant, lmh::MatchPlan* plan, LmScanArgs* out);
void launch_scan(lm_detector::Lane& ln, const lmh::MatchPlan& plan, LmScanArgs& a);
inline int scan_form_code(const LmScanArgs& a) { return a.lds_form ? 1000 + a.R : a.L1; }   // lm_get_scan_form_stats out[3]
int enqueue_threshold(lm_detector::Lane& ln, float threshold);
int enqueue_upload_wait(lm_detector* d, lm_detector::Lane& ln, int first, int n);
int enqueue_match(lm_detector* d, lm_detector::Lane& ln, int first, int n, float threshold, std::vector<int>& classes, bool timed = false, bool prepared = false);
int enqueue_match(lm_detector* d, lm_detector::Lane& ln, int first, int n, float threshold, int class_idx, bool timed = false);
int collect_slot(lm_detector* d, int slot, lm_match_t* out, size_t cap, size_t* n_out);
int ready_for_compute(lm_detector* d);
int ensure_scratch(lm_detector* d, size_t bytes);
int ensure_lane(lm_detector* d, int l);
void account_profile(lm_detector* d, const lm_detector::Lane& ln, int n, const std::vector<int>& classes, bool gathered = false);
int wait_stream(lm_detector* d, lm_detector::Lane& ln);
int wait_lane_done(lm_detector* d, lm_detector::Lane& ln);
// defined in lm_detector_upload.hip
bool lane_holds_slots(const lm_detector* d, int first, int n);      // a lane's match in flight holds one of slots [first, first + n)
int claim_slots(const lm_detector* d, int first, int n);            // LM_ERR_INVALID unless the slots may be written: no lane holds them, nothing in flight reads them
void frame_replaced(Slot& s);                                       // the slot's frame is about to change: its a3-a10 results, lists, colour mask, staging and match masks are void
int issue_ticket(lm_detector* d, Slot& s, int cs, hipStream_t st);  // behind the slot's copies on copy stream cs: ev_up and the stream's next ticket
int issue_run_ticket(lm_detector* d, int first, int n, int cs, bool ev_bgr, bool has_depth);   // one ticket for slots [first, first + n), filled by one transfer or launch on copy stream cs
                                                                                // (lm_upload_frames_pinned, lm_detector_ingest.hip); each then holds a new frame
int check_frame_source(const lm_detector* d, const uint8_t* bgr, size_t* bgr_stride, const uint16_t* depth, size_t* depth_stride);
int wait_slot_upload(lm_detector* d, Slot& s);
int wait_uploads(lm_detector* d, hipStream_t stream, int first, int n, unsigned long long* seqs);
struct UploadOpts {
    bool pinned = false;                   // the source is pinned host memory: no staging copy
    hipStream_t inline_stream = nullptr;   // the copies go on this stream, not on a copy stream (and the slot gets no ticket)
    int shift_x = 0, shift_y = 0;          // the frame translated by so many pixels, zeros shifted in
};
inline UploadOpts inline_on(hipStream_t st, bool pinned = false) { UploadOpts o; o.inline_stream = st; o.pinned = pinned; return o; }
int upload_frame(lm_detector* d, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride, UploadOpts o = UploadOpts());
int upload_match_mask(lm_detector* d, int slot, int modality, const uint8_t* mask, size_t stride, hipStream_t inline_stream = nullptr);
bool is_pinned_host(const void* p, size_t bytes);
// defined in lm_detector_icp.hip
void free_icp(lm_detector* d);
// defined in lm_detector_gen.hip
void free_gen(lm_detector* d);
// a resident render mesh (lm_set_render_mesh): LM_ERR_INVALID for a bad index or an empty one
int render_mesh(lm_detector* d, int mesh_idx, const float** xyz, int* nv, const u32** idx, int* ntri);
// defined in lm_detector_eval.hip
void free_eval(lm_detector* d);
// defined in lm_detector_gather.hip
void free_gather(lm_detector* d);
int enqueue_gather(lm_detector* d, lm_detector::Lane& ln, int first, int n);

}  // namespace lmd
