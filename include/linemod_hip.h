/*
 * linemod_hip.h -- C ABI of the MI355X-native LINE-MOD detector (liblinemod_hip.so).
 *
 * Drop-in boundary: this library replaces the object the reference holds as
 *     cv::Ptr<cv::linemod::Detector> detector;      /root/reference/include/HighLevelLinemod.h:102
 * Every entry point below names the cv::linemod::Detector call of the reference it stands in for
 * (complete list of calls crossing that seam: SURVEY.md section 8b).  Plain C types only: opaque
 * handle, caller-owned buffers with explicit strides/capacities, int status (0 = LM_OK), no
 * exceptions across the ABI; lm_last_error() returns the text of the last failure on the calling
 * thread.  All compute runs in hand-written HIP kernels for gfx950; there is NO CPU fallback --
 * every compute entry point fails with LM_ERR_NO_DEVICE when no HIP device is usable.
 *
 * Image formats (SURVEY.md 8b "Conventions"): colour = 8-bit BGR interleaved (CV_8UC3 as
 * delivered by cv::VideoCapture, detector.cpp:24), depth = uint16 millimetres (CV_16UC1,
 * detector.cpp:25-26).  Strides are in bytes.
 */
#ifndef LINEMOD_HIP_H
#define LINEMOD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LM_MAX_LEVELS 4
#define LM_MAX_FEATURES 63 /* upstream CV_Assert(features.size() <= 63): 63*4 = 252 fits a byte */

enum {
    LM_OK = 0,
    LM_ERR_INVALID = 1,    /* bad argument / violated precondition (the upstream CV_Assert cases)   */
    LM_ERR_NO_DEVICE = 2,  /* no usable HIP device: the product path has no CPU fallback            */
    LM_ERR_HIP = 3,        /* a HIP runtime call failed                                              */
    LM_ERR_OVERFLOW = 4,   /* more candidates/matches than the configured capacity    */
    LM_ERR_IO = 5,
    LM_ERR_EXTRACT = 6     /* addTemplate could not extract enough features (upstream returns -1)   */
};

/* cv::linemod::Feature {int x, y, label} */
typedef struct lm_feature { int32_t x, y, label; } lm_feature;
/* cv::linemod::Template header: {width, height, pyramid_level, features.size()} */
typedef struct lm_template_desc { int32_t width, height, pyramid_level, num_features; } lm_template_desc;
/* cv::linemod::Match {x, y, similarity, class_id, template_id}; class_id as index into lm_class_id() */
typedef struct lm_match_t { int32_t x, y; float similarity; int32_t template_id; int32_t class_idx; } lm_match_t;
typedef struct lm_rect { int32_t x, y, width, height; } lm_rect;

typedef struct lm_config {
    int32_t width, height;        /* level-0 frame size; fixed per detector (buffers are sized for it)      */
    int32_t num_modalities;       /* 1 = {ColorGradient}; 2 = {ColorGradient, DepthNormal}                   */
    int32_t pyramid_levels;       /* T_pyramid.size(); the reference uses 2                                  */
    int32_t T[LM_MAX_LEVELS];     /* {5,8} RGB-D, {2,8} colour only  (HighLevelLinemod.cpp:32,40)            */
    float   weak_threshold;       /* ColorGradient: 10                                                       */
    int32_t num_features;         /* ColorGradient: 63                                                       */
    float   strong_threshold;     /* ColorGradient: 55                                                       */
    int32_t distance_threshold;   /* DepthNormal: 2000                                                       */
    int32_t difference_threshold; /* DepthNormal: 50                                                         */
    int32_t depth_num_features;   /* DepthNormal: 63                                                         */
    int32_t extract_threshold;    /* DepthNormal: 2                                                          */
    int32_t device;               /* HIP device ordinal                                                      */
    int32_t shard_rank;           /* template-bank shard held by this detector: templates of every class     */
    int32_t shard_size;           /*   are split into shard_size contiguous template_id ranges (8e)          */
    int32_t max_candidates;       /* capacity of the device candidate buffer (0 = default 1<<18)             */
    int32_t max_matches;          /* capacity of the device match buffer     (0 = default 1<<18)             */
    int32_t frame_slots;          /* resident-frame slots for lm_match_batch (0 = default 8)                 */
    int32_t flags;                /* LM_FLAG_* (0 = defaults)                                                */
} lm_config;

/* Keep the lowest pyramid level's response memories at one byte per position (upstream's layout) instead
 * of the default two positions per byte.  Results are identical; this only selects the scan kernel. */
#define LM_FLAG_BYTE_RESPONSES 1
/* lm_match* / lm_match_end sleep on a blocking HIP event instead of spinning in hipStreamSynchronize: for hosts
 * that have fewer CPUs than busy processes (several GPUs' worth of matcher + exchange processes under a small
 * cgroup CPU quota).  Costs some wake-up latency per wait. */
#define LM_FLAG_BLOCKING_SYNC 2
/* 0.13 additive.  A detector with num_modalities == 1 keeps a level-0 uint16 depth frame in every slot beside the colour frame
 * (DESIGN.md section 22): the reference's shipped mode, `only use color modality: 1` with `use depth improvement: 1`, where the
 * detector matches on colour alone and the depth image drives the depth check, the ICP and the mask rules' depth gate.  The depth
 * frame is NEVER a match source: no quantised plane, no linear memory, no template feature comes from it, and a match enqueues
 * exactly what it enqueues without the flag.  With the flag
 *   - the depth image is OPTIONAL in every upload and ingest form (lm_upload_frame*, lm_stage_rows, the `depth` argument of lm_match /
 *     lm_match_classes / lm_match_masked, the depth descriptors of lm_ingest_frames*): a call that brings one marks the slot as holding
 *     depth, a call that brings none clears the mark and leaves the plane's bytes alone;
 *   - lm_upload_frames_pinned takes the RGB-D layout [colour dense | depth dense] per frame and marks every slot;
 *   - lm_depth_counts_*, lm_depth_select_*, lm_icp_refine, lm_icp_refine_slots, lm_icp_verify, lm_set_mask_rule with use_depth
 *     (`modalities` stays restricted to bit 0: the gate masks the COLOUR modality) and lm_read_frame's depth_out work as on an RGB-D
 *     detector.  A slot whose frame came without depth is refused by each of them with LM_ERR_INVALID, the slot's number in
 *     lm_last_error(), before anything is enqueued or claimed; so is a match on a ruled slot whose rule has a depth gate.
 * On an RGB-D detector the flag is legal and changes nothing.  Without it every call behaves as before. */
#define LM_FLAG_KEEP_DEPTH 4

typedef struct lm_detector lm_detector;

const char* lm_last_error(void);
const char* lm_version(void);

/* Fills the reference's two constructions (HighLevelLinemod.cpp:26-43): color_only=0 ->
 * {ColorGradient, DepthNormal}, T={5,8}; color_only=1 -> {ColorGradient}, T={2,8}. */
void lm_default_config(lm_config* cfg, int color_only, int width, int height);

/* cv::linemod::Detector(modalities, T_pyramid)            HighLevelLinemod.cpp:33-34,41-42 */
int  lm_create(const lm_config* cfg, lm_detector** out);
/* cv::Ptr::release()                                      HighLevelLinemod.cpp:50          */
void lm_destroy(lm_detector* det);

/* SIMILARITY_LUT / NORMAL_LUT are data parameters. */
int lm_set_similarity_lut(lm_detector* det, const uint8_t lut[256]);
int lm_set_normal_lut(lm_detector* det, const uint8_t lut[8000]);
int lm_get_similarity_lut(const lm_detector* det, uint8_t lut[256]);
int lm_get_normal_lut(const lm_detector* det, uint8_t lut[8000]);
/* 1 while the built-in NORMAL_LUT is active.  It is a documented SUBSTITUTE (azimuth of the cell centre, 8 bins), not
 * OpenCV's normal_lut.i, which could not be restated: DepthNormal labels then differ from cv::linemod's,
 * so a DepthNormal bank written by OpenCV must not be matched with it (lm_load_yaml warns on stderr).  Banks generated
 * through this library are self-consistent.  lm_set_normal_lut(det, <the 8000 bytes of normal_lut.i>) clears the flag. */
int lm_normal_lut_is_substitute(const lm_detector* det);

/* Detector::numClasses()  HighLevelLinemod.cpp:60,527 ; numTemplates() :65 ; classIds() :55,145,262,526 */
int         lm_num_classes(const lm_detector* det);
int         lm_num_templates(const lm_detector* det);                   /* total, all classes, whole bank */
int         lm_class_num_templates(const lm_detector* det, int class_idx);
const char* lm_class_id(const lm_detector* det, int class_idx);
int         lm_find_class(const lm_detector* det, const char* class_id); /* -1 if absent */
/* Detector::getT(level) :184 ; getModalities().size() :119 ; pyramidLevels() */
int lm_get_T(const lm_detector* det, int level);
int lm_num_modalities(const lm_detector* det);
/* 1: the slots keep a depth frame (an RGB-D detector, or a colour-only one created with LM_FLAG_KEEP_DEPTH); 0: they keep none;
 * -1 for NULL.  "Is depth a modality" is lm_num_modalities() == 2, a different question. */
int lm_keeps_depth(const lm_detector* det);
int lm_pyramid_levels(const lm_detector* det);

/* Detector::readClass / bulk template upload              HighLevelLinemod.cpp:299
 * Appends n_templates pre-extracted template pyramids to class `class_id` (created if new).
 * descs: n_templates * pyramid_levels * num_modalities entries ordered [template][level*M + modality];
 * features: concatenated in the same order.  Template ids continue from the class's current count.
 * Returns the class index in *class_idx_out (may be NULL). */
int lm_add_class(lm_detector* det, const char* class_id, int n_templates, const lm_template_desc* descs,
                 const lm_feature* features, int* class_idx_out);

/* Detector::addTemplate(sources, class_id, object_mask, &bounding_box) -> template_id or -1
 *                                                         HighLevelLinemod.cpp:93-97
 * Quantisation runs on the GPU, feature selection on the host.  depth may be NULL for a colour-only
 * detector (LM_FLAG_KEEP_DEPTH or not: templates are never learned from a kept depth frame); mask may be NULL.  *template_id_out = -1 and status LM_ERR_EXTRACT when extraction fails. */
int lm_add_template(lm_detector* det, const char* class_id, const uint8_t* bgr, size_t bgr_stride,
                    const uint16_t* depth, size_t depth_stride, const uint8_t* mask, size_t mask_stride,
                    int* template_id_out, lm_rect* bbox_out);

/* Detector::getTemplates(class_id, template_id)[level*M + modality]   HighLevelLinemod.cpp:115-116,181-183
 * features may be NULL to query the count. */
int lm_get_template(const lm_detector* det, int class_idx, int template_id, int level, int modality,
                    int* width, int* height, lm_feature* features, int* num_features);

/* Detector::match(sources, threshold, matches, class_ids)             HighLevelLinemod.cpp:152
 * class_idx >= 0: that class only (the reference always passes exactly one id, :145); -1: all classes.
 * Host frame in, sorted unique matches out (total order SURVEY.md A.9: similarity desc, template_id
 * asc, class asc, y asc, x asc; adjacent-unique on (x, y, similarity, class)).  *n_out receives the
 * number of matches found; if it exceeds `cap` only the first cap are written and LM_ERR_OVERFLOW
 * is returned.  With shard_size > 1 only this shard's templates are searched (ids stay global).
 * Frames that lie inside a block from lm_host_alloc (pinned memory; e.g. a cv::Mat constructed over it) go to the
 * device without the staging copy (one transfer when the depth image directly follows the colour image).
 * depth: required on an RGB-D detector; ignored on a colour-only one -- unless it was created with LM_FLAG_KEEP_DEPTH: then the image,
 * if given, goes into slot 0's depth plane beside the colour image (NULL: slot 0 holds no depth), here and in lm_match_classes /
 * lm_match_masked.  It is never a match source. */
int lm_match(lm_detector* det, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
             float threshold, int class_idx, lm_match_t* out, size_t cap, size_t* n_out);

/* The same with upstream's class LIST (std::vector<String> class_ids; the reference builds a one-element list, :145):
 * the linear memories are built once and every named class is scanned against them; the list holds the matches of all
 * named classes in the total order (lm_match_t.class_idx tells them apart).  n_classes == 0 or {-1} = all classes. */
int lm_match_classes(lm_detector* det, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                     float threshold, const int32_t* class_idxs, int n_classes, lm_match_t* out, size_t cap, size_t* n_out);

/* Detector::match(sources, threshold, matches, class_ids, quantized_images, masks) with its per-modality MASKS (0.4): one uint8 byte per
 * level-0 pixel (width x height, row stride in bytes, 0 = dense), nonzero = search there.  As OpenCV's quantize() does
 * (dst = 0; angle.copyTo(dst, mask)), every level's quantised colour image is ANDed with that level's mask -- the level-0 mask resized
 * with INTER_NEAREST, mask0[y << l][x << l] -- and so is the quantised depth image (its pyramid is the NN one). Templates are untouched.
 * A NULL mask leaves that modality unmasked; with both NULL this is lm_match.  depth_mask must be NULL on a colour-only detector. */
int lm_match_masked(lm_detector* det, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                    const uint8_t* color_mask, size_t color_mask_stride, const uint8_t* depth_mask, size_t depth_mask_stride,
                    float threshold, int class_idx, lm_match_t* out, size_t cap, size_t* n_out);
/* The same masks for the frame resident in `slot` (every slot path: lm_match_slot / _batch / _batch_classes / _prepared, the lanes,
 * the gathered calls).  modality 0 = colour, 1 = depth, -1 = the same mask for every modality; mask == NULL clears that modality's
 * mask.  A mask belongs to the frame in its slot: upload the frame first -- every frame upload (lm_upload_frame*, lm_upload_frames_pinned,
 * lm_upload_staged) clears the slot's masks.  Setting or clearing one makes the slot un-prepared (lm_match_prepared refuses it until
 * the slot is matched or prepared again) and drops its last lists (lm_match_collect refuses them: they belong to the old mask).  Asynchronous like lm_upload_frame (the source may be reused on return); refused
 * (LM_ERR_INVALID) for a slot that a match in flight, a colour check or depth counts in flight reads.  A call whose slots hold a mask
 * pre-processes with the separate (not level-fused) kernels plus one mask pass; calls without masks are unchanged. */
int lm_upload_match_mask(lm_detector* det, int slot, int modality, const uint8_t* mask, size_t stride);

/* Mask RULES (0.9): a match-time mask that the GPU computes from the frame resident in the slot -- a working-distance gate, a colour
 * gate, a rectangle of interest -- instead of a mask built on the host and uploaded per frame.  A rule is set once on a range of slots
 * and is STICKY: frame uploads (lm_upload_frame*, lm_upload_frames_pinned, lm_upload_staged) and template generation into slots do not
 * clear it; every pre-processing of a ruled slot evaluates it again from the frame the slot then holds (one kernel, k_mask_rule, on the
 * match's own stream: no host work, no transfer).  lm_match_prepared on an already prepared slot does not re-evaluate.
 *
 * The level-0 mask of a rule, for a frame of the detector's width x height:
 *   seed      the enabled gates ANDed; with no gate enabled every pixel is inside.
 *             depth gate (use_depth): inside iff zmin <= d <= zmax on the slot's uint16 depth frame; d == 0 (no measurement) is inside
 *               iff keep_invalid.  0 <= zmin <= zmax <= 65535, otherwise LM_ERR_INVALID.  LM_ERR_INVALID on a colour-only detector
 *               that keeps no depth frame on the device (lm_keeps_depth() == 0; see lm_depth_counts_begin).  With LM_FLAG_KEEP_DEPTH
 *               the gate reads the kept depth frame and masks the colour modality; a match on a ruled slot whose frame came
 *               without depth is refused (LM_ERR_INVALID, the slot's number in lm_last_error(), nothing enqueued).
 *             HSV gate (use_hsv): cv::inRange(cv::cvtColor(BGR2HSV), lower, upper) on the 8-bit images, the colour check's rule and
 *               its device code (bounds rounded and clamped as lm_color_check_counts does).
 *   grow = r  0 <= r <= 16: the seed dilated with a (2r + 1) x (2r + 1) square; the window is clipped to the image (a pixel outside the
 *             image is never inside).  Keeps the silhouette gradients, which straddle a depth edge.
 *   rect      applied after the dilation: width == 0 && height == 0 means no rectangle; otherwise x, y >= 0, width, height > 0 and the
 *             rectangle lies inside the frame (LM_ERR_INVALID if not).  The mask is 255 inside the rectangle where the dilated seed is
 *             set, 0 elsewhere.
 * The mask is applied to the modalities named in `modalities` (bit 0 colour, bit 1 depth; nonzero, and only modalities the detector
 * has) exactly as an uploaded mask is (lm_upload_match_mask: every level's INTER_NEAREST mask).  Where the slot also holds an uploaded
 * mask of a modality, the effective mask is the AND of the two.  A call with a ruled slot pre-processes like a call with a masked slot
 * (the separate kernels); calls without masks and rules are unchanged. */
typedef struct lm_mask_rule {
    int32_t modalities;
    int32_t use_depth, keep_invalid, zmin, zmax;
    int32_t use_hsv;
    double lower[3], upper[3];
    int32_t grow;
    lm_rect rect;
    int32_t reserved;           /* 0 */
} lm_mask_rule;
/* Sets (rule == NULL: clears) the rule of slots [first_slot, first_slot + n_slots).  Like lm_upload_match_mask it makes the slots
 * un-prepared and drops their last lists, and is refused (LM_ERR_INVALID) for slots that a match in flight, a colour check or depth
 * counts in flight reads. */
int lm_set_mask_rule(lm_detector* det, int first_slot, int n_slots, const lm_mask_rule* rule);
/* *is_set = 1 and *out = the slot's rule as it was set, or *is_set = 0 (out untouched). */
int lm_get_mask_rule(const lm_detector* det, int slot, lm_mask_rule* out, int* is_set);
/* Stage hook: the level-0 mask of `rule` (dense w x h bytes, 0 / 255) for host images of the detector's size; bgr may be NULL without
 * an HSV gate, depth without a depth gate. */
int lm_stage_mask_rule(lm_detector* det, const uint8_t* bgr, const uint16_t* depth, int w, int h, const lm_mask_rule* rule,
                       uint8_t* mask_out);

/* Resident-frame path used by the benchmark and by batch-of-frames serving: upload once, match many.
 *
 * Streaming input (the reference's real call pattern is one fresh camera frame per detect() call,
 * detector.cpp:17-42 -> PoseDetection.cpp:66): uploads are ASYNCHRONOUS.  lm_upload_frame packs the (pageable,
 * strided) source into the slot's pinned staging buffer and enqueues the H2D copies on one of the detector's copy streams,
 * behind which it records the slot's "uploaded" event; it returns without waiting for the copy and without touching
 * any compute stream.  Every lm_match_slot / lm_match_batch / lm_match_begin makes its stream wait for the uploads
 * of the slots it reads (hipStreamWaitEvent), so
 *     begin(lane, A);  upload(B ...);  end(lane);  begin(lane, B);  upload(A ...);  ...
 * overlaps the transfer of step k + 1 with the compute of step k.  A slot that belongs to a match in flight cannot
 * be uploaded to (LM_ERR_INVALID).  The source buffer may be reused as soon as lm_upload_frame returns. */
int lm_upload_frame(lm_detector* det, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth,
                    size_t depth_stride);
/* lm_upload_frame of the frame translated by (shift_x, shift_y) pixels with zeros shifted in -- the reference's translateImg on
 * both images before the match (principal-point shift: PoseDetection.cpp:54-59, 192-197) -- done while the staging buffer is
 * filled: one pass over the frame instead of a translated host copy followed by the staging copy.  Same asynchronous contract. */
int lm_upload_frame_shifted(lm_detector* det, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth,
                            size_t depth_stride, int shift_x, int shift_y);
/* The same for a source in PINNED host memory (lm_host_alloc, hipHostMalloc, hipHostRegister): no staging copy, the
 * DMA engine reads the caller's buffer, which therefore must stay untouched until lm_upload_wait(det, slot) returns
 * or a match that covers the slot has been collected.  This is the path that reaches the PCIe rate. */
int lm_upload_frame_pinned(lm_detector* det, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth,
                           size_t depth_stride);
/* A run of frames in ONE strided transfer: host frame i = [colour dense | depth dense] (colour only for a colour-only
 * detector that keeps no depth; with LM_FLAG_KEEP_DEPTH a colour-only detector takes the RGB-D layout, 5 bytes per pixel, and every
 * slot of the run then holds depth) at frames + i * frame_stride (0 = densely packed), pinned, into slots [first_slot, first_slot + n_slots).
 * lm_upload_frame_pinned makes the same single copy per frame when it is handed such a contiguous pair. */
int lm_upload_frames_pinned(lm_detector* det, int first_slot, int n_slots, const uint8_t* frames, size_t frame_stride);
/* lm_upload_frame_shifted for a source in PINNED host memory (r05): the DMA engine copies the overlapping rectangle row by row
 * (hipMemcpy2DAsync) behind a memset of the destination: no staging copy and no host pass over the pixels.  Same contract as
 * lm_upload_frame_pinned.  Shifts beyond the frame size are clamped (an all-zero frame either way). */
int lm_upload_frame_pinned_shifted(lm_detector* det, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth,
                                   size_t depth_stride, int shift_x, int shift_y);
/* Staged uploads of PAGEABLE frames (r05): lm_upload_frame[_shifted] in three steps, so that a pool of host threads fills the pinned
 * staging buffers of a whole batch in parallel (the staging copy of a 1280 x 960 RGB-D frame is 6 MB: 277 us on one thread) while
 * the thread that owns the detector goes on:
 *     lm_stage_reserve(det, first, n)                    owner thread: the slots' earlier uploads have landed, their staging buffers exist
 *     lm_stage_rows(det, slot, ..., row0, row1) x many   ANY thread, disjoint row ranges of a slot concurrently: rows [row0, row1) of both
 *                                                        images, translated by (shift_x, shift_y) with zeros shifted in; host memory only
 *     lm_upload_staged(det, slot)                        owner thread, after all rows of the slot are in: the H2D copies + upload ticket
 * The source may be reused as soon as the lm_stage_rows calls covering it have returned.
 * LM_FLAG_KEEP_DEPTH on a colour-only detector: depth may be NULL in lm_stage_rows; the calls that fill one slot between its
 * lm_stage_reserve and its lm_upload_staged all bring a depth image or none of them does -- lm_upload_staged refuses a slot that was
 * staged both ways (LM_ERR_INVALID, nothing sent; the slot stays reserved and may be staged again after a new lm_stage_reserve). */
int lm_stage_reserve(lm_detector* det, int first_slot, int n_slots);
int lm_stage_rows(lm_detector* det, int slot, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth, size_t depth_stride,
                  int shift_x, int shift_y, int row0, int row1);
int lm_upload_staged(lm_detector* det, int slot);
/* Host waits until the upload of `slot` (-1: of every slot) has landed in device memory. */
int lm_upload_wait(lm_detector* det, int slot);
/* Pinned host memory for frame sources (hipHostMalloc); needs a HIP device. */
int  lm_host_alloc(size_t bytes, void** out);
void lm_host_free(void* p);
/* Pageable sources: number of pieces the staging memcpy is cut into so that it overlaps the DMA (default 1:
 * on the MI355X host every extra hipMemcpyAsync call cost more than the overlap won). */
int lm_set_stage_chunks(lm_detector* det, int chunks);
/* Launch-shape knobs (results never depend on them; tools/ and the tests flip them for A/B runs).  Keys 1, 2 and 10 (three concurrent
 * pre-processing chains for single frames; lm_match's copies on the copy streams; level-1 kernels inside the level-0 grids) lost their
 * A/B runs in r02 / r03 (DESIGN_HISTORY.md) and were removed with their code in r05: lm_set_tuning rejects them. */
/* LM_TUNE_COPY_STREAMS: copy streams the uploads are dealt to, slot -> stream round-robin (1..4, default 4: one
 *   in-order stream moved 0.6-0.9 MB images at 25.6 GB/s, several keep several DMA engines busy). */
#define LM_TUNE_COPY_STREAMS 3
/* LM_TUNE_CBLUR_VARIANT (process-wide): Gaussian blur kernel 0 = by batch size and frame size (default: one-shot below 16 frames;
 *   batches: frames of up to 2 MB on the matrix cores, larger ones the row walker), 1 = one-shot, (2 = r02's sliding window: deleted in r05, rejected,)
 *   3 = row walker with the column sums shared between neighbouring lanes (r03), 4 = the two banded products of the 8-bit
 *   Gaussian as v_mfma_i32_32x32x32_i8 (r04; rows of a multiple of 32 bytes, other shapes take 3).  Same bytes from all. */
#define LM_TUNE_CBLUR_VARIANT 4
/* LM_TUNE_CGRAD_VARIANT (process-wide): gradient orientation + 3x3 vote 0 = by batch size (default: two kernels below 16
 *   frames, the fused strip kernel from there), 1 = two kernels, 2 = fused, 3 = fused with 32-row strips (what tall
 *   images take in large batches). */
#define LM_TUNE_CGRAD_VARIANT 5
/* LM_TUNE_PHASE_MAX_SLOTS: calls of at most this many frames run the pre-processing (a3-a10) as five launches, each
 *   holding the independent kernels of one dependency level on ranges of the block index, instead of fourteen dependent
 *   ones (default 15: from 16 frames the batch kernels take over; 0 = off; two-level T = {5, 8} pyramids only, anything else takes the plain sequence). */
#define LM_TUNE_PHASE_MAX_SLOTS 6
/* LM_TUNE_BATCH_PHASES: calls of 16 or more frames run the pre-processing as launches in which batch kernels of one
 *   dependency level (and one register class) share a grid -- the level-1 kernels fill the tail of the level-0 ones: four
 *   (colour only) or seven (RGB-D) dependent launches instead of eleven.  0 = never, 1 = always, 2 (default) = when no
 *   other lane has a match in flight: measured r03, the fused launches win when a lane has the chip to itself and lose
 *   beside other lanes, whose kernels fill the tails anyway.  Two-level T = {5, 8} / {2, 8} pyramids of 32-pixel-aligned
 *   frames only; anything else takes the plain sequence.  Results never depend on it. */
#define LM_TUNE_BATCH_PHASES 7
/* LM_TUNE_PYRDOWN_VARIANT (process-wide): cv::pyrDown kernel 0 = by batch size (default: one lane per 8 output pixels below 16
 *   frames, the row-walking kernel whose column sums travel between lanes from there), 1 / 2 = force either. */
#define LM_TUNE_PYRDOWN_VARIANT 8
/* LM_TUNE_BLUR_PYR (process-wide): batches run the level-0 Gaussian blur and cv::pyrDown level 0 -> 1 as ONE launch whose
 *   blocks are interleaved per frame slot: 1 = [all blur tiles | all pyrDown tiles] of a slot back to back (r03); 2 = a slot's blur
 *   and pyrDown tiles dealt out evenly (r04), so the tiles of a band of rows run side by side and the second reader finds the
 *   rows in the L2; 3 (default) = 2 for frames of more than 2 MB, 1 below (measured: pays at 1280 x 960, not at 640 x 480);
 *   0 = two launches. */
#define LM_TUNE_BLUR_PYR 9
/* LM_TUNE_DMEDIAN_VARIANT (process-wide): 5 x 5 median of the normals' labels, output rows per lane 0 = by batch size (default:
 *   4 below 16 frames -- many short waves --, 16 from there: 20 rows of horizontal sums per 16 outputs instead of 8 per 4),
 *   1 / 2 = force either. */
#define LM_TUNE_DMEDIAN_VARIANT 11
/* LM_TUNE_BLUR_STRIP (process-wide): rows per strip of the level-0 Gaussian blur inside the blur + pyrDown launch of a batch:
 *   0 = by frame shape and batch size (default: as tall as still fills the chip), 16 / 32 / 64 = forced. */
#define LM_TUNE_BLUR_STRIP 12
/* LM_TUNE_WORK_WEIGHT: 1 (default, r04) = the few-frame / batch kernel selection of the pre-processing (the keys above that say
 *   "below 16 frames") counts a frame as (level-0 pixels / (640 x 480)) frames, at least one -- a call's WORK decides, so
 *   eight 1280 x 960 frames take the batch kernels; 0 = by frame count alone (r03).  Results never depend on it. */
#define LM_TUNE_WORK_WEIGHT 13
/* LM_TUNE_SORT_SPLIT: the device sort (a15) of lists longer than 1024 matches 0 = one workgroup per frame (r03), 1 = four chunk
 *   workgroups per frame + a merge launch, 2 (default) = the latter while the lists this detector collected lately were that
 *   long.  Same lists either way. */
#define LM_TUNE_SORT_SPLIT 14
/* LM_TUNE_SCAN_LIST_ORDER: order of a template's feature list at the scanned level: 0 = ascending linear-memory offsets (r01-r03:
 *   all features of orientation 0 first), 1 = dealt round-robin over the eight orientations, 2 = descending, 3 (default, r04) =
 *   greedy farthest-point order in (x, y, orientation): the first features sample the template's whole extent and all its
 *   orientations, so the exact pruning gives up on a work item sooner (49.7 -> 46.3 % of the feature loads on config 2).
 *   The similarity sums, and therefore every result, do not depend on it; changing it rebuilds the device bank. */
#define LM_TUNE_SCAN_LIST_ORDER 15
/* LM_TUNE_SCAN_FORM (r05): which kernel scans the lowest level when it keeps nibble-packed memories: 0 (default) = by cost -- the
 *   bit-plane scan k_scan1 (counts the features a position MISSES on one bit per position and orientation, then takes the exact
 *   sums of the few positions the miss bound leaves: k_scan1_exact) for detectors of ONE modality and calls of at least 8 frames
 *   (and a whole group of frames per wave), when it needs at least a fifth fewer waves than the nibble scan k_scan4 and the
 *   threshold is at least LM_TUNE_SCAN1_MIN_THRESHOLD (measured: +9-10 % on the
 *   colour-only 1280 x 960 workload, a loss with two modalities, where k_scan4's exact pruning stops far sooner than the miss
 *   bound); 1 = always k_scan4; 2 = k_scan1 whenever the level has planes.  The candidate lists, and therefore every result, are
 *   the same.  Under 0, a call whose own scan is k_scan1 writes the scanned level of its slots as one spread byte + the bit planes,
 *   WITHOUT the response memories: those slots are scanned by k_scan1 from then on (also by lm_match_prepared at a lower threshold),
 *   and a call that mixes them with slots prepared without planes is refused (LM_ERR_INVALID).
 *   r06: 3 = the bit-plane scan with a frame's planes in LDS (k_scanl) wherever they fit -- the scanned level's planes of all modalities
 *   within 153 600 bytes: 640 x 480 RGB-D at T = {5, 8} exactly --, k_scan1 where they do not.  One 1024-thread workgroup copies a frame's
 *   planes into its CU's LDS, counts misses from there (k_scan1 on such frames is bound by the L2 -> L1 line rate: every frame and feature
 *   is two 128-byte lines) and takes the survivors' exact sums from the frame's spread bytes, in LDS as well, in the same launch.  Under 0
 *   it is picked for calls of at least 24 frames at a threshold of at least LM_TUNE_SCAN1_MIN_THRESHOLD, for one modality or two; its
 *   slots too keep the spread byte + the planes instead of the response memories.  lm_get_scan_form_stats reports 1000 + the workgroups
 *   per frame as the "lanes per frame" of such a launch. */
#define LM_TUNE_SCAN_FORM 16
/* LM_TUNE_SCAN1_MIN_THRESHOLD (r05): similarity threshold in percent (0..100, default 50) below which LM_TUNE_SCAN_FORM 0 keeps
 *   k_scan4: the lower the threshold the more positions survive the miss bound and need their exact sums. */
#define LM_TUNE_SCAN1_MIN_THRESHOLD 17
/* LM_TUNE_CGRAD_LEVELS (r06): 1 (default) = a batch's colour-gradient orientation + vote passes of pyramid levels 0 and 1 run in ONE launch (level 1 of a
 *   640 x 480 frame is a handful of waves: behind level 0's workgroups they fill idle SIMDs instead of a launch of their own that leaves half the chip
 *   without a wave); 0 = one launch per level (r02-r05).  Same labels either way. */
#define LM_TUNE_CGRAD_LEVELS 18
/* LM_TUNE_SURVIVOR_QUEUE (r06): entries of a lane's survivor queues of the bit-plane scan k_scan1 (64 .. 16 777 216, rounded up to a multiple of 8; default
 *   1 048 576 = 131 072 per XCD queue; 8 bytes each, allocated on a lane's first bit-plane scan).  A wave whose survivors do not fit takes their exact sums itself, so
 *   the lists never depend on the value; small values exist for the tests that drive the full-queue path (concurrent reservations at the capacity, partial
 *   fits).  Setting it waits for the device and frees the queues of all lanes. */
#define LM_TUNE_SURVIVOR_QUEUE 19
/* LM_TUNE_RECTIFY_REDUCE_GRID: the order in which the workgroups of lm_ingest_frames_rectified_reduced's kernel are dispatched: 0
 * (default) = all tiles of a frame, then the next frame's; 1 = the frames of the call fastest, so that the workgroups that read one patch of
 * the rectification map run together.  Both give the same bytes; DESIGN.md section 19 has both measured. */
#define LM_TUNE_RECTIFY_REDUCE_GRID 20
/* LM_TUNE_ICP_BATCH_MB: megabytes of scratch a chunk of queries of an ICP refinement may take (1 .. 4096, default 512, the figure
 * lm_icp_verify uses): consecutive queries run side by side in the same launches while their scratch stays within it; a query that
 * exceeds it alone runs alone.  The refined poses never depend on the value; small values exist for the test that drives a call
 * through several chunks at small shapes. */
#define LM_TUNE_ICP_BATCH_MB 21
int lm_set_tuning(lm_detector* det, int key, int value);
int lm_match_slot(lm_detector* det, int slot, float threshold, int class_idx, lm_match_t* out, size_t cap, size_t* n_out);
/* Matches slots [0, n_slots) back-to-back on the detector's streams; out is n_slots * cap_per_frame
 * records, counts n_slots entries. */
int lm_match_batch(lm_detector* det, int n_slots, float threshold, int class_idx, lm_match_t* out, size_t cap_per_frame,
                   int32_t* counts);
/* Detector::match(sources, threshold, matches, class_ids) with upstream's class LIST      HighLevelLinemod.cpp:145,152
 * on the resident frames of slots [first_slot, first_slot + n_slots): a3-a10 run ONCE per frame, every named class is
 * scanned against the same linear memories (one scan launch per run of neighbouring class indices), one refinement,
 * one sort.  A list holds the matches of all named classes in the total order; lm_match_t.class_idx tells them apart.
 * n_classes == 0 or {-1} = all classes; duplicates are ignored.  The per-class incremental cost is scan + refine only. */
int lm_match_batch_classes(lm_detector* det, int first_slot, int n_slots, float threshold, const int32_t* class_idxs,
                           int n_classes, lm_match_t* out, size_t cap_per_frame, int32_t* counts);
/* a11-a15 ONLY, for slots whose a3-a10 results are current: a match or lm_prepare_slot has run on the frame the slot
 * holds and neither an upload nor a LUT change has happened since (LM_ERR_INVALID otherwise -- never a silent
 * re-use of stale memories).  This is the reference's call pattern for several objects in one camera frame
 * (PoseDetection::detect per class name, PoseDetection.cpp:45-66 -> HighLevelLinemod.cpp:145-152): upload + prepare
 * once, one lm_match_prepared per class. */
int lm_match_prepared(lm_detector* det, int first_slot, int n_slots, float threshold, const int32_t* class_idxs,
                      int n_classes, lm_match_t* out, size_t cap_per_frame, int32_t* counts);

/* Asynchronous halves of lm_match_batch on one of four LANES (lane 0 = the detector's stream, lanes 1-3 = further
 * HIP streams with their own events and threshold tables; two lanes are what bench.py drives).  lm_match_begin enqueues a3-a15 for the resident frames
 * of slots [first_slot, first_slot + n_slots) and returns; lm_match_end waits for that lane and delivers the
 * lists exactly like lm_match_batch (out + i * cap_per_frame, counts[i]; i counts from first_slot).  Two lanes
 * working on disjoint slot ranges overlap each other's stages on the GPU (the scan is L1/L2-bound, the
 * preprocess passes VALU / fabric-bound) from ONE host thread:
 *     begin(0, A); begin(1, B);  loop { end(0); begin(0, A');  end(1); begin(1, B'); }
 * A lane's slots must not be uploaded to while it is busy (lm_upload_frame* refuse); uploads to the OTHER slots
 * may be issued at any time and are ordered against the lane that later reads them by per-slot events.  The
 * synchronous entry points refuse to run while a lane is busy. */
int lm_match_begin(lm_detector* det, int lane, int first_slot, int n_slots, float threshold, int class_idx);
/* lm_match_begin with a class list (see lm_match_batch_classes); collected by lm_match_end. */
int lm_match_begin_classes(lm_detector* det, int lane, int first_slot, int n_slots, float threshold,
                           const int32_t* class_idxs, int n_classes);
/* hipDeviceSynchronize() on the detector's device (what torch.cuda.synchronize() is for a torch program). */
int lm_synchronize(lm_detector* det);
int lm_match_end(lm_detector* det, int lane, lm_match_t* out, size_t cap_per_frame, int32_t* counts);

/* The lists of the last COMPLETED match on slots [first_slot, first_slot + n_slots) once more -- they stay in the slots' result blocks
 * until the next upload to / match on the slot: what a caller does after LM_ERR_OVERFLOW (counts[] held the capacity needed) instead
 * of a second pass over the GPU.  LM_ERR_INVALID when a slot holds no completed match or belongs to a match in flight. */
int lm_match_collect(lm_detector* det, int first_slot, int n_slots, lm_match_t* out, size_t cap_per_frame, int32_t* counts);

/* ---- f1: the colour check of the reference's match post-processing, batched on the GPU ----------
 * For every match of the list (any class / template of the bank, e.g. a merged multi-GPU list): templateMask =
 * fillPoly of the convex hull of the template's level-0 features moved to (match.x, match.y)
 * (HighLevelLinemod.cpp:113-135), counted once alone and once AND-ed with the colour mask = inRange(cvtColor(frame,
 * BGR2HSV), lower, upper) (:159-161): in_hull[i] and in_both[i] are the two countNonZero of colorCheck (:424-434),
 * whose verdict is in_both * 100 / in_hull > percentToPassCheck.  The frame is the one resident in `slot`.  The
 * reference builds a full-frame mask and counts the full frame once per tested match; here the colour mask is
 * one bit per pixel, built once per call, and one wave rasterises one hull. */
int lm_color_check_counts(lm_detector* det, int slot, const double lower_hsv[3], const double upper_hsv[3],
                          const lm_match_t* matches, size_t n, int64_t* in_hull, int64_t* in_both);

/* The same for a list whose matches lie in SEVERAL resident frames (slot_of_match[i] = the slot of match i's frame): one colour-mask
 * launch for the slots the list names, one hull launch for all matches, one wait -- a batch's colour checks in one call.
 * r05: both forms run on a stream and buffers of their own and only refuse slots that belong to a match in flight, so the checks of
 * batch k overlap the match of batch k + 1 on another lane. */
int lm_color_check_counts_slots(lm_detector* det, const int32_t* slot_of_match, const double lower_hsv[3], const double upper_hsv[3],
                                const lm_match_t* matches, size_t n, int64_t* in_hull, int64_t* in_both);
/* The colour masks of slots [first_slot, first_slot + n_slots) for one HSV range, enqueued on `lane`'s stream AHEAD of the match the
 * caller begins on that lane next: when the lane has been collected the masks are there, and a colour check of those slots for the
 * same range skips its mask launch (only the hull launch is left between lm_match_end and the counts).  An upload to a slot, or a
 * colour check with another range, invalidates the slot's mask. */
int lm_color_mask_prepare(lm_detector* det, int lane, int first_slot, int n_slots, const double lower_hsv[3], const double upper_hsv[3]);
/* The two halves of lm_color_check_counts_slots: begin enqueues the copies and the two launches on the colour-check stream and returns,
 * end waits and delivers the counts of the list begun (one check in flight per detector; `matches` may be reused after begin returns).
 * Between them the calling thread is free -- HighLevelLineMOD starts the first depth checks of a batch's groups meanwhile. */
int lm_color_check_begin_slots(lm_detector* det, const int32_t* slot_of_match, const double lower_hsv[3], const double upper_hsv[3],
                               const lm_match_t* matches, size_t n);
int lm_color_check_end(lm_detector* det, int64_t* in_hull, int64_t* in_both);

/* r06: the depth check's early verdicts on the GPU (the reference's medianMat + depthCheck, HighLevelLinemod.cpp:336-349,437-457).  The check wants to
 * know whether v[n / 5] after std::nth_element(v, v + n / 4) -- v the crop of the (translated) depth frame under the template's bounding box with depths
 * <= 1 replaced by 65535 -- lies inside the window [lo, hi] of medians that pass |depthDiff| < stepSize.  That element is one of the n / 4 + 1 smallest:
 * when more than n / 4 values lie below lo, or none lies inside [lo, hi], the verdict "outside" is certain without the selection.  For every query this
 * call counts, in the frame resident in slot `slot`, the values of the crop [x0, x1) x [y0, y1) (the caller clips it to the frame) below lo and inside
 * [lo, hi] -- one wave per query on the colour-check stream, beside the lanes.  The host then runs std::nth_element (it must stay the host library's: WHICH
 * of those elements comes back is implementation-defined) only for the checks no early verdict decides.  Detectors without a depth modality keep no
 * depth frame on the device unless they were created with LM_FLAG_KEEP_DEPTH: LM_ERR_INVALID (and so is, on such a detector, a slot whose frame came
 * without a depth image).  begin / end as the colour check's halves (one depth query list in flight per detector, independent of a
 * colour check in flight). */
typedef struct lm_depth_query { int32_t x0, y0, x1, y1; int32_t lo, hi; int32_t slot; int32_t reserved; } lm_depth_query;
int lm_depth_counts_begin(lm_detector* det, const lm_depth_query* queries, size_t n);
int lm_depth_counts_end(lm_detector* det, uint32_t* below, uint32_t* inside);

/* The depth check's SORTED order statistic on the GPU (0.13 additive).  The reference's medianMat returns v[n / 5] after
 * std::nth_element(v, v + n / 4): which element that is depends on the library's partition order, and the default post-processing keeps the host
 * library's answer (lm_depth_counts_begin above).  This call serves the opt-in statistic that is well defined -- the element a std::nth_element that
 * sorts the whole range, as a conforming one may, leaves in that place -- so that host and device can be compared bit for bit and a caller whose
 * frames never touch the host (lm_ingest_frames*) reaches poses.
 *
 * The rule, to the last word.  For query i, in the depth plane of the frame resident in slot `slot` (the plane as the slot holds it: translated by
 * the upload's or the ingest's shift, zeros shifted in), take the crop of columns [x0, x1) and rows [y0, y1) and n = (x1 - x0) * (y1 - y0).  Every
 * pixel d of the crop gives t = (d <= 1) ? 65535 : d (threshold(.., 1, 65535) inverted and added: holes, and the zeros a shift moved in, count
 * as the farthest value).  value[i] is the element at 0-based index `rank` of the ascending sort of the n values t; equal values are
 * indistinguishable, so the value is unique.  An empty crop (n == 0) gives 65535 whatever `rank` holds.  The depth check asks for rank = n / 5 in
 * integer division (medianMat's n / position with position 5).
 *
 * One workgroup per query on the colour-check stream, beside the lanes: an exact radix select over the 16-bit key, two passes over the crop.  No
 * byte outside the crop's rows of the slot's depth plane is read.  begin / end behave as the depth counts' halves: begin checks everything, waits
 * (on the stream) for the uploads and ingests of the named slots, enqueues and returns; end waits and delivers value[0 .. n) in the queries' order.
 * One selection list is in flight per detector, independent of a colour check or depth counts in flight; the named slots refuse uploads until end.
 * n == 0 is legal (end then delivers nothing and `value` may be NULL).
 * LM_ERR_INVALID, before anything is enqueued: a NULL detector, NULL queries with n > 0 (end: NULL value with n > 0, or no list in flight); a slot
 * out of range or without a frame; a crop outside the frame, x1 < x0 or y1 < y0; a non-empty crop with rank < 0 or rank >= n; a detector without a
 * depth modality (it keeps no depth frame on the device); a selection list already in flight. */
typedef struct lm_depth_select_query { int32_t x0, y0, x1, y1; int32_t rank; int32_t slot; } lm_depth_select_query;
int lm_depth_select_begin(lm_detector* det, const lm_depth_select_query* queries, size_t n);
int lm_depth_select_end(lm_detector* det, uint16_t* value);
/* Measurement only (tools/time_depth_select.py): the milliseconds, between two HIP events on the colour-check stream, of ONE kernel launch for
 * the n queries (already on the device when the first event is recorded) -- what = 0: k_depth_select; 1: k_depth_select with the naive histogram
 * (one shared LDS histogram, one atomic per pixel: the yard-stick of the contention decision); 2: k_depth_counts for the same crops with the
 * window [0, 65535].  Synchronous; refuses what lm_depth_select_begin refuses, and a call while a selection list or depth counts are in flight. */
int lm_time_depth_select(lm_detector* det, const lm_depth_select_query* queries, size_t n, int what, float* ms);

/* ---- multi-GPU: template-bank shards + the ONE exchange step of the path ------------------------
 * One process per GPU; every rank creates its detector with lm_config.shard_rank / shard_size (contiguous template_id
 * ranges, global ids preserved), uploads the SAME frames and calls the same sequence of lm_match_begin_gathered /
 * lm_match_end_gathered.  lm_comm_init creates the RCCL communicators (librccl is loaded then, not before; one
 * communicator per lane so that the lanes' collectives never wait for each other); the ncclUniqueId goes from rank 0
 * to the others over TCP addr:port (one node: "127.0.0.1", e.g. MASTER_PORT + 1) -- no torch, no MPI, no second
 * process.  recs_per_frame_cap (0 = 256): average records per frame a rank may contribute to one gather; the gather
 * buffers have a fixed size of n_frames * recs_per_frame_cap records per rank so that no host round trip sits between
 * the two collectives.  More records than that -- or a frame with more than 4096 matches on some shard, which the
 * single-GPU path hands to the host sort -- is NOT an error: lm_match_end_gathered then runs a second, exactly sized
 * exchange (every rank sees the same status words, so all ranks take it together) and returns the same lists the
 * single-GPU path returns (the reference consumes ALL matches: HighLevelLinemod.cpp:206-253).  Only a shard that
 * overflows its own lm_config.max_candidates / max_matches fails (LM_ERR_OVERFLOW on every rank), as on one GPU.
 * The ids of the lanes' communicators travel in ONE rendezvous on `port`; on any failure nothing is left behind and
 * the call may be repeated. */
int lm_comm_init(lm_detector* det, int rank, int world, const char* addr, int port, int recs_per_frame_cap);
/* The rendezvous lm_comm_init uses, on its own (host only, no GPU): n bytes from rank 0's buf into every rank's buf. */
int lm_rendezvous_broadcast(int rank, int world, const char* addr, int port, void* buf, size_t n, int timeout_s);
int lm_comm_destroy(lm_detector* det);
int lm_comm_info(const lm_detector* det, int* rank, int* world);
/* lm_match_begin + behind the sort kernel, on the lane's stream: k_pack_lists (the lane's sorted lists back to back +
 * their lengths, device buffers), ncclAllGather of the lengths, ncclAllGather of the packed records, D2H of the lengths. */
int lm_match_begin_gathered(lm_detector* det, int lane, int first_slot, int n_slots, float threshold, int class_idx);
/* Waits for the lane, fetches from every rank's gathered run exactly the records of the frames THIS RANK OWNS (one
 * contiguous piece per rank: with R ranks 1 / R of the records crosses the PCIe link, not R x the gather capacity) and
 * merges them (R-way merge + adjacent-unique, lm_merge_frames): frames [n * rank / R, n * (rank + 1) / R) of the lane's n
 * frames (*first_frame, *n_frames), so neither the host work nor the D2H volume per rank grows with R.  out: the owned frames' merged lists back to back (cap records), counts[i] their lengths. */
int lm_match_end_gathered(lm_detector* det, int lane, lm_match_t* out, size_t cap, int32_t* counts, int* first_frame,
                          int* n_frames, size_t* n_out);
/* Every rank has reached this call and every rank's device is idle (ncclAllReduce + hipDeviceSynchronize): the
 * "barrier + synchronize" that brackets a timed region.  lm_comm_max: element-wise maximum of n <= 32 doubles. */
int lm_comm_barrier(lm_detector* det);
int lm_comm_max(lm_detector* det, double* values, int n);
/* "0000:c1:00.0"-style PCI bus id of the detector's device (hipDeviceGetPCIBusId): bench.py checks that the N ranks of
 * a node really sit on N different GPUs. */
int lm_device_pci_bus_id(lm_detector* det, char* out, size_t cap);

/* R-way merge of per-shard sorted lists + adjacent-unique: the step after the all-gather (8e).  Host-side. */
int lm_merge_matches(const lm_match_t* lists, const int32_t* counts, int n_lists, size_t stride, lm_match_t* out,
                     size_t cap, size_t* n_out);

/* The same for a whole batch (8e, one call per step instead of one per frame).  lm_pack_matches turns the
 * fixed-stride output of lm_match_batch into one contiguous run (what a rank sends); lm_merge_batch takes the
 * R gathered runs (rank r at packed + r * rank_stride, counts[r * n_frames + i] records for frame i) and writes
 * the merged + unique lists of all frames back to back with out_counts[i].  Host-side, multi-threaded. */
int lm_pack_matches(const lm_match_t* recs, size_t stride, const int32_t* counts, int n_frames, lm_match_t* out,
                    size_t cap, size_t* n_out);
int lm_merge_batch(const lm_match_t* packed, size_t rank_stride, const int32_t* counts, int n_ranks, int n_frames,
                   lm_match_t* out, size_t cap, int32_t* out_counts, size_t* n_out);
/* The same for the frames [frame_lo, frame_hi) only (out_counts: frame_hi - frame_lo entries): with R ranks each rank
 * merges the frames it owns, so the host work of the exchange does not grow with R. */
int lm_merge_frames(const lm_match_t* packed, size_t rank_stride, const int32_t* counts, int n_ranks, int n_frames,
                    int frame_lo, int frame_hi, lm_match_t* out, size_t cap, int32_t* out_counts, size_t* n_out);
/* The bookkeeping of lm_match_end_gathered on its own (host-only, no GPU, no RCCL: unit-testable at any world size).  all_cnt =
 * the all-gathered lengths, n_ranks runs of n_frames + 1 ints (per-frame record counts of the rank's packed run, then the rank's
 * status word: bit 0 lists exceed the fixed gather capacity, bit 1 a frame left to the host sort, bit 2 shard capacity overflow).
 * Out: OR of the status words; first rank with bit 2 (-1: none); the frames [*f0, *f1) = [n * rank / R, n * (rank + 1) / R) this
 * rank merges; counts[r * n_frames + i]; per rank the piece (start, length in records) of its packed run that holds exactly the
 * owned frames -- the only records lm_match_end_gathered copies to the host.  counts / piece_* may be NULL. */
int lm_gather_plan(const int32_t* all_cnt, int n_ranks, int n_frames, int rank, int* status, int* bad_rank, int* f0, int* f1,
                   int32_t* counts, uint64_t* piece_start, uint64_t* piece_len);
/* Records of the largest rank's packed run (at least 1): the per-rank buffer size of the sized second exchange. */
int lm_gather_max_total(const int32_t* counts, int n_ranks, int n_frames, uint64_t* max_total);

/* Template-bank persistence (Detector::write/writeClass/read/readClass, HighLevelLinemod.cpp:260,267,294,299):
 * own compact binary format, see DESIGN.md. */
int lm_save_bank(const lm_detector* det, const char* path);
int lm_load_bank(lm_detector* det, const char* path);
/* The reference's own file, "linemod_templates.yml.gz": cv::FileStorage YAML of Detector::write(fs) followed
 * by "classes" [ { Detector::writeClass } ... ] (HighLevelLinemod.cpp:256-270), gzip when the path ends in
 * .gz.  lm_load_yaml = Detector::read(fs.root()) + readClass per entry (HighLevelLinemod.cpp:292-303): the
 * file's pyramid_levels, T and modality types must equal the detector's, the modality parameters are taken
 * from the file, classes already present are left alone. */
int lm_save_yaml(const lm_detector* det, const char* path);
int lm_load_yaml(lm_detector* det, const char* path);
/* Top-level entries of a cv::FileStorage YAML file (plain or .gz): what the reference reads with fs["key"] >> x
 * from linemod_settings.yml (utility.cpp), models/<name>.yml (HighLevelLinemod.cpp:523-543) and
 * benchmark/pose0.yml.  Numbers: a scalar, a flow sequence, or the data of an !!opencv-matrix. */
int lm_yaml_numbers(const char* path, const char* key, double* out, size_t cap, size_t* n_out);
int lm_yaml_string(const char* path, const char* key, char* out, size_t cap);

/* ---- stage-level hooks (parity tests diff intermediate buffers against the oracle) ------------ */
/* a3 ColorGradient quantisation of an arbitrary w x h BGR image (dense).  magnitude may be NULL. */
int lm_stage_color_quantize(lm_detector* det, const uint8_t* bgr, int w, int h, float weak_threshold,
                            uint8_t* quantized, float* magnitude);
/* a4 cv::pyrDown of a dense BGR image -> (w/2) x (h/2) */
int lm_stage_pyrdown(lm_detector* det, const uint8_t* bgr, int w, int h, uint8_t* out);
/* a5 DepthNormal quantisation of a dense uint16 image */
int lm_stage_depth_quantize(lm_detector* det, const uint16_t* depth, int w, int h, uint8_t* quantized);
/* a8+a9+a10 spread(T) -> response maps -> linearize; out is 8 * T*T * (w/T)*(h/T) bytes [ori][memory][pos] */
int lm_stage_linear_memories(lm_detector* det, const uint8_t* quantized, int w, int h, int T, uint8_t* out);
/* Runs a3-a10 on the frame in `slot` and stops (no matching). */
int lm_prepare_slot(lm_detector* det, int slot);
/* Reads back an intermediate buffer of `slot` after lm_prepare_slot / lm_match_slot:
 * what 0 = quantized image [h][w], 2 = linear memories [ori][memory][pos] (pads stripped).
 * Returns the byte size in *size_out; copies min(size, cap). */
int lm_debug_read(lm_detector* det, int slot, int what, int level, int modality, uint8_t* out, size_t cap,
                  size_t* size_out);
/* a11-a13 only: candidates of the global scan at the lowest level as (template_id, class_idx, x, y)
 * quadruples of int32, sorted; for parity tests of the scan kernel in isolation. */
int lm_stage_scan(lm_detector* det, int slot, float threshold, int class_idx, int32_t* out, size_t cap_records,
                  size_t* n_out);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------- */
/* Times `iters` back-to-back launches of the similarity-scan kernel alone on the linear memories of
 * `slot` with HIP events on the launch stream; returns the average launch duration in microseconds
 * and the algorithmic bytes one launch reads (sum over templates/modalities of F*P). */
int lm_time_scan(lm_detector* det, int slot, float threshold, int class_idx, int iters, int variant,
                 double* avg_us_out, double* algorithmic_bytes_out);
/* The same over a batch of PREPARED slots (one launch = n_slots frames, what a lane-step launches); candidates are
 * counted, not stored.  variant 8 | 64 runs the exhaustive scan WITHOUT its shift-undo instructions -- wrong sums, a
 * timing experiment only (the upper bound of what pre-shifted copies of the linear memories could save). */
int lm_time_scan_batch(lm_detector* det, int first_slot, int n_slots, float threshold, int class_idx, int iters, int variant,
                       double* avg_us_out);
/* Self-test (no upstream counterpart): the depth-normal kernel's float tail takes 1 / len and sqrt by sequences that drop the
 * compiler's exponent-range handling; this runs every float of the tail's domain through both forms on the device, the reference
 * being the correctly rounded 1.0f / x and sqrtf.  out[0] / out[1] = number of floats whose reciprocal / square root differ
 * (0 / 0 expected); out[2] = floats on which the bare v_sqrt_f32 instruction differs (information only: the kernel does not
 * rely on it); out[3], out[4], out[5] = the same counts for the longer sequences the kernel used before (v_rcp + six fused steps;
 * v_sqrt + the +-1 ulp fix-up) and for v_sqrt + one step with v_rsq: all 0 expected; out[6] = floats on which a REJECTED candidate
 * (the reciprocal taken from the root's own v_rsq plus one Newton step) differs -- non-zero (84) by design: it shows that the sweep
 * discriminates; out[7] = 0.  The 8-word form dates from lm_version "0.3": a caller built against an older header passes 2 words. */
int lm_selftest_float_tail(lm_detector* det, uint64_t out[8]);
/* Per-stage average microseconds of the last lm_match_slot-style pipeline, measured with HIP events
 * over `iters` runs: out[0]=preprocess (a3-a10), out[1]=scan, out[2]=refine, out[3]=sort+copy. */
int lm_time_stages(lm_detector* det, int slot, float threshold, int class_idx, int iters, double out_us[4]);
/* Live profile of lm_match / lm_match_slot / lm_match_batch: when enabled every call brackets its
 * stages with HIP events on the launch stream and accumulates, per call: stage_us[0] preprocess
 * (a3-a10), [1] similarity scan (ONE kernel launch covering all frames of the call), [2] refinement,
 * [3] sort+publish; the algorithmic bytes the scan launches read; launches and frames.
 * lm_set_profiling(det, x) also resets the accumulators. */
int lm_set_profiling(lm_detector* det, int enable);
int lm_get_profile(lm_detector* det, double stage_us[4], double* scan_algorithmic_bytes, int64_t* launches,
                   int64_t* frames);
/* Accumulated with the profile above: HIP-event span of the exchange of lm_match_begin_gathered (behind the sort
 * kernel: k_pack_lists, the two ncclAllGather, the two D2H copies), the number of exchanges, and (counted with
 * profiling off too) how many lane-steps needed the sized second exchange because a rank's lists overflowed the
 * fixed gather capacity or a frame was left to the host sort (raise recs_per_frame_cap if that is the common case). */
int lm_get_exchange_profile(lm_detector* det, double* exchange_us, int64_t* exchanges, int64_t* fallbacks);
/* Work counters since lm_set_profiling: out[0] frames that went through a3-a10, out[1] scan launches, out[2]
 * refinement launches, out[3] sort launches (they count with profiling off too). */
int lm_get_stage_counts(lm_detector* det, int64_t out[4]);
/* Debug: HIP resources the library holds in this process right now -- out[0] device buffers, out[1] pinned host buffers, out[2]
 * streams, out[3] events -- over all detectors, the blocks of lm_device_alloc / lm_host_alloc included.  Takes no detector and
 * needs no device; after the last lm_destroy and the last lm_*_free every count is back where it was before the first lm_create. */
int lm_debug_live_resources(int64_t out[4]);
/* Debug: how often the kernels of the ingest routes and of lm_export_frames have been launched in this process, over all detectors --
 * out[0 .. 4] the kernels of a colour family on any route (k_ingest / k_rectify / k_reduce / k_rectify_reduce and their _yuv, _bayer, _raw,
 * _float forms, in that order: RGB, grey and YUV, Bayer, raw, float), out[5] k_reduce_conv (the reduced route's kernel for every family
 * but RGB), out[6] k_export, out[7] k_export_float.  A kernel is launched only when the call has a frame for it: a call without float
 * frames leaves out[4] and out[7] as they are.  Takes no detector; the counts only grow. */
int lm_debug_launch_counts(int64_t out[8]);
/* Bytes the similarity scan's vector loads request per frame for `class_idx` (-1 = all classes): the on-chip
 * (L2 -> L1) traffic of the hot kernel, next to the algorithmic bytes lm_get_profile reports. */
int lm_scan_load_bytes(lm_detector* det, int class_idx, double* bytes_per_frame);
/* Counters of the last match on `slot`: scan candidates and refined matches before sort + unique. */
int lm_last_counts(lm_detector* det, int slot, uint32_t* candidates, uint32_t* matches_before_unique);
/* The nibble scan kernel stops loading a work item's features as soon as NO position it holds can still exceed the raw
 * threshold (partial sum + 4 x features to come <= threshold: exact, the candidate list never changes).  With the
 * statistics switched on every wave adds the (feature, work item) loads it made and the loads an exhaustive scan makes
 * to device counters (per wave pair of frames; lm_set_scan_stats also zeroes them). */
int lm_set_scan_stats(lm_detector* det, int enable);
int lm_get_scan_stats(lm_detector* det, uint64_t* features_loaded, uint64_t* features_unpruned);
/* The same at lane granularity (nibble kernel): with per-lane pruning a lane none of whose 32 positions can still reach
 * the threshold leaves the exec mask of the loads that follow.  lane_loads_issued: 16-byte lane-loads really made (a live
 * lane's right neighbour included); lane_loads_unpruned: 64 x the feature loads of an exhaustive scan. */
int lm_get_scan_lane_stats(lm_detector* det, uint64_t* lane_loads_issued, uint64_t* lane_loads_unpruned);
/* r05, the bit-plane scan (LM_TUNE_SCAN_FORM): out[0] = scan launches of lm_match* that took k_scan1 and out[1] = all of them since
 * the detector was created; out[2] = positions that survived k_scan1's miss bound and had their exact sums taken since
 * lm_set_scan_stats(1) (a superset of the candidates); out[3] = lanes per frame of the last scan launch (0: it was k_scan4). */
int lm_get_scan_form_stats(lm_detector* det, int64_t out[4]);
/* Selects the similarity-scan kernel variant used by lm_match* (0 = default; bits 0-1: features per load block;
 * bit 3 (value 8): no pruning, the plain exhaustive scan; bit 4 (value 16): wave-level pruning only, without the
 * per-lane exec masking; bit 5 (value 32): per-lane pruning also for one-modality detectors, which default to the
 * wave-level rule; see lm_k_scan.hip).  Bits 0-5 address the nibble scan k_scan4; bit 8 (value 256), the bit-plane scan k_scan1: the
 * waves take their survivors' exact sums themselves instead of queueing them for k_scan1_exact.  Every variant this call accepts gives
 * the SAME lists as variant 0.  The two timing experiments that skip work -- bit 6 (value 64, with bit 3: k_scan4 without its shift-undo)
 * and bit 7 (value 128: k_scan1 without the survivors' exact sums) -- and unknown bits are refused with LM_ERR_INVALID (r06): they exist
 * only as the `variant` argument of lm_time_scan / lm_time_scan_batch, which count candidates and store none. */
int lm_set_scan_variant(lm_detector* det, int variant);

/* ---- ICP pose refinement (0.5; HighLevelLinemodIcp of the reference pipeline).
 * lm_icp_set_model keeps the model cloud of a class resident: rows 0, step, 2 step, ... (n / step rows) of xyzn, n rows of
 * x y z nx ny nz (the PLY's vertices with their normals).  lm_icp_refine refines, per query, num_poses poses (4x4 row-major doubles,
 * in place, from poses[16 * first_pose]) of the query's class against the scene cloud of the query's bbox in the depth frame the
 * slot holds.  That frame is the principal-point-shifted one, so the intrinsics used are (fx, fy, width / 2, height / 2); the query's
 * cx, cy are not read.  The call is synchronous and runs on a stream of its own, ordered after the slot's last upload; an upload to
 * the slot from another thread while it runs is refused (LM_ERR_INVALID).  It is the one-slot case of lm_icp_refine_slots below: the
 * queries of a call run side by side in the same launches.
 * Errors: LM_ERR_INVALID for an empty or out-of-frame bbox, a class without a model, bad parameters, or a scene cloud of fewer than 6
 * points (that query's poses are left unchanged; every other query is refined); LM_ERR_OVERFLOW when a cloud exceeds lm_icp_params'
 * limits (that query's poses are left unchanged too).  With several such queries the code of the first in query order is returned.  A level of fewer than 6 pairs ends that level for that pose, which is the contract's own stop, not an error.
 * Cost: the normals and the 1-NN are exact brute force, O(points^2) per query (measured: 7012 scene points, one pose, 5.1 ms per call).
 * max_points = 0 caps a scene cloud at LM_ICP_DEFAULT_MAX_POINTS points (about 0.1 s of normals); a larger bbox fails with
 * LM_ERR_OVERFLOW unless the caller raises max_points and accepts the quadratic cost.
 * Threading: like the rest of the detector, the lm_icp_* calls belong to its owner thread.  lm_icp_set_model, lm_icp_refine and the two
 * stage hooks share the ICP scratch and models without a lock; the only cross-thread rule is the refusal of uploads named above. */
#define LM_ICP_DEFAULT_MAX_POINTS 32768
typedef struct lm_icp_query {
    int32_t x, y, width, height;   /* bbox in the frame's pixels: must lie inside the frame, width and height > 0 */
    int32_t class_idx;
    int32_t first_pose, num_poses;
    int32_t reserved;
    double fx, fy, cx, cy;         /* intrinsics (cx, cy: lm_stage_icp_refine_host and lm_stage_icp_scene only) */
} lm_icp_query;
typedef struct lm_icp_params {
    int32_t step;                  /* icp subsampling factor of the scene cloud (linemod_settings.yml), >= 1 */
    int32_t iterations;            /* ICP(iterations, tolerance, rejection_scale, levels): the reference's 6, 0.1, 2.5, 8 */
    double tolerance;
    double rejection_scale;
    int32_t levels;
    int32_t max_points;            /* capacity of a scene cloud (0: min(bbox pixels / step, LM_ICP_DEFAULT_MAX_POINTS)) */
} lm_icp_params;
int lm_icp_set_model(lm_detector* det, int class_idx, const float* xyzn, int n, int step);
int lm_icp_refine(lm_detector* det, int slot, const lm_icp_query* queries, int n_queries, const lm_icp_params* params, double* poses);
/* lm_icp_refine over a batch of frames (0.13 additive): query k is refined against the resident depth frame of
 * slots[k] under exactly lm_icp_refine's rule -- the principal-point-shifted frame of that slot, read with the intrinsics
 * (fx, fy, width / 2, height / 2); the query's cx, cy are not read.  The queries are independent and run side by side in the same
 * launches (in chunks of LM_TUNE_ICP_BATCH_MB of scratch); a pose's result does not depend on the queries it shares a call with, and
 * equals lm_icp_refine's on that slot byte for byte.  Queries whose pose ranges overlap run one after the other, in query order.
 * status (may be NULL) receives one code per query: LM_OK; LM_ERR_INVALID for a scene cloud of fewer than 6 points; LM_ERR_OVERFLOW for a
 * cloud over the capacity.  The poses of a query that is not LM_OK stay byte for byte; every other query is refined.  The call returns
 * LM_OK when all queries are, otherwise the code of the first non-OK query in query order, lm_last_error naming that query.
 * Refused with LM_ERR_INVALID before anything is enqueued or claimed, poses and status untouched: null arguments with n_queries > 0, or
 * n_queries < 0; bad parameters; a slot out of range or without a frame; a colour-only detector that keeps no depth (lm_keeps_depth() == 0), or a slot whose frame
 * came without a depth image; an empty or out-of-frame bbox; a class
 * without a model; a bad pose range or bad intrinsics; an ICP call already in flight.  n_queries == 0 is legal, and so is a query with
 * num_poses == 0 (LM_OK).  Synchronous, on the ICP's stream, ordered after the last upload of every distinct slot named; while it runs,
 * uploads from other threads to the span [min slot, max slot] are refused (lm_icp_refine and lm_icp_verify claim their spans alike). */
int lm_icp_refine_slots(lm_detector* det, const int32_t* slots, const lm_icp_query* queries, int n_queries, const lm_icp_params* params,
                        double* poses, int32_t* status /* may be NULL */);
/* Stage hook: out[3] = the chunks, kernel launches and host synchronisations of the detector's last refinement (any of the three calls). */
int lm_stage_icp_batch_stats(lm_detector* det, int32_t* out);
/* Stage hooks: the scene cloud of one bbox of a host depth frame (w x h, uint16 mm) with intrinsics K = (fx, fy, cx, cy):
 * out[*n_out][6]; LM_ERR_OVERFLOW (and *n_out = the count) when it exceeds cap rows.  lm_stage_icp_refine_host = lm_icp_refine on a host
 * depth frame of the detector's size with the queries' own cx, cy. */
int lm_stage_icp_scene(lm_detector* det, const uint16_t* depth, int w, int h, const double* K, const int32_t* bbox, int step, float* out,
                       size_t cap, int* n_out);
int lm_stage_icp_refine_host(lm_detector* det, const uint16_t* depth, const lm_icp_query* queries, int n_queries, const lm_icp_params* params,
                             double* poses);

/* ---- Template-bank generation on the GPU (0.6): the same bank as the host generator (TemplateGenerator.cpp
 * generate_templates = SoftRender + HighLevelLineMOD::addTemplate per viewpoint), bit for bit.
 * lm_set_render_mesh keeps a triangle mesh resident under mesh_idx (0 .. LM_MAX_RENDER_MESHES - 1): xyz[n_vertices][3], indices[n_indices]
 * (triangles; every index < n_vertices).  lm_add_templates_rendered renders the mesh under view_proj[n_views][16] (projection * view,
 * column-major as SoftRender's Mat4, computed on the host) at the detector's frame size, rotates every view by every angle
 * (angles_deg[n_angles], addTemplate's in-plane sweep), extracts the templates and adds them to class_id in the order view-major,
 * angle-minor -- the host generator's order.  Like addTemplate, a view stops at its first angle whose extraction fails: that template
 * and the view's later angles get template_ids_out[v * n_angles + a] = -1 and are not added (lm_last_error() then names the failure,
 * the call itself returns LM_OK).  bboxes_out[k] = the added template's bbox; crops_out receives, packed, the rotated depth image of
 * every added template cropped to its bbox (clipped to the frame, row-major), crop_offsets_out[k] = where template k's crop starts,
 * crop_offsets_out[n_views * n_angles] = the total (elements).  LM_ERR_OVERFLOW (nothing added, the total in
 * crop_offsets_out[n_views * n_angles]) when the crops exceed crop_capacity elements.  Needs the detector's frame slots: the images are
 * processed in chunks of at most frame_slots, and every slot's frame is consumed. */
#define LM_MAX_RENDER_MESHES 16
int lm_set_render_mesh(lm_detector* det, int mesh_idx, const float* xyz, int n_vertices, const uint32_t* indices, int n_indices);
int lm_add_templates_rendered(lm_detector* det, const char* class_id, int mesh_idx, const float* view_proj, int n_views,
                              const float* angles_deg, int n_angles, int* template_ids_out, lm_rect* bboxes_out, uint16_t* crops_out,
                              size_t crop_capacity, size_t* crop_offsets_out);
/* Stage hooks: SoftRender::render_view of a resident mesh at w x h (coverage 255 / 0 = the colour image's channels, depth in mm), and
 * warp_rotate_u8 (one channel) + warp_rotate_u16 of a w x h image pair by angle_deg. */
int lm_stage_render(lm_detector* det, int mesh_idx, const float* view_proj, int w, int h, uint8_t* coverage, uint16_t* depth);
int lm_stage_rotate(lm_detector* det, const uint8_t* src8, const uint16_t* src16, int w, int h, float angle_deg, uint8_t* dst8,
                    uint16_t* dst16);

/* ---- Pose-error evaluation on the GPU (0.7): the reference's Benchmark (Benchmark.cpp) metrics, batched.
 * lm_pose_error_vsd: the error of Hodan et al. (calculateErrorHodan).  Per query, the resident render mesh mesh_idx (lm_set_render_mesh)
 * is rendered under view_proj_gt and view_proj_est (projection * view, column-major like lm_add_templates_rendered's, computed on the
 * host) at w x h, exactly as lm_stage_render renders it, and compared with depth[frame] (depth: n_frames frames of h x w uint16 mm,
 * row-major) by calculateVisibilityMasks' rules on 16-bit data: saturating subtractions, occluded where render - scene > delta,
 * rendered where render > 1, an estimate pixel also visible where the GT is visible and the estimate render is non-zero, within where
 * |gt - est| <= tau.  error = 1.f - (float)within_tau / (float)combination in float: NaN when the union is empty (the reference's 0 / 0).
 * lm_pose_error_add: ADD (symmetric = 0, calculateErrorLM) or ADD-S (symmetric = 1, calculateErrorLMAmbigous) over the vertices 0, step,
 * 2 step, ... (m = ceil(n_vertices / step)) of the resident render mesh: per vertex |R_gt v + t_gt - (R_est v + t_est)| (ADD) or the
 * smallest distance from the GT vertex to any estimate vertex, starting from the reference's 999999 (ADD-S); mean_out[q] = (float)(the
 * double sum / m).  R row-major; the per-vertex float expression is DESIGN.md section 11's contract.  per_vertex_out [n][m] may be null.
 * lm_stage_vsd_counts: the counting rule alone on host images (gt, est, scene: h x w uint16).
 * The calls are synchronous, belong to the detector's owner thread and run on a stream of their own; they touch no frame slot or lane.
 * Errors: LM_ERR_INVALID for a bad mesh index, a bad frame index or size, step < 1 or null pointers; n = 0 does nothing. */
typedef struct lm_vsd_query {
    int32_t frame, mesh_idx;
    float view_proj_gt[16];
    float view_proj_est[16];
} lm_vsd_query;
typedef struct lm_vsd_result {
    uint32_t rendered_gt, rendered_est;   /* render > 1 */
    uint32_t visible_gt, visible_est;
    uint32_t intersection, combination;   /* visible in both / in either (the reference's visibilityCombination) */
    uint32_t within_tau;                  /* visible in both with |gt - est| <= tau */
    float error;
} lm_vsd_result;
typedef struct lm_add_query {
    float R_gt[9], t_gt[3];
    float R_est[9], t_est[3];
} lm_add_query;
int lm_pose_error_vsd(lm_detector* det, const uint16_t* depth, int n_frames, int w, int h, const lm_vsd_query* queries, int n, int delta, int tau,
                      lm_vsd_result* results);
int lm_pose_error_add(lm_detector* det, int mesh_idx, int step, int symmetric, const lm_add_query* queries, int n, float* mean_out,
                      float* per_vertex_out);
int lm_stage_vsd_counts(lm_detector* det, const uint16_t* gt_depth, const uint16_t* est_depth, const uint16_t* scene, int w, int h, int delta,
                        int tau, lm_vsd_result* out);

/* ---- Best-pose check of the ICP branch on the GPU (0.8): HighLevelLinemodIcp::estimateBestMatch's mean depth
 * difference, batched.  Per query, the resident render mesh mesh_idx (lm_set_render_mesh) is rendered under view_proj (projection *
 * view, column-major, computed on the host, as for lm_pose_error_vsd), exactly as lm_stage_render renders it, and compared with the
 * query's depth frame:  m0 = render > 1 && scene > scene_min (the reference's 600);  mask = m0 eroded 3x3 twice, a neighbour outside
 * the image counting as set (cv::erode's default border: the border does not erode);  count = the mask's pixels, sum = the sum of
 * |scene - render| over them (integers), mean = count ? (double)sum / (double)count : 0.0 (computed on the host).
 * lm_stage_icp_verify_host: depth = n_frames images of h x w uint16 mm, query.frame indexes them.
 * lm_icp_verify: query.frame is a frame slot; the render has the detector's frame size.  Its chunks run across the slots: like
 * lm_icp_refine_slots it is ordered after the last upload of every distinct slot named, and uploads from another thread to the span
 * [min slot, max slot] are refused while it runs.
 * lm_stage_icp_verify_counts: the counting rule alone on host images (render, scene: h x w uint16), like lm_stage_vsd_counts.
 * The calls are synchronous, run on the ICP's stream and follow the threading rule of lm_icp_* above (they share its scratch).
 * Errors: LM_ERR_INVALID for a bad mesh index or a mesh that is not resident, a bad frame or slot index, a slot without a depth frame
 * or a detector that keeps no depth frame, or a slot whose frame came without one (slot form), w or h < 1, null pointers; n = 0 does nothing. */
typedef struct lm_icp_verify_query {
    int32_t frame;                 /* index into depth (host form) or frame slot (lm_icp_verify) */
    int32_t mesh_idx;
    float view_proj[16];
} lm_icp_verify_query;
typedef struct lm_icp_verify_result {
    uint32_t count;
    uint32_t reserved;
    uint64_t sum;
    double mean;
} lm_icp_verify_result;
int lm_stage_icp_verify_host(lm_detector* det, const uint16_t* depth, int n_frames, int w, int h, const lm_icp_verify_query* queries, int n,
                             int scene_min, lm_icp_verify_result* results);
int lm_icp_verify(lm_detector* det, const lm_icp_verify_query* queries, int n, int scene_min, lm_icp_verify_result* results);
int lm_stage_icp_verify_counts(lm_detector* det, const uint16_t* render, const uint16_t* scene, int w, int h, int scene_min,
                               lm_icp_verify_result* out);

/* ---- Frames that already live in DEVICE memory, in the producer's format (0.10): a decoder, a renderer, a
 * simulator, a tensor pipeline -- or a camera frame copied to the device as the driver delivered it.  ONE kernel launch per call turns
 * n_slots source frames into the slots' resident frames (dense BGR8, and uint16 millimetres on an RGB-D detector):
 *     device image(s) -> crop -> channel order -> float-to-u16 -> mirror -> shift -> slot
 * Per image, output pixel (x, y) of the cfg.width x cfg.height frame (W, H):
 *     xs = x - shift_x, ys = y - shift_y;  outside [0, W) x [0, H): 0       (zeros shifted in, as lm_upload_frame_shifted)
 *     u  = flip_x ? W - 1 - xs : xs                                         (cv::flip(.., 1) of the cropped window)
 *     p  = source pixel (crop_x + u, crop_y + ys);   colour: (B, G, R) of p,   depth: to_u16(p)
 * -- the reference's order: convert, crop, flip (Kinect2.cpp:52-60), then translate (PoseDetection.cpp:54-59).
 * to_u16 of LM_PIX_DEPTH_F32: t = v * scale (one IEEE single-precision multiply); 0 if t is NaN, +-inf or <= 0; 65535 if t >= 65535;
 * otherwise t rounded to nearest, ties to even.  LM_PIX_DEPTH_U16 is copied as it is.
 * (Float COLOUR sources, LM_PIX_*_F32 / _F16, take the same road through to_u8: "Float colour sources" below.)
 * Formats: BGR8 / RGB8 interleaved, 3 bytes per pixel; BGRA8 / RGBA8 interleaved, 4 bytes per pixel, alpha ignored; BGR8_PLANAR /
 * RGB8_PLANAR three planes plane_stride bytes apart in the named order; DEPTH_U16 / DEPTH_F32 one channel.  8-bit sources may have ANY
 * byte alignment of data, row_stride and plane_stride; u16 / f32 sources must be naturally aligned (data and strides multiples of 2 / 4).
 * The frame width must be a multiple of 16 (every two-level configuration's is).
 *
 * Grey and YUV colour sources (0.12), what a mono camera, a video decoder (NV12) and a UVC or RealSense colour stream (YUY2, UYVY)
 * deliver.  Valid in `colour` only, 8-bit, any byte alignment like the other 8-bit formats:
 *     GRAY8   1 byte per pixel; B = G = R = the byte (cvtColor(GRAY2BGR))
 *     NV12    the Y plane at data, 1 byte per pixel; the interleaved chroma plane at data + plane_stride (> 0), half as many rows.  Both
 *             planes have row_stride.  Pixel (x, y) takes chroma row y >> 1: byte 2 * (x >> 1) of it is U, the next byte is V.
 *     NV21    as NV12, V first and then U
 *     YUY2    packed 4:2:2: the 4 bytes at 4 * (x >> 1) of row y are Y0 U Y1 V; pixel x takes Y0 when x is even and Y1 when it is odd
 *     UYVY    the same with the bytes U Y0 V Y1
 * Chroma is REPLICATED (the nearest sample, no interpolation), as cvtColor(COLOR_YUV2BGR_NV12 / _NV21 / _YUY2 / _UYVY) does.
 * LM_PIX_YUV_BT709 and LM_PIX_YUV_FULL may be ORed into the format of NV12 .. UYVY, and of those alone: they choose the row of
 *     matrix / range                 Y0   CY        CVR       CVG       CUG       CUB
 *     BT.601 limited (no flag)       16   1220542   1673527   -852492   -409993   2116026     OpenCV's ITUR_BT_601_* constants
 *     BT.709 limited (BT709)         16   1220945   1879825   -558796   -223607   2215014     round(coefficient * 2^20)
 *     BT.601 full (FULL; JPEG)        0   1048576   1470104   -748826   -360853   1858077     of the standard matrices
 *     BT.709 full (BT709 | FULL)      0   1048576   1651297   -490864   -196424   1945738
 * and a pixel with the samples Y, U, V becomes, in 32-bit signed integers (>> an arithmetic shift, sat8 a clamp to [0, 255]):
 *     y = max(0, Y - Y0) * CY;   u = U - 128;   v = V - 128
 *     R = sat8((y + (1 << 19) + CVR * v) >> 20)
 *     G = sat8((y + (1 << 19) + CVG * v + CUG * u) >> 20)
 *     B = sat8((y + (1 << 19) + CUB * u) >> 20)
 * The order stays convert, crop, flip, shift: ingesting a YUV image equals ingesting, as LM_PIX_BGR8 with the same window, mirror and
 * shift, the BGR image this rule yields from the whole source.  crop_x, crop_y and the shifts may be odd: a window that starts on the
 * second pixel of a chroma pair, or on the second row of a 4:2:0 pair, reads the chroma of the pair that covers it.  The source's width
 * (NV12 / NV21: and height) must be even.  Any other value of `format` -- a flag on another format, any other bit, a negative value --
 * is an unknown pixel format.
 *
 * Raw Bayer colour sources (0.13 additive), what a machine-vision camera (GigE Vision, USB3 Vision, CoaXPress) delivers: GenICam's
 * BayerRG8 / BayerGR8 / BayerGB8 / BayerBG8.  Valid in `colour` only; one byte per pixel, row_stride >= width, data and row_stride of
 * any byte alignment, plane_stride ignored; the source's width and height must be even (and so at least 2).
 *     LM_PIX_BAYER_RGGB8 = 16, LM_PIX_BAYER_GRBG8 = 17, LM_PIX_BAYER_GBRG8 = 18, LM_PIX_BAYER_BGGR8 = 19
 * are named by the colours of the source's top-left 2 x 2 tile in reading order; format - 16 = red_x | red_y << 1 gives the place of the
 * red sample inside the tile.  13, 14 and 15 name no format, and a YUV flag ORed onto a Bayer format is an unknown pixel format.
 * The demosaic is the classic bilinear one, of the WHOLE source, in 32-bit integers.  Let S(x, y) be the source byte with coordinates
 * reflected without repeating the edge (-1 -> 1, w -> w - 2, rows alike: an even distance, so the colour of a site is kept).  Per pixel:
 *     c = S(x, y)
 *     h = (S(x-1,y) + S(x+1,y) + 1) >> 1
 *     v = (S(x,y-1) + S(x,y+1) + 1) >> 1
 *     p = (S(x-1,y) + S(x+1,y) + S(x,y-1) + S(x,y+1) + 2) >> 2
 *     d = (S(x-1,y-1) + S(x+1,y-1) + S(x-1,y+1) + S(x+1,y+1) + 2) >> 2
 *     dx = (x ^ red_x) & 1,  dy = (y ^ red_y) & 1
 *     (dx, dy) = (0, 0)  red site:             R = c, G = p, B = d
 *                (1, 1)  blue site:            B = c, G = p, R = d
 *                (1, 0)  green in a red row:   G = c, R = h, B = v
 *                (0, 1)  green in a blue row:  G = c, B = h, R = v
 * The order stays convert, crop, flip, shift: ingesting a Bayer image equals ingesting, as LM_PIX_BGR8 with the same window, mirror and
 * shift, the BGR image this rule yields from the whole source.  The neighbours of a window pixel come from the source OUTSIDE the window;
 * only the source's own edges reflect.  crop_x, crop_y and the shifts may be odd.  Parity with cv::cvtColor(COLOR_Bayer*2BGR) is not
 * claimed (its border handling differs); edge-aware demosaics are not served.  (Bayer in 16-bit containers and bit-packed: below.)
 *
 * High-bit raw sources and the raw pipeline (0.13 additive): what such a camera delivers at its sensor's 10 .. 16 bits -- GenICam's
 * BayerRG10 / 12 / 14 / 16 and Mono10 .. Mono16 in 16-bit containers, BayerRG10p / 12p and Mono10p / 12p bit-packed (PFNC).  Colour
 * formats, valid in `colour` only:
 *     format = LM_PIX_RAW | storage | pattern,   LM_PIX_RAW = 0x1000
 *     pattern (bits 0 .. 3): 0 .. 3 = red_x | red_y << 1, exactly as format - 16 of the 8-bit Bayer formats; 4 = mono; 5 .. 15 name nothing
 *     storage (bits 4 .. 7): 0x00 10 bits in a u16, 0x10 12 bits in a u16, 0x20 14 bits in a u16, 0x30 16 bits in a u16,
 *                            0x40 10-bit packed (PFNC "10p"), 0x50 12-bit packed ("12p"); 0x60 and above name nothing
 * Every other bit set, a YUV flag included, is an unknown pixel format.  The thirty values are named below (LM_PIX_BAYER_RGGB10 ..
 * LM_PIX_MONO12P).  N = the sample's bits.
 *   Container (u16): little-endian, the sample in the low N bits; a sample is min(s, 2^N - 1) -- stray high bits clamp, they do not wrap.
 *     data and row_stride are multiples of 2 and row_stride >= 2 * width.
 *   Packed: row y starts at data + y * row_stride, bit 0; sample c of a row is bits [N c, N c + N) of the row read as a little-endian bit
 *     string: ((b[k] | b[k+1] << 8) >> (N c & 7)) & (2^N - 1) with k = N c >> 3 (12p: the familiar "two pixels in three bytes").  Any byte
 *     alignment of data and row_stride; row_stride >= ceil(width * N / 8).  The 10p samples 1, 2, 3, 1023 are the bytes 1, 8, 48, 192, 255;
 *     the 12p samples 0xABC, 0x123 are the bytes 0xBC, 0x3A, 0x12.
 *   A Bayer source has even width and height; mono may have any size.  `width` above is the SOURCE's: a row holds the whole source row.
 * The raw pipeline (lm_set_raw_processing; integers only, >> an arithmetic shift, every step 32-bit), per source:
 *     1. s' = max(s - black, 0) on every unpacked sample
 *     2. Bayer: the bilinear rule above on s' (c, h, v, p, d, the reflection and the site table verbatim) gives N-bit (R, G, B); the
 *        largest sum is 4 * 65535 + 2.   Mono: R = G = B = s'
 *     3. x_c = v_c << (16 - N)
 *     4. x'_c = min((x_c * gain[c] + 512) >> 10, 65535)                                 unsigned: 65535 * 65535 + 512 < 2^32
 *     5. y_i = clamp((ccm[3i] * x'_R + ccm[3i+1] * x'_G + ccm[3i+2] * x'_B + 512) >> 10, 0, 65535)   signed: |sum| <= 3 * 8192 * 65535 + 512 < 2^31
 *     6. out_i = tone[y_i >> 4];  the slot stores (B, G, R) = (out_2, out_1, out_0)
 * The identity -- black 0, gains 1024, the matrix 1024 * I, tone[i] = i >> 4 -- yields v >> (N - 8): what a high-bit source gets while
 * nothing is set.  While a pipeline IS set it also applies to the 8-bit Bayer formats, with N = 8 (the identity gives them the bytes
 * they get with nothing set, from the unchanged kernel).  LM_PIX_GRAY8 is not a raw format and is never processed.
 * The order stays convert, crop, flip, shift: ingesting a raw image equals ingesting, as LM_PIX_BGR8, the image this rule yields from the
 * WHOLE source.  On the rectified route a tap is the processed pixel (the conversion comes before the blend, as for every format) and 0
 * outside the source; the registered route's colour images are the plain ingest's.
 * Pins.  The 12-bit source [[100, 2000], [3000, 4095]], black 64, gains (2048, 1024, 1536), ccm 1536 on the diagonal and -256 elsewhere,
 * tone[i] = (7 i + 3) & 255.  As RGGB, (B, G, R) in reading order: (252,111,3) (252,237,3) (252,241,3) (252,111,3), from the N-bit
 * (R, G, B) (36,2436,4031) (36,1936,4031) (36,2936,4031) (36,2436,4031).  As mono: (125,157,86) (107,25,252) (252,111,252) (252,85,252).
 * As RGGB12 with the identity and black 0: (255,156,6) (255,125,6) (255,187,6) (255,156,6).
 * Not served: MIPI CSI-2 RAW10 / RAW12 packing, MSB-aligned containers, lens shading, per-site black levels.
 *
 * Float colour sources (0.13 additive), what a tensor pipeline holds (float32 / float16, [3, H, W] or [H, W, 3 | 4], values in 0 .. 1 or
 * 0 .. 255) and what a renderer or a simulator draws into (RGBA16F, RGBA32F).  Colour formats, valid in `colour` only:
 *     format = LM_PIX_FLOAT | element | layout,   LM_PIX_FLOAT = 0x2000
 *     layout (bits 0 .. 3): the value of the 8-bit format with the same memory order -- 0 BGR interleaved, 1 RGB interleaved, 2 BGRA,
 *                           3 RGBA (alpha ignored), 4 BGR planar, 5 RGB planar, 8 grey (B = G = R); 6, 7 and 9 .. 15 name nothing
 *     element (bit 4): 0 = IEEE binary32, 0x10 = IEEE binary16, both little-endian
 * Every other bit set, a YUV flag and LM_PIX_RAW included, is an unknown pixel format.  The fourteen values are named below
 * (LM_PIX_BGR_F32 .. LM_PIX_GRAY_F16).  With es = 4 or 2 bytes: interleaved pixels are 3 es or 4 es bytes apart; the planar formats have
 * three planes plane_stride bytes apart in the named order; data, row_stride and, where planes are, plane_stride are multiples of es;
 * row_stride is at least a window row (on the routes that read the whole source: a source row, as for every format).
 * to_u8(v, scale), per channel; scale is the descriptor's field, finite and > 0 (255 for a 0 .. 1 tensor, 1 for 0 .. 255 floats):
 *     1. a binary16 value is converted to binary32 first: exact, subnormals included
 *     2. t = v * scale: ONE IEEE single-precision multiply, rounded to nearest, never fused; subnormal operands and results are honoured
 *     3. 0 if t is NaN or t <= 0 (-0 and -inf too);  255 if t >= 255 (+inf too);  otherwise t rounded to nearest, ties to even
 * +inf is the one deliberate difference from to_u16 of the float depth: there it is a missing measurement (0), here a saturated sample.
 * The order stays convert, crop, flip, shift: ingesting a float image equals ingesting, as LM_PIX_BGR8 with the same window, mirror and
 * shift, the 8-bit BGR image this rule yields from the WHOLE source -- on every route: on the rectified route a tap is the converted
 * pixel and 0 outside the source; on the reduced and the rectify-and-reduce routes the conversion stands in front of the average; the
 * registered route's colour images are the plain ingest's.
 * Pins.  F32, scale 1: 0.5, 1.5, 2.5, 254.5, nextafter(254.5, up), 255, -0.0, NaN, +inf, -inf -> 0, 2, 2, 254, 255, 255, 0, 0, 255, 0.
 * F32, scale 255: 0, 1, 0.5, 0.1f, 0.25, 0.75, -0.2 -> 0, 255, 128, 26, 64, 191, 0.  F32 bits 0x00400000 (2^-127), scale 2^127 -> 1.
 * F16 bits 0x3800, 0x3C00, 0x0001, 0x7C00, 0xFC00, 0x7E00, 0x8000, 0x2E66 at scale 255 -> 128, 255, 0, 255, 0, 0, 0, 25; 0x0001 at scale
 * 2^24 -> 1.  Over all 65536 binary16 bit patterns at scale 255 the outputs sum to 4569216, 16389 are 255, 39940 are 0 and all 256
 * values occur.
 * Not served: bfloat16, 16-bit integer RGB, a transfer curve for linear-light renders, binary16 depth. */
enum {
    LM_PIX_BGR8 = 0, LM_PIX_RGB8 = 1, LM_PIX_BGRA8 = 2, LM_PIX_RGBA8 = 3, LM_PIX_BGR8_PLANAR = 4, LM_PIX_RGB8_PLANAR = 5,
    LM_PIX_DEPTH_U16 = 6, LM_PIX_DEPTH_F32 = 7,
    LM_PIX_GRAY8 = 8, LM_PIX_NV12 = 9, LM_PIX_NV21 = 10, LM_PIX_YUY2 = 11, LM_PIX_UYVY = 12,
    LM_PIX_BAYER_RGGB8 = 16, LM_PIX_BAYER_GRBG8 = 17, LM_PIX_BAYER_GBRG8 = 18, LM_PIX_BAYER_BGGR8 = 19,
    LM_PIX_YUV_BT709 = 0x100, LM_PIX_YUV_FULL = 0x200,
    LM_PIX_RAW = 0x1000,
    LM_PIX_BAYER_RGGB10 = 0x1000, LM_PIX_BAYER_GRBG10 = 0x1001, LM_PIX_BAYER_GBRG10 = 0x1002, LM_PIX_BAYER_BGGR10 = 0x1003, LM_PIX_MONO10 = 0x1004,
    LM_PIX_BAYER_RGGB12 = 0x1010, LM_PIX_BAYER_GRBG12 = 0x1011, LM_PIX_BAYER_GBRG12 = 0x1012, LM_PIX_BAYER_BGGR12 = 0x1013, LM_PIX_MONO12 = 0x1014,
    LM_PIX_BAYER_RGGB14 = 0x1020, LM_PIX_BAYER_GRBG14 = 0x1021, LM_PIX_BAYER_GBRG14 = 0x1022, LM_PIX_BAYER_BGGR14 = 0x1023, LM_PIX_MONO14 = 0x1024,
    LM_PIX_BAYER_RGGB16 = 0x1030, LM_PIX_BAYER_GRBG16 = 0x1031, LM_PIX_BAYER_GBRG16 = 0x1032, LM_PIX_BAYER_BGGR16 = 0x1033, LM_PIX_MONO16 = 0x1034,
    LM_PIX_BAYER_RGGB10P = 0x1040, LM_PIX_BAYER_GRBG10P = 0x1041, LM_PIX_BAYER_GBRG10P = 0x1042, LM_PIX_BAYER_BGGR10P = 0x1043, LM_PIX_MONO10P = 0x1044,
    LM_PIX_BAYER_RGGB12P = 0x1050, LM_PIX_BAYER_GRBG12P = 0x1051, LM_PIX_BAYER_GBRG12P = 0x1052, LM_PIX_BAYER_BGGR12P = 0x1053, LM_PIX_MONO12P = 0x1054,
    LM_PIX_FLOAT = 0x2000, LM_PIX_FLOAT_F16 = 0x10,
    LM_PIX_BGR_F32 = 0x2000, LM_PIX_RGB_F32 = 0x2001, LM_PIX_BGRA_F32 = 0x2002, LM_PIX_RGBA_F32 = 0x2003, LM_PIX_BGR_F32_PLANAR = 0x2004,
    LM_PIX_RGB_F32_PLANAR = 0x2005, LM_PIX_GRAY_F32 = 0x2008,
    LM_PIX_BGR_F16 = 0x2010, LM_PIX_RGB_F16 = 0x2011, LM_PIX_BGRA_F16 = 0x2012, LM_PIX_RGBA_F16 = 0x2013, LM_PIX_BGR_F16_PLANAR = 0x2014,
    LM_PIX_RGB_F16_PLANAR = 0x2015, LM_PIX_GRAY_F16 = 0x2018
};
typedef struct lm_image_desc {
    const void* data;        /* DEVICE pointer to source pixel (0, 0) */
    int64_t row_stride;      /* bytes between rows, > 0 and at least one window row */
    int64_t plane_stride;    /* planar formats: bytes between planes, NV12 / NV21: from the Y plane to the chroma plane, > 0; else ignored */
    int32_t width, height;   /* source size in pixels */
    int32_t format;          /* LM_PIX_*, NV12 .. UYVY: | LM_PIX_YUV_BT709 | LM_PIX_YUV_FULL */
    int32_t crop_x, crop_y;  /* top-left of the cfg.width x cfg.height window inside the source */
    float   scale;           /* DEPTH_F32: millimetres per unit (1 = mm, 1000 = metres); the float colour formats: to_u8's factor; finite, > 0 */
} lm_image_desc;
typedef struct lm_ingest_opts { int32_t flip_x, shift_x, shift_y; } lm_ingest_opts;
/* colour, depth: HOST arrays of n_slots descriptors, frame i -> slot first_slot + i (depth: required on an RGB-D detector, ignored
 * on a colour-only one that keeps no depth; with LM_FLAG_KEEP_DEPTH a colour-only detector takes them if they are there -- NULL is legal and
 * leaves the slots without depth); opts: n_slots entries, or NULL = no mirror, no shift.  Shifts beyond the frame give an all-zero frame.
 * An upload like lm_upload_frames_pinned: asynchronous, one upload ticket for all the slots; every consumer (lm_match_*, the lanes, the
 * mask rules, the colour check, the depth counts) sees an ingested slot as an uploaded one, and the slots' match masks are cleared.
 * producer_stream: NULL = the sources are complete when the call is made; otherwise a hipStream_t -- the ingest waits for the work
 * enqueued on it so far.  The sources must stay unchanged until lm_upload_wait(slot) returns or until work ordered behind
 * lm_ingest_release runs: lm_ingest_release makes `stream` (a hipStream_t) wait for the pending uploads of the slots.
 * Refused (LM_ERR_INVALID, before anything is enqueued): null arrays or n_slots <= 0; an unknown format, a colour format in `depth` or a
 * depth format in `colour`; a window outside the source (the message names the image); an NV12 / NV21 source of odd width or height, a
 * YUY2 / UYVY source of odd width; a Bayer source of odd width or height; a row_stride shorter than a window row (width bytes for
 * GRAY8 / NV12 / NV21, 2 * width for YUY2 / UYVY; a Bayer source: shorter than the source's own width; a high-bit raw source: shorter than
 * 2 * width container bytes or ceil(width * N / 8) packed bytes of the source's own width); a plane_stride <= 0 where planes are; misaligned u16 / f32 / f16 sources (a raw u16 container is a u16 source; a float colour source's plane_stride counts too); a scale that is not finite and positive (float depth and float colour); then the slot refusals of every upload. */
int lm_ingest_frames(lm_detector* det, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                     const lm_ingest_opts* opts, void* producer_stream);
int lm_ingest_release(lm_detector* det, int first_slot, int n_slots, void* stream);
/* The raw pipeline of the raw colour formats (0.13 additive; the rule: above).  lm_set_raw_processing copies *p; NULL resets the
 * pipeline to the identity and to "nothing set" (the 8-bit Bayer formats then take their unprocessed path again).  It holds host state
 * and needs no device: the tables travel with the first ingest that needs them.  It waits for pending uploads.  Refused
 * (LM_ERR_INVALID, the message begins "raw processing:", the previous setting stays): black outside 0 .. 65535; a gain above 65535; a
 * matrix entry outside -8192 .. 8192; a lane with a match in flight.  lm_get_raw_processing returns what the device uses: unset, the
 * identity. */
typedef struct lm_raw_processing {
    int32_t  black;        /* source sample units, 0 .. 65535 */
    uint32_t gain[3];      /* R, G, B;  Q10 (1024 = 1.0), 0 .. 65535 */
    int32_t  ccm[9];       /* row-major, rows = output R, G, B, columns = input R, G, B;  Q10, -8192 .. 8192 */
    uint8_t  tone[4096];
} lm_raw_processing;
int lm_set_raw_processing(lm_detector* det, const lm_raw_processing* p);
int lm_get_raw_processing(lm_detector* det, lm_raw_processing* out);
/* The slot's resident frame as it lies in device memory, dense (bgr_out: H x W x 3, depth_out: H x W; either may be NULL), after the
 * slot's upload has landed.  Synchronous.  depth_out: LM_ERR_INVALID on a detector that keeps no depth frame (lm_keeps_depth() == 0) and
 * for a slot whose frame came without a depth image (LM_FLAG_KEEP_DEPTH; the slot's number is in lm_last_error()). */
int lm_read_frame(lm_detector* det, int slot, uint8_t* bgr_out, uint16_t* depth_out);
/* Device memory on the calling thread's current HIP device, and a synchronous copy (kind 0 host -> device, 1 device -> host, 2 device ->
 * device): for tests and small callers whose frames start on the host in camera format. */
int  lm_device_alloc(size_t bytes, void** out);
void lm_device_free(void* p);
int  lm_device_copy(void* dst, const void* src, size_t bytes, int kind);

/* ---- Resident frames out again, with detections drawn, in the consumer's format (0.13 additive): the mirror image
 * of lm_ingest_frames.  ONE kernel launch per call composites a list of drawing primitives onto the colour frames of slots
 * first_slot .. first_slot + n_slots - 1, undoes the ingest's mirror and shift if asked, converts and writes the result to DEVICE
 * memory the caller owns -- an encoder's NV12 surface, a display's BGRA buffer, a tensor.  No frame touches the host.
 * Everything below is exact integer arithmetic.  F_i = the frame of slot first_slot + i (W x H, dense BGR8).
 * 1. The annotated frame A_i: F_i with the primitives whose `frame` == i applied IN LIST ORDER.  A pixel (x, y) -- integer pixel centres,
 *    FRAME coordinates, where matches and poses live -- that a primitive with colour (b, g, r) and opacity a covers becomes, per channel,
 *        blend(c, p, a) = (t + (t >> 8)) >> 8,   t = c * (255 - a) + p * a + 128
 *    which is round-to-nearest of (c (255 - a) + p a) / 255 (a = 255 gives p, a = 0 gives c).  Later primitives composite over earlier
 *    ones.  Coverage, t = thickness (1 .. 64), every coordinate in [-8192, 8191]:
 *      LM_DRAW_RING     centre (x0, y0), radius r = x1 in 0 .. 8191, y1 == 0.  q = 4 ((x - x0)^2 + (y - y0)^2); covered iff
 *                       q < (2 r + t)^2 and, when 2 r >= t, q >= (2 r - t)^2 (otherwise a disc).  With t = 1 the radii 0 .. 5 cover
 *                       1, 8, 12, 16, 32, 28 pixels.
 *      LM_DRAW_SEGMENT  from A = (x0, y0) to B = (x1, y1): the pixel centre's distance to the segment is at most t / 2, round caps.
 *                       d = B - A, L2 = |d|^2, w = P - A, s = w . d.  L2 == 0 or s <= 0: covered iff 4 |w|^2 <= t^2; else s >= L2:
 *                       iff 4 |P - B|^2 <= t^2; else iff 4 cross^2 <= t^2 L2, cross = w.x d.y - w.y d.x (64-bit).  A t = 1 segment is
 *                       8-connected.  (2,2)-(10,5) covers 10 pixels at t = 1 and 22 at t = 2; a zero-length segment 1, 5, 9 at t = 1, 2, 3.
 *      LM_DRAW_BOX      the outline of the inclusive rectangle x0 <= x <= x1, y0 <= y <= y1 (x0 <= x1, y0 <= y1): inside it and not
 *                       inside x0 + t <= x <= x1 - t, y0 + t <= y <= y1 - t.
 *    Primitives may lie partly or wholly outside the frame; only pixels inside it exist.
 * 2. The exported image E_i (W x H): A_i with the ingest options undo[i] undone.  Window pixel (u, v):
 *        xs = flip_x ? W - 1 - u : u;   x = xs + shift_x,  y = v + shift_y;   E(u, v) = A(x, y) inside the frame, else (0, 0, 0)
 *    undo == NULL: E = A.  A ring drawn on a match therefore lands on the object in the un-shifted picture too.
 * 3. The destination dst[i], an lm_image_desc: data = a DEVICE pointer that is WRITTEN; width, height = the destination surface's size;
 *    crop_x, crop_y = the top-left of the W x H window inside it; scale is ignored; format = LM_PIX_BGR8, RGB8, BGRA8, RGBA8 (alpha
 *    written as 255), BGR8_PLANAR, RGB8_PLANAR, or LM_PIX_NV12, which may be ORed with LM_PIX_YUV_BT709 / LM_PIX_YUV_FULL.  Any byte
 *    alignment of data and strides.  No byte outside the window is written -- for NV12 that includes the chroma bytes of pairs outside
 *    the window.  NV12: crop_x, crop_y, the surface's width and height and the frame's height are even.
 *    Float destinations (0.13 additive): the twelve non-grey LM_PIX_*_F32 / _F16 values (LM_PIX_FLOAT | element | layout, layout 0 .. 5),
 *    what a network behind the detector takes.  Channel value c (0 .. 255) is written as f = (float)c * scale: ONE single-precision
 *    multiply, scale the descriptor's field, finite and > 0 (1 / 255 for a 0 .. 1 tensor).  F16 stores f rounded ONCE to binary16,
 *    nearest, ties to even; it overflows to +inf for an absurd scale, which is the caller's affair.  Alpha is written as (float)255 *
 *    scale through the same path.  data, row_stride and plane_stride are multiples of the element size; no byte outside the window is
 *    written; the overlap check counts element bytes.  With scale = 1.0f / 255 (bits 0x3b808081) the bytes 0, 1, 127, 128, 254, 255
 *    become the F32 bits 0x0, 0x3b808081, 0x3efeff00, 0x3f008081, 0x3f7eff00, 0x3f800000 and the F16 bits 0x0, 0x1c04, 0x37f8, 0x3804,
 *    0x3bf8, 0x3c00; byte * (1 / 255)f * 255 rounds back to the byte for all 256 values, so an F32 export at 1 / 255 ingested again at
 *    255 is the identity.  The grey float formats are source formats: not served as a destination, like GRAY8.
 *    NV12, with (R, G, B) of E, sat8 a
 *    clamp to [0, 255] and >> an arithmetic shift of 32-bit signed integers:
 *        Y = sat8((cyr R + cyg G + cyb B + (Y0 << 16) + 32768) >> 16)
 *        U = sat8((cur SR + cug SG + cub SB + (128 << 18) + (1 << 17)) >> 18),  V likewise with cvr, cvg, cvb
 *    SR, SG, SB = the sums over the four pixels of E of the destination's 2 x 2 block (the blocks are the DESTINATION's: an odd shift
 *    moves the frame under them).  The coefficients are round(c * 2^16) of the standard matrices:
 *        matrix / range              Y0   cyr, cyg, cyb         cur, cug, cub             cvr, cvg, cvb
 *        BT.601 limited (no flag)    16   16829, 33039, 6416    -9714, -19071, 28784      28784, -24103, -4681
 *        BT.709 limited              16   11966, 40254, 4064    -6596, -22189, 28784      28784, -26145, -2639
 *        BT.601 full                  0   19595, 38470, 7471    -11058, -21710, 32768     32768, -27439, -5329
 *        BT.709 full                  0   13933, 46871, 4732    -7509, -25259, 32768      32768, -29763, -3005
 *    White gives (Y, U, V) = (235,128,128), (235,128,128), (255,128,128), (255,128,128) in row order; pure red (R = 255) gives
 *    (81,90,240), (63,102,240), (76,85,255), (54,99,255).
 * The call is synchronous: the images are complete in device memory when it returns.  It waits for the slots' pending uploads, only
 * READS the slots (a match in flight on them is no obstacle) and, while it runs, an upload into one of them from another thread is
 * refused.  prims == NULL with n_prims == 0 is a plain format-converting export.
 * Refused (LM_ERR_INVALID, before anything is enqueued or claimed; the message names the image or the primitive): a null dst or
 * n_slots <= 0; slots out of range or without a frame; a frame wider or higher than 8192, or a width that is no multiple of 16; an
 * unknown or unserved format (a depth format, a YUV flag on another format than NV12, a source-only format); a window outside the
 * surface; a row_stride shorter than a surface row of the format; a plane_stride <= 0 where planes are; a float destination whose data,
 * row_stride or plane_stride is no multiple of its element size, or whose scale is not finite and positive; odd NV12 geometry; two
 * destination windows of one call that overlap in memory (byte ranges per plane, compared by first and last byte: conservative); a
 * primitive with an unknown kind, a frame outside [0, n_slots), a coordinate outside [-8192, 8191], a thickness outside 1 .. 64, a ring
 * with y1 != 0 or a negative radius, an inverted box; n_prims > 65536; an export already in flight on another thread.
 * LM_ERR_OVERFLOW, nothing written: the call's tile-binning table (one entry per primitive and 64 x 32 tile its inflated bounding box
 * touches) would exceed 4194304 (2^22) entries.
 * Parity with cv::circle / cv::line is NOT claimed: their rasterisers (Bresenham variants with their own rounding and caps) are not this
 * rule.  Not served: YUY2 / UYVY / NV21 / grey destinations, per-channel mean / std normalisation and NV12-style float surfaces, depth export, text, filled polygons, anti-aliasing, a match's convex-hull
 * mask, and an asynchronous form with a consumer stream. */
enum { LM_DRAW_RING = 0, LM_DRAW_SEGMENT = 1, LM_DRAW_BOX = 2 };
typedef struct lm_draw_prim {
    int32_t kind;            /* LM_DRAW_* */
    int32_t frame;           /* 0 .. n_slots - 1: the frame of slot first_slot + frame */
    int32_t x0, y0, x1, y1;  /* ring: centre, radius, 0;  segment: A, B;  box: the inclusive corners */
    int32_t thickness;       /* 1 .. 64 */
    uint8_t b, g, r, a;      /* colour and opacity */
} lm_draw_prim;              /* 32 bytes */
int lm_export_frames(lm_detector* det, int first_slot, int n_slots, const lm_image_desc* dst, const lm_ingest_opts* undo,
                     const lm_draw_prim* prims, size_t n_prims);

/* ---- Learning templates from resident frames (0.11).
 * lm_add_templates_slots: for every slot of [first_slot, first_slot + n_slots) in order, the template that
 *     lm_add_template(class_id, <the slot's frame as lm_read_frame returns it>, <the slot's object mask>)
 * would add: the same features at every level and modality, the same widths, heights and bbox, consecutive template ids.  One call takes
 * at most frame_slots slots and learns them in one batch; no image and no candidate list leaves the device (the quantisers, the mask
 * pyramid, the candidate lists and the feature selection run there; the host reads back row counts and at most 63 features per level
 * and modality, and crops them to the bounding box).
 * masks: n_slots entries, or NULL = every slot unmasked.  An entry is one of
 *     data != NULL           one byte per level-0 pixel, row_stride bytes between rows (0 = dense), in host (on_device = 0) or device
 *                            (on_device = 1) memory; the bytes are used raw, exactly as lm_add_template uses its mask.  A device mask
 *                            must be complete when the call is made;
 *     data == NULL, rule     the level-0 mask of `rule` on the slot's frame, as lm_stage_mask_rule defines it (rule->modalities is
 *                            ignored: the object mask belongs to the template, not to a modality);
 *     both NULL              no mask, as lm_add_template with mask == NULL.
 * A slot whose extraction fails (too few candidates at some level) gets template_ids_out[k] = -1, bboxes_out[k] = {0, 0, 0, 0} and is
 * skipped; the others are added, the call returns LM_OK and lm_last_error() names the failure.
 * Afterwards the frames are still resident (the slots can be matched right away) and the slots are un-prepared; their mask rules
 * (lm_set_mask_rule) and uploaded match masks are match-time state and stay as they were.  The call waits for the slots' pending uploads.
 * Refused (LM_ERR_INVALID, before anything is enqueued): null arguments or n_slots <= 0; a range outside the slots; a slot without a
 * frame; a lane with a match in flight; slots that a colour check, depth counts or an ICP refinement in flight reads; a rule that
 * lm_set_mask_rule would refuse (a depth gate on a detector that keeps no depth frame, a rectangle outside the frame, ...); a row_stride below the width. */
typedef struct lm_object_mask {
    const void* data;          /* uint8, one byte per level-0 pixel; NULL: see rule */
    int64_t row_stride;        /* bytes between rows, 0 = dense */
    int32_t on_device;         /* 0: data is a host pointer, 1: a device pointer */
    const lm_mask_rule* rule;  /* data == NULL: the rule's level-0 mask of the slot's frame; both NULL: unmasked */
} lm_object_mask;
int lm_add_templates_slots(lm_detector* det, const char* class_id, int first_slot, int n_slots, const lm_object_mask* masks,
                           int* template_ids_out, lm_rect* bboxes_out);
/* Stage hook: the feature selection of addTemplate (select_color for modality 0, select_depth for modality 1) on n_lists host-supplied
 * candidate lists, run by the kernels lm_add_templates_slots uses.  List i = candidates [list_offsets[i], list_offsets[i + 1]) in
 * row-major order: xy[k][2] (int16 x, y at the level), labels[k] (0 .. 7), scores[k] (finite, >= 0: the squared gradient magnitude, or
 * the chessboard distance before the per-label division); want[i] = the features wanted (1 .. 63); area[i] = the depth interior's pixel
 * count (modality 1 only; NULL for modality 0).  features_out[i][63] receives list i's n_out[i] = want[i] features in the host's
 * order; n_out[i] = -1 and nothing written when the list has fewer than want[i] candidates. */
int lm_stage_select(lm_detector* det, int modality, int n_lists, const int32_t* list_offsets, const int16_t* xy, const int32_t* labels,
                    const float* scores, const int32_t* want, const float* area, lm_feature* features_out, int32_t* n_out);

/* ---- Raw depth registered onto the colour camera (0.13): what registration->apply(rgb, depth, .., &depth2rgb)
 * (Kinect2.cpp:50), cv::rgbd::registerDepth and librealsense's align do on the host, as a stage of the ingest.  The depth image arrives
 * in DEVICE memory in the DEPTH camera's geometry -- another size, lens and viewpoint than the colour image -- and the slot receives
 * depth that lies pixel for pixel on the colour image: unproject, rigid transform, project through the colour lens, z-buffer.
 *
 * A registration belongs to the detector (the rig is fixed).  It holds a depth camera and a colour camera (fx, fy, cx, cy, k1, k2, p1,
 * p2, k3, width, height each: pinhole + Brown-Conrady), a rotation R (row-major 3 x 3) and a translation t in millimetres with
 * P_colour = R * P_depth + t, splat_x, splat_y in 0 .. 3, and optionally a caller's HOST ray table.
 *
 * Rays.  Depth pixel (i, j) (integers are pixel centres) has the ray (rx, ry) = rays[2 * (j * width + i)], rays[2 * (j * width + i) + 1]: its
 * undistorted normalised coordinate.  Without a caller's table it is computed on the host in double and rounded once to float:
 * (xd, yd) = ((i - cx) / fx, (j - cy) / fy) pushed through the inverse Brown model by 20 rounds of the fixed-point iteration
 *     r2 = x x + y y;  rad = 1 + r2 (k1 + r2 (k2 + r2 k3));  dx = 2 p1 x y + p2 (r2 + 2 x x);  dy = p1 (r2 + 2 y y) + 2 p2 x y
 *     x = (xd - dx) / rad;  y = (yd - dy) / rad                       starting at (xd, yd)
 * With all five coefficients zero it is exactly the rounded quotient.  A caller's table (2 * width * height floats, all finite) replaces
 * it: the way in for a camera that is no pinhole (libfreenect2's Kinect polynomial, a fisheye).  The table is uploaded once.
 *
 * Per depth pixel with the value v.  IEEE single precision, every operation rounded on its own in exactly the order written, no
 * contraction into fused multiply-adds, `/` the correctly rounded division:
 *     t  = v * scale (LM_PIX_DEPTH_F32)  or  (float)v (LM_PIX_DEPTH_U16);                 dropped unless t is finite and > 0
 *     X  = rx * t;   Y = ry * t
 *     X' = ((r00 * X + r01 * Y) + r02 * t) + tx;   Y', Z' the same from rows 1 and 2;     dropped unless Z' is finite and > 0
 *     a  = X' / Z';  b = Y' / Z';  r2 = a * a + b * b
 *     rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))                                           (k, p, f, c below: the COLOUR camera's)
 *     ad = a * rad + ((2 * p1) * (a * b) + p2 * (r2 + 2 * (a * a)))
 *     bd = b * rad + (p1 * (r2 + 2 * (b * b)) + (2 * p2) * (a * b))
 *     xf = fx * ad + cx;   yf = fy * bd + cy
 *     u  = floorf(xf + 0.5f);   v = floorf(yf + 0.5f);                                    dropped unless both are finite (compared as floats)
 *     m  = min(rintf(Z'), 65535)  (ties to even);                                         dropped if m < 1
 * and the pixel contributes m to every colour pixel of [u - splat_x, u + splat_x] x [v - splat_y, v + splat_y] inside the colour image.
 * The registered image Rg has the colour camera's size and type u16: a pixel is the MINIMUM of its contributions, or 0 without any.  The
 * minimum does not depend on the order of the contributions: the result is the same bits on every run.
 * The slot receives what lm_ingest_frames makes of Rg handed over as LM_PIX_DEPTH_U16 with the descriptor's crop_x, crop_y and the frame's
 * lm_ingest_opts: registering equals ingesting the image this rule yields from the WHOLE raw image.  So a depth pixel whose centre
 * projects outside the window but whose splat reaches into it contributes; the window must lie inside the colour geometry; the raw depth
 * image may have any width and height (no multiple-of-16 rule), naturally aligned as the depth formats of lm_ingest_frames are.
 * The colour image is NOT undistorted or resampled: depth is projected through the colour lens and lands on the raw colour pixels.
 * (Undistorting the colour image is the rectification's business: "Lens rectification at ingest" below.) */
typedef struct lm_camera {
    float fx, fy, cx, cy;          /* pixels; fx, fy > 0 */
    float k1, k2, p1, p2, k3;      /* Brown-Conrady, OpenCV's order */
    int32_t width, height;         /* 1 .. 16384 */
} lm_camera;
typedef struct lm_registration_desc {
    lm_camera depth, colour;
    float rotation[9];             /* row-major */
    float translation[3];          /* millimetres */
    int32_t splat_x, splat_y;      /* 0 .. 3 */
    const float* rays;             /* HOST, 2 * depth.width * depth.height floats, or NULL = built from `depth` */
} lm_registration_desc;
/* Sets the detector's registration (copied; desc == NULL clears it).  Host state: no device is needed, the table travels to the device
 * with the first registered ingest.  Refused (LM_ERR_INVALID): a number that is not finite (the rays included); fx or fy <= 0; a width or
 * height outside 1 .. 16384; a splat outside 0 .. 3; a lane with a match in flight.  The call waits for pending uploads. */
int lm_set_registration(lm_detector* det, const lm_registration_desc* desc);
/* The ray table as the device uses it: 2 * depth.width * depth.height floats into `out`.  LM_ERR_INVALID without a registration. */
int lm_get_registration_rays(lm_detector* det, float* out);
/* lm_ingest_frames with the depth image registered first.  colour, opts, producer_stream, the ticket, lm_ingest_release and the slot
 * refusals: exactly as lm_ingest_frames.  depth_raw[i] describes the RAW depth image of frame i: data, row_stride, format (LM_PIX_DEPTH_U16
 * / _F32), scale, and width, height equal to the registration's depth camera; its crop_x, crop_y place the cfg.width x cfg.height window
 * inside the COLOUR geometry (colour[i].crop_x, crop_y place it inside the colour SOURCE: the two differ when the source is not the whole
 * sensor image).  The number of launches does not depend on n_slots; the z-buffer (4 * width * height bytes per slot of the call) is the
 * detector's and grows to the largest call.
 * Refused (LM_ERR_INVALID, before anything is enqueued) on top of lm_ingest_frames' refusals: no registration set; a colour-only detector that keeps no
 * depth frame (with LM_FLAG_KEEP_DEPTH the route is served; depth_raw is then required);
 * a raw image whose size is not the depth camera's; a window outside the colour geometry; a colour format in depth_raw; a row_stride
 * smaller than a raw row; misaligned data or row_stride; a scale that is not finite and positive. */
int lm_ingest_frames_registered(lm_detector* det, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth_raw,
                                const lm_ingest_opts* opts, void* producer_stream);
/* Stage hook: the whole registered image Rg (the window is the entire colour geometry; crop_x, crop_y of depth_raw are ignored) of one raw
 * depth image in DEVICE memory -> out_host, colour.width * colour.height uint16, dense.  Synchronous. */
int lm_stage_register_depth(lm_detector* det, const lm_image_desc* depth_raw, uint16_t* out_host);

/* ---- Lens rectification at ingest (0.13, additive): what cv::initUndistortRectifyMap + cv::remap do on the host,
 * as a stage of the ingest.  Everything behind a slot assumes an ideal pinhole camera; the frames arrive in DEVICE memory as the real
 * camera delivered them, and the slot receives the frame the ideal camera would have seen.
 *
 * A rectification belongs to the detector (the camera is fixed).  It holds a SOURCE camera (pinhole + Brown-Conrady; width, height: the
 * source images' size), an IDEAL camera (all five coefficients 0; width, height: the rectified geometry, which may differ from the
 * source's) and optionally a caller's HOST map.
 *
 * The map.  Built on the host, once, in double from the cameras' floats promoted to double, every operation rounded on its own in the
 * order written (no contraction into fused multiply-adds, only + - * /).  Per ideal pixel (i, j) (integers are pixel centres):
 *     x  = (i - cx') / fx';   y = (j - cy') / fy'                                         (the IDEAL camera's)
 *     r2 = x x + y y;   rad = 1 + r2 (k1 + r2 (k2 + r2 k3))                               (k, p, f, c below: the SOURCE camera's)
 *     xd = x rad + ((2 p1)(x y) + p2 (r2 + 2 (x x)));   yd = y rad + (p1 (r2 + 2 (y y)) + (2 p2)(x y))
 *     sx = fx xd + cx;   sy = fy yd + cy
 *     qx = quant(sx, source.width);   qy = quant(sy, source.height)
 *     quant(s, n): -64 if s is not finite; otherwise rint(32 s) (ties to even) clamped into [-64, 32 n + 32], as int32
 * -- the forward Brown model, the expression shape of the registration's projection, no iteration.  A caller's table (2 * ideal.width *
 * ideal.height floats, (sx, sy) of ideal pixel (i, j) at 2 * (j * ideal.width + i); NaN and infinities allowed) replaces (sx, sy) by its
 * floats, and quant is applied all the same: the way in for a fisheye or any other model.  The map travels to the device once, with the
 * first rectified call; lm_get_rectification_map returns what the device uses.
 *
 * Per pixel of the rectified images Rc (BGR8) and Rd (u16), both of the ideal geometry; integers only, >> an arithmetic shift:
 *     ix = qx >> 5;   ax = qx & 31;   iy = qy >> 5;   ay = qy & 31
 *     tap(k, l) = (B, G, R) of source pixel (ix + k, iy + l) by its format's own rule (the channel order, the grey and YUV conversions
 *                 above: the conversion comes BEFORE the interpolation), (0, 0, 0) when the pixel lies outside the source
 *                 (BORDER_CONSTANT, per tap)
 *     Rc channel = ((32 - ax)(32 - ay) tap(0,0) + ax (32 - ay) tap(1,0) + (32 - ax) ay tap(0,1) + ax ay tap(1,1) + 512) >> 10
 *     Rd = to_u16 of source pixel ((qx + 16) >> 5, (qy + 16) >> 5), 0 when outside       (nearest: depth is never blended across an edge)
 * The depth VALUE is not changed: Z along the optical axis does not depend on the lens.  This is cv::remap's 5-bit fixed-point scheme
 * (INTER_LINEAR, INTER_BITS = 5) with EXACT weight products; parity with OpenCV's rounded weight table is not claimed (DESIGN.md
 * section 3).
 *
 * The slot receives what lm_ingest_frames makes of Rc handed over as LM_PIX_BGR8, and of Rd as LM_PIX_DEPTH_U16, with the descriptors'
 * crop_x, crop_y and the frame's lm_ingest_opts: rectifying equals ingesting the images this rule yields from the WHOLE source.  So
 * crop_x, crop_y place the cfg.width x cfg.height window inside the IDEAL geometry and must lie inside it, and width, height of every
 * source descriptor must equal the source camera's (a producer whose depth image has extra rows passes the address of the first sensor
 * row).  All colour formats of lm_ingest_frames are accepted, 8-bit sources at any byte alignment; no load touches a byte outside a
 * source.  row_stride must hold a SOURCE row. */
typedef struct lm_rectification_desc {
    lm_camera source, ideal;
    const float* map;              /* HOST, 2 * ideal.width * ideal.height floats (sx, sy), or NULL = built from the cameras */
} lm_rectification_desc;
enum { LM_RECTIFY_DEPTH_ALIGNED = 0, LM_RECTIFY_DEPTH_REGISTERED = 1 };
/* Sets the detector's rectification (copied, the map built; desc == NULL clears it).  Host state: no device is needed.  Refused
 * (LM_ERR_INVALID, every message begins "rectification:", the previous rectification stays in place): a camera number that is not
 * finite; fx or fy <= 0 in either camera; a width or height outside 1 .. 16384; a non-zero coefficient in `ideal`; a lane with a match in
 * flight.  The caller's map may hold anything.  The call waits for pending uploads. */
int lm_set_rectification(lm_detector* det, const lm_rectification_desc* desc);
/* The map as the device uses it: 2 * ideal.width * ideal.height int32, (qx, qy) per ideal pixel.  LM_ERR_INVALID without a rectification. */
int lm_get_rectification_map(lm_detector* det, int32_t* out);
/* lm_ingest_frames through the rectifier.  opts, producer_stream, the ticket, lm_ingest_release and the slot refusals: exactly as
 * lm_ingest_frames; the number of launches does not depend on n_slots.
 * depth_route = LM_RECTIFY_DEPTH_ALIGNED: depth[i] is a depth image of the source camera (aligned to the colour image, same lens) and is
 * rectified by the nearest rule.  depth_route = LM_RECTIFY_DEPTH_REGISTERED: depth[i] is a RAW depth image and takes exactly
 * lm_ingest_frames_registered's route -- that rule is unchanged -- while only the colour image goes through the rectifier; a registration
 * must be set and its colour camera must have the ideal camera's width and height.  To register onto the IDEAL camera the caller gives the
 * registration's colour camera the ideal camera's fx, fy, cx, cy and zero coefficients (not enforced).
 * Refused (LM_ERR_INVALID, before anything is enqueued; the rectifier's own refusals begin "rectification:"): no rectification set; a
 * source whose size is not the source camera's; a window outside the ideal geometry; an unknown depth_route; the REGISTERED route without
 * a registration or with a registration whose colour size is not the ideal camera's; and everything lm_ingest_frames (REGISTERED: and
 * lm_ingest_frames_registered) refuses, in their words. */
int lm_ingest_frames_rectified(lm_detector* det, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                               const lm_ingest_opts* opts, int depth_route, void* producer_stream);
/* Stage hook: the whole Rc and / or Rd (the window is the entire ideal geometry, which may have ANY width and height here; crop_x, crop_y
 * are ignored) of one source pair in DEVICE memory -> dense host buffers, ideal.width * ideal.height * 3 bytes and ideal.width *
 * ideal.height uint16.  colour with bgr_out_host, depth with depth_out_host; either pair may be NULL.  Synchronous. */
int lm_stage_rectify(lm_detector* det, const lm_image_desc* colour, const lm_image_desc* depth, uint8_t* bgr_out_host, uint16_t* depth_out_host);

/* ---- Area-averaged reduction at ingest (0.13, additive): what cv::resize(..., INTER_AREA) does on the host, as a
 * stage of the ingest.  A slot is cfg.width x cfg.height; a camera delivers more pixels.  lm_ingest_frames can only crop a window out of
 * them; this route brings the whole field of view into the slot with the box filter: every source pixel under a reduced pixel's
 * footprint contributes in proportion to its overlap.
 *
 * A reduction belongs to the detector.  It holds a rational ratio per axis, source pixels per reduced pixel = num / den, with
 * 1 <= den <= 16 and den <= num <= 8 den (the fractions are reduced by their gcd: 18/8 is 9/4), which images of a frame it applies to,
 * and the depth rule.  Downscaling only; 1 / 1 on both axes is the identity.
 *
 * Geometry and weights, per axis, for a source of n pixels (integers only, / is the floor division of non-negative numbers):
 *     R = (n den) / num                              the reduced pixels; the source pixels beyond R num / den are not used
 *     in units of 1 / den source pixel, reduced pixel X covers [X num, (X + 1) num) and source pixel i covers [i den, (i + 1) den)
 *     w(X, i) = max(0, min((X + 1) num, (i + 1) den) - max(X num, i den))          the overlap, 0 .. den
 *     w(X, i) != 0 for i in [(X num) / den, ((X + 1) num - 1) / den]: at most ceil(num / den) + 1 <= 9 taps, and sum_i w(X, i) = num
 * Colour, per channel of the reduced image Ac (BGR8), 32-bit unsigned:
 *     Ac(X, Y) = (sum_ij wx(X, i) wy(Y, j) p(i, j) + ((num_x num_y) >> 1)) / (num_x num_y)
 * p(i, j) is the (B, G, R) of source pixel (i, j) by its format's own rule -- the channel order, the grey and YUV conversions, the
 * demosaic with the SOURCE's own reflecting edges, the raw pipeline when one is set: the conversion comes BEFORE the blend, as in the
 * rectified route.  The largest accumulator is 255 * 128 * 128 + 8192.
 * Depth, the reduced image Ad (u16), is never blended.  Values are to_u16 of the source as in lm_ingest_frames, 0 = invalid:
 *     LM_REDUCE_DEPTH_NEAREST    Ad(X, Y) = source pixel (((2 X + 1) num_x) / (2 den_x), ((2 Y + 1) num_y) / (2 den_y)): the one that contains
 *                                the footprint's centre
 *     LM_REDUCE_DEPTH_MIN_VALID  Ad(X, Y) = the minimum of the non-zero values among the source pixels (i, j) whose CENTRE lies in the
 *                                footprint, 2 X num <= (2 i + 1) den < 2 (X + 1) num per axis, and 0 when there is none -- the
 *                                registration's conflict rule: it does not depend on any order and keeps the foreground
 * Pins.  9/4 on the row 10 20 30 40 50 60 70 80 90 (num_y = den_y = 1): weights 4 4 1 | 3 4 2 | 2 4 3 | 1 4 4, Ac = 17 39 61 83.
 * 7/3 x 5/2 on the 7 x 5 image with the rows 10 20 30 40 50 60 70 / 80 90 100 110 120 130 140 / 150 160 170 180 190 200 210 /
 * 220 230 240 250 255 0 5 / 15 25 35 45 55 65 75: column weights 3 3 1 | 2 3 2 | 1 3 3, row weights 2 2 1 | 1 2 2,
 * Ac = 73 96 119 / 131 153 83.  9/4 x 2/1 on the 9 x 2 depth image 0 500 0 700 800 900 1000 1100 1200 / 300 0 0 650 0 950 0 1150 1250:
 * NEAREST gives 0 650 950 1150, MIN_VALID gives 300 650 800 1100.
 *
 * The slot receives what lm_ingest_frames makes of Ac handed over as LM_PIX_BGR8, and of Ad as LM_PIX_DEPTH_U16, with the descriptors'
 * crop_x, crop_y and the frame's lm_ingest_opts: crop_x, crop_y place the cfg.width x cfg.height window inside the REDUCED geometry and
 * must lie inside it; then the mirror, then the shift.  Every image has its own size, from which its reduced geometry follows.  An image
 * whose `apply` bit is clear is not reduced: it takes lm_ingest_frames' rule, its crop placing the window in the source itself (a depth
 * stream that is already at slot resolution beside a 1080p colour stream).  All colour formats of lm_ingest_frames are accepted, 8-bit
 * sources at any byte alignment; no load touches a byte outside a source.  row_stride must hold a SOURCE row.
 * Not served: enlargement (a ratio below 1 is refused); filters other than the box.  A lens map in front of the reduction, and a
 * registered depth beside it, are lm_ingest_frames_rectified_reduced's (below); a reduction behind a plain lm_ingest_frames_registered,
 * without a rectification, is served by that route with an identity rectification (zero coefficients, ideal = source). */
enum { LM_REDUCE_COLOUR = 1, LM_REDUCE_DEPTH = 2 };              /* apply: which images of a frame are reduced */
enum { LM_REDUCE_DEPTH_NEAREST = 0, LM_REDUCE_DEPTH_MIN_VALID = 1 };
typedef struct lm_reduction_desc {
    int32_t num_x, den_x, num_y, den_y;   /* source pixels per reduced pixel = num / den per axis */
    int32_t apply;                        /* LM_REDUCE_COLOUR | LM_REDUCE_DEPTH, at least one */
    int32_t depth_rule;
} lm_reduction_desc;
/* Sets the detector's reduction (copied, the fractions in lowest terms; desc == NULL clears it).  Host state: no device is needed.
 * Refused (LM_ERR_INVALID, every message begins "reduction:", the previous reduction stays in place): a den outside 1 .. 16; num < den
 * (an enlargement); num > 8 den; apply 0 or with unknown bits; an unknown depth_rule; a lane with a match in flight.  The call waits for
 * pending uploads. */
int lm_set_reduction(lm_detector* det, const lm_reduction_desc* desc);
/* The reduction as the device uses it (lowest terms) and whether one is set; without one, *out is all zero. */
int lm_get_reduction(lm_detector* det, lm_reduction_desc* out, int* is_set);
/* lm_ingest_frames through the reduction.  opts, producer_stream, the ticket, lm_ingest_release and the slot refusals: exactly as
 * lm_ingest_frames; the number of launches does not depend on n_slots, and the frames of a call may differ in format and in source size.
 * Refused (LM_ERR_INVALID, before anything is enqueued; the route's own refusals begin "reduction:"): no reduction set; a reduced source
 * with a side outside 1 .. 32768; a window outside the reduced geometry; a row_stride smaller than a source row; and everything
 * lm_ingest_frames refuses, in its words. */
int lm_ingest_frames_reduced(lm_detector* det, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                             const lm_ingest_opts* opts, void* producer_stream);
/* Stage hook: the whole Ac and / or Ad (the window is the image's entire reduced geometry, of ANY width and height; crop_x, crop_y are
 * ignored; an image whose apply bit is clear comes back whole, converted) of one source pair in DEVICE memory -> dense host buffers,
 * Rx * Ry * 3 bytes and Rx * Ry uint16, each from its own image's size.  colour with bgr_out_host, depth with depth_out_host; either pair
 * may be NULL.  Synchronous. */
int lm_stage_reduce(lm_detector* det, const lm_image_desc* colour, const lm_image_desc* depth, uint8_t* bgr_out_host, uint16_t* depth_out_host);
/* Host only: the intrinsics of the slot's frame for a source camera, a reduction and the w x h window at (crop_x, crop_y) of the reduced
 * geometry.  Computed in double from the camera's floats and rounded once (pixel centres are integers, so the half pixel moves with the
 * ratio):
 *     fx' = fx den_x / num_x                                   fy' = fy den_y / num_y
 *     cx' = (cx + 0.5) den_x / num_x - 0.5 - crop_x            cy' = (cy + 0.5) den_y / num_y - 0.5 - crop_y
 * The coefficients are copied (they live in normalised coordinates); width, height = w, h.  Refused (LM_ERR_INVALID): a null pointer; a
 * ratio lm_set_reduction refuses, in its words. */
int lm_reduced_camera(const lm_camera* source, const lm_reduction_desc* reduction, int crop_x, int crop_y, int w, int h, lm_camera* out);

/* ---- Rectify and reduce in one ingest pass (0.13, additive): what cv::remap followed by cv::resize(..., INTER_AREA)
 * does on the host -- the configuration a real camera at its own resolution needs: a 1920 x 1080 stream through a real lens into 640 x 480
 * slots that hold the ideal pinhole geometry of the WHOLE field of view.  No new setter and no new struct: the route uses the detector's
 * rectification (lm_set_rectification) and its reduction (lm_set_reduction) as they are, and both must be set.
 *
 * The rule is the composition of the two rules above, to the last rounding.  Let Rc (BGR8) and Rd (u16) be the images the rectification
 * rule yields from the WHOLE source: ideal.width x ideal.height pixels -- the map, the four converted taps, (... + 512) >> 10, depth by the
 * nearest source pixel.  The slot receives what lm_ingest_frames_reduced would make of Rc handed over as LM_PIX_BGR8 and of Rd handed over
 * as LM_PIX_DEPTH_U16: the detector's reduction with its ratios, its `apply` bits and its depth rule applied to Rd's pixels (NEAREST: the
 * ideal pixel that contains the footprint's centre; MIN_VALID: the minimum of the non-zero Rd among the ideal pixels whose centre lies in
 * the footprint); crop_x, crop_y place the cfg.width x cfg.height window in the REDUCED geometry of the ideal size, R = (ideal side * den)
 * / num per axis, and must lie inside it; then the mirror, then the shift.  An image whose `apply` bit is clear takes the rectified rule
 * alone: its crop places the window in the ideal geometry.  Nothing is rounded anywhere else: the 8-bit Rc pixel is what the box sums.
 * Rc and Rd are never stored; the device forms each of their pixels where the box needs it.
 * The slot's camera -- the one to render templates and to compute poses with -- is lm_reduced_camera(&ideal, &reduction, crop_x, crop_y,
 * cfg.width, cfg.height, &slot_camera).
 *
 * opts, producer_stream, the ticket, lm_ingest_release and the slot refusals: exactly as lm_ingest_frames; the number of launches does not
 * depend on n_slots.  All colour formats of lm_ingest_frames are accepted (Bayer and raw ones, under the raw pipeline, too), 8-bit sources
 * at any byte alignment; every image has the source camera's size; no load touches a byte outside a source.
 * depth_route = LM_RECTIFY_DEPTH_ALIGNED: depth[i] is a depth image of the source camera and takes the rule above.
 * depth_route = LM_RECTIFY_DEPTH_REGISTERED: depth[i] is a RAW depth image and takes exactly lm_ingest_frames_registered's route,
 * unchanged: it lands on the SLOT's camera directly.  A registration must be set, and its colour camera must have the size of the colour
 * image's geometry in this route: the reduced ideal geometry when LM_REDUCE_COLOUR is set, the ideal geometry otherwise; depth crop_x,
 * crop_y place the window in it.  The caller gives that camera lm_reduced_camera(&ideal, &reduction, 0, 0, ...)'s fx, fy, cx, cy and zero
 * coefficients (not enforced).  The reduction's LM_REDUCE_DEPTH bit and its depth rule have no effect on a registered depth.
 * Refused (LM_ERR_INVALID, before anything is enqueued): no rectification set ("rectification: ..."); no reduction set ("reduction: ...");
 * a source whose size is not the source camera's; a window outside the geometry it is placed in (the reduced ideal one, or the ideal one
 * for an image outside `apply`); an unknown depth_route; the REGISTERED route without a registration, or with one whose colour camera has
 * another size (the sentence names both sizes); and everything lm_ingest_frames (REGISTERED: and lm_ingest_frames_registered) refuses, in
 * their words.
 * Not served: enlargement; filters other than the box. */
int lm_ingest_frames_rectified_reduced(lm_detector* det, int first_slot, int n_slots, const lm_image_desc* colour, const lm_image_desc* depth,
                                       const lm_ingest_opts* opts, int depth_route, void* producer_stream);
/* Stage hook: the whole Ac and / or Ad of the rule above (the window is the image's entire reduced ideal geometry, of ANY width and height;
 * crop_x, crop_y are ignored; an image whose apply bit is clear comes back as the whole Rc / Rd) of one source pair in DEVICE memory ->
 * dense host buffers, Rx * Ry * 3 bytes and Rx * Ry uint16, each from its own image's ratio.  colour with bgr_out_host, depth with
 * depth_out_host; either pair may be NULL.  Synchronous. */
int lm_stage_rectify_reduce(lm_detector* det, const lm_image_desc* colour, const lm_image_desc* depth, uint8_t* bgr_out_host, uint16_t* depth_out_host);

#ifdef __cplusplus
}
#endif
#endif /* LINEMOD_HIP_H */
