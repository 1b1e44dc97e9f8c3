// lm_kernels.h -- host-callable launchers of the gfx950 kernels in lm_k_preprocess.hip (a3-a10), lm_k_scan.hip (a11-a13) and lm_k_refine.hip
// (a14-a15) -- one executor each of a plan made on the host (lm_host.h plan_preprocess / plan_match): they launch the plan's steps with the
// pointers and strides of an argument struct and decide nothing --, of 8e's k_pack_lists, lm_k_post.hip (f1) and lm_k_ingest.hip
// (device-resident frames into the slots).
// Every launcher processes `nslots` consecutive frame slots (grid.z) whose buffers are `*_slot_stride`
// bytes apart; pass stride 0 / nslots 1 for a single set of buffers.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/linemod_hip.h"
#include "lm_common.h"
#include "lm_ingest_check.h"
#include "lm_register.h"
#include "lm_rectify.h"
#include "lm_reduce.h"
#include "lm_export_check.h"
#include "lm_draw.h"

// ---- a3-a10 (lm_k_preprocess.hip).  WHICH kernels run on which grids is planned on the host, from values alone (lm_host.h plan_preprocess
// and the single-stage planners plan_pyrdown .. plan_linear_memories); lmk_preprocess_run launches steps [from, to) of such a plan with
// these pointers.  Buffers of slot 0 of the call, slot_stride bytes between slots (0 / nslots 1 for a single set of buffers).
//   a4  cv::pyrDown on dense BGR: level l from level l - 1
//   a3  ColorGradient quantisation of a dense BGR image: blur into the level's scratch (lmk_color_scratch_bytes), orientation + vote; the
//       LDS-tiled k_color_quantize for shapes the streaming kernels do not take.  mag[l] (may be null): the gradient magnitudes
//   a5  DepthNormal quantisation (normals + LUT + 5x5 median); ds: w * h bytes per slot (rank codes between the two streaming passes)
//   a6+a8+a9+a10  spread(T) -> 8 response maps -> linear memories of lm[l][m] (the modality's first orientation block), read from
//       quant[l][m] or, for depth above level 0, from quant[l - 1][1] at (2y, 2x).  mode[l] 0: 8 response memories (1 byte per position);
//       1: one spread memory (refinement levels); 2: response memories packed two positions per byte for the nibble scan
struct LmPreArgs {
    int L;                                           // levels in use
    int w[LM_MAX_LEVELS], h[LM_MAX_LEVELS], T[LM_MAX_LEVELS], mode[LM_MAX_LEVELS];
    u32 ori_stride[LM_MAX_LEVELS];                   // bytes between a level's response memories
    u8* bgr[LM_MAX_LEVELS];                          // colour images (level 0 read only)
    u8* cs[LM_MAX_LEVELS];                           // colour scratch
    float* mag[LM_MAX_LEVELS];
    u8* quant[LM_MAX_LEVELS][2];                     // quantised images [level][modality]
    u8* lm[LM_MAX_LEVELS][2];                        // linear memories [level][modality]
    const u16* depth; u8* ds;                        // depth image (null: colour only) and depth scratch
    float weak_threshold; int dist_thr, diff_thr;
    const u8* normal_lut; const u64* resp_tab;
    u32 planes;                                      // the scanned level's plane word (lmh::PreInputs::planes)
    size_t slot_stride; int nslots;
};
namespace lmh { struct PrePlan; struct MatchPlan; }
size_t lmk_color_scratch_bytes(int w, int h);
void lmk_preprocess_run(hipStream_t s, const lmh::PrePlan& plan, int from, int to, const LmPreArgs& a);

// Detector::match's masks (lm_k_mask.hip): the quantised images of up to LM_MASK_SLOTS masked slots ANDed with their level-0 masks,
// after the last quantiser and before the depth NN pyramid / the linear memories.  Only masked slots have an entry: the unmasked
// slots of a mixed call cost nothing.  A mask is [height][mask_pitch] bytes, nonzero = keep; mask_pitch % 64 == 0.
#define LM_MASK_SLOTS 128
#define LM_MASK_LEVELS 4                // = LM_MAX_LEVELS of include/linemod_hip.h (static_assert in lm_detector.hip)
struct LmMaskArgs {
    u8* frame;                      // frame arena (slot 0)
    size_t slot_stride;
    u32 off_quant[LM_MASK_LEVELS][2];// quant[l][m] inside a slot (256-byte aligned)
    u32 w[LM_MASK_LEVELS];           // level widths
    u32 vec_begin[LM_MASK_LEVELS + 1];// 16-byte vectors of the colour levels below l ([levels] = all colour levels)
    u32 vec_depth;                  // 16-byte vectors of depth level 0
    u32 mask_pitch;
    int levels;
    int vec_rows;                   // every level's width is a multiple of 16 (a vector never straddles two rows)
    int n;                          // entries
    u16 slot[LM_MASK_SLOTS];        // entry -> slot index
    const u8* cmask[LM_MASK_SLOTS]; // the slot's colour / depth mask, nullptr = that modality unmasked
    const u8* dmask[LM_MASK_SLOTS];
};
void lmk_match_mask(hipStream_t s, const LmMaskArgs& a);

// Mask rules (lm_set_mask_rule): the level-0 mask of a ruled slot computed from the slot's resident frame --
// seed = depth gate AND HSV gate, dilated with a (2 grow + 1)^2 square clipped to the image, then cut to a rectangle -- into the slot's
// rule plane ([height][mask_pitch] bytes, 0 / 255), which lmk_match_mask then applies like an uploaded mask.  One launch over up to
// LM_MASK_SLOTS ruled slots that share at most LM_RULE_KINDS different rules.
#define LM_RULE_KINDS 8
#define LM_RULE_MAX_GROW 16
struct LmHsvRange { int lo[3], hi[3]; };
struct LmRule {
    LmHsvRange hsv;                 // inRange bounds of the 8-bit HSV image (use_hsv)
    int use_depth, keep_invalid, use_hsv;
    int zmin, zmax;                 // depth gate: zmin <= d <= zmax; d == 0 is inside iff keep_invalid
    int grow;                       // 0 .. LM_RULE_MAX_GROW
    int rx, ry, rw, rh;             // the rectangle, inside the frame (the whole frame: no rectangle)
};
struct LmRuleArgs {
    const u8* bgr; const u16* depth;    // level-0 images of slot 0 (depth may be null when no rule gates on it); slot_stride apart
    size_t slot_stride;
    const int* divtab;                  // HSV division tables (hsv_in_range); may be null when no rule gates on HSV
    int w, h;
    u32 mask_pitch;                     // = 64 * ceil(w / 64): a row of the plane holds whole 64-pixel words
    int rows_out;                       // output rows per workgroup (filled by lmk_mask_rule)
    int vec;                            // a lane's 8 pixels are one aligned 16-byte depth load and three 8-byte colour loads (filled by lmk_mask_rule)
    int n;                              // entries
    LmRule rule[LM_RULE_KINDS];
    u16 slot[LM_MASK_SLOTS];            // entry -> slot index
    u8 kind[LM_MASK_SLOTS];             // entry -> rule
    u8* plane[LM_MASK_SLOTS];           // entry -> the slot's rule plane
};
// false: frames this wide do not fit a workgroup's row words into LDS (no rule can be set on such a detector)
bool lmk_mask_rule_fits(int w);
void lmk_mask_rule(hipStream_t s, LmRuleArgs& a);

// ---- device-resident frames in the producer's format -> the slots: the four ingest routes (DESIGN.md sections 13 and 17-19; what their
// kernels share on the device: lm_dev_ingest.h).  LmIngestImage, LmIngestDesc and the LM_INGEST_* kinds are lm_ingest_check.h's, with the
// host check that fills them.  Frame i of the call reads table entry first + i: colour and depth describe the SOURCE images (data, strides,
// kind, swap_rb, scale, matrix, src_w x src_h; `aligned`: lmc::AlignedRule of the route), crop_x, crop_y of each place the w x h window in
// the geometry the route reads it from.  The colour plane of frame i goes to out_bgr + (first + i) * out_stride, the depth plane to
// out_depth + (first + i) * out_stride (the slots' planes; the stage hook: plain images, first = 0, stride 0); a null plane is not written.
// One struct for all four launchers; a kernel ignores what its route has no use for:
//   lmk_ingest (lm_k_ingest.hip)  the window lies in the source itself; w % 16 == 0; out_bgr is also the 16-byte aligned memory a masked
//      load is pointed at
//   lmk_rectify (lm_k_rectify.hip)  the window lies in the IDEAL geometry mw x mh, whose map (qx, qy per ideal pixel, int32, row-major)
//      is `map`; every source has the source camera's size sw x sh.  Any w, h; w % 4 == 0: vector stores
//   lmk_reduce (lm_k_reduce.hip)  the window lies in the image's own REDUCED geometry: `colour` and `depth` are the images' ratios in
//      lowest terms, 1 / 1 for an image the reduction does not apply to (the plain rule: a window of the source).  Any w, h
//   lmk_rectify_reduce (lm_k_rectify_reduce.hip)  map and cameras as lmk_rectify's, ratios as lmk_reduce's: the window lies in the
//      image's REDUCED IDEAL geometry, ((mw den_x) / num_x) x ((mh den_y) / num_y) (1 / 1: the rectified rule alone).  Any w, h
struct LmIngestArgs {
    const LmIngestDesc* table;          // device table, one entry per frame SLOT
    const int32_t* map;
    int mw, mh, sw, sh;
    u8* out_bgr;
    u8* out_depth;
    size_t out_stride;
    int first, n;                       // slots [first, first + n)
    int n_family[LM_INGEST_FAMILIES];                   // how many of the n frames each lm_ingest_family has (a kernel without frames is not launched; a depth-only stage call: RGB's)
    int w, h;
    lmx::Ratio colour, depth;
    int depth_rule;                     // LM_REDUCE_DEPTH_NEAREST / LM_REDUCE_DEPTH_MIN_VALID
    int frame_fast;                     // lmk_rectify_reduce's grid order (LM_TUNE_RECTIFY_REDUCE_GRID): 0 = blockIdx.y is the frame, 1 = blockIdx.x is
    const lm_raw_processing* raw;       // device copy of the raw pipeline, read for the raw kinds alone; null while n_family[LM_INGEST_FAMILY_RAW] == 0
    lmx::Tile tile;                     // the tiled kernels': lmx::plan_tile(colour), filled by lmk_reduce / lmk_rectify_reduce
};
// How often each kernel of the ingest routes and of the export has been launched in this process (lm_debug_launch_counts): the family
// kernels of all four routes under their lm_ingest_family, k_reduce_conv (which serves four families) and the two export kernels apart.
// A launcher counts where it launches -- lmk_count_launch returns true so that it stands in the launch's own condition -- and nowhere else.
enum { LMK_LAUNCH_REDUCE_CONV = LM_INGEST_FAMILIES, LMK_LAUNCH_EXPORT, LMK_LAUNCH_EXPORT_FLOAT, LMK_LAUNCH_KINDS };
bool lmk_count_launch(int kind);
long long lmk_launch_count(int kind);
void lmk_ingest(hipStream_t s, const LmIngestArgs& a);
void lmk_rectify(hipStream_t s, const LmIngestArgs& a);
void lmk_reduce(hipStream_t s, LmIngestArgs& a);
void lmk_rectify_reduce(hipStream_t s, LmIngestArgs& a);

// ---- raw depth images registered onto the colour camera (lm_k_register.hip).  Frame i of the call reads table entry
// first + i: its `depth` image describes the RAW depth image (data, row_stride, kind LM_INGEST_U16 / LM_INGEST_F32, scale; crop_x, crop_y =
// where the w x h window lies in the COLOUR geometry), its flip_x / shift_x / shift_y are what the resolve applies.  zbuf: n windows of
// w * h u32 each, frame i's at zbuf + i * w * h.  k_register_scatter takes the minimum of every contribution there (the sentinel
// 0xFFFFFFFF = none); k_register_resolve turns a window into u16 (sentinel -> 0), mirrors and shifts it as k_ingest does and writes it
// to out + (first + i) * out_stride (the slot's depth plane; the stage hook: a plain image, first = 0).
struct LmRegisterArgs {
    const LmIngestDesc* table;
    const float* rays;                  // [dh][dw][2]
    lmr::Rig rig;
    int splat_x, splat_y;
    int dw, dh;                         // the raw depth image's size
    int first, n;
    int w, h;                           // the window
    u32* zbuf;
    u8* out;
    size_t out_stride;
};
void lmk_register(hipStream_t s, const LmRegisterArgs& a);

struct LmScanArgs {
    const u8* lm;            // lowest level arena of slot 0
    size_t lm_slot_stride;
    const u32* item_t;       // work items: bank-local template index
    const u32* item_chunk;   //             chunk of LM_SCAN_CHUNK positions
    int item_lo, n_items;
    int nibble;              // 1: two positions per byte (k_scan4), scan_off in nibbles, fpad % 3 == 0
    const u32* scan_off;     // [nt][M][fpad] byte offsets into the arena
    const int* scan_P;       // [nt] template_positions
    const int* scan_n;       // [nt] total number of features at the lowest level | per-modality in-bounds counts << 8, << 16
    int M, fpad;
    const int* raw_thr_by_n; // [128]
    int W, T;
    LmDevHeader* hdr;        // slot 0; aux_slot_stride apart
    LmCand* cand;
    size_t aux_slot_stride;
    u32 cand_cap;
    unsigned long long* stat; // optional [1024][4] counters: features loaded / features an unpruned scan loads / lane-loads issued / (k_scan1) survivors whose exact sums were taken
    int wgs_per_slot, nslots; // workgroups' worth of work items per frame (lmh::MatchPlan), frames of the launch
    // bit-plane form (k_scan1, r05), L1 != 0: item_t / item_chunk are then the items of chunks of 128 L1 - 31 positions
    int L1, G1;               // lanes per frame, frames per wave (64 / L1)
    u32 L1_rcp16;             // ceil(65536 / L1): lane / L1 = (lane * L1_rcp16) >> 16 for lane < 64
    u32 delta_rcp16;          // ceil(65536 / delta), delta = 4 - the largest response below 4 of the similarity table
    const u32* off1;          // [nt][fpad1] BIT offsets of the features' miss planes in the arena (all modalities, one list)
    const u32* offn;          // [nt][fpad1] the same features' nibble offsets (exact sums of the survivors)
    int fpad1;
    int no_exact;             // measurement only (scan variant bit 7, WRONG lists): the survivors' exact sums are skipped
    unsigned long long* surv; // survivor queues of the launch's stream, one per XCD: [16 + x * (surv_cap / 8) + i] = template << 32 | slot << 20 | position;
    u32 surv_cap;             //    k_scan1_exact takes their exact sums (null / overflow: the wave does it itself).  [8 * surv_set + x] = entries appended
    int surv_set;             //    to queue x: two sets of counters, a launch uses one and its k_scan1_exact zeroes the other for the next launch
    int exact_spread;         // 1: the slots keep ONE spread byte per position instead of the response memories (d_lm_fast, bit 31 of plane_ori): the exact
    const u32* offs3;         //    sums go through the response table.  offs3 [nt][fpad1]: orientation << 29 | byte offset of the feature's spread memory
    const u64* resp_tab;      //    [256] responses of the 8 orientations to a spread byte
    // r06, the bit-plane scan with a frame's planes in LDS (k_scanl), lds_form != 0: one 1024-thread workgroup = (frame, share of the templates)
    int lds_form, R;          // R: workgroups per frame
    const u32* offl;          // [nt][fpad1] (LDS byte address of the feature's first dword) << 8 | bit shift
    const u32* offsl;         // [nt][fpad1] orientation << 29 | offset in the LDS image of the spread bytes
    const u32* litem;         // lane items [.][4]: template << 8 | unit of 128 positions (0xFFFFFFFF: none), the template's scan_n, scan_P, 0
    int litem_lo, n_litems;   // the launch's lane items
    u32 pb;                   // bytes of one miss plane, T*T*wh / 8
    u32 mod_stride, planes_off, plane_ori;   // arena: modality block stride, offset of a block's planes (8 * ori_stride), stride between them
    u32 tbl_bytes;            // LDS behind the image: zeros during the first stage (the padded list entries of ANY unit read them: ceil(wh / 128) * 16 + 32 bytes
                              //    at least), the response table during the second; then 16 bytes of queue header and the queue
    u32 queue_cap;            // survivor entries the LDS queue holds
    int dbg;                  // timing experiments of lm_time_scan_batch only (variant bits 9..11), WRONG lists: see k_scanl
};
// a11+a12+a13: similarity scan over the lowest level fused with the threshold scan.  Which kernel runs on which grid, and every field above
// that is a number derived from the call, comes from lmh::plan_match (lm_host.h: the variant bits are listed there); lmk_scan_run launches
// the plan's scan steps.  queue: the lane's survivor queue (a SurvReset step zeroes its counters; a.surv may be null).
// The variants lm_set_scan_variant accepts: bits 0-5 (k_scan4's load blocks and pruning rules) and bit 8 (k_scan1's survivors summed by the
// wave itself) leave the candidate lists as they are; bits 6 / 7 skip work and belong to lm_time_scan* alone.
#define LM_SCAN_VARIANT_SETTABLE (0x3F | 0x100)
void lmk_scan_run(hipStream_t s, const lmh::MatchPlan& plan, const LmScanArgs& a, unsigned long long* queue);
// k_scanl takes all of a CU's LDS: raises its dynamic-LDS limit on the current device (the attribute is per device); false: k_scanl cannot run there
bool lmk_scanl_raise_lds();

struct LmRefineArgs {
    const u8* lm;            // arena of the level being refined at, slot 0
    size_t lm_slot_stride;
    LmLevelGeom g;
    int M;
    const LmRefMeta* meta;   // [nt] for this level
    const LmRefFeat* feats;
    const u32* sim_lut;      // SIMILARITY_LUT as 64 dwords: [ori][lo 16 B | hi 16 B]
    LmDevHeader* hdr;
    LmCand* cand;
    u64* keys;               // [match_cap][2]
    size_t aux_slot_stride;
    u32 cand_cap;
    u32 match_cap;
    float threshold;
    const int* t_global;
    const int* t_class;
    const u32* plan;         // slot -> XCD plan of k_refine_plan ([8][plan_cap] slots + [8] lengths), or nullptr
    int plan_cap;
    int blocks_per_slot, nslots;  // lmh::MatchPlan::blocks_per_slot, frames of the launch
    unsigned long long* stat;     // counting experiment (LM_REFINE_STAT=1): [0] candidates refined alone, [1] in pairs, [2] pair candidates the pruning dropped, [3] pairs in which BOTH were,
                                  //   [4] single candidates the pruning dropped, [5] candidates dropped by the final test; nullptr otherwise
};
struct LmSortArgs {
    LmDevHeader* hdr;
    u64* keys;               // (hi, lo) per match; the split form sorts chunks of LM_SORT_CHUNK in place
    LmOutMatch* out;         // [LM_SORT_CAP] per slot
    size_t aux_slot_stride;
    LmHostBlock* host;       // host-mapped, slot 0
    size_t host_slot_stride;
    u32 cand_cap, match_cap;
    int split;               // 1: lists longer than LM_SORT_CHUNK keys are sorted as chunks by LM_SORT_CAP / LM_SORT_CHUNK workgroups per
                             // slot and merged by a second launch (k_merge_unique); same lists either way
};
// a14-a15, steps [from, to) of a plan's refinement and sort launches (lmh::plan_match):
//   k_refine_plan     balanced slot -> XCD lists for k_refine from the slots' candidate counts (nslots <= 1024, nslots % 8 == 0) into plan_buf
//   k_refine          similarityLocal + argmax + rescore (+ threshold filter) at a step's level, with by_level[level]; the launch at level 0
//                     also emits sort keys
//   k_emit_unrefined  pyramid_levels == 1: candidates become matches unrefined
//   k_sort_unique     sort + adjacent-unique of up to LM_SORT_CAP keys, one workgroup per slot (split: four, and k_merge_unique behind them)
void lmk_refine_run(hipStream_t s, const lmh::MatchPlan& plan, int from, int to, const LmRefineArgs* by_level, const LmSortArgs& sort, u32* plan_buf);

struct LmPackArgs {
    const LmDevHeader* hdr;  // slot 0 of the range; aux_slot_stride apart (pad[0] = length of the sorted list)
    const LmOutMatch* out;   // sorted lists, LM_SORT_CAP records per slot
    size_t aux_slot_stride;
    int nslots;
    u32 cap_total;           // records `rec` can hold
    int* cnt;                // [nslots + 1]: list lengths, then the status word
    LmOutMatch* rec;         // packed lists
};
// 8e: the sorted lists of nslots frames back to back + their lengths (a rank's contribution to the all-gather).
void lmk_pack_lists(hipStream_t s, const LmPackArgs& a);

// ---- f1: batched colour check (HighLevelLinemod.cpp:113-135,159-161,424-434) -------------------------------------
#define LM_HULL_MAX 128      // hull vertices per template (two modalities x 63 features at most = 126 points)
// one bit per pixel: 8-bit HSV of the BGR image inside [lo, hi]; divtab = sdiv_table[256] | hdiv_table180[256]
void lmk_hsv_mask(hipStream_t s, const u8* bgr, int w, int h, const LmHsvRange& rg, const int* divtab, u32* mask, int wpr,
                  size_t in_stride, size_t mask_stride, int nslots);
// the device NORMAL_LUT buffer holds the 8000-byte table and, behind it, the same table as the rank codes k_dnormal writes
#define LMK_NORMAL_CODE_OFFSET 8000
// What a level-fused launch (k_phase: few frames; k_bphase / k_bsplit: a lone lane of a batch; the default two-level pyramid only) works
// on; lmk_preprocess_run fills it from LmPreArgs.  The routes and their launches: lm_host.cpp plan_phases / plan_batch_phases.
struct LmPhaseArgs {
    const u8* bgr0; u8* bgr1; const u16* depth;      // level-0 colour image, level-1 colour image (written by launch 1), depth (or null)
    u8 *cs0, *cs1, *ds;                              // scratch: colour level 0 / 1 (lmk_color_scratch_bytes each), depth (w * h)
    u8 *qc0, *qc1, *qd0;                             // quantised images
    u8 *lm_c0, *lm_c1, *lm_d0, *lm_d1;               // linear memories: modality base pointers of levels 0 and 1
    int w, h;                                        // level 0; level 1 is w / 2 x h / 2
    float weak_threshold; int dist_thr, diff_thr;
    const u8* normal_lut; const u64* resp_tab;
    u32 ori_stride1;                                 // bytes between the response memories of level 1 (nibble packed)
    u32 plane_ori1;                                  // bytes between level 1's miss-bit planes (behind the 8 response memories of a modality), 0: none
    size_t slot_stride; int nslots;
};
// out2[0] / out2[1] += floats of k_dnormal's tail domain on which its short reciprocal / square root differ from the compiler's
// correctly rounded ones (device counters, zeroed by the caller)
void lmk_selftest_float_tail(hipStream_t s, unsigned long long* out2);

struct LmHullArgs {
    const LmOutMatch* matches; u32 n;
    const u32* class_base;       // [n_classes] first hull of the class in hull_off
    const u32* hull_off;         // [n_templates + 1] first vertex of every template's hull
    const int16_t* hull_xy;      // vertices (x, y) relative to the template origin
    const u32* mask; int wpr;    // colour bit mask of the frame
    const int* match_slot;       // optional [n]: match i lies in the frame whose mask starts mask_slot_words * match_slot[i] words behind `mask`
    size_t mask_slot_words;
    int w, h;
    long long* out;              // [n][2]: pixels in the hull, pixels in the hull with the colour bit set
};
// false: the frame has more rows than the kernel's per-wave row table fits into LDS (nothing was launched)
bool lmk_hull_counts(hipStream_t s, const LmHullArgs& a);

// r06, the depth check's early verdicts on the GPU (medianMat, HighLevelLinemod.cpp:336-349,437-457): per query the crop [x0, x1) x [y0, y1) of a resident
// depth frame with depths <= 1 counted as 65535 -- how many values lie below `lo`, how many inside [lo, hi]
struct LmDepthQuery { int x0, y0, x1, y1; int lo, hi; int slot; int pad; };      // (same layout as lm_depth_query of the C ABI)
struct LmDepthArgs {
    const u16* depth;            // depth image of slot 0 (the resident, already translated frame)
    size_t slot_stride;          // bytes between the slots' frames
    int w, h;
    const LmDepthQuery* q; u32 n;
    u32* out;                    // [n][2]: values below lo, values in [lo, hi]
};
void lmk_depth_counts(hipStream_t s, const LmDepthArgs& a);

// The depth check's sorted order statistic (lm_k_depth_select.hip): per query the element at 0-based index `rank` of the
// ascending sort of the crop [x0, x1) x [y0, y1) with depths <= 1 taken as 65535; an empty crop gives 65535.  One workgroup per query.
struct LmDepthSelQuery { int x0, y0, x1, y1; int rank; int slot; };              // (same layout as lm_depth_select_query of the C ABI)
struct LmDepthSelArgs {
    const u16* depth;            // depth image of slot 0
    size_t slot_stride;          // bytes between the slots' frames
    int w, h;
    const LmDepthSelQuery* q; u32 n;
    u16* out;                    // [n]
};
// naive_histogram: one shared LDS histogram, one atomic per pixel -- the yard-stick of the contention decision (LM_TUNE_DEPTH_SELECT_HIST), same values
void lmk_depth_select(hipStream_t s, const LmDepthSelArgs& a, bool naive_histogram);

// ---- ICP pose refinement (lm_k_icp.hip, DESIGN.md sections 9 and 21).  The records are lm_common.h's; which launches run on which grids
// is planned on the host (lm_host.h plan_icp_batch / plan_icp_levels): the two launchers execute a plan and decide nothing.
namespace lmh { struct IcpChunkPlan; struct IcpLevelsPlan; }
// What a chunk's kernels read: the scratch base the records' offsets count from, and the chunk's tables inside it.
struct LmIcpBatchArgs {
    u8* base;
    const LmIcpSceneRec* scene;      // [queries of the chunk]
    unsigned long long* zsum;        // [queries]: sum of the bbox's blurred z, zeroed by the caller on the stream
    u32* counts;                     // [queries][2]: pixels kept by the 300 mm test, points written = kept / step
    const LmIcpRegRec* reg;          // [queries]
    const LmIcpLevel* lev;           // [queries][levels]
    LmIcpPose* st;                   // [poses of the live queries]; P, q and li set by the caller
    double* out;                     // [poses][16]: the refined 4x4 poses (row-major)
    int W, H, step, nlevels;
    double rejection_scale;
};
// Scene clouds of prepareDepthForIcp of every query of the chunk (five launches): cloud[counts[2 q + 1]][6] (x y z nx ny nz, float).
void lmk_icp_scene(hipStream_t st, const lmh::IcpChunkPlan& chunk, const LmIcpBatchArgs& a);
// registerModelToScene of every pose of the chunk's live queries
void lmk_icp_register(hipStream_t st, const lmh::IcpLevelsPlan& plan, const LmIcpBatchArgs& a);

// ---- best-pose check (lm_k_verify.hip)
// meanDepthDifference's count and sum of nq queries on w x h images: renders = z-buffers (from_z; u32 [nq][w * h], as lmk_gen_zbuffer
// leaves them) or depth images (u16, same layout); query q's scene = scenes + scene_idx[q] * scene_stride (elements);
// out[nq] = {u32 count, u32 unused, u64 sum} (zeroed by the caller)
void lmk_icp_verify(hipStream_t s, bool from_z, const void* renders, const u16* scenes, const int* scene_idx, size_t scene_stride, int nq, int w,
                    int h, int scene_min, u32* out);

// ---- template-bank generation (lm_k_gen.hip)
// One candidate of a template level: (x, y) at the level, label = quantised bin (label_of), score = squared gradient magnitude
// (colour) or chessboard distance (depth, before the per-label division).
struct LmGenCand { int16_t x, y; int32_t label; float score; };
// Geometry of a chunk's per-image level buffers (flags: img_px bytes, row distances: 8 x img_px u16 per image; level l at off[l]) and
// of the detector's slots (quantised level l, modality m at q_off[l][m] in a slot; the colour magnitudes at mag_off[l] in the mag arena,
// slot_stride apart).  rows = level-0 height (the candidate launch's grid.x).
struct LmGenGeom {
    int L, M, rows;
    int w[4], h[4], et[4];              // (4 = LM_MAX_LEVELS)
    size_t off[4], img_px;
    size_t q_off[4][2], mag_off[4];
    float min_mag;
};
// SoftRender::render_view of one mesh under nviews view-projection matrices (vp[nviews][16], Mat4::m order): sv[nviews][nv] window
// coordinates, zbuf / cov / depth [nviews][W * H] (zbuf: float bits of the nearest accepted window z)
void lmk_gen_render(hipStream_t s, const float* xyz, int nv, const u32* idx, int ntri, const float* vp, int nviews, int W, int H,
                    float4* sv, u32* zbuf, u8* cov, u16* depth);
// its first three stages alone: the z-buffers (gen_z_to_mm in lm_dev.h turns a value into the depth image's mm)
void lmk_gen_zbuffer(hipStream_t s, const float* xyz, int nv, const u32* idx, int ntri, const float* vp, int nviews, int W, int H,
                     float4* sv, u32* zbuf);
// addTemplate's in-plane rotation of nimg images (img_view / img_angle index the rendered views and the angle tables, tabs[angle] =
// adelta[W] | bdelta[W] | X0[H] | Y0[H]): rmask / rdepth [nimg][W * H], the slots' colour (and depth_slot, may be null) images slot_stride
// apart, and the eroded mask er [nimg][W * H] (er may be null: no erosion)
void lmk_gen_rotate(hipStream_t s, const u8* cov, const u16* dep, const int* img_view, const int* img_angle, const int* tabs, int nimg,
                    int W, int H, u8* rmask, u16* rdepth, u8* bgr_slot, u16* depth_slot, size_t slot_stride, u8* er);
// pass 0: mask flags and depth row distances of every level, then per (image, list, row) the candidate count cnt and, for depth, the
// interior count icnt ([image][L][rows]); pass 1: the candidates at rowoff ([image][L * M][rows], absolute indices into out).
// slot0 = the first slot's base, mag = the magnitude arena's first slot (both slot_stride apart).
// er = the images' level-0 masks, W bytes per row and W * H per image (W is only their pitch here: at least the frame's width; the
// levels' sizes are g's).  unmasked (may be null; one int per image): non-zero = the image has no mask -- colour candidates anywhere,
// the depth interior is the whole level, er is not read for it.
void lmk_gen_candidates(hipStream_t s, int pass, const u8* er, const int* unmasked, int W, int H, int nimg, const LmGenGeom& g, u8* flags,
                        u16* hp, const u8* slot0, const u8* mag, size_t slot_stride, u32* cnt, u32* icnt, const u32* rowoff, LmGenCand* out);

// ---- feature selection (lm_k_select.hip): select_color / select_depth of lm_extract.cpp on device-resident lists
// One list: candidates [lo, lo + n) of the candidate array in row-major order, `want` features wanted, distance = pick_scattered's
// initial distance (computed on the host), depth != 0: the scores are divided by their label's count first; alive_lo = the list's first
// word in the alive bitmap, which holds lmk_select_alive_words(n) words for it.
#define LM_SELECT_THREADS 1024
struct LmSelList { u32 lo, n; int want; float distance; int depth; u32 alive_lo; };
inline size_t lmk_select_alive_words(size_t n) { return (n + 32u * LM_SELECT_THREADS - 1) / (32u * LM_SELECT_THREADS) * LM_SELECT_THREADS; }
// features[list][LM_MAX_FEATURES] in the host's order, n_out[list] = want, or -1 for fewer than want candidates (nothing written);
// skey: one word per candidate of the array (scratch)
void lmk_select(hipStream_t s, const LmSelList* lists, int n_lists, const LmGenCand* cand, u32* skey, u32* alive, lm_feature* features,
                int* n_out);

// ---- pose-error evaluation (lm_k_eval.hip)
// Hodan / VSD counts of nq queries: renders = z-buffers (from_z; u32 [2 nq][npx], view 2q the GT, 2q + 1 the estimate) or depth images
// (u16, same layout); scenes[scene_idx[q]][npx]; counts[nq][8] (zeroed by the caller) += rendered GT, rendered estimate, visible GT,
// visible estimate, intersection, union, within tau
void lmk_eval_vsd(hipStream_t s, bool from_z, const void* renders, const u16* scenes, const int* scene_idx, int nq, size_t npx, int delta,
                  int tau, u32* counts);
// ADD (symmetric = 0) / ADD-S (1) of nq queries (queries[nq][24] = R_gt t_gt R_est t_est) over the m = ceil(nv / step) vertices 0, step, ...
// of xyz: dist[nq][m] per-vertex distances, mean[nq]; scratch gt / est [nq][m] float4, minbits [nq][m], part [nq][lmk_eval_add_parts(m)]
size_t lmk_eval_add_parts(int m);
void lmk_eval_add(hipStream_t s, const float* xyz, int step, int m, const float* queries, int nq, int symmetric, float4* gt, float4* est,
                  u32* minbits, float* dist, double* part, float* mean);

// ---- resident frames out again, with primitives drawn (lm_k_export.hip).  Frame i of the call is slot first + i and
// reads images[i]; its tile t (row-major, tiles_x x tiles_y tiles of lmh::EXPORT_TILE_W x EXPORT_TILE_H window pixels) walks the records
// recs[idx[tile_off[i * tiles + t] .. tile_off[i * tiles + t + 1])] in that order.  All four tables lie in one device block.
struct LmExportArgs {
    const u8* frame;                    // frame arena (slot 0), slot_stride apart; the level-0 colour frame at off_bgr
    size_t slot_stride, off_bgr;
    int first, n;
    int w, h;                           // w % 16 == 0
    int tiles_x, tiles_y;
    int n_plain, n_float;               // how many of the n frames have an 8-bit / a float destination (a kernel without frames is not launched)
    const LmExportImage* images;
    const u32* tile_off;
    const u32* idx;
    const lmw::Rec* recs;
};
void lmk_export(hipStream_t s, const LmExportArgs& a);
