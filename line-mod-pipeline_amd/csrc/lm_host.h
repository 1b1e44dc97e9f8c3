// lm_host.h -- host-only parts of liblinemod_hip.so: the template bank as the caller sees it
// (classes -> template pyramids -> features, cv::linemod::Detector's class_templates map), its
// translation into the device bank of one shard, the bank file format, the default tables and the
// host-side sort/merge of match records.
#pragma once
#include <string>
#include <vector>

#include "../../include/linemod_hip.h"
#include "lm_common.h"
#include "lm_draw.h"

namespace lmh {

struct Template {  // cv::linemod::Template
    int width = 0, height = 0, pyramid_level = 0;
    std::vector<lm_feature> features;
};
typedef std::vector<Template> TemplatePyramid;  // [level * M + modality]

struct ClassEntry {
    std::string id;
    std::vector<TemplatePyramid> pyramids;  // index = template_id
};

struct Bank {
    std::vector<ClassEntry> classes;
    int find(const std::string& id) const;
    // returns class index or -1 (err set)
    int add_class(const std::string& id, int n_templates, const lm_template_desc* descs, const lm_feature* features,
                  int levels, int modalities, std::string& err);
    int add_pyramid(const std::string& id, TemplatePyramid&& tp);  // returns template id
};

// What every template pyramid of the bank must satisfy, whoever built it (lm_add_class, lm_load_bank, lm_load_yaml --
// the YAML reader parses files this library did not write): levels x modalities templates ordered [level * M + modality],
// at most 63 features each (upstream CV_Assert), at least one feature per level (similarity divides by their number),
// labels 0..7, coordinates and sizes in 0..32767 (16-bit fields of the device records).
bool check_template_pyramid(const TemplatePyramid& tp, int levels, int modalities, std::string& err);
// The modality parameters a detector can run with (lm_create, lm_load_yaml): finite non-negative thresholds, feature
// counts in 1..63.
bool check_modality_params(const lm_config& cfg, std::string& err);

// Host image of the device bank of one shard (uploaded verbatim by lm_detector.hip).
struct DeviceBankHost {
    int fpad = LM_SCAN_FPAD;
    std::vector<int> t_global, t_class;            // [nt] global template id / class index
    std::vector<u32> scan_off;                     // [nt][M][fpad]
    std::vector<int> scan_P, scan_n;               // [nt]
    std::vector<u32> item_t, item_chunk;           // scan work items, contiguous per class
    std::vector<int> class_item_lo, class_item_hi; // [n_classes]
    std::vector<int> class_t_lo, class_t_hi;       // bank-local template range per class
    std::vector<double> class_alg_bytes;           // sum_t sum_m F_m(t) * P(t) per class
    std::vector<double> class_load_bytes;          // bytes the scan's vector loads request per frame, per class
    std::vector<LmRefMeta> ref_meta[LM_MAX_LEVELS];
    std::vector<LmRefFeat> ref_feat[LM_MAX_LEVELS];
    // bit-plane scan (k_scan1, r05; only when the scanned level has planes): the in-bounds features of all modalities as ONE list per
    // template, in the lists' order -- bit offsets of the miss planes and the same features' nibble offsets
    int fpad1 = 0;
    std::vector<u32> off1, offn, offs3;            // [nt][fpad1]; offs3: orientation << 29 | byte offset of the feature in the modality's spread memory (the level written without response memories)
    long long items1_by_L[65] = {};                // work items when a frame takes L lanes: sum over templates of ceil(P / (128 L - 31))
    // r06, the same scan with a frame's planes in LDS (k_scanl; lds_ok: the level's planes of all modalities fit LM_SCANL_IMAGE_MAX bytes, a plane is a
    // whole number of 16-byte pieces, positions and templates fit the survivor entry): the lists once more in the LDS image's layout
    // [modality][orientation][T*T*wh / 8 bytes], without the arena's pads
    bool lds_ok = false;
    std::vector<u32> offl;                         // [nt][fpad1] (LDS byte address of the dword holding the feature's first bit) << 8 | bit shift; pad: the zero block
    std::vector<u32> offsl;                        // [nt][fpad1] orientation << 29 | byte offset in the LDS image of the spread bytes [modality][T*T*wh]
    std::vector<u32> litem;                        // lane items, template-major: template << 8 | unit of 128 positions (0xFFFFFFFF: a filler)
    std::vector<u32> lrec;                         // [n lane items][4] the same with the template's records: item, scan_n, scan_P, 0 -- ONE load per lane item
    std::vector<int> lbegin;                       // [nt + 1] first lane item of a bank-local template
};
// k_scan1's work items for L lanes per frame (chunks of 128 L - 31 positions), template-major like item_t / item_chunk; begin[t] =
// first item of bank-local template t (begin[nt] = number of items)
void build_items1(const DeviceBankHost& hb, int L, std::vector<u32>& item_t, std::vector<u32>& item_chunk, std::vector<int>& begin);
// the scanned level has miss planes, and those of all M modalities fit the LDS image of k_scanl
bool lds_image_fits(const LmLevelGeom& g, int M);

// ---- Which similarity scan runs, and so which layout the pre-processing writes for the scanned level (lm_detector.hip consumes the plan).
// k_scan4 / k_scan read the response memories; the bit-plane scans k_scan1 (planes from L2) and k_scanl (planes in LDS) read the miss planes
// and take their survivors' exact sums from the response memories or, where those were not written, from the spread byte.
enum class Layout : unsigned char {
    Responses,            // the response memories alone
    ResponsesAndPlanes,   // ... and the miss planes
    SpreadAndPlanes,      // one spread byte per position and the planes, WITHOUT the response memories: only a bit-plane scan can read it
};
inline unsigned layout_bit(Layout l) { return 1u << (unsigned)l; }
// a launch reads ONE layout of the scanned level (LmScanArgs::exact_spread): spread-byte slots mix with no other
inline bool layouts_mixed(unsigned held) {
    return (held & layout_bit(Layout::SpreadAndPlanes)) && held != layout_bit(Layout::SpreadAndPlanes);
}

// What the planner looks at, filled from the detector.
struct ScanInputs {
    int form = 0;                       // LM_TUNE_SCAN_FORM
    int M = 1;                          // modalities
    bool nibble = false, planes = false;   // the scanned level's memories are nibble-packed / it has miss planes
    bool lds_fits = false;              // lds_image_fits
    bool bank_built = false;            // the device bank is current (the fields below describe it)
    bool scanl_bank = false;            // the bank's lists fit k_scanl (lds_ok) and its lane items are uploaded
    bool scanl_device = false;          // the device took k_scanl's LDS size
    int fpad1 = 0;                      // DeviceBankHost::fpad1 (0: no bit-plane lists)
    const long long* items1_by_L = nullptr;   // DeviceBankHost::items1_by_L, [65]
    long long items4 = 0;               // k_scan4's work items of the bank
    size_t frame_stride = 0;            // bytes between two frames' arenas
    u32 arena_bytes = 0;                // the scanned level's arena
    float threshold = -1.0f;            // the similarity threshold in force
    float scan1_min_threshold = 50.0f;  // LM_TUNE_SCAN1_MIN_THRESHOLD
    int scanl_min_slots = 24;           // form 0 takes k_scanl from this many frames per call
    int scanl_R = 0;                    // LM_SCANL_R (experiments): k_scanl's shares per frame instead of the cost model's, 0 = unset
};

// The layout a call of n frames writes.
Layout plan_layout(const ScanInputs& in, int n);

struct ScanPlan {
    enum Kind {
        Scan4,            // k_scan4 (nibble level) or k_scan (byte level)
        Scan1,            // k_scan1, param = lanes per frame
        ScanL,            // k_scanl, param = workgroups (shares of the lane items) per frame
        Mixed,            // refused: spread-byte slots with slots of another layout
        NoBitPlaneForm,   // refused: spread-byte slots no bit-plane scan can take
    };
    Kind kind = Scan4;
    int param = 0;
};
// The scan of nslots frames over one range of classes: `layouts` = the layout_bit of every slot's layout, n_litems = the range's
// k_scanl lane items.
ScanPlan plan_scan(const ScanInputs& in, int nslots, unsigned layouts, int n_litems);

// ---- Which kernels a call's pre-processing (a3-a10) launches, on which grids (lm_detector.hip fills the inputs, lm_k_preprocess.hip
// lmk_preprocess_run executes the steps; no decision is taken anywhere else).  Values only: no HIP, no pointers.
// The LM_TUNE_* knobs of the pre-processing are process-wide (include/linemod_hip.h).  lm_set_tuning stores them here; a call takes ONE
// snapshot at its start, so all of its launches see the same values whatever another detector's thread sets meanwhile.
struct PreKnobs {
    int cblur_variant = 0;      // 0: by work (one-shot k_cblur for few frames; batches: k_cblur_sh, or k_cblur_mx for frames of up to 2 MB), 1: k_cblur, 3: k_cblur_sh, 4: k_cblur_mx
    int cgrad_variant = 0;      // 0: by work (fused k_cgrad for batches), 1: k_corient + k_cvote, 2: k_cgrad, 3: k_cgrad with 32-row strips
    int pyrdown_variant = 0;    // 0: by work (k_pyrdown8 for few frames, the row-walking k_pyrdown16 for batches), 1: k_pyrdown8, 2: k_pyrdown16
    int dmedian_variant = 0;    // 0: by work (DM_ROWS output rows per lane for few frames, DM_ROWS_BATCH for batches), 1 / 2: force either
    int blur_pyr = 1;           // level-0 blur and cv::pyrDown of a batch in one slot-interleaved launch (k_blur_pyr / k_blur_mx_pyr); 0: two launches
    int blur_pyr_interleave = 2;   // k_blur_pyr deals a slot's blur and pyrDown tiles out evenly by rows: 0 never, 1 always, 2 frames of more than 2 MB
    int blur_strip = 0;         // rows per strip of the level-0 blur inside k_blur_pyr / of the matrix-core blur: 0 = by shape and work, 16 / 32 / 64 forced
    int cgrad_levels = 1;       // the two levels' gradients of a batch in one grid (k_cgrad_levels); 0: one launch per level
};
PreKnobs pre_knobs();                       // the snapshot
bool set_pre_knob(int key, int value);      // key: an LM_TUNE_* key of the pre-processing kernels; false: not one of them, or value out of range

struct PreLevel {
    int w = 0, h = 0, T = 0;
    int mode = 0;               // what the level's linear memories hold: 0 response memories, 1 one spread memory, 2 nibble-packed response memories
    // low four address bits of the level's colour image, colour scratch, quantised images and linear memories (per modality)
    u32 a_bgr = 0, a_cs = 0, a_quant[2] = {0, 0}, a_lm[2] = {0, 0};
};
struct PreInputs {
    int M = 1, L = 1;
    int n = 1;                  // frames of the call
    int weight = 1;             // a frame counts as this many 640 x 480 frames in the few-frame / batch selection
    PreLevel lv[LM_MAX_LEVELS];
    bool masked = false;        // a slot of the call has a match mask or a mask rule
    bool lut_onehot = true;     // the normal LUT holds 0 or one-hot bytes (the streaming depth kernels count on it)
    bool others_busy = false;   // another lane has work in flight
    bool want_mag = false;      // the caller reads the gradient magnitudes (template extraction)
    int phase_max_slots = 15, batch_phases = 2;    // LM_TUNE_PHASE_MAX_SLOTS, LM_TUNE_BATCH_PHASES
    u32 planes = 0;             // the scanned level's plane stride when the planes are written (bit 31: spread bytes, no response memories), 0: none
    u32 ori_stride = 0;         // bytes between the scanned level's response memories
    u32 a_depth = 0, a_ds = 0;  // low four address bits of the depth image and the depth scratch ...
    u32 a_stride = 0;           // ... and of the byte stride between slots
    PreKnobs knobs;
};

enum class PreKernel : unsigned char {
    Pyrdown, Pyrdown8, Pyrdown16, NnHalf,
    BlurPyr16, BlurPyr32, BlurPyr64, BlurMxPyr,
    Cblur, CblurSh16, CblurSh32, CblurMx,
    Corient, Cvote, Cgrad8, Cgrad16, Cgrad32, ColorQuantize,
    CgradLevels32_16, CgradLevels32_8, CgradLevels16_16, CgradLevels16_8, CgradLevels8_8,
    Dnormal, Dmedian4, Dmedian16, DepthQuantize,
    MaskRules, MatchMasks,      // built from the slots by the detector (enqueue_mask_rules / enqueue_match_masks)
    LmSpread2, LmSpread5, LmFast2_128, LmFast4_64, LmFast5_128, LmFast8_40, LmFast8_80, LinearMemories,
    Phase1, Phase2, Phase3, Phase4_T5, Phase4_T2,
    Bsplit0, Bsplit1_16, Bsplit1_32, Bsplit2,
    Bphase1_T5_16, Bphase2_T5_16, Bphase3_T5_16, Bphase1_T5_32, Bphase2_T5_32, Bphase3_T5_32,
    Bphase1_T2_16, Bphase2_T2_16, Bphase3_T2_16, Bphase1_T2_32, Bphase2_T2_32, Bphase3_T2_32,
    Count
};
const char* pre_kernel_name(PreKernel k);

struct PreStep {
    PreKernel k = PreKernel::Count;
    unsigned char level = 0, modality = 0;      // the level (pyrDown, NN half: the level WRITTEN) and modality the launch works on
    unsigned char src_shift = 0;                // linear memories: read the finer level's depth image at (2y, 2x)
    int param = 0;              // rows per strip (k_cblur_mx, k_blur_mx_pyr) / columns per segment (k_linear_memories); k_blur_pyr: deal the tiles out evenly
    u32 gx = 0, gy = 1, gz = 1; // the grid (256 threads per workgroup throughout)
    u32 lds = 0;                // dynamic LDS bytes
    LmPhaseGrid pg = {{0, 0, 0, 0}, {0, 0, 0, 0}};   // g: blocks per slot of the launch's parts (one part: g[0]); nb: a fused launch's blocks per part
};
enum class PreRoute : unsigned char { Phases, BatchPhases, Separate, Stage };
struct PrePlan {
    // the longest plan, the separate route with masks: per level pyrDown, blur, orientation, vote and two linear memories, plus the NN half
    // above level 0; the two depth kernels and the two mask steps
    static const int CAP = 7 * LM_MAX_LEVELS + 4;
    PreRoute route = PreRoute::Stage;
    int n = 0;
    int mask_step = -1;         // index of the MaskRules step (MatchMasks follows it), -1: none
    PreStep step[CAP];
    PreStep& add(PreKernel k, int level, int modality);
};

// One helper per grid formula and strip rule.
inline int pre_ceil(int a, int b) { return (a + b - 1) / b; }
inline int pre_per(int lanes) { return (lanes + 255) / 256; }                     // workgroups of 256 lanes
inline int pre_waves62(int pairs) { return (pairs + 61) / 62; }                   // the row walkers: lanes 0 and 63 of a wave only feed their neighbours
inline int pre_wg4(int waves) { return (waves + 3) / 4; }
inline int cblur_blocks(int w, int h) { return pre_per((w * 3 / 16) * pre_ceil(h, CB_ROWS)); }       // k_cblur: 16-byte blocks x row bands
inline int corient_blocks(int w, int h) { return pre_per((w / 16) * h); }                            // k_corient: 16-pixel groups
inline int cvote_blocks(int w, int h) { return pre_per((w / 16) * pre_ceil(h, CVT_ROWS)); }          // k_cvote: 16-pixel groups x bands
inline int dnormal_blocks(int w, int h) { return pre_per((w / 8) * h); }                             // k_dnormal: 8-pixel groups
inline int dmedian_blocks(int w, int h, int rows) { return pre_per((w / 8) * pre_ceil(h, rows)); }   // k_dmedian<rows>
inline int pyrdown8_blocks(int sw, int sh) { return pre_per(((sw / 2) / 8) * (sh / 2)); }            // k_pyrdown8: 8 output pixels per lane
inline int lm_spread2_blocks(int w, int h) { return pre_per((w / 32) * (h / 2)); }                   // k_lm_spread2
inline int lm_spread5_blocks(int w, int h) { return pre_per(((w / 5) / 8) * (h / 5)); }              // k_lm_spread5: eight positions per lane
inline int cblur_sh_blocks(int w, int h, int strip) { return pre_wg4(pre_waves62((w * 3 / 16) * pre_ceil(h, strip))); }
inline int cblur_sh_strip(int h) { return h > 640 ? 32 : CBS_STRIP; }
inline int cgrad_waves(int w, int h, int strip) { return pre_waves62((w / 16) * pre_ceil(h, strip)); }
inline int cgrad_blocks(int w, int h, int strip) { return pre_wg4(cgrad_waves(w, h, strip)); }
// rows per strip of k_cgrad launched alone: 32 for tall images that still fill the chip (2 of 34 label rows recomputed instead of 2 of 18),
// 16, or 8 when 16 would leave SIMDs without a wave (a 320 x 240 level is 5 waves per frame at 16)
inline int cgrad_strip(int w, int h, int n, bool force32) {
    if (force32 || (h > 640 && (long)cgrad_waves(w, h, 32) * n >= 3072)) return 32;
    return (long)cgrad_waves(w, h, CG_STRIP) * n >= 1536 ? CG_STRIP : 8;
}
inline int cgrad_strip_upper(int w, int h, int n) { return (long)cgrad_waves(w, h, 16) * n >= 1536 ? 16 : 8;}   // a level above the first: never 32
inline int pyrdown16_blocks(int sw, int sh) { return pre_wg4(pre_waves62((sw / 16) * pre_ceil(sh / 2, PD_STRIP))); }
struct MxGrid { int gx, gy, rows; };
// k_cblur_mx: a workgroup = four waves side by side, each MX_WAVE_BYTES byte columns wide, walking down a strip of rows.  96 rows measured
// best (48 / 96 / 192 / 480 within 1 % of each other); LM_TUNE_BLUR_STRIP forces 16 / 32 / 64
inline MxGrid cblur_mx_grid(int w, int h, int blur_strip) {
    const int rows = blur_strip ? blur_strip : 96;
    return {pre_ceil(w * 3, 4 * MX_WAVE_BYTES), pre_ceil(h, rows), rows};
}
inline int lm_fast_segs(int W, int seg) { return pre_ceil(W, seg); }
// k_lm_fast<8, 80>: whole segments of 80 columns take 16-column units (half the scattered stores); everything else 40-column segments
inline bool lm_fast8_wide(int W, int h, int mode, u32 a_lm, u32 a_stride, u32 ori_stride, u32 planes) {
    return mode == 2 && (W % 80) == 0 && (((size_t)W * (h / 8)) % 16) == 0 && a_lm == 0 && a_stride == 0 && (ori_stride % 8) == 0 && (planes % 2) == 0;
}
// nibble-packed response memories (two positions per byte) exist for these shapes
inline bool nibble_supported(int w, int T) { return (T == 2 || T == 4 || T == 5 || T == 8) && (w % 4 == 0) && ((w / T) % 8 == 0); }

// Single stages (the stage hooks, lm_add_template, the generator): each appends its launches to `p`.  Level l's pyrDown reads level l - 1.
void plan_pyrdown(const PreInputs& in, int l, PrePlan& p);
void plan_color_quantize(const PreInputs& in, int l, bool blurred, PrePlan& p);
void plan_depth_quantize(const PreInputs& in, PrePlan& p);
void plan_nn_half(const PreInputs& in, int l, PrePlan& p);
void plan_linear_memories(const PreInputs& in, int l, int m, u32 planes, PrePlan& p);
// a3-a10 of a call
void plan_preprocess(const PreInputs& in, PrePlan& p);

// ---- Which kernels the match stages (a11-a15) launch for one range of classes, on which grids, and every number the kernels' argument
// structs derive from the call (lm_detector.hip fills the inputs and binds the pointers; lm_k_scan.hip lmk_scan_run and lm_k_refine.hip
// lmk_refine_run execute the steps; no decision is taken anywhere else).  Values only: no HIP, no device pointers.
struct MatchInputs {
    ScanInputs scan;
    unsigned layouts = 0;       // layout_bit of every slot's layout
    int nslots = 1;
    // the range's work items: of the nibble / byte scan; of k_scan1 for items1_L lanes per frame (items1_L 0: there are none -- the planner
    // never asked, or they could not be built); k_scanl's lane items
    int n_items = 0, items1_L = 0, n_items1 = 0, n_litems = 0;
    int T = 0; u32 wh = 0, ori_stride = 0; bool nibble = false;    // the scanned level
    int M = 1, L = 1;           // modalities, pyramid levels
    int level_W[LM_MAX_LEVELS] = {};   // W of every level (the refined ones are read)
    int miss_delta = 1;
    bool have_queue = false;    // the lane has a survivor queue (Lane::d_surv)
    bool have_plan = false;     // ... and a slice of the refine plan buffer, of plan_stride_cap pieces per XCD list
    int plan_stride_cap = 0;
    int variant = 0;            // the scan variant of the launch (lm_set_scan_variant; lm_time_scan*'s own)
    int sort_split_mode = 2, sort_long_score = 0;
};
// k_scan1's lanes per frame if plan_match is going to pick it for these inputs (the caller then builds that lane count's items and the
// lane's queue, and says in items1_L / have_queue what it got), 0 otherwise
int match_scan1_lanes(const MatchInputs& in);

enum class MatchKernel : unsigned char {
    SurvReset,                  // stream memset of both counter sets of the survivor queue (16 counters)
    Scan8X, Scan4X, Scan2X,     // k_scan<U, true>: slot -> XCD mapping
    Scan8, Scan4, Scan2,        // k_scan<U, false>: slot = grid.z
    Scan4_6_P0, Scan4_6_P1, Scan4_6_P2, Scan4_12_P0, Scan4_12_P1, Scan4_12_P2, Scan4_3_P0, Scan4_3_P1, Scan4_3_P2,    // k_scan4<FB, true, PRUNE>
    Scan4NoShift,               // k_scan4<6, true, 0, true>
    Scan1, Scan1Exact, ScanL,
    RefinePlan, Refine, RefineW4, RefineLast, RefineLastW4,     // k_refine<last, W % 4 == 0>
    EmitUnrefined, SortUnique, MergeUnique,
    Count
};
const char* match_kernel_name(MatchKernel k);

struct MatchStep {
    MatchKernel k = MatchKernel::Count;
    unsigned char level = 0;    // the level a refinement launch works at
    u32 gx = 1, gy = 1, gz = 1; // the grid in workgroups
    u32 block = 256;            // threads per workgroup
    u32 lds = 0;                // dynamic LDS bytes
};
struct MatchPlan {
    static const int CAP = 3 + 1 + (LM_MAX_LEVELS - 1) + 2;    // reset, k_scan1, k_scan1_exact; the refine plan; a launch per refined level; sort, merge
    ScanPlan::Kind kind = ScanPlan::Scan4;     // Mixed / NoBitPlaneForm: refused, no steps
    // ---- what LmScanArgs takes from the plan
    int n_items = 0;            // work items of the form that runs (k_scanl: the nibble scan's, as wgs_per_slot counts them)
    int wgs_per_slot = 0;
    int L1 = 0, G1 = 1;         // k_scan1: lanes per frame, frames per wave
    u32 L1_rcp16 = 0, delta_rcp16 = 0;
    int R = 1;                  // k_scanl: workgroups per frame
    u32 pb = 0, planes_off = 0, tbl_bytes = 0, queue_cap = 0;
    int no_exact = 0, dbg = 0;
    bool exact_spread = false;  // the slots keep the spread byte, not the response memories
    bool queue = false;         // k_scan1 appends its survivors to the lane's queue (false: the waves take the exact sums themselves)
    bool flip_surv_set = false; // behind this scan's steps the lane's next launch takes the other set of queue counters
    // ---- LmRefineArgs, LmSortArgs
    int blocks_per_slot = 256, plan_cap = 0;
    bool refine_plan = false;
    int split = 0;
    // ---- the launches: scan [0, scan_end), refinement [scan_end, refine_end), sort [refine_end, n)
    int scan_end = 0, refine_end = 0, n = 0;
    MatchStep step[CAP];
    MatchStep& add(MatchKernel k, u32 gx, u32 gy, u32 gz, u32 block, u32 lds = 0);
};
// a11-a15 of nslots frames over one range of classes.  An empty range (n_items <= 0) plans no scan launch.
void plan_match(const MatchInputs& in, MatchPlan& p);

// ---- The ICP refinement of a list of queries (lm_detector_icp.hip refine()): which queries run together in a
// chunk, where every region of a chunk's scratch lies, every grid, and -- once the scene clouds' row counts are known -- every query's
// level schedule and the rounds to enqueue.  Values only: no HIP, no pointers.  lm_k_icp.hip's launchers execute it.
struct IcpQueryIn {
    int npx = 0;                // bbox pixels
    int nm = 0;                 // rows of the class's resident model cloud
    int first_pose = 0, np = 0; // the query's pose range; np == 0: the query takes no part
};
struct IcpQueryPlan {
    int query = 0;              // index into the call's queries
    int npx = 0, nb = 0;        // bbox pixels and their tiles of LM_ICP_TILE
    int nm = 0, np = 0;
    int ns_cap = 0;             // bound of the scene cloud's rows: max(npx / step, 1)
    int nch_cap = 0, nblk_cap = 0;  // 1-NN chunks and accumulation blocks of ns_cap rows
    size_t z = 0, blockcnt = 0, blockoff = 0, cloud = 0;                           // byte offsets in the chunk's scratch, 256-aligned
    size_t src0 = 0, srcL = 0, part = 0, nd = 0, nidx = 0, keys = 0, acc = 0;
};
struct IcpRegion { const char* name; int query; size_t off, bytes; };              // query -1: a table of the chunk
struct IcpChunkPlan {
    std::vector<IcpQueryPlan> q;
    int np = 0;                 // poses of all its queries (the pose table's capacity)
    int nlevels = 0;
    size_t zsum = 0, counts = 0, scene_recs = 0, reg_recs = 0, levels = 0, st = 0, out = 0;    // the chunk's tables
    size_t bytes = 0;
    u32 g_px = 0, g_normals = 0;   // grid.x of the per-pixel kernels and of k_icp_normals (the largest query's); grid.y = q.size()
    std::vector<IcpRegion> regions() const;   // every region, for whoever wants to check them
};
struct IcpBatchPlan { std::vector<IcpChunkPlan> chunks; };
// Consecutive queries are packed into a chunk while its scratch stays within `budget` bytes; a query is never split (one that exceeds the
// budget alone runs alone), and a query whose pose range overlaps an earlier one's of the chunk starts a new chunk.
void plan_icp_batch(const std::vector<IcpQueryIn>& q, int step, int levels, size_t budget, IcpBatchPlan& p);

// The level schedule of registerModelToScene for a model of n rows and a scene of ns rows, coarsest level first (see lm_host.cpp)
std::vector<LmIcpLevel> icp_schedule(int n, int ns, int iterations, int levels, double tolerance);
struct IcpLevelLaunch { int rounds = 0; u32 g_src = 0, g_chunks = 0, g_dst = 0; };   // rounds to enqueue; tiles of nL, 1-NN chunks, tiles of ndL
struct IcpLevelsPlan {
    int nlevels = 0, np = 0;            // np: poses of the live queries = rows of the pose table
    std::vector<int> pose0;             // [chunk query] its first row of the pose table, -1: not live
    std::vector<LmIcpLevel> lev;        // [chunk query][level]; rounds 0 everywhere for a query that is not live
    std::vector<IcpLevelLaunch> level;  // [level]: the maximum over the live queries
};
// scene_rows[chunk query]: rows of its scene cloud, negative = the query is not refined (a short cloud, one over the capacity)
void plan_icp_levels(const IcpChunkPlan& c, const std::vector<int>& scene_rows, int iterations, int levels, double tolerance, IcpLevelsPlan& p);

// Contiguous template_id range of shard `rank` of `size` for a class of n templates.
inline void shard_range(int n, int rank, int size, int* lo, int* hi) {
    *lo = (int)((long long)n * rank / size);
    *hi = (int)((long long)n * (rank + 1) / size);
}

// scan_list_order: how a (template, modality) list of the scanned level is ordered -- 0 ascending offsets (r01-r03), 1 dealt round-robin over the
// orientation labels, 2 descending offsets, 3 (default) greedy farthest-point order in (x, y, orientation); the sums do not depend on it
bool build_device_bank(const Bank& bank, const lm_config& cfg, const LmLevelGeom* geom, DeviceBankHost& out,
                       int scan_list_order, std::string& err);

// Convex hulls of the level-0 features (all modalities) of EVERY template of the bank, not only this shard's: the
// colour check runs on merged match lists (host/PostProcess.cpp color_check; HighLevelLinemod.cpp:113-135).
// Monotone chain: points sorted by (x, y), duplicates and collinear points dropped, counter-clockwise from the
// leftmost-lowest point -- the vertex ORDER matters, the outline is drawn edge by edge in that direction.
struct HullTable {
    std::vector<u32> class_base;   // [n_classes] index of the class's first template in hull_off
    std::vector<u32> hull_off;     // [n_templates + 1]
    std::vector<int16_t> hull_xy;  // x, y per vertex
};
void build_hull_table(const Bank& bank, int modalities, HullTable& out);

void default_similarity_lut(u8 lut[256]);
void default_normal_lut(u8 lut[8000]);

// Total order of SURVEY.md A.9 and upstream Match::operator==.
bool match_less(const lm_match_t& a, const lm_match_t& b);
bool match_eq(const lm_match_t& a, const lm_match_t& b);
void sort_unique(std::vector<lm_match_t>& v);

bool save_bank(const Bank& bank, const lm_config& cfg, const char* path, std::string& err);
bool load_bank(Bank& bank, const lm_config& cfg, const char* path, std::string& err);


// memcpy for the staging copies of uploads (r05): the destination -- a pinned staging buffer -- is read next by the DMA engine, never by
// this CPU, so the bytes go out with non-temporal stores (no read-for-ownership of the destination lines, no cache pollution: a
// third less DRAM traffic for a copy that is bound by it).  Falls back to memcpy without AVX2 or for short runs.  copy_stream_fence()
// once after a batch of calls, before the buffer is handed to the DMA engine.
void copy_stream(void* dst, const void* src, size_t n);
void copy_stream_fence();

// A w x h image translated by (ox, oy) pixels: the destination columns [x0, x1) and rows [y0, y1) that have a source pixel (destination
// (x, y) shows source (x - ox, y - oy)); empty when x1 <= x0 or y1 <= y0.
struct ShiftRect { int x0, x1, y0, y1; };
ShiftRect shift_rect(int w, int h, int ox, int oy);
inline int clamp_shift(int v, int extent) { return v < -extent ? -extent : (v > extent ? extent : v); }
// Rows [r0, r1) of the image translated by (ox, oy) pixels, zeros shifted in (cv::warpAffine with a pure translation as the
// reference's translateImg does, PoseDetection.cpp:54-59,192-197), into the dense staging buffer: the shift happens while the staging
// buffer is filled, so a shifted upload costs one pass over the image instead of two.  px = bytes per pixel.  Host memory only:
// any thread may fill disjoint row ranges (lm_stage_rows).  |ox| <= w and |oy| <= h (callers clamp: anything beyond is an all-zero frame).
void stage_rows_shifted(u8* staging, const u8* src, size_t stride, int w, int h, int px, int ox, int oy, int r0, int r1);

// ---- lm_export_frames (lm_k_export.hip): the tiles of a call and which primitives each must look at.  No HIP, no
// pointers.  Every exported image (w x h, the same for all frames of a call) is cut into tiles of EXPORT_TILE_W x EXPORT_TILE_H pixels --
// even, so an NV12 chroma block never straddles two tiles; a workgroup of k_export owns one.  A primitive is listed by every tile its
// bounding box touches: the box of lmw::make_rec (inflated by the thickness: conservative), clipped to the frame, carried into the
// exported image through the frame's undo options, clipped again.  The result of an export does not depend on the tile shape.
//   recs[k]      primitive k as the kernel reads it (list order)
//   tile_off     CSR offsets, [n_frames * tiles_x * tiles_y + 1]: tile t of frame f lists idx[tile_off[f * tiles + t] .. tile_off[.. + 1])
//   idx          primitive indices, ascending within a tile: list order is compositing order
// EXPORT_MAX_ENTRIES bounds idx (16 MiB of indices): a list of 65536 primitives that each touch 64 tiles just fits.  plan_export returns
// false, with p.entries = the entries the call needs and nothing else filled, when they exceed max_entries.
enum { EXPORT_TILE_W = lmw::TILE_W, EXPORT_TILE_H = lmw::TILE_H };
constexpr size_t EXPORT_MAX_ENTRIES = (size_t)1 << 22;
struct ExportUndo { int flip_x, shift_x, shift_y; };      // per frame, shifts clamped to the frame
struct ExportPlan {
    int tiles_x = 0, tiles_y = 0;
    size_t entries = 0;
    std::vector<lmw::Rec> recs;
    std::vector<u32> tile_off, idx;
};
bool plan_export(int w, int h, int n_frames, const ExportUndo* undo, const lm_draw_prim* prims, size_t n_prims, size_t max_entries, ExportPlan& p);
}  // namespace lmh
