// The match-stage planner (lm_host.cpp plan_match) against a table of its decisions: which kernels a11-a15 launch for one range of classes,
// in which order, on which grids, with which workgroup size and dynamic LDS, and the numbers the kernels' argument structs derive from the
// call.  Built with g++ together with lm_host.cpp (tests/test_match_plan_cpu.py); no GPU.
// WHERE THE EXPECTATIONS COME FROM: not from the planner.  tests/cpp/match_plan_expect.inc was printed by the code of the commit BEFORE the
// planner existed -- the launcher arithmetic of lmk_scan, lmk_refine_plan, lmk_refine, lmk_emit_unrefined and lmk_sort_unique and the
// formulas of make_scan_args, launch_scan, enqueue_match_stages and make_sort_args of that commit, copied into a harness whose launch macro
// records (kernel, grid, workgroup, dynamic LDS) and run for the inputs of every row.  WHICH scan runs is lmh::plan_scan's choice on both
// sides (it is that commit's, unchanged, with its own table: scan_plan_table.cpp); the rows steer it with the layouts, the form, a work-item
// table whose minimum lies at the wanted lane count, and LM_SCANL_R.  For the calls a detector can make the same launches were traced on the
// GPU on that commit and on this code (tools/match_launches.py): profiles/match_launches.txt is the reduction, identical for both, and the
// rows whose name is a label of that file are held to it (tests/test_match_plan_cpu.py).
// A row reads  <derived numbers> | step; step; ...   with a step  kernel grid b<workgroup> [+lds] [@level].
// usage: match_plan_table          prints OK and the number of rows, or the rows that differ
//        match_plan_table --dump   prints every row: index|what|text
#include "lm_host.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace match_table {

using lmh::Layout;
using lmh::ScanPlan;

struct Case {
    std::string what;
    // ---- the scan: `want` steers lmh::plan_scan
    ScanPlan::Kind want = ScanPlan::Scan4;
    bool spread = false;                // the slots keep the spread byte (SpreadAndPlanes); Scan1 otherwise runs on ResponsesAndPlanes
    bool nibble = true;
    int M = 1, nslots = 1, variant = 0;
    int n_items = 12;                   // of the nibble / byte scan
    int L1 = 0, n_items1 = 0;           // Scan1: the lane count with the fewest waves and its items
    bool items_built = true;            // ... which the detector could build
    bool have_queue = true;
    int R = 0, n_litems = 64 * 16 * 32; // ScanL: LM_SCANL_R (the lane items allow up to 32 shares)
    int T = 8; unsigned wh = 48, ori_stride = 0x700; int miss_delta = 1;
    // ---- refinement and sort
    int L = 2;
    int level_W[4] = {64, 8, 0, 0};
    bool have_plan = true; int plan_stride_cap = 136;
    int sort_mode = 2, sort_score = 0;
};

inline std::vector<Case> cases() {
    std::vector<Case> v;
    const auto named = [](const char* what) { Case c; c.what = what; return c; };
    // ---- k_scan, byte responses: every slot -> XCD mapping (1, 2, 4 frames share the 8 XCDs, multiples of 8 take whole ones, the rest slot =
    // grid.z), variant bit 2, both XCD grid formulas at item counts where the rounding shows
    for (int n : {1, 2, 3, 4, 8, 24}) for (int var : {0, 4}) { Case c = named("k_scan"); c.nibble = false; c.nslots = n; c.variant = var; v.push_back(c); }
    for (int items : {1, 13, 18, 4000}) for (int n : {1, 2, 4, 16}) { Case c = named("k_scan, item counts"); c.nibble = false; c.nslots = n; c.n_items = items; v.push_back(c); }
    for (int var : {1, 2, 3, 5, 6}) for (int n : {1, 3, 8}) { Case c = named("k_scan, unroll variants"); c.nibble = false; c.nslots = n; c.variant = var; v.push_back(c); }
    // ---- k_scan4: pairs of slots, the load-block variants, the pruning rule by modality count and bits 3-5, the no-shift instantiation
    for (int n : {1, 2, 97}) for (int var : {0, 1, 2, 3}) { Case c = named("k_scan4, load blocks"); c.nslots = n; c.variant = var; v.push_back(c); }
    for (int M : {1, 2}) for (int var : {0, 8, 16, 32, 8 | 16, 16 | 32, 8 | 32, 1 | 16, 2 | 32}) { Case c = named("k_scan4, pruning"); c.M = M; c.nslots = 8; c.variant = var; v.push_back(c); }
    for (int M : {1, 2}) for (int var : {8 | 64, 64, 8 | 64 | 1}) { Case c = named("k_scan4, no shift-undo"); c.M = M; c.nslots = 2; c.variant = var; c.n_items = 300; v.push_back(c); }
    { Case c = named("k_scan4, variant bits of the bit-plane scans"); c.variant = 128 | 256 | 512; v.push_back(c); }
    // ---- k_scan1: lanes per frame -> frames per wave -> groups (nslots a multiple of G1 and not), queue present and absent, the entry's 20-bit
    // position and 12-bit slot, the measurement variants (reset yes, k_scan1_exact no, the counter set flips as before)
    const auto scan1 = [&](const char* what, int L1, int n) { Case c = named(what); c.want = ScanPlan::Scan1; c.L1 = L1; c.n_items1 = 30; c.nslots = n; return c; };
    for (int L1 : {1, 3, 9, 16, 32, 64}) for (int n : {1, 5, 8, 24}) v.push_back(scan1("k_scan1", L1, n));
    for (int L1 : {9, 64}) for (int n : {1, 24}) { Case c = scan1("k_scan1, no queue", L1, n); c.have_queue = false; v.push_back(c); }
    for (unsigned wh : {(1u << 20) - 1u, 1u << 20}) { Case c = scan1("k_scan1, 20-bit position", 16, 8); c.wh = wh; v.push_back(c); }
    for (int n : {4096, 4097}) { Case c = scan1("k_scan1, 12-bit slot", 16, n); v.push_back(c); }
    for (int var : {128, 256, 128 | 256, 1 | 8, 512}) for (int q : {1, 0}) { Case c = scan1("k_scan1, variants", 9, 8); c.variant = var; c.have_queue = q; v.push_back(c); }
    { Case c = scan1("k_scan1, variant 256, slots beyond the entry", 16, 4097); c.variant = 256; v.push_back(c); }
    for (int md : {1, 2, 3, 4}) { Case c = scan1("k_scan1, miss delta", 9, 8); c.miss_delta = md; v.push_back(c); }
    for (int sp : {0, 1}) { Case c = scan1("k_scan1, spread-byte slots", 9, 8); c.spread = sp; v.push_back(c); }
    { Case c = scan1("k_scan1, an empty range", 9, 8); c.n_items = 0; c.n_items1 = 0; v.push_back(c); }
    { Case c = scan1("k_scan1, many items", 16, 24); c.n_items1 = 100001; v.push_back(c); }
    // ---- the two resource fallbacks: no work items for the lane count
    { Case c = scan1("no items for L1, response memories", 9, 8); c.items_built = false; v.push_back(c); }
    { Case c = scan1("no items for L1, response memories, two modalities", 9, 8); c.items_built = false; c.M = 2; c.variant = 1; v.push_back(c); }
    { Case c = scan1("no items for L1, spread bytes", 9, 8); c.items_built = false; c.spread = true; v.push_back(c); }
    // ---- k_scanl: R from the plan, the table behind the image at its floor and above it, the LDS queue, the timing bits
    const auto scanl = [&](const char* what, int R, int n) { Case c = named(what); c.want = ScanPlan::ScanL; c.spread = true; c.R = R; c.nslots = n; c.M = 2; c.wh = 1200; c.ori_stride = 0x9700; return c; };
    for (int R : {1, 4, 5, 32}) for (int n : {1, 24, 96}) v.push_back(scanl("k_scanl", R, n));
    for (unsigned wh : {16128u, 16129u, 32768u}) { Case c = scanl("k_scanl, table bytes", 4, 24); c.M = 1; c.T = 2; c.wh = wh; v.push_back(c); }
    // (the queue's 2^16 clamp lies above what a CU's LDS leaves -- 40316 entries without any image; only an image that does not fit, which no
    // detector plans, wraps the u32 difference and meets it)
    for (unsigned wh : {48u, 1200u, 2500u}) { Case c = scanl("k_scanl, queue entries", 4, 24); c.wh = wh; v.push_back(c); }
    { Case c = scanl("k_scanl, queue entries, one modality", 4, 24); c.M = 1; v.push_back(c); }
    for (int var : {128, 512, 1024, 2048, 3584, 128 | 3584, 256, 8 | 64}) { Case c = scanl("k_scanl, variants", 5, 24); c.variant = var; v.push_back(c); }
    { Case c = scanl("k_scanl, an empty range", 4, 24); c.n_items = 0; v.push_back(c); }
    // ---- refinement: one level (candidates become matches), two, three, four; the refine plan for multiples of 8 up to 1016 frames that fit
    // the lane's plan buffer; W % 4 per level
    for (int n : {1, 7, 24}) { Case c = named("one level"); c.L = 1; c.nslots = n; v.push_back(c); }
    for (int L : {2, 3}) for (int n : {1, 7, 8, 16, 1016, 1024}) { Case c = named("levels"); c.L = L; c.level_W[1] = 40; c.level_W[2] = 8; c.nslots = n; c.plan_stride_cap = 136; v.push_back(c); }
    for (int cap : {8, 9, 10}) { Case c = named("plan_cap against the buffer's"); c.nslots = 8; c.plan_stride_cap = cap; v.push_back(c); }
    for (int n : {8, 24}) { Case c = named("no plan buffer"); c.nslots = n; c.have_plan = false; v.push_back(c); }
    for (int w0 : {160, 161, 162, 163}) for (int w1 : {80, 81}) for (int n : {7, 8}) { Case c = named("W % 4"); c.L = 3; c.level_W[0] = w0; c.level_W[1] = w1; c.level_W[2] = 8; c.nslots = n; v.push_back(c); }
    { Case c = named("four levels"); c.L = 4; c.level_W[0] = 128; c.level_W[1] = 62; c.level_W[2] = 32; c.level_W[3] = 8; c.nslots = 16; v.push_back(c); }
    // ---- sort: the split form by mode and by the detector's recent list lengths
    for (int mode : {0, 1, 2}) for (int score : {0, 1, 4096}) for (int n : {1, 24}) { Case c = named("sort"); c.sort_mode = mode; c.sort_score = score; c.nslots = n; v.push_back(c); }
    // ---- calls of tools/match_launches.py, named by their labels in profiles/match_launches.txt (tests/test_match_plan_cpu.py holds these rows to the
    // GPU trace): its banks of 12 templates are 12 work items of every form at these sizes, and one lane per frame has the fewest waves
    char label[128];
    const auto traced = [&](bool color, int w0, int w1, unsigned wh) { Case c = named(label); c.M = color ? 1 : 2; c.level_W[0] = w0; c.level_W[1] = w1; c.wh = wh; return c; };
    const auto traced_scan1 = [&](Case c) { c.want = ScanPlan::Scan1; c.L1 = 1; c.n_items1 = 12; return c; };
    for (int f : {1, 2}) for (int n : {1, 7, 8, 16, 24}) {
        snprintf(label, sizeof label, "colour 128x96 form %d n %d", f, n);
        Case c = traced(true, 64, 8, 48); c.nslots = n; v.push_back(f == 2 ? traced_scan1(c) : c);
    }
    for (int var : {1, 2, 3, 4, 8, 16, 32, 256, 9, 18}) for (int f : {1, 2}) for (int n : {1, 8}) {
        snprintf(label, sizeof label, "colour 128x96 form %d n %d variant %d", f, n, var);
        Case c = traced(true, 64, 8, 48); c.nslots = n; c.variant = var; v.push_back(f == 2 ? traced_scan1(c) : c);
    }
    for (int var : {0, 1, 2, 4}) for (int n : {1, 2, 3, 4, 7, 8, 16, 24}) {
        snprintf(label, sizeof label, "colour 128x96 byte responses n %d variant %d", n, var);
        Case c = traced(true, 64, 8, 48); c.nibble = false; c.nslots = n; c.variant = var; v.push_back(c);
    }
    for (int var : {8, 16, 32, 256}) for (int f : {1, 2}) {
        snprintf(label, sizeof label, "rgbd 128x96 form %d n 8 variant %d", f, var);
        Case c = traced(false, 64, 8, 48); c.nslots = 8; c.variant = var; v.push_back(f == 2 ? traced_scan1(c) : c);
    }
    for (int mode : {0, 1}) for (int n : {1, 8}) {
        snprintf(label, sizeof label, "rgbd 128x96 form 2 n %d SORT_SPLIT %d", n, mode);
        Case c = traced(false, 64, 8, 48); c.nslots = n; c.sort_mode = mode; v.push_back(traced_scan1(c));
    }
    for (int n : {1, 7}) {
        snprintf(label, sizeof label, "colour 128x96 one level form 0 n %d", n);
        Case c = traced(true, 16, 0, 192); c.L = 1; c.nslots = n; v.push_back(c);
    }
    {   // (level 2 is 40 x 30 positions: some templates take two chunks of 1016)
        snprintf(label, sizeof label, "rgbd 320x240 three levels form 0 n 7");
        Case c = traced(false, 80, 20, 1200); c.L = 3; c.level_W[2] = 40; c.T = 2; c.n_items = 16; c.nslots = 7; v.push_back(c);
    }
    for (int n : {1, 24}) {     // (so few lane items that one workgroup per frame takes them)
        snprintf(label, sizeof label, "rgbd 640x480 form 3 n %d", n);
        Case c = traced(false, 128, 40, 1200); c.want = ScanPlan::ScanL; c.spread = true; c.R = 1; c.ori_stride = 0x9700; c.nslots = n; v.push_back(c);
    }
    return v;
}

// the work items per lane count: the wanted one has the fewest waves whatever the frame count
inline const long long* items1_table(int L1) {
    static long long t[65];
    for (int L = 0; L <= 64; ++L) t[L] = L == L1 ? 1 : 1LL << 40;
    return t;
}

inline lmh::MatchInputs inputs(const Case& c) {
    lmh::MatchInputs in;
    lmh::ScanInputs& s = in.scan;
    s.M = c.M; s.nibble = c.nibble; s.planes = c.want != ScanPlan::Scan4; s.lds_fits = true;
    s.bank_built = s.scanl_bank = s.scanl_device = true;
    s.fpad1 = 64; s.items1_by_L = items1_table(c.L1); s.items4 = 12;
    s.frame_stride = 1u << 20; s.arena_bytes = 1u << 18;
    s.threshold = 90.0f;
    s.form = c.want == ScanPlan::Scan4 ? 1 : c.want == ScanPlan::Scan1 ? 2 : 3;
    s.scanl_R = c.R;
    in.layouts = lmh::layout_bit(c.want == ScanPlan::Scan4 ? Layout::Responses : c.spread ? Layout::SpreadAndPlanes : Layout::ResponsesAndPlanes);
    in.nslots = c.nslots;
    in.n_items = c.n_items;
    in.n_litems = c.want == ScanPlan::ScanL ? c.n_litems : 0;
    if (c.want == ScanPlan::Scan1 && c.items_built) { in.items1_L = c.L1; in.n_items1 = c.n_items1; in.have_queue = c.have_queue; }
    in.T = c.T; in.wh = c.wh; in.ori_stride = c.ori_stride; in.nibble = c.nibble;
    in.M = c.M; in.L = c.L;
    for (int l = 0; l < 4; ++l) in.level_W[l] = c.level_W[l];
    in.miss_delta = c.miss_delta;
    in.have_plan = c.have_plan; in.plan_stride_cap = c.plan_stride_cap;
    in.variant = c.variant;
    in.sort_split_mode = c.sort_mode; in.sort_long_score = c.sort_score;
    return in;
}

// what a row's text is made of (the expectations were printed through the same two functions)
struct Derived {
    int n_items, wgs_per_slot, L1, G1; unsigned L1_rcp16, delta_rcp16; int R; unsigned pb, planes_off, tbl_bytes, queue_cap; int no_exact, dbg;
    int exact_spread, queue, flip, blocks_per_slot, plan_cap, refine_plan, split;
};
inline std::string head_text(const Derived& d, int L) {
    char b[512];
    int k = snprintf(b, sizeof b, "items %d wgs %d L1 %d G1 %d rcp %u/%u R %d pb %u planes_off %u tbl %u qcap %u no_exact %d dbg %d spread %d queue %d flip %d",
                     d.n_items, d.wgs_per_slot, d.L1, d.G1, d.L1_rcp16, d.delta_rcp16, d.R, d.pb, d.planes_off, d.tbl_bytes, d.queue_cap, d.no_exact, d.dbg,
                     d.exact_spread, d.queue, d.flip);
    if (L > 1) k += snprintf(b + k, sizeof b - k, " bps %d", d.blocks_per_slot);       // (one level: no launch reads it)
    snprintf(b + k, sizeof b - k, " plan_cap %d refine_plan %d split %d | ", d.plan_cap, d.refine_plan, d.split);
    return b;
}
inline std::string step_text(const char* name, unsigned gx, unsigned gy, unsigned gz, unsigned block, unsigned lds, int level) {
    char b[160];
    int k = snprintf(b, sizeof b, "%s %u", name, gx);
    if (gy != 1 || gz != 1) k += snprintf(b + k, sizeof b - k, "x%ux%u", gy, gz);
    k += snprintf(b + k, sizeof b - k, " b%u", block);
    if (lds) k += snprintf(b + k, sizeof b - k, " +%u", lds);
    if (level >= 0) k += snprintf(b + k, sizeof b - k, " @%d", level);
    snprintf(b + k, sizeof b - k, "; ");
    return b;
}

#include "match_plan_expect.inc"

}  // namespace match_table

#ifndef MATCH_PLAN_TABLE_NO_MAIN
using namespace match_table;

static std::string planned(const Case& c) {
    lmh::MatchPlan p;
    lmh::plan_match(inputs(c), p);
    if (p.kind == ScanPlan::Mixed) return "refused: mixed layouts";
    if (p.kind == ScanPlan::NoBitPlaneForm) return "refused: no bit-plane form";
    const Derived d = {p.n_items, p.wgs_per_slot, p.L1, p.G1, p.L1_rcp16, p.delta_rcp16, p.R, p.pb, p.planes_off, p.tbl_bytes, p.queue_cap, p.no_exact, p.dbg,
                       p.exact_spread, p.queue, p.flip_surv_set, p.blocks_per_slot, p.plan_cap, p.refine_plan, p.split};
    std::string out = head_text(d, c.L);
    if (!(0 <= p.scan_end && p.scan_end <= p.refine_end && p.refine_end <= p.n && p.n <= lmh::MatchPlan::CAP)) out += "STEP RANGES? ";
    for (int i = 0; i < p.n; ++i) {
        const lmh::MatchStep& s = p.step[i];
        const bool refine = s.k >= lmh::MatchKernel::Refine && s.k <= lmh::MatchKernel::RefineLastW4;
        // the stage groups say what the kernels say
        const bool scan = s.k <= lmh::MatchKernel::ScanL, sort = s.k >= lmh::MatchKernel::SortUnique;
        if (scan != (i < p.scan_end) || sort != (i >= p.refine_end)) out += "GROUP? ";
        out += step_text(lmh::match_kernel_name(s.k), s.gx, s.gy, s.gz, s.block, s.lds, refine ? s.level : -1);
    }
    return out;
}

int main(int argc, char** argv) {
    const bool dump = argc > 1 && !strcmp(argv[1], "--dump");
    const std::vector<Case> v = cases();
    const size_t n_expect = sizeof(EXPECT) / sizeof(EXPECT[0]);
    if (n_expect != v.size()) { printf("FAIL: %zu rows, %zu expectations\n", v.size(), n_expect); return 1; }
    int bad = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        const std::string got = planned(v[i]);
        if (dump) printf("%zu|%s|%s\n", i, v[i].what.c_str(), got.c_str());
        if (got != EXPECT[i]) {
            printf("row %zu (%s, n %d, variant %d):\n  planned  %s\n  expected %s\n", i, v[i].what.c_str(), v[i].nslots, v[i].variant, got.c_str(), EXPECT[i]);
            ++bad;
        }
    }
    if (bad) { printf("FAIL: %d of %zu rows\n", bad, v.size()); return 1; }
    printf("OK %zu rows\n", v.size());
    return 0;
}
#endif
