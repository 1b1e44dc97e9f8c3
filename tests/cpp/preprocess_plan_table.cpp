// The pre-processing planner (lm_host.cpp plan_preprocess and the single-stage planners) against a table of its decisions: which kernels
// a call's a3-a10 launch, in which order, on which grids.  Built with g++ together with lm_host.cpp (tests/test_preprocess_plan_cpu.py);
// no GPU.
// WHERE THE EXPECTATIONS COME FROM: not from the planner.  They are the launches of the commit BEFORE the planner existed -- the
// launchers of lm_k_preprocess.hip and lm_detector.hip's enqueue_preprocess of that commit, run for the same inputs with the launch macro
// recording (kernel, grid, dynamic LDS, the fused launches' LmPhaseGrid).  For every call a detector can make (resident frames, the stage
// hooks) the same launches were also traced on the GPU under rocprofv3 on that commit and on this code: profiles/preprocess_launches.txt
// holds the reduction, identical for both.  Rows no detector call reaches (misaligned buffers, odd strides: the arenas are 256-byte
// aligned) are derived from that commit's source alone.  One unreachable input is planned differently on purpose: level 1's quantised
// image misaligned with everything else aligned took the level-1 blur and then fell back to one launch per level; the planner never
// starts the two-level gradient route for it (the three rows marked in preprocess_plan_expect.inc).
// A step reads  kernel param grid [+lds] [nb/g]:  param = rows per strip of the matrix-core blur, k_blur_pyr's interleave flag, columns per
// segment of k_linear_memories; nb/g = a fused launch's LmPhaseGrid.
// usage: preprocess_plan_table          prints OK and the number of rows, or the rows that differ
//        preprocess_plan_table --dump   prints every row's plan: index|what|w x h|n|steps
#include "lm_host.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace plan_table {

enum Buf { NONE, BGR0, BGR1, CS0, CS1, QC0, QC1, QD0, LMC0, LMC1, LMD0, LMD1, DEPTH, DS, STRIDE };
enum Stage { CALL, ST_COLOR, ST_PYRDOWN, ST_DEPTH, ST_LM };
// PreKnobs' fields in a row: LM_TUNE_* values as lm_set_tuning takes them
struct Knobs { int cblur = 0, cgrad = 0, pyrdown = 0, dmedian = 0, blur_pyr = 1, blur_strip = 0, cgrad_levels = 1; };

struct Case {
    std::string what;
    Stage stage = CALL;
    int w = 640, h = 480, M = 2, L = 2;
    int T[4] = {5, 8, 8, 8};
    int n = 1;
    int work_weight = 1;                // LM_TUNE_WORK_WEIGHT
    int phase_max_slots = 15, batch_phases = 2;
    bool others_busy = false, masked = false, onehot = true, byte_responses = false, want_mag = false;
    unsigned planes = 0;                // the scanned level's plane word (0: the response memories alone)
    unsigned ori_stride = 0x12c00;      // of the scanned level
    Buf mis = NONE; unsigned mis_by = 0;     // one buffer (or the slot stride) off its 16-byte alignment by so many bytes
    Knobs k;
};

inline int level_w(const Case& c, int l) { return c.w >> l; }
inline int level_h(const Case& c, int l) { return c.h >> l; }
// a level's memory mode as lm_create derives it
inline int level_mode(const Case& c, int l) {
    if (c.stage == ST_LM) return 0;
    if (l + 1 < c.L) return 1;
    return !c.byte_responses && lmh::nibble_supported(level_w(c, l), c.T[l]) ? 2 : 0;
}
inline int weight(const Case& c) {
    const int wt = c.work_weight ? (int)((long)c.w * c.h / (640L * 480L)) : 1;
    return wt < 1 ? 1 : wt;
}

inline std::vector<Case> cases() {
    std::vector<Case> v;
    const auto rgbd = [](const char* what, int n) { Case c; c.what = what; c.n = n; return c; };
    const auto color = [](const char* what, int w, int h, int n) { Case c; c.what = what; c.w = w; c.h = h; c.M = 1; c.T[0] = 2; c.n = n; return c; };
    const unsigned P = 0x2600, SPREAD = 0x80000000u;
    // ---- RGB-D 640 x 480, T {5, 8}: few frames, the 15 / 16 boundary, batches
    for (int n : {1, 15, 16, 24, 96}) v.push_back(rgbd("rgbd vga", n));
    for (int bp : {0, 1, 2}) for (int busy : {0, 1}) { Case c = rgbd("rgbd vga, BATCH_PHASES x busy lanes", 16); c.batch_phases = bp; c.others_busy = busy; v.push_back(c); }
    for (int busy : {0, 1}) { Case c = rgbd("rgbd vga 96, busy lanes", 96); c.others_busy = busy; c.planes = P | SPREAD; v.push_back(c); }
    for (int cl : {0, 1}) { Case c = rgbd("CGRAD_LEVELS", 96); c.others_busy = true; c.k.cgrad_levels = cl; v.push_back(c); }
    for (int bp : {0, 1, 2, 3}) for (int bs : {0, 16, 32, 64}) { Case c = rgbd("BLUR_PYR x BLUR_STRIP", 24); c.others_busy = true; c.k.blur_pyr = bp; c.k.blur_strip = bs; v.push_back(c); }
    for (int bp : {0, 1}) for (int bs : {0, 32}) { Case c = rgbd("BLUR_PYR x BLUR_STRIP, fused", 24); c.k.blur_pyr = bp; c.k.blur_strip = bs; v.push_back(c); }
    for (int x : {1, 3, 4}) for (int n : {1, 24}) for (int busy : {0, 1}) { Case c = rgbd("CBLUR_VARIANT", n); c.others_busy = busy; c.phase_max_slots = busy ? 0 : 15; c.k.cblur = x; v.push_back(c); }
    for (int x : {1, 2, 3}) for (int n : {1, 24}) { Case c = rgbd("CGRAD_VARIANT", n); c.others_busy = true; c.phase_max_slots = 0; c.k.cgrad = x; v.push_back(c); }
    for (int x : {1, 2}) for (int n : {1, 24}) { Case c = rgbd("PYRDOWN_VARIANT", n); c.others_busy = true; c.phase_max_slots = 0; c.k.pyrdown = x; v.push_back(c); }
    for (int x : {1, 2}) for (int n : {1, 24}) { Case c = rgbd("DMEDIAN_VARIANT", n); c.others_busy = true; c.phase_max_slots = 0; c.k.dmedian = x; v.push_back(c); }
    for (int n : {1, 16}) { Case c = rgbd("PHASE_MAX_SLOTS 0", n); c.phase_max_slots = 0; v.push_back(c); }
    for (int n : {1, 16, 96}) { Case c = rgbd("a masked slot", n); c.masked = true; v.push_back(c); }
    for (unsigned pl : {P, P | SPREAD, P + 1}) for (int n : {1, 24}) { Case c = rgbd("planes", n); c.planes = pl; v.push_back(c); }
    { Case c = rgbd("ori_stride % 8", 24); c.planes = P; c.ori_stride = 0x12c04; v.push_back(c); }
    // ---- colour only 640 x 480, T {2, 8}
    for (int n : {1, 15, 16, 96}) v.push_back(color("colour vga", 640, 480, n));
    { Case c = color("colour vga, busy lanes", 640, 480, 96); c.others_busy = true; v.push_back(c); }
    { Case c = color("colour vga, T {5, 8}", 640, 480, 24); c.T[0] = 5; v.push_back(c); }
    { Case c = color("colour vga, T {5, 8}", 640, 480, 1); c.T[0] = 5; v.push_back(c); }
    // ---- colour only 1280 x 960: a frame weighs 4, n = 4 is a batch, n = 8 crosses k_blur_pyr's 768-workgroup rule
    for (int ww : {1, 0}) for (int n : {1, 3, 4, 8}) { Case c = color("colour 1280 x 960, WORK_WEIGHT", 1280, 960, n); c.work_weight = ww; v.push_back(c); }
    for (int n : {4, 8, 32}) { Case c = color("colour 1280 x 960, busy lanes", 1280, 960, n); c.others_busy = true; v.push_back(c); }
    for (int n : {8, 32}) { Case c = color("colour 1280 x 960, BLUR_PYR 0", 1280, 960, n); c.k.blur_pyr = 0; v.push_back(c); }
    for (int n : {2, 8}) { Case c = rgbd("rgbd 1280 x 960", n); c.w = 1280; c.h = 960; v.push_back(c); }
    for (int n : {8, 32}) { Case c = rgbd("rgbd 1280 x 960, busy lanes", n); c.w = 1280; c.h = 960; c.others_busy = true; v.push_back(c); }
    { Case c = rgbd("rgbd 1280 x 960, BLUR_PYR 0", 8); c.w = 1280; c.h = 960; c.k.blur_pyr = 0; v.push_back(c); }
    // ---- RGB-D 320 x 240: level 1 takes 8-row gradient strips
    for (int n : {24, 96}) for (int busy : {0, 1}) { Case c = rgbd("rgbd 320 x 240", n); c.w = 320; c.h = 240; c.others_busy = busy; v.push_back(c); }
    // ---- three and four levels, a non-one-hot LUT, byte responses
    for (int n : {1, 24}) { Case c = rgbd("three levels", n); c.L = 3; c.T[0] = 4; c.T[1] = 8; c.T[2] = 8; v.push_back(c); }
    { Case c = color("four levels, colour", 640, 480, 1); c.L = 4; c.T[0] = 5; v.push_back(c); }
    { Case c = rgbd("one level", 24); c.L = 1; c.T[0] = 8; v.push_back(c); }
    for (int n : {1, 24}) { Case c = rgbd("LUT not one-hot", n); c.onehot = false; v.push_back(c); }
    for (int n : {1, 24}) { Case c = rgbd("LM_FLAG_BYTE_RESPONSES", n); c.byte_responses = true; v.push_back(c); }
    { Case c = rgbd("T {4, 8}", 1); c.T[0] = 4; v.push_back(c); }
    { Case c = rgbd("rgbd 480 x 360 (w % 32 != 0)", 24); c.w = 480; c.h = 360; c.T[0] = 4; c.T[1] = 4; v.push_back(c); }
    // ---- one row per address-bit test that can fail
    for (Buf b : {BGR0, BGR1, CS0, CS1, QC0, QC1, QD0, LMC0, LMC1, LMD0, LMD1, DEPTH, DS, STRIDE})
        for (unsigned by : {8u, 4u})
            for (int n : {1, 24}) { Case c = rgbd("misaligned", n); c.mis = b; c.mis_by = by; c.planes = P; v.push_back(c); }
    for (Buf b : {QC0, LMC0, STRIDE}) for (int n : {1, 24}) { Case c = color("misaligned, colour", 640, 480, n); c.mis = b; c.mis_by = 8; v.push_back(c); }
    for (Buf b : {BGR1, CS1, QC1}) { Case c = rgbd("misaligned, busy lanes", 24); c.others_busy = true; c.mis = b; c.mis_by = 8; v.push_back(c); }
    // ---- the single stages, at the shapes of tests/test_gpu_stages.py and the detector's
    const int shapes[][2] = {{37, 53}, {16, 64}, {8, 8}, {17, 80}, {23, 91}, {33, 8}, {64, 48}, {640, 480}, {1280, 960}};
    for (const auto& s : shapes) for (int mag : {0, 1}) { Case c; c.what = "stage colour"; c.stage = ST_COLOR; c.w = s[0]; c.h = s[1]; c.want_mag = mag; v.push_back(c); }
    for (const auto& s : shapes) { Case c; c.what = "stage pyrDown"; c.stage = ST_PYRDOWN; c.w = s[0]; c.h = s[1]; v.push_back(c); }
    for (const auto& s : shapes) { Case c; c.what = "stage depth"; c.stage = ST_DEPTH; c.w = s[0]; c.h = s[1]; v.push_back(c); }
    { Case c; c.what = "stage depth, LUT not one-hot"; c.stage = ST_DEPTH; c.onehot = false; v.push_back(c); }
    { Case c; c.what = "stage colour, CGRAD_VARIANT 2"; c.stage = ST_COLOR; c.k.cgrad = 2; v.push_back(c); }
    { Case c; c.what = "stage colour, CBLUR_VARIANT 4"; c.stage = ST_COLOR; c.k.cblur = 4; v.push_back(c); }
    { Case c; c.what = "stage pyrDown, PYRDOWN_VARIANT 2"; c.stage = ST_PYRDOWN; c.k.pyrdown = 2; v.push_back(c); }
    const int lms[][3] = {{640, 480, 2}, {640, 480, 4}, {640, 480, 5}, {640, 480, 8}, {320, 240, 8}, {48, 36, 3}, {40, 20, 5}, {24, 24, 8}, {66, 30, 6}, {70, 35, 7}, {160, 160, 16}, {36, 36, 2}};
    for (const auto& s : lms) { Case c; c.what = "stage linear memories"; c.stage = ST_LM; c.w = s[0]; c.h = s[1]; c.T[0] = s[2]; v.push_back(c); }
    return v;
}

inline std::string step_text(const char* name, int param, unsigned gx, unsigned gy, unsigned gz, unsigned lds, const LmPhaseGrid* pg) {
    char b[256];
    int k = snprintf(b, sizeof b, "%s %d %u", name, param, gx);
    if (gy != 1 || gz != 1) k += snprintf(b + k, sizeof b - k, "x%ux%u", gy, gz);
    if (lds) k += snprintf(b + k, sizeof b - k, " +%u", lds);
    if (pg) snprintf(b + k, sizeof b - k, " %u,%u,%u,%u/%d,%d,%d,%d", pg->nb[0], pg->nb[1], pg->nb[2], pg->nb[3], pg->g[0], pg->g[1], pg->g[2], pg->g[3]);
    return b;
}

// the planner's inputs for a row, and the row's plan as text (tests/cpp/preprocess_route_dump.cpp reads both)
inline lmh::PreInputs inputs(const Case& c) {
    lmh::PreInputs in;
    in.M = c.M; in.L = c.L; in.n = c.n; in.weight = weight(c);
    for (int l = 0; l < c.L; ++l) { in.lv[l].w = level_w(c, l); in.lv[l].h = level_h(c, l); in.lv[l].T = c.T[l]; in.lv[l].mode = level_mode(c, l); }
    in.masked = c.masked; in.lut_onehot = c.onehot; in.others_busy = c.others_busy; in.want_mag = c.want_mag;
    in.phase_max_slots = c.phase_max_slots; in.batch_phases = c.batch_phases;
    in.planes = c.planes; in.ori_stride = c.ori_stride;
    unsigned* const where[] = {nullptr, &in.lv[0].a_bgr, &in.lv[1].a_bgr, &in.lv[0].a_cs, &in.lv[1].a_cs, &in.lv[0].a_quant[0], &in.lv[1].a_quant[0],
                               &in.lv[0].a_quant[1], &in.lv[0].a_lm[0], &in.lv[1].a_lm[0], &in.lv[0].a_lm[1], &in.lv[1].a_lm[1], &in.a_depth, &in.a_ds, &in.a_stride};
    if (c.mis != NONE) *where[c.mis] = c.mis_by;
    if (c.mis == LMC0) in.lv[0].a_lm[1] = c.mis_by;     // (a level's modality blocks lie a multiple of 256 bytes apart)
    if (c.mis == LMC1) in.lv[1].a_lm[1] = c.mis_by;
    in.knobs.cblur_variant = c.k.cblur; in.knobs.cgrad_variant = c.k.cgrad; in.knobs.pyrdown_variant = c.k.pyrdown; in.knobs.dmedian_variant = c.k.dmedian;
    in.knobs.blur_pyr = c.k.blur_pyr != 0; in.knobs.blur_pyr_interleave = c.k.blur_pyr == 2 ? 1 : c.k.blur_pyr == 3 ? 2 : 0;
    in.knobs.blur_strip = c.k.blur_strip; in.knobs.cgrad_levels = c.k.cgrad_levels;
    return in;
}

inline std::string planned(const Case& c) {
    lmh::PreInputs in = inputs(c);
    lmh::PrePlan p;
    switch (c.stage) {
        case CALL: lmh::plan_preprocess(in, p); break;
        case ST_COLOR: in.M = 1; in.L = 1; lmh::plan_color_quantize(in, 0, false, p); break;
        case ST_PYRDOWN: in.M = 1; in.L = 2; lmh::plan_pyrdown(in, 1, p); break;
        case ST_DEPTH: in.M = 2; in.L = 1; lmh::plan_depth_quantize(in, p); break;
        case ST_LM: in.M = 1; in.L = 1; lmh::plan_linear_memories(in, 0, 0, 0u, p); break;
    }
    std::string out;
    // the route and the mask position say what the steps say
    if (c.stage == CALL) {
        const lmh::PreKernel k0 = p.step[0].k;
        const bool phases = k0 >= lmh::PreKernel::Phase1 && k0 <= lmh::PreKernel::Phase4_T2;
        bool fused_batch = false;
        int mask_at = -1;
        for (int i = 0; i < p.n; ++i) {
            fused_batch |= p.step[i].k >= lmh::PreKernel::Bsplit0;
            if (p.step[i].k == lmh::PreKernel::MaskRules) mask_at = i;
        }
        const lmh::PreRoute want = phases ? lmh::PreRoute::Phases : fused_batch ? lmh::PreRoute::BatchPhases : lmh::PreRoute::Separate;
        if (p.route != want) out += "ROUTE? ";
        if (p.mask_step != mask_at || (mask_at >= 0 && (!c.masked || p.step[mask_at + 1].k != lmh::PreKernel::MatchMasks)) || (c.masked && mask_at < 0)) out += "MASK STEP? ";
    }
    for (int i = 0; i < p.n; ++i) {
        const lmh::PreStep& s = p.step[i];
        const bool fused = s.k >= lmh::PreKernel::Phase1;
        out += step_text(lmh::pre_kernel_name(s.k), s.param, s.gx, s.gy, s.gz, s.lds, fused ? &s.pg : nullptr) + "; ";
    }
    return out;
}

#include "preprocess_plan_expect.inc"

}  // namespace plan_table

#ifndef PREPROCESS_PLAN_TABLE_NO_MAIN
using namespace plan_table;

int main(int argc, char** argv) {
    const bool dump = argc > 1 && !strcmp(argv[1], "--dump");
    const std::vector<Case> v = cases();
    const size_t n_expect = sizeof(EXPECT) / sizeof(EXPECT[0]);
    if (n_expect != v.size()) { printf("FAIL: %zu rows, %zu expectations\n", v.size(), n_expect); return 1; }
    int bad = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        const std::string got = planned(v[i]);
        if (dump) printf("%zu|%s|%dx%d|%d|%s\n", i, v[i].what.c_str(), v[i].w, v[i].h, v[i].n, got.c_str());
        if (got != EXPECT[i]) {
            printf("row %zu (%s, %d x %d, M %d, L %d, n %d):\n  planned  %s\n  expected %s\n", i, v[i].what.c_str(), v[i].w, v[i].h, v[i].M, v[i].L, v[i].n, got.c_str(), EXPECT[i]);
            ++bad;
        }
    }
    if (bad) { printf("FAIL: %d of %zu rows\n", bad, v.size()); return 1; }
    printf("OK %zu rows\n", v.size());
    return 0;
}
#endif
