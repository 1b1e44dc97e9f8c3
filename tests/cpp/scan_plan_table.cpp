// The scan planner (lm_host.cpp plan_layout / plan_scan) against a table of its decisions: which layout a call of n frames writes for
// the scanned level, and which scan then runs over those slots.  Built with g++ together with lm_host.cpp (tests/test_scan_plan_cpu.py);
// no GPU.  The expected values are the outputs of the rules the planner replaced (lm_detector.hip's planes_wanted / scanl_rule /
// scan1_rule / pick_scanl / pick_scan1_lanes / check_scan_args) for the same inputs; LM_SCANL_R outside its range is clamped now.
// usage: scan_plan_table          prints OK and the number of rows, or the rows that differ
#include "lm_host.h"

#include <cstdio>

using namespace lmh;

namespace {

// The base detector: 300 templates of 4000 positions each on a 640 x 480 frame's level 1 (T = 8), nibble memories with planes that fit
// k_scanl's LDS image, threshold 80.
long long g_items1[65];
ScanInputs base(int form, int M) {
    for (int L = 1; L <= 64; ++L) g_items1[L] = 300LL * ((4000 + 128 * L - 31 - 1) / (128 * L - 31));
    ScanInputs in;
    in.form = form; in.M = M;
    in.nibble = in.planes = in.lds_fits = true;
    in.bank_built = in.scanl_bank = in.scanl_device = true;
    in.fpad1 = 64; in.items1_by_L = g_items1; in.items4 = 300LL * 4;
    in.frame_stride = 8u << 20; in.arena_bytes = 2u << 20;
    in.threshold = 80.0f; in.scan1_min_threshold = 50.0f;
    in.scanl_min_slots = 24; in.scanl_R = 0;
    return in;
}
const int N_LITEMS = 300 * 32;     // lane items: 32 units of 128 positions per template (r_max = 9 shares)

enum : unsigned {
    THR_BELOW = 1, THR_AT = 2, NO_BANK = 4, NO_SCANL_BANK = 8, NO_SCANL_DEVICE = 16, NO_FIT = 32, NO_FPAD1 = 64,
    STRIDE_1G = 128, STRIDE_3G = 256, R_2 = 512, R_100 = 1024,
};
const Layout RS = Layout::Responses, RP = Layout::ResponsesAndPlanes, SP = Layout::SpreadAndPlanes;
const unsigned bR = 1u << 0, bRP = 1u << 1, bSP = 1u << 2;     // layout_bit
const ScanPlan::Kind K4 = ScanPlan::Scan4, K1 = ScanPlan::Scan1, KL = ScanPlan::ScanL, KMIX = ScanPlan::Mixed, KNONE = ScanPlan::NoBitPlaneForm;

struct Row {
    const char* what;
    int form, M, n;
    unsigned change;      // the inputs that differ from the base
    Layout layout;        // plan_layout(n)
    unsigned held;        // the slots' layouts at scan time (0: `layout`, the call prepares its own slots)
    int n_litems;         // the range's lane items (-1: N_LITEMS)
    ScanPlan::Kind kind; int param;
};

const Row ROWS[] = {
    // ---- every form, one and two modalities, around the 8-frame and the scanl_min_slots (24) boundaries
    {"form 0", 0, 1, 1, 0, RS, 0, -1, K4, 0},
    {"form 0", 0, 1, 7, 0, RS, 0, -1, K4, 0},
    {"form 0", 0, 1, 8, 0, SP, 0, -1, K1, 16},
    {"form 0", 0, 1, 23, 0, SP, 0, -1, K1, 16},
    {"form 0", 0, 1, 24, 0, SP, 0, -1, KL, 5},
    {"form 0", 0, 1, 96, 0, SP, 0, -1, KL, 5},
    {"form 0", 0, 2, 1, 0, RS, 0, -1, K4, 0},
    {"form 0", 0, 2, 7, 0, RS, 0, -1, K4, 0},
    {"form 0", 0, 2, 8, 0, RS, 0, -1, K4, 0},
    {"form 0", 0, 2, 23, 0, RS, 0, -1, K4, 0},
    {"form 0", 0, 2, 24, 0, SP, 0, -1, KL, 5},
    {"form 0", 0, 2, 96, 0, SP, 0, -1, KL, 5},
    {"form 1", 1, 1, 1, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 1, 7, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 1, 8, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 1, 23, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 1, 24, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 1, 96, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 2, 1, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 2, 7, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 2, 8, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 2, 23, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 2, 24, 0, RS, 0, -1, K4, 0},
    {"form 1", 1, 2, 96, 0, RS, 0, -1, K4, 0},
    {"form 2", 2, 1, 1, 0, RP, 0, -1, K1, 32},
    {"form 2", 2, 1, 7, 0, RP, 0, -1, K1, 9},
    {"form 2", 2, 1, 8, 0, RP, 0, -1, K1, 16},
    {"form 2", 2, 1, 23, 0, RP, 0, -1, K1, 16},
    {"form 2", 2, 1, 24, 0, RP, 0, -1, K1, 16},
    {"form 2", 2, 1, 96, 0, RP, 0, -1, K1, 16},
    {"form 2", 2, 2, 1, 0, RP, 0, -1, K1, 32},
    {"form 2", 2, 2, 7, 0, RP, 0, -1, K1, 9},
    {"form 2", 2, 2, 8, 0, RP, 0, -1, K1, 16},
    {"form 2", 2, 2, 23, 0, RP, 0, -1, K1, 16},
    {"form 2", 2, 2, 24, 0, RP, 0, -1, K1, 16},
    {"form 2", 2, 2, 96, 0, RP, 0, -1, K1, 16},
    {"form 3", 3, 1, 1, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 1, 7, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 1, 8, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 1, 23, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 1, 24, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 1, 96, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 2, 1, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 2, 7, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 2, 8, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 2, 23, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 2, 24, 0, SP, 0, -1, KL, 5},
    {"form 3", 3, 2, 96, 0, SP, 0, -1, KL, 5},
    // ---- the threshold just below and at scan1_min_threshold
    {"threshold below", 0, 1, 8, THR_BELOW, RP, 0, -1, K4, 0},
    {"threshold at", 0, 1, 8, THR_AT, SP, 0, -1, K1, 16},
    {"threshold below", 0, 2, 96, THR_BELOW, RS, 0, -1, K4, 0},
    {"threshold at", 0, 2, 96, THR_AT, SP, 0, -1, KL, 5},
    {"threshold below, form 3", 3, 2, 96, THR_BELOW, SP, 0, -1, KL, 5},
    // ---- the bank not built: form 0 writes no spread byte, form 3 does whatever the bank (and its slots take k_scan1)
    {"bank not built", 0, 1, 96, NO_BANK, RP, 0, -1, K1, 16},
    {"bank not built", 0, 2, 96, NO_BANK, RS, 0, -1, K4, 0},
    {"bank not built", 3, 2, 96, NO_BANK, SP, 0, -1, K1, 16},
    // ---- k_scanl unavailable, from the bank's lists and from the device's LDS attribute: form 0 takes the k_scan1 / k_scan4 rules,
    // form 3 k_scan1
    {"no k_scanl (bank)", 0, 1, 96, NO_SCANL_BANK, SP, 0, -1, K1, 16},
    {"no k_scanl (bank)", 0, 2, 96, NO_SCANL_BANK, RS, 0, -1, K4, 0},
    {"no k_scanl (bank)", 3, 2, 96, NO_SCANL_BANK, SP, 0, -1, K1, 16},
    {"no k_scanl (device)", 0, 1, 96, NO_SCANL_DEVICE, SP, 0, -1, K1, 16},
    {"no k_scanl (device)", 0, 2, 96, NO_SCANL_DEVICE, RS, 0, -1, K4, 0},
    {"no k_scanl (device)", 3, 2, 96, NO_SCANL_DEVICE, SP, 0, -1, K1, 16},
    {"no k_scanl (device), prepared", 0, 2, 96, NO_SCANL_DEVICE, RS, bSP, -1, K1, 16},
    // ---- planes that do not fit LDS (nor, then, the bank's lists): form 3 writes responses and planes for k_scan1
    {"no LDS fit", 3, 2, 96, NO_FIT | NO_SCANL_BANK, RP, 0, -1, K1, 16},
    {"no LDS fit", 0, 2, 96, NO_FIT | NO_SCANL_BANK, RS, 0, -1, K4, 0},
    // ---- spread-byte slots prepared earlier at a higher threshold, scanned at a lower one: k_scanl without the threshold test, below
    // scanl_min_slots k_scan1 with the fewest waves whatever the rules say
    {"spread slots, lower threshold", 0, 2, 96, THR_BELOW, RS, bSP, -1, KL, 5},
    {"spread slots, lower threshold", 0, 2, 8, THR_BELOW, RS, bSP, -1, K1, 16},
    {"spread slots, lower threshold", 0, 1, 1, THR_BELOW, RS, bSP, -1, K1, 32},
    {"spread slots, form 1 now", 1, 1, 24, 0, RS, bSP, -1, K1, 16},
    {"spread slots, no lane items", 3, 2, 96, 0, SP, 0, 0, K1, 16},
    {"spread slots, no bit-plane lists", 0, 2, 96, NO_FPAD1 | NO_SCANL_BANK, RS, bSP, -1, KNONE, 0},
    // ---- mixed layouts
    {"mixed: spread + planes", 0, 1, 96, 0, SP, bSP | bRP, -1, KMIX, 0},
    {"mixed: spread + responses", 0, 1, 96, 0, SP, bSP | bR, -1, KMIX, 0},
    {"planes + responses", 0, 1, 96, 0, SP, bRP | bR, -1, K4, 0},
    {"planes, threshold below", 0, 1, 96, THR_BELOW, RP, bRP, -1, K4, 0},
    // ---- the 2^31 arena limit of a wave's buffer descriptor excludes the lane counts of large groups of frames
    {"frame stride 1 GB", 2, 1, 8, STRIDE_1G, RP, 0, -1, K1, 32},
    {"frame stride 3 GB", 2, 1, 8, STRIDE_3G, RP, 0, -1, K1, 33},
    {"frame stride 1 GB", 0, 1, 96, STRIDE_1G | NO_SCANL_BANK, SP, 0, -1, K1, 32},
    // ---- LM_SCANL_R: within [1, min(32, n_w / 16)] as given, beyond it clamped
    {"LM_SCANL_R 2", 3, 2, 96, R_2, SP, 0, -1, KL, 2},
    {"LM_SCANL_R 100", 3, 2, 96, R_100, SP, 0, -1, KL, 9},
    {"LM_SCANL_R 100, small range", 3, 2, 96, R_100, SP, 0, 64 * 40, KL, 2},
};

const char* kind_name(ScanPlan::Kind k) {
    switch (k) {
        case ScanPlan::Scan4: return "k_scan4"; case ScanPlan::Scan1: return "k_scan1"; case ScanPlan::ScanL: return "k_scanl";
        case ScanPlan::Mixed: return "refused (mixed)"; default: return "refused (no bit-plane form)";
    }
}

}  // namespace

int main() {
    int bad = 0, i = 0;
    for (const Row& r : ROWS) {
        ScanInputs in = base(r.form, r.M);
        if (r.change & THR_BELOW) in.threshold = 49.99f;
        if (r.change & THR_AT) in.threshold = 50.0f;
        if (r.change & NO_BANK) in.bank_built = false;
        if (r.change & NO_SCANL_BANK) in.scanl_bank = false;
        if (r.change & NO_SCANL_DEVICE) in.scanl_device = false;
        if (r.change & NO_FIT) in.lds_fits = false;
        if (r.change & NO_FPAD1) in.fpad1 = 0;
        if (r.change & STRIDE_1G) in.frame_stride = (size_t)1 << 30;
        if (r.change & STRIDE_3G) in.frame_stride = (size_t)3 << 30;
        if (r.change & R_2) in.scanl_R = 2;
        if (r.change & R_100) in.scanl_R = 100;
        const Layout lay = plan_layout(in, r.n);
        const unsigned held = r.held ? r.held : layout_bit(lay);
        const ScanPlan p = plan_scan(in, r.n, held, r.n_litems < 0 ? N_LITEMS : r.n_litems);
        if (lay != r.layout || p.kind != r.kind || p.param != r.param) {
            printf("row %d (%s, form %d, M %d, n %d): layout %d scan %s %d, expected layout %d scan %s %d\n", i, r.what, r.form, r.M, r.n,
                   (int)lay, kind_name(p.kind), p.param, (int)r.layout, kind_name(r.kind), r.param);
            ++bad;
        }
        ++i;
    }
    if (bad) { printf("FAIL: %d of %d rows\n", bad, i); return 1; }
    printf("OK %d rows\n", i);
    return 0;
}
