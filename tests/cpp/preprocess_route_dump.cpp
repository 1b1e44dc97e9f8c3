// What the pre-processing planner (lm_host.cpp plan_preprocess) plans for the calls of tests/preprocess_routes.py: the route and every
// launch.  Built with g++ together with lm_host.cpp (tests/test_preprocess_routes_cpu.py); no GPU.  The planner's inputs are filled as
// tests/cpp/preprocess_plan_table.cpp fills them for its rows (plan_table::Case, inputs(), planned()), with the values a detector passes:
// every buffer 16-byte aligned (the arenas are 256-byte aligned), the scanned level's ori_stride and plane stride multiples of 256.
// usage: preprocess_route_dump --kernels      every name of lmh::pre_kernel_name, one per line
//        preprocess_route_dump < rows         one row per line:
//            name w h M L T0 T1 T2 T3 n phase_max_slots batch_phases others_busy lut_onehot byte_responses
//            cblur cgrad pyrdown dmedian blur_pyr blur_strip cgrad_levels          (the LM_TUNE_* values as lm_set_tuning takes them)
//        prints   name|route|kernel param grid [+lds] [nb/g]; ...
#define PREPROCESS_PLAN_TABLE_NO_MAIN
#include "preprocess_plan_table.cpp"

#include <iostream>
#include <sstream>

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--kernels")) {
        for (int k = 0; k < (int)lmh::PreKernel::Count; ++k) printf("%s\n", lmh::pre_kernel_name((lmh::PreKernel)k));
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        plan_table::Case c;
        std::string name;
        int busy = 0, onehot = 1, bytes = 0;
        is >> name >> c.w >> c.h >> c.M >> c.L >> c.T[0] >> c.T[1] >> c.T[2] >> c.T[3] >> c.n >> c.phase_max_slots >> c.batch_phases >> busy >> onehot >> bytes
           >> c.k.cblur >> c.k.cgrad >> c.k.pyrdown >> c.k.dmedian >> c.k.blur_pyr >> c.k.blur_strip >> c.k.cgrad_levels;
        if (!is || c.L < 1 || c.L > 4 || c.M < 1 || c.M > 2 || c.n < 1) { printf("%s|BAD ROW|\n", name.c_str()); return 1; }
        c.what = name; c.others_busy = busy != 0; c.onehot = onehot != 0; c.byte_responses = bytes != 0;
        c.ori_stride = 0x100;
        lmh::PreInputs in = plan_table::inputs(c);
        lmh::PrePlan p;
        lmh::plan_preprocess(in, p);
        const char* const route = p.route == lmh::PreRoute::Phases ? "phases" : p.route == lmh::PreRoute::BatchPhases ? "batch_phases" : p.route == lmh::PreRoute::Separate ? "separate" : "stage";
        printf("%s|%s|%s\n", name.c_str(), route, plan_table::planned(c).c_str());
    }
    return 0;
}
