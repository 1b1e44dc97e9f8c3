// keep_depth_check_host.cpp -- what an lm_ingest_frames* call does with its depth descriptors (csrc/lm_ingest_check.cpp: lmc::keeps_depth,
// lmc::depth_required, lmc::check_depth_call) on the host, with no detector and no GPU.  Built by tests/test_keep_depth_cpu.py with g++,
// plain and under ASan / UBSan, and compared there with a table written out in the test.
//   keep_depth_check_host      one line per (num_modalities 1|2, flags 0|LM_FLAG_KEEP_DEPTH|other bits, registered 0|1, depth_given 0|1):
//       "M FLAGS REGISTERED GIVEN | keeps required takes | refusal"
#include <cstdio>
#include <string>

#include "lm_ingest_check.h"

int main() {
    std::printf("OK\n");
    for (int M = 1; M <= 2; ++M)
        for (int flags : {0, LM_FLAG_KEEP_DEPTH, LM_FLAG_BYTE_RESPONSES | LM_FLAG_BLOCKING_SYNC, LM_FLAG_KEEP_DEPTH | LM_FLAG_BLOCKING_SYNC})
            for (int registered = 0; registered < 2; ++registered)
                for (int given = 0; given < 2; ++given) {
                    lm_config c = lm_config();
                    c.width = 160; c.height = 80; c.num_modalities = M; c.flags = flags;
                    bool takes = true;
                    const std::string refusal = lmc::check_depth_call(c, registered != 0, given != 0, &takes);
                    std::printf("%d %d %d %d | %d %d %d | %s\n", M, flags, registered, given, lmc::keeps_depth(c) ? 1 : 0,
                                lmc::depth_required(c, registered != 0) ? 1 : 0, takes ? 1 : 0, refusal.c_str());
                }
    return 0;
}
