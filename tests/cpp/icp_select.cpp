// HighLevelLinemodIcp::selectBestMatch (the selection loop of estimateBestMatch, shared by the host and the GPU check) on lists of
// means given on the command line: one list per argument, comma-separated, "-" for the empty list.  Prints "<accepted> <best index>"
// per list (the index as passed in when the list is rejected: 65535).  Needs no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../line-mod-pipeline_amd/host/HighLevelLinemodIcp.h"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        std::vector<double> means;
        if (std::strcmp(argv[a], "-") != 0) {
            const char* p = argv[a];
            while (*p) {
                char* end;
                means.push_back(std::strtod(p, &end));
                p = *end == ',' ? end + 1 : end;
            }
        }
        uint16_t best = 65535;
        const bool ok = lmamd::HighLevelLinemodIcp::selectBestMatch(means, best);
        std::printf("%d %u\n", ok ? 1 : 0, (unsigned)best);
    }
    return 0;
}
