// readSettings' "keep depth on device" and the combinations that imply it (no GPU needed): tests/test_keep_depth_cpu.py.
// usage: keep_depth_settings <linemod_settings.yml> ...     one line per file:
//   "read <ok> colourOnly <0|1> statistic <0|1> icp <0|1> key <keepDepthOnDevice> keeps <keepsDepthOnDevice(ts)>"
#include <cstdio>

#include "../../line-mod-pipeline_amd/host/HighLevelLinemod.h"

using namespace lmamd;

int main(int argc, char** argv) {
    TemplateGenerationSettings def;
    std::printf("defaults key %d keeps %d\n", def.keepDepthOnDevice ? 1 : 0, keepsDepthOnDevice(def) ? 1 : 0);
    for (int k = 1; k < argc; ++k) {
        CameraParameters cam;
        TemplateGenerationSettings ts;
        const bool ok = readSettings(argv[k], cam, ts);
        std::printf("read %d colourOnly %d statistic %d icp %d key %d keeps %d\n", ok ? 1 : 0, ts.onlyUseColorModality ? 1 : 0, ts.depthStatistic, ts.useIcp ? 1 : 0,
                    ts.keepDepthOnDevice ? 1 : 0, keepsDepthOnDevice(ts) ? 1 : 0);
    }
    // set on the struct, without the file: the field alone decides (nothing is implied: that is readSettings')
    TemplateGenerationSettings a;
    a.onlyUseColorModality = true;
    std::printf("struct plain %d", keepsDepthOnDevice(a) ? 1 : 0);
    a.keepDepthOnDevice = true;
    std::printf(" key %d", keepsDepthOnDevice(a) ? 1 : 0);
    a.keepDepthOnDevice = false; a.depthStatistic = 1;
    std::printf(" statistic %d", keepsDepthOnDevice(a) ? 1 : 0);
    a.depthStatistic = 0; a.useIcp = true;
    std::printf(" icp %d", keepsDepthOnDevice(a) ? 1 : 0);
    a.onlyUseColorModality = false; a.keepDepthOnDevice = true;
    std::printf(" rgbd %d\n", keepsDepthOnDevice(a) ? 1 : 0);
    return 0;
}
