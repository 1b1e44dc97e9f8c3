// The readers of host/Benchmark.h (readGroundTruthPose, readGroundTruthLinemodDataset, loadDepthLineModDataset) and the view matrix of
// a pose, printed for tests/test_pose_error_cpu.py to compare with numpy; no GPU is used.
// usage: benchmark_readers <pose.yml> <tra> <rot> <dpt>
#include <cstdio>

#include "../../line-mod-pipeline_amd/host/Benchmark.h"

using namespace lmamd;

static void print_pose(const char* tag, bool ok, const Benchmark& b, const ObjectPose& p) {
    if (!ok) { std::printf("%s error '%s'\n", tag, b.lastError().c_str()); return; }
    std::printf("%s q %.9g %.9g %.9g %.9g t %.9g %.9g %.9g\n", tag, p.quaternions.w, p.quaternions.x, p.quaternions.y, p.quaternions.z,
                p.translation.x, p.translation.y, p.translation.z);
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    CameraParameters cam;
    cam.fx = 1044.87f; cam.fy = 1045.69141f; cam.cx = 320; cam.cy = 240; cam.videoWidth = 640; cam.videoHeight = 480;
    Benchmark b(nullptr, cam);
    ObjectPose p;
    bool ok = b.readGroundTruthPose(argv[1], p);
    print_pose("pose", ok, b, p);
    if (ok) {
        float vp[16];
        b.viewProj(p, vp);
        std::printf("viewproj");
        for (float v : vp) std::printf(" %.9g", v);
        std::printf("\n");
    }
    print_pose("linemod", b.readGroundTruthLinemodDataset(argv[2], argv[3], p), b, p);
    std::vector<uint16_t> d;
    int rows = 0, cols = 0;
    if (b.loadDepthLineModDataset(argv[4], d, rows, cols)) {
        unsigned long long sum = 0;
        for (uint16_t v : d) sum += v;
        std::printf("dpt %d %d %llu %u %u\n", rows, cols, sum, d.empty() ? 0u : d.front(), d.empty() ? 0u : d.back());
    } else {
        std::printf("dpt error '%s'\n", b.lastError().c_str());
    }
    print_pose("missing pose", b.readGroundTruthPose("no_such_dir/pose0.yml", p), b, p);
    print_pose("missing tra", b.readGroundTruthLinemodDataset("no_such_dir/tra0.tra", argv[3], p), b, p);
    print_pose("missing rot", b.readGroundTruthLinemodDataset(argv[2], "no_such_dir/rot0.rot", p), b, p);
    std::printf("missing dpt %d '%s'\n", b.loadDepthLineModDataset("no_such_dir/depth0.dpt", d, rows, cols) ? 1 : 0, b.lastError().c_str());
    return 0;
}
