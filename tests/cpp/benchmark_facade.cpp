// PoseDetection::setupBenchmark on the reference's fixture (benchmark/img0.png + depth0.png, pose0.yml), test-side only: the shipped
// 1950-template bank (made on the GPU, the same bank as hodan_pose0.cpp's), detect() without and with the benchmark, the GPU Hodan
// counts beside hodan_pose0.cpp's host counts for the same estimate, and the batch form (which does not score).
// usage: benchmark_facade <mesh.bin: nv nf | xyz | faces> <bgr.raw> <depth.raw>   (run where benchmark/pose0.yml exists)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "../../line-mod-pipeline_amd/host/PoseDetection.h"

using namespace lmamd;

static std::vector<char> slurp(const char* p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// hodan_pose0.cpp's counts: SoftRender renders of both poses (its view matrix takes pi in float; float_pi = false: in double, as
// Benchmark::calculateViewMat), then its per-pixel loop
static void host_counts(const SoftRender& render, const Mesh& mesh, const ObjectPose& gt, const ObjectPose& est, const uint16_t* in, int W,
                        int H, bool float_pi, long c[7]) {
    std::vector<uint16_t> r[2];
    const ObjectPose* p[2] = {&gt, &est};
    for (int k = 0; k < 2; ++k) {
        Mat4 view;
        if (float_pi) {
            const Vec3 e = glm_euler_angles(p[k]->quaternions);
            view = toMat4(glm_quat_from_euler(Vec3{e.x - 3.14159265358979323846f, -e.y, -e.z}));
            view.m[3][0] = p[k]->translation.x; view.m[3][1] = -p[k]->translation.y; view.m[3][2] = -p[k]->translation.z; view.m[3][3] = 1.0f;
        } else {
            view = benchmark_view_mat(*p[k]);
        }
        std::vector<uint8_t> bgr;
        render.render_view(mesh, view.m, bgr, r[k]);
    }
    const int delta = 15, tau = 20;
    for (int k = 0; k < 7; ++k) c[k] = 0;
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        const int g = r[0][i], e = r[1][i], d = in[i];
        c[0] += g > 1; c[1] += e > 1;
        const bool vg = (g > 1) && !((g > d ? g - d : 0) > delta);
        bool ve = (e > 1) && !((e > d ? e - d : 0) > delta);
        if (vg && e != 0) ve = true;
        c[2] += vg; c[3] += ve; c[4] += vg && ve; c[5] += vg || ve;
        const int ad = g > e ? g - e : e - g;
        c[6] += (vg && ve) && !(ad > tau);
    }
}

static void print_pose(const char* tag, const std::vector<ObjectPose>& v) {
    std::printf("%s %zu", tag, v.size());
    for (const ObjectPose& p : v)
        std::printf(" t %.9g %.9g %.9g q %.9g %.9g %.9g %.9g", p.translation.x, p.translation.y, p.translation.z, p.quaternions.w, p.quaternions.x,
                    p.quaternions.y, p.quaternions.z);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    std::vector<char> mb = slurp(argv[1]);
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(mb.data());
    const uint32_t nv = hdr[0], nf = hdr[1];
    const float* v = reinterpret_cast<const float*>(mb.data() + 8);
    const int32_t* fi = reinterpret_cast<const int32_t*>(mb.data() + 8 + (size_t)nv * 12);
    Mesh mesh;
    mesh.vertices.resize(nv);
    for (uint32_t i = 0; i < nv; ++i) mesh.vertices[i] = Vec3{v[3 * i], v[3 * i + 1], v[3 * i + 2]};
    mesh.indices.assign(fi, fi + (size_t)nf * 3);
    const int W = 640, H = 480;
    CameraParameters cam;   // linemod_settings.yml
    cam.fx = 1044.87f; cam.fy = 1045.69141f; cam.cx = 320; cam.cy = 240; cam.videoWidth = W; cam.videoHeight = H;
    TemplateGenerationSettings ts;   // linemod_settings.yml:20-27 as shipped
    ts.onlyUseColorModality = true;
    ts.detectorThreshold = 80.f;
    ts.modelFolder = "no-such-folder/";
    PoseDetection pd(cam, ts);
    SoftRender render(cam);
    SymmetryProperties sym;
    sym.rotationallySymmetrical = true; sym.planesOfSymmetry = Vec3{1, 1, 1};
    GeneratorSettings gs;
    std::printf("templates %d\n", generate_templates_gpu(*pd.lineMod(), render, mesh, "lagergehaeuse.ply", sym, gs));
    double lo[3] = {0, 0, 0}, hi[3] = {255, 150, 255};
    pd.lineMod()->setColorRange(0, lo, hi);
    pd.refreshClassIds();
    std::vector<char> bgr = slurp(argv[2]), depth = slurp(argv[3]);
    std::vector<Image> imgs(2);
    imgs[0].data = bgr.data(); imgs[0].width = W; imgs[0].height = H;
    imgs[1].data = depth.data(); imgs[1].width = W; imgs[1].height = H; imgs[1].type = 1;
    std::vector<ObjectPose> out;
    pd.detect(imgs, "lagergehaeuse.ply", 1, out, true);
    print_pose("without benchmark:", pd.getFinalObjectPoses());
    std::printf("benchmark before setup %d\n", pd.benchmark() ? 1 : 0);
    std::printf("setup unknown class %d\n", pd.setupBenchmark("no-such-class.ply", mesh) ? 1 : 0);
    std::printf("setup from missing file %d\n", pd.setupBenchmark("lagergehaeuse.ply") ? 1 : 0);
    std::printf("setup %d '%s'\n", pd.setupBenchmark("lagergehaeuse.ply", mesh) ? 1 : 0, pd.lastError().c_str());
    out.clear();
    pd.detect(imgs, "lagergehaeuse.ply", 1, out, true);
    print_pose("with benchmark:", pd.getFinalObjectPoses());
    Benchmark* b = pd.benchmark();
    const lm_vsd_result& r = b->lastCounts();
    std::printf("benchmark error %.9g score %g counter %d hodan %d\n", pd.lastBenchmarkError(), b->hodanScore(), b->imageCounter, b->hodanCounter);
    std::printf("gpu counts %u %u %u %u %u %u %u\n", r.rendered_gt, r.rendered_est, r.visible_gt, r.visible_est, r.intersection, r.combination,
                r.within_tau);
    if (pd.getFinalObjectPoses().empty()) return 0;
    ObjectPose gt;
    if (!b->readGroundTruthPose("benchmark/pose0.yml", gt)) { std::printf("no ground truth '%s'\n", b->lastError().c_str()); return 3; }
    const uint16_t* in = reinterpret_cast<const uint16_t*>(depth.data());   // cx = w/2, cy = h/2: the shift is zero
    const ObjectPose& est = pd.getFinalObjectPoses()[0];
    for (int fp = 0; fp < 2; ++fp) {
        long c[7];
        host_counts(render, mesh, gt, est, in, W, H, fp == 1, c);
        std::printf("%s counts %ld %ld %ld %ld %ld %ld %ld\n", fp ? "hodan_pose0" : "host", c[0], c[1], c[2], c[3], c[4], c[5], c[6]);
    }
    // do the two forms of the view matrix agree on these poses? (pi in float, as hodan_pose0.cpp, or in double, as the reference)
    int same = 1;
    const ObjectPose* both[2] = {&gt, &est};
    for (const ObjectPose* p : both) {
        const Vec3 e = glm_euler_angles(p->quaternions);
        same &= (e.x - 3.14159265358979323846f) == (float)((double)e.x - 3.14159265358979323846);
    }
    std::printf("view forms agree %d\n", same);
    // the second frame scores against pose1.yml, which does not exist: NaN and the reason
    pd.detect(imgs, "lagergehaeuse.ply", 1, out, false);
    std::printf("second frame error %g '%s' counter %d\n", pd.lastBenchmarkError(), pd.lastError().c_str(), b->imageCounter);
    // the batch form does not score
    std::vector<std::vector<Image>> frames{imgs};
    std::vector<std::vector<ObjectPose>> bout;
    const bool ok = pd.detectBatch(frames, "lagergehaeuse.ply", 1, bout);
    std::printf("batch %d counter %d\n", ok ? 1 : 0, b->imageCounter);
    return 0;
}
