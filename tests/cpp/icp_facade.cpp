// PoseDetection with "use icp" = 1 on the reference's fixture (benchmark/img0.png + depth0.png, pose0.yml), test-side only: the shipped
// 1950-template bank (as hodan_pose0.cpp builds it), detect() with the ICP branch (HighLevelLinemodIcp on the GPU + estimateBestMatch),
// the Hodan error of the final pose and of the unrefined one, and two frames estimateBestMatch must reject.
// usage: icp_facade <mesh.bin: nv nf | xyz | faces | normals> <bgr.raw> <depth.raw> <gt.txt: 9 rotation entries row-major, 3 position entries>
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

// Benchmark::calculateViewMat + renderDepthToFrontBuff, as hodan_pose0.cpp
static void render_pose(const SoftRender& render, const Mesh& mesh, const ObjectPose& p, std::vector<uint16_t>& depth) {
    float e[3];
    icp_euler_angles(p.quaternions, e);
    const float f[3] = {e[0] - 3.14159265358979323846f, -e[1], -e[2]};
    Mat4 view = toMat4(icp_quat_from_euler(f));
    view.m[3][0] = p.translation.x; view.m[3][1] = -p.translation.y; view.m[3][2] = -p.translation.z; view.m[3][3] = 1.0f;
    std::vector<uint8_t> bgr;
    render.render_view(mesh, view.m, bgr, depth);
}

// Benchmark.cpp:18-38,133-169 (delta 15 mm, tau 20 mm), as hodan_pose0.cpp
static double hodan(const SoftRender& render, const Mesh& mesh, const ObjectPose& gt, const ObjectPose& est, const uint16_t* in, int W, int H) {
    std::vector<uint16_t> dg, de;
    render_pose(render, mesh, gt, dg);
    render_pose(render, mesh, est, de);
    const int delta = 15, tau = 20;
    long uni = 0, good = 0;
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        const int g = dg[i], e = de[i], d = in[i];
        const bool vg = (g > 1) && !((g > d ? g - d : 0) > delta);
        bool ve = (e > 1) && !((e > d ? e - d : 0) > delta);
        if (vg && e != 0) ve = true;
        uni += vg || ve;
        const int ad = g > e ? g - e : e - g;
        good += (vg && ve) && !(ad > tau);
    }
    return uni ? 1.0 - (double)good / (double)uni : 1.0;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    std::vector<char> mb = slurp(argv[1]);
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(mb.data());
    const uint32_t nv = hdr[0], nf = hdr[1];
    const float* v = reinterpret_cast<const float*>(mb.data() + 8);
    const int32_t* fi = reinterpret_cast<const int32_t*>(mb.data() + 8 + (size_t)nv * 12);
    const float* nrm = reinterpret_cast<const float*>(mb.data() + 8 + (size_t)nv * 12 + (size_t)nf * 12);
    Mesh mesh;
    mesh.vertices.resize(nv);
    mesh.normals.resize(nv);
    for (uint32_t i = 0; i < nv; ++i) {
        mesh.vertices[i] = Vec3{v[3 * i], v[3 * i + 1], v[3 * i + 2]};
        mesh.normals[i] = Vec3{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
    }
    mesh.indices.assign(fi, fi + (size_t)nf * 3);
    const int W = 640, H = 480;
    CameraParameters cam;   // linemod_settings.yml
    cam.fx = 1044.87f; cam.fy = 1045.69141f; cam.cx = 320; cam.cy = 240; cam.videoWidth = W; cam.videoHeight = H;
    TemplateGenerationSettings ts;   // linemod_settings.yml:20-37 as shipped, with "use icp: 1"
    ts.onlyUseColorModality = true;
    ts.detectorThreshold = 80.f;
    ts.useIcp = true;
    ts.icpSubsamplingFactor = 2;
    ts.modelFolder = "no-such-folder/";   // the model is handed in below (setModel) instead of read from modelFolder + class id
    PoseDetection pd(cam, ts);
    SoftRender render(cam);
    SymmetryProperties sym;
    sym.rotationallySymmetrical = true; sym.planesOfSymmetry = Vec3{1, 1, 1};
    GeneratorSettings gs;
    const int n = generate_templates(*pd.lineMod(), render, mesh, "lagergehaeuse.ply", sym, gs);
    std::printf("templates %d\n", n);
    double lo[3] = {0, 0, 0}, hi[3] = {255, 150, 255};
    pd.lineMod()->setColorRange(0, lo, hi);
    pd.refreshClassIds();
    if (!pd.icpRefiner() || !pd.icpRefiner()->setModel(0, mesh)) { std::printf("no icp model\n"); return 3; }
    std::vector<char> bgr = slurp(argv[2]), depth = slurp(argv[3]);
    std::vector<Image> imgs(2);
    imgs[0].data = bgr.data(); imgs[0].width = W; imgs[0].height = H;
    imgs[1].data = depth.data(); imgs[1].width = W; imgs[1].height = H; imgs[1].type = 1;
    std::vector<ObjectPose> out;
    pd.detect(imgs, "lagergehaeuse.ply", 1, out, true);
    std::printf("detect error '%s'\n", pd.lastError().c_str());
    std::vector<std::vector<ObjectPose>> groups = pd.lineMod()->getObjectPoses();   // the unrefined groups
    if (groups.empty() || groups[0].empty()) { std::printf("no pose\n"); return 0; }
    std::ifstream gtf(argv[4]);
    double R[9], T[3];
    for (double& r : R) gtf >> r;
    for (double& t : T) gtf >> t;
    double G[16] = {R[0], R[1], R[2], T[0], R[3], R[4], R[5], T[1], R[6], R[7], R[8], T[2], 0, 0, 0, 1};
    ObjectPose gt;
    matrix_to_pose(G, gt);
    const uint16_t* in = reinterpret_cast<const uint16_t*>(depth.data());   // cx = w/2, cy = h/2: the shift is zero
    const ObjectPose& raw = groups[0][0];
    std::printf("without icp: hodan %.6f translation error %.3f\n", hodan(render, mesh, gt, raw, in, W, H),
                std::sqrt(std::pow(raw.translation.x - T[0], 2) + std::pow(raw.translation.y - T[1], 2) + std::pow(raw.translation.z - T[2], 2)));
    std::printf("accepted %zu\n", out.size());
    if (out.empty()) return 0;
    const ObjectPose& fin = out[0];
    std::printf("with icp: hodan %.6f translation error %.3f\n", hodan(render, mesh, gt, fin, in, W, H),
                std::sqrt(std::pow(fin.translation.x - T[0], 2) + std::pow(fin.translation.y - T[1], 2) + std::pow(fin.translation.z - T[2], 2)));
    HighLevelLinemodIcp* icp = pd.icpRefiner();
    uint16_t best = 0;
    std::vector<ObjectPose> one{fin};
    std::printf("final pose mean %.3f accepted %d\n", icp->meanDepthDifference(in, fin, render, 0), icp->estimateBestMatch(in, one, render, 0, best) ? 1 : 0);
    ObjectPose far = fin;
    far.translation.z += 100.f;
    one[0] = far;
    std::printf("displaced 100 mm: mean %.3f accepted %d\n", icp->meanDepthDifference(in, far, render, 0), icp->estimateBestMatch(in, one, render, 0, best) ? 1 : 0);
    // the part removed from the depth frame: every pixel the final pose renders goes 150 mm behind the part (the table it stood on)
    std::vector<uint16_t> rd, moved(in, in + (size_t)W * H);
    render_pose(render, mesh, fin, rd);
    for (size_t i = 0; i < moved.size(); ++i) if (rd[i] > 1) moved[i] = (uint16_t)(rd[i] + 150);
    one[0] = fin;
    std::printf("part removed: mean %.3f accepted %d\n", icp->meanDepthDifference(moved.data(), fin, render, 0), icp->estimateBestMatch(moved.data(), one, render, 0, best) ? 1 : 0);
    // the part zeroed out: the mask (render > 1 and scene > 600) is empty, the mean 0 -- the reference's rule keeps pose 0 with mean 0
    std::vector<uint16_t> zeroed(in, in + (size_t)W * H);
    for (size_t i = 0; i < zeroed.size(); ++i) if (rd[i] > 1) zeroed[i] = 0;
    std::printf("part zeroed: mean %.3f accepted %d\n", icp->meanDepthDifference(zeroed.data(), fin, render, 0), icp->estimateBestMatch(zeroed.data(), one, render, 0, best) ? 1 : 0);
    // the batch form refuses with the reason
    std::vector<std::vector<Image>> frames{imgs};
    std::vector<std::vector<ObjectPose>> bout;
    const bool ok = pd.detectBatch(frames, "lagergehaeuse.ply", 1, bout);
    std::printf("batch %d '%s'\n", ok ? 1 : 0, pd.lastError().c_str());
    return 0;
}
