// The best-pose check of the ICP branch, host against GPU (HighLevelLinemodIcp::meanDepthDifference / estimateBestMatch with SoftRender
// against meanDepthDifferencesGpu / estimateBestMatchGpu over lm_stage_icp_verify_host), test-side only.  No template bank: a detector,
// the ICP class and setModel.  Every mean is printed with %.17g, the host's first and the GPU's second, so equal strings are equal doubles.
// usage: icp_verify_facade <mesh.bin: nv nf | xyz | faces | normals> <depth.raw> <gt.txt: 9 rotation entries row-major, 3 position entries>
//        [time <n>]   (with "time": the median wall time of n host meanDepthDifference calls, after 3 untimed ones)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "../../line-mod-pipeline_amd/host/HighLevelLinemodIcp.h"

using namespace lmamd;

static std::vector<char> slurp(const char* p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static bool report(const char* name, HighLevelLinemodIcp& icp, const SoftRender& render, const uint16_t* scene, const std::vector<ObjectPose>& poses) {
    std::vector<double> gpu;
    if (!icp.meanDepthDifferencesGpu(scene, render.width, render.height, poses, render, 0, gpu)) {
        std::printf("%s: gpu call failed: %s\n", name, icp.lastError().c_str());
        return false;
    }
    for (size_t i = 0; i < poses.size(); ++i)
        std::printf("%s pose %zu: host %.17g gpu %.17g\n", name, i, icp.meanDepthDifference(scene, poses[i], render, 0), gpu[i]);
    uint16_t hb = 65535, gb = 65535;
    const bool hok = icp.estimateBestMatch(scene, poses, render, 0, hb);
    const bool gok = icp.estimateBestMatchGpu(scene, poses, render, 0, gb);
    std::printf("%s verdict: host %d best %u gpu %d best %u error '%s'\n", name, hok ? 1 : 0, (unsigned)hb, gok ? 1 : 0, (unsigned)gb,
                icp.lastError().c_str());
    return true;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
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
    lm_config cfg;
    lm_default_config(&cfg, 0, W, H);
    lm_detector* det = nullptr;
    if (lm_create(&cfg, &det) != LM_OK) { std::printf("lm_create: %s\n", lm_last_error()); return 3; }
    int rc = 0;
    {
        HighLevelLinemodIcp icp(det, 6, 0.1f, 2.5f, 8, 2, {}, "");
        SoftRender render(cam);
        if (!icp.setModel(0, mesh)) { std::printf("setModel: %s\n", icp.lastError().c_str()); lm_destroy(det); return 3; }
        std::vector<char> depth = slurp(argv[2]);
        if (depth.size() != (size_t)W * H * 2) { std::printf("bad depth file\n"); lm_destroy(det); return 2; }
        const uint16_t* in = reinterpret_cast<const uint16_t*>(depth.data());
        std::ifstream gtf(argv[3]);
        double R[9], T[3];
        for (double& r : R) gtf >> r;
        for (double& t : T) gtf >> t;
        double G[16] = {R[0], R[1], R[2], T[0], R[3], R[4], R[5], T[1], R[6], R[7], R[8], T[2], 0, 0, 0, 1};
        ObjectPose gt;
        matrix_to_pose(G, gt);

        if (argc >= 6 && std::strcmp(argv[4], "time") == 0) {
            const int n = std::atoi(argv[5]);
            std::vector<double> ms;
            double sink = 0;
            for (int i = 0; i < n + 3; ++i) {
                const auto t0 = std::chrono::steady_clock::now();
                sink += icp.meanDepthDifference(in, gt, render, 0);
                const auto t1 = std::chrono::steady_clock::now();
                if (i >= 3) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            std::printf("host meanDepthDifference median ms %.6f (n %d, mean %.17g)\n", ms.empty() ? 0.0 : ms[ms.size() / 2], n, sink / (n + 3));
        } else {
            bool ok = report("gt", icp, render, in, {gt});
            ObjectPose far = gt;
            far.translation.z += 100.f;
            ok = ok && report("displaced 100 mm", icp, render, in, {far});
            // the part removed from the depth frame: every pixel the pose renders goes 150 mm behind the part
            Mat4 view = icp_view_matrix(gt);
            std::vector<uint8_t> bgr;
            std::vector<uint16_t> rd, moved(in, in + (size_t)W * H), zeroed(in, in + (size_t)W * H);
            render.render_view(mesh, view.m, bgr, rd);
            for (size_t i = 0; i < moved.size(); ++i)
                if (rd[i] > 1) { moved[i] = (uint16_t)(rd[i] + 150); zeroed[i] = 0; }
            ok = ok && report("part removed", icp, render, moved.data(), {gt});
            // the part zeroed out: the mask is empty, the mean 0 -- the reference's rule keeps pose 0 with mean 0
            ok = ok && report("part zeroed", icp, render, zeroed.data(), {gt});
            // a group of five perturbed poses
            const float dt[5][3] = {{3, 0, 0}, {0, -2, 5}, {0, 0, 0}, {-4, 3, -6}, {0, 0, 20}};
            std::vector<ObjectPose> group(5, gt);
            for (int k = 0; k < 5; ++k) {
                group[k].translation.x += dt[k][0]; group[k].translation.y += dt[k][1]; group[k].translation.z += dt[k][2];
            }
            Quat q = group[3].quaternions;   // one of them turned a little
            q.x += 0.02f;
            const float len = std::sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
            q.w /= len; q.x /= len; q.y /= len; q.z /= len;
            group[3].quaternions = q;
            ok = ok && report("group", icp, render, in, group);
            ok = ok && report("empty group", icp, render, in, {});
            // a class without a resident mesh: the GPU form fails with the reason
            std::vector<double> means;
            const bool bad = icp.meanDepthDifferencesGpu(in, W, H, {gt}, render, 7, means);
            std::printf("no mesh: %d '%s'\n", bad ? 1 : 0, icp.lastError().c_str());
            rc = ok ? 0 : 4;
        }
    }
    lm_destroy(det);
    return rc;
}
