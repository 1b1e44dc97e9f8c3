// Test driver of PoseDetection::exportResults (tests/test_gpu_export_facade.py): the set-up of pose_slots_e2e.cpp -- an RGB-D
// PoseDetection with templates of the mesh made on the GPU, a camera whose principal point is off centre (the shift is (-12, +10)) -- on
// the golden frame and a copy moved along the optical axis, both ingested from device memory with the shift in the ingest's opts.
//   export_facade <mesh.bin: nv nf | xyz | faces> <bgr.raw> <depth.raw> <threshold> <step size> <out.raw>
// detectBatchSlots, then exportResults into two dense BGR8 images in device memory with the shift undone; prints
//   "camera fx fy w h", "final <frame> <k> t x y z r <9 rotation floats, row-major> bb x y w h" (%.9g) and "prims <n>",
// and writes the two exported images to <out.raw>.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../line-mod-pipeline_amd/host/PoseDetection.h"

using namespace lmamd;

static std::vector<char> slurp(const char* p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    std::vector<char> mb = slurp(argv[1]);
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(mb.data());
    const uint32_t nv = hdr[0], nf = hdr[1];
    const float* v = reinterpret_cast<const float*>(mb.data() + 8);
    const int32_t* fi = reinterpret_cast<const int32_t*>(mb.data() + 8 + (size_t)nv * 12);
    Mesh mesh;
    mesh.vertices.resize(nv);
    for (uint32_t i = 0; i < nv; ++i) mesh.vertices[i] = Vec3{v[3 * i], v[3 * i + 1], v[3 * i + 2]};
    mesh.indices.assign(fi, fi + (size_t)nf * 3);
    const int W = 640, H = 480, NF = 2;
    CameraParameters cam;
    cam.fx = 1044.87f; cam.fy = 1045.69141f; cam.cx = 332; cam.cy = 230; cam.videoWidth = W; cam.videoHeight = H;
    const int ox = (int)(-cam.cx + W / 2), oy = (int)(-cam.cy + H / 2);
    TemplateGenerationSettings ts;
    ts.onlyUseColorModality = false;
    ts.detectorThreshold = (float)std::atof(argv[4]);
    ts.stepSize = (uint16_t)std::atoi(argv[5]);
    ts.numberWantedPoses = 2;
    ts.modelFolder = "no-such-folder/";
    PoseDetection pd(cam, ts);
    HighLevelLineMOD& line = *pd.lineMod();
    CameraParameters rcam = cam; rcam.cx = W / 2; rcam.cy = H / 2;
    SoftRender render(rcam);
    SymmetryProperties sym;
    sym.rotationallySymmetrical = true; sym.planesOfSymmetry = Vec3{1, 1, 1};
    GeneratorSettings gs;
    gs.startDistance = 550; gs.endDistance = 700; gs.stepSize = 50; gs.subdivisions = 3;
    std::printf("templates %d\n", generate_templates_gpu(line, render, mesh, "lagergehaeuse.ply", sym, gs));
    double lo[3] = {0, 0, 0}, hi[3] = {255, 150, 255};
    line.setColorRange(0, lo, hi);
    line.setDepthStatistic(1);
    pd.refreshClassIds();
    std::vector<char> bgr = slurp(argv[2]), depth0 = slurp(argv[3]);
    if (bgr.size() != (size_t)W * H * 3 || depth0.size() != (size_t)W * H * 2) return 3;
    const int dz[NF] = {0, 45};
    const int first = HighLevelLineMOD::kBatchSlots;
    const size_t cbytes = (size_t)W * H * 3, dbytes = (size_t)W * H * 2;
    void* dev = nullptr;
    if (lm_device_alloc((2 * cbytes + dbytes) * NF, &dev) != LM_OK) { std::printf("lm_device_alloc failed: %s\n", lm_last_error()); return 1; }
    std::vector<lm_image_desc> col(NF), dep(NF), dst(NF);
    std::vector<lm_ingest_opts> opts(NF);
    std::vector<uint16_t> depth((size_t)W * H);
    for (int k = 0; k < NF; ++k) {
        for (size_t i = 0; i < (size_t)W * H; ++i) {
            const uint16_t d = reinterpret_cast<const uint16_t*>(depth0.data())[i];
            depth[i] = d > 1 ? (uint16_t)((int)d + dz[k]) : d;
        }
        char* c = static_cast<char*>(dev) + (size_t)k * (2 * cbytes + dbytes);
        if (lm_device_copy(c, bgr.data(), cbytes, 0) != LM_OK || lm_device_copy(c + cbytes, depth.data(), dbytes, 0) != LM_OK) { std::printf("lm_device_copy failed: %s\n", lm_last_error()); return 1; }
        std::memset(&col[k], 0, sizeof(lm_image_desc)); std::memset(&dep[k], 0, sizeof(lm_image_desc)); std::memset(&dst[k], 0, sizeof(lm_image_desc));
        col[k].data = c; col[k].row_stride = (int64_t)W * 3; col[k].width = W; col[k].height = H; col[k].format = LM_PIX_BGR8;
        dep[k].data = c + cbytes; dep[k].row_stride = (int64_t)W * 2; dep[k].width = W; dep[k].height = H; dep[k].format = LM_PIX_DEPTH_U16; dep[k].scale = 1.0f;
        dst[k].data = c + cbytes + dbytes; dst[k].row_stride = (int64_t)W * 3; dst[k].width = W; dst[k].height = H; dst[k].format = LM_PIX_BGR8;
        opts[k].flip_x = 0; opts[k].shift_x = ox; opts[k].shift_y = oy;
    }
    if (lm_ingest_frames(line.handle(), first, NF, col.data(), dep.data(), opts.data(), nullptr) != LM_OK) { std::printf("lm_ingest_frames failed: %s\n", lm_last_error()); return 1; }
    const std::vector<std::string> names{"lagergehaeuse.ply"};
    std::vector<std::vector<std::vector<ObjectPose>>> poses;
    const bool ok = pd.detectBatchSlots(first, NF, names, 2, poses);
    std::printf("run pd_slots %d '%s'\n", ok ? 1 : 0, pd.lastError().c_str());
    if (!ok || poses.empty()) return 1;
    std::printf("camera %.9g %.9g %d %d shift %d %d\n", cam.fx, cam.fy, W, H, ox, oy);
    for (size_t i = 0; i < poses[0].size(); ++i)
        for (size_t k = 0; k < poses[0][i].size(); ++k) {
            const ObjectPose& p = poses[0][i][k];
            double R[9];
            poseRotation(p, R);
            std::printf("final %zu %zu t %.9g %.9g %.9g r", i, k, p.translation.x, p.translation.y, p.translation.z);
            for (double e : R) std::printf(" %.9g", e);
            std::printf(" bb %d %d %d %d\n", p.boundingBox.x, p.boundingBox.y, p.boundingBox.width, p.boundingBox.height);
        }
    const bool exported = pd.exportResults(first, NF, poses[0], dst.data(), opts.data());
    std::printf("run export %d '%s'\n", exported ? 1 : 0, pd.lastError().c_str());
    std::printf("prims %zu\n", pd.lastExportPrims().size());
    if (!exported) return 1;
    std::vector<char> out(cbytes * NF);
    for (int k = 0; k < NF; ++k)
        if (lm_device_copy(out.data() + (size_t)k * cbytes, dst[k].data, cbytes, 1) != LM_OK) { std::printf("lm_device_copy failed: %s\n", lm_last_error()); return 1; }
    std::ofstream(argv[6], std::ios::binary).write(out.data(), (std::streamsize)out.size());
    // a refused call says why and leaves the facade usable
    lm_image_desc bad = dst[0];
    bad.format = LM_PIX_GRAY8;
    const bool r = pd.exportResults(first, 1, poses[0], &bad, nullptr);
    std::printf("refused gray %d '%s'\n", r ? 0 : 1, pd.lastError().c_str());
    lm_device_free(dev);
    return 0;
}
