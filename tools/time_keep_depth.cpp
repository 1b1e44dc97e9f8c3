// tools/time_keep_depth.py's driver: the shipped mode -- the reference's settings file plus `depth statistic: 1` --
// through the streamed PoseDetection::detectBatchBegin / End with pinned frames, timed per batch, in two arms over the same frames:
//   keep    readSettings turns `keep depth on device` on: the depth image goes up beside the colour image (5 bytes per pixel), the depth
//           checks read values the GPU selected
//   host    the same settings with TemplateGenerationSettings::keepDepthOnDevice cleared: the detector keeps no depth frame (3 bytes per
//           pixel go up) and every depth check takes its statistic on the host (median_mat_sorted) -- what the settings ran before the flag
// Prints one line per arm and batch: "batch <arm> <k> wall_us_per_frame <v> depth_cpu_us_per_frame <v> upload_us_per_frame <v> poses <n>"
// and "same_poses <0|1>".
// usage: time_keep_depth <settings.yml> <mesh.bin: nv nf | xyz | faces> <bgr.raw> <depth.raw> <frames per batch> <batches> <warm-up batches>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../line-mod-pipeline_amd/host/PoseDetection.h"
#include "../line-mod-pipeline_amd/host/PostProcess.h"

using namespace lmamd;
using clk = std::chrono::steady_clock;
typedef std::vector<std::vector<std::vector<ObjectPose>>> Poses;       // [class][frame][pose]

static std::vector<char> slurp(const char* p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    const int NF = std::atoi(argv[5]), NB = std::atoi(argv[6]), WARM = std::atoi(argv[7]);
    if (NF < 1 || NF > HighLevelLineMOD::kBatchSlots || NB < 1) return 2;
    std::vector<char> mb = slurp(argv[2]);
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(mb.data());
    const uint32_t nv = hdr[0], nf = hdr[1];
    const float* v = reinterpret_cast<const float*>(mb.data() + 8);
    const int32_t* fi = reinterpret_cast<const int32_t*>(mb.data() + 8 + (size_t)nv * 12);
    Mesh mesh;
    mesh.vertices.resize(nv);
    for (uint32_t i = 0; i < nv; ++i) mesh.vertices[i] = Vec3{v[3 * i], v[3 * i + 1], v[3 * i + 2]};
    mesh.indices.assign(fi, fi + (size_t)nf * 3);
    std::vector<char> bgr = slurp(argv[3]), depth0 = slurp(argv[4]);
    std::vector<std::vector<Poses>> all(2);
    for (int arm = 0; arm < 2; ++arm) {
        const char* arm_name = arm == 0 ? "keep" : "host";
        CameraParameters cam;
        TemplateGenerationSettings ts;
        if (!readSettings(argv[1], cam, ts)) { std::fprintf(stderr, "settings file not read\n"); return 3; }
        if (arm == 1) ts.keepDepthOnDevice = false;
        ts.modelFolder = "no-such-folder/";
        const int W = cam.videoWidth, H = cam.videoHeight;
        if (bgr.size() != (size_t)W * H * 3 || depth0.size() != (size_t)W * H * 2) return 3;
        PoseDetection pd(cam, ts);
        HighLevelLineMOD& line = *pd.lineMod();
        std::printf("arm %s keeps_depth %d statistic %d\n", arm_name, lm_keeps_depth(line.handle()), line.depthStatistic());
        SoftRender render(cam);
        SymmetryProperties sym;
        sym.rotationallySymmetrical = true; sym.planesOfSymmetry = Vec3{1, 1, 1};
        GeneratorSettings gs;
        gs.startDistance = 550; gs.endDistance = 700; gs.stepSize = 50; gs.subdivisions = 3;
        std::printf("templates %d\n", generate_templates_gpu(line, render, mesh, "lagergehaeuse.ply", sym, gs));
        double lo[3] = {0, 0, 0}, hi[3] = {255, 150, 255};
        line.setColorRange(0, lo, hi);
        pd.refreshClassIds();
        // pinned frames: [colour | depth] per frame, the scene of frame k moved (k % 4) * 15 mm along the optical axis
        const size_t cb = (size_t)W * H * 3, db = (size_t)W * H * 2;
        uint8_t* pin = nullptr;
        if (lm_host_alloc((cb + db) * (size_t)NF, reinterpret_cast<void**>(&pin)) != LM_OK) { std::fprintf(stderr, "lm_host_alloc: %s\n", lm_last_error()); return 1; }
        std::vector<std::vector<Image>> frames((size_t)NF, std::vector<Image>(2));
        for (int k = 0; k < NF; ++k) {
            uint8_t* c = pin + (size_t)k * (cb + db);
            uint16_t* d = reinterpret_cast<uint16_t*>(c + cb);
            std::memcpy(c, bgr.data(), cb);
            for (size_t i = 0; i < (size_t)W * H; ++i) {
                const uint16_t z = reinterpret_cast<const uint16_t*>(depth0.data())[i];
                d[i] = z > 1 ? (uint16_t)(z + (k % 4) * 15) : z;
            }
            Image& ci = frames[(size_t)k][0]; Image& di = frames[(size_t)k][1];
            ci.data = c; ci.width = W; ci.height = H; ci.pinned = true;
            di.data = d; di.width = W; di.height = H; di.type = 1; di.pinned = true;
        }
        const std::vector<std::string> names{"lagergehaeuse.ply"};
        // streamed: batch k + 1 begins before batch k ends
        Poses out;
        bool ok = pd.detectBatchBegin(frames, names);
        for (int k = 0; k < NB + WARM && ok; ++k) {
            line.resetTimes();
            PostProcessor::resetTimes();
            const clk::time_point t0 = clk::now();
            ok = pd.detectBatchBegin(frames, names) && pd.detectBatchEnd(1, out);
            const double wall = std::chrono::duration<double>(clk::now() - t0).count();
            size_t poses = 0;
            for (const auto& c : out) for (const auto& f : c) poses += f.size();
            if (k >= WARM) {
                std::printf("batch %s %d wall_us_per_frame %.3f depth_cpu_us_per_frame %.3f upload_us_per_frame %.3f poses %zu\n", arm_name, k - WARM, wall * 1e6 / NF,
                            PostProcessor::times().depth * 1e6 / NF, line.times().upload * 1e6 / NF, poses);
                all[(size_t)arm].push_back(out);
            }
        }
        if (ok) ok = pd.detectBatchEnd(1, out);
        if (!ok) { std::fprintf(stderr, "arm %s failed: %s\n", arm_name, pd.lastError().c_str()); return 1; }
        lm_host_free(pin);
    }
    bool same = all[0].size() == all[1].size();
    for (size_t k = 0; same && k < all[0].size(); ++k) {
        const Poses &a = all[0][k], &b = all[1][k];
        same = a.size() == b.size();
        for (size_t c = 0; same && c < a.size(); ++c) {
            same = a[c].size() == b[c].size();
            for (size_t i = 0; same && i < a[c].size(); ++i) {
                same = a[c][i].size() == b[c][i].size();
                for (size_t p = 0; same && p < a[c][i].size(); ++p) same = std::memcmp(&a[c][i][p], &b[c][i][p], sizeof(ObjectPose)) == 0;
            }
        }
    }
    std::printf("same_poses %d\n", same ? 1 : 0);
    return 0;
}
