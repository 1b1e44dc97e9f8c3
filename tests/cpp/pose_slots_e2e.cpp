// Test driver of the sorted depth statistic through the facade, and of poses from frames that never touch the host
// (tests/test_gpu_pose_slots.py): an RGB-D PoseDetection with templates of the mesh made on the GPU, the golden frame and three copies of
// it with the scene moved along the optical axis, a camera whose principal point is off centre (the shift is (-12, +10)).
//   pose_slots_e2e <mesh.bin: nv nf | xyz | faces> <bgr.raw> <depth.raw> <threshold> <step size>
// Runs, each printing "matches <run> <frame> <count> <hash>" and "pose <run> <frame> <group> <k> ..." lines:
//   mode0          detectTemplatesBatch, the reference's element (the default)
//   sorted_host    sorted statistic, the host's median_mat_sorted (setGpuDepthSelect(false))
//   sorted_gpu     sorted statistic, the GPU's selections; "selected sorted_gpu pass <n> fail <n>" = depth checks decided on a selected value
//   sorted_one     detectTemplateBatch (one class) in sorted mode
//   stream0/1      the streamed Begin / End, two batches in flight
//   slots          the same frames copied to device memory, ingested with lm_ingest_frames (the shift in its opts) into slot set 1,
//                  detectTemplatesSlots; no host depth pointer is handed to the facade
//   pd_batch / pd_slots   PoseDetection::detectBatch against detectBatchSlots ("final <run> <frame> ...")
// and the refusals of detectTemplatesSlots ("refused <what> '<lastError>'").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../line-mod-pipeline_amd/host/PoseDetection.h"
#include "../../line-mod-pipeline_amd/host/PostProcess.h"

using namespace lmamd;

static std::vector<char> slurp(const char* p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void print_pose(const char* kind, const std::string& run, size_t frame, size_t g, size_t k, const ObjectPose& p) {
    std::printf("%s %s %zu %zu %zu t %.9g %.9g %.9g q %.9g %.9g %.9g %.9g bb %d %d %d %d\n", kind, run.c_str(), frame, g, k, p.translation.x, p.translation.y,
                p.translation.z, p.quaternions.w, p.quaternions.x, p.quaternions.y, p.quaternions.z, p.boundingBox.x, p.boundingBox.y,
                p.boundingBox.width, p.boundingBox.height);
}

static void dump(const std::string& run, const std::vector<std::vector<lm_match_t>>& m, const std::vector<std::vector<std::vector<ObjectPose>>>& poses) {
    for (size_t i = 0; i < m.size(); ++i) {
        uint64_t hsh = 1469598103934665603ull;
        const unsigned char* b = reinterpret_cast<const unsigned char*>(m[i].data());
        for (size_t k = 0; k < m[i].size() * sizeof(lm_match_t); ++k) { hsh ^= b[k]; hsh *= 1099511628211ull; }
        std::printf("matches %s %zu %zu %016llx\n", run.c_str(), i, m[i].size(), (unsigned long long)hsh);
    }
    for (size_t i = 0; i < poses.size(); ++i)
        for (size_t g = 0; g < poses[i].size(); ++g)
            for (size_t k = 0; k < poses[i][g].size(); ++k) print_pose("pose", run, i, g, k, poses[i][g][k]);
}

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    std::vector<char> mb = slurp(argv[1]);
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(mb.data());
    const uint32_t nv = hdr[0], nf = hdr[1];
    const float* v = reinterpret_cast<const float*>(mb.data() + 8);
    const int32_t* fi = reinterpret_cast<const int32_t*>(mb.data() + 8 + (size_t)nv * 12);
    Mesh mesh;
    mesh.vertices.resize(nv);
    for (uint32_t i = 0; i < nv; ++i) mesh.vertices[i] = Vec3{v[3 * i], v[3 * i + 1], v[3 * i + 2]};
    mesh.indices.assign(fi, fi + (size_t)nf * 3);
    const int W = 640, H = 480, NF = 4;
    CameraParameters cam;   // linemod_settings.yml with the principal point moved off centre: the shift is (-12, +10)
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
    CameraParameters rcam = cam; rcam.cx = W / 2; rcam.cy = H / 2;        // templates are rendered with the principal point at the centre
    SoftRender render(rcam);
    SymmetryProperties sym;
    sym.rotationallySymmetrical = true; sym.planesOfSymmetry = Vec3{1, 1, 1};
    GeneratorSettings gs;
    gs.startDistance = 550; gs.endDistance = 700; gs.stepSize = 50; gs.subdivisions = 3;
    std::printf("templates %d\n", generate_templates_gpu(line, render, mesh, "lagergehaeuse.ply", sym, gs));
    double lo[3] = {0, 0, 0}, hi[3] = {255, 150, 255};   // models/lagergehaeuse.yml
    line.setColorRange(0, lo, hi);
    pd.refreshClassIds();
    std::vector<char> bgr = slurp(argv[2]), depth0 = slurp(argv[3]);
    if (bgr.size() != (size_t)W * H * 3 || depth0.size() != (size_t)W * H * 2) return 3;
    // frame k: the golden frame with every measured depth moved by dz[k] mm -- the depth checks of the copies pass and fail elsewhere
    const int dz[NF] = {0, 45, -45, 90};
    std::vector<std::vector<uint16_t>> depth(NF, std::vector<uint16_t>((size_t)W * H));
    for (int k = 0; k < NF; ++k)
        for (size_t i = 0; i < (size_t)W * H; ++i) {
            const uint16_t d = reinterpret_cast<const uint16_t*>(depth0.data())[i];
            depth[k][i] = d > 1 ? (uint16_t)((int)d + dz[k]) : d;
        }
    auto make_frames = [&](int sx, int sy) {
        std::vector<std::vector<Image>> fr(NF, std::vector<Image>(2));
        for (int k = 0; k < NF; ++k) {
            fr[k][0].data = bgr.data(); fr[k][0].width = W; fr[k][0].height = H;
            fr[k][1].data = depth[k].data(); fr[k][1].width = W; fr[k][1].height = H; fr[k][1].type = 1;
            for (Image& im : fr[k]) { im.shift_x = sx; im.shift_y = sy; }
        }
        return fr;
    };
    std::vector<std::vector<Image>> frames = make_frames(ox, oy);
    const std::vector<uint16_t> cls{0};
    std::vector<std::vector<std::vector<lm_match_t>>> m;
    std::vector<std::vector<std::vector<std::vector<ObjectPose>>>> p;
    auto batch = [&](const char* run) {
        PostProcessor::resetTimes();
        const bool ok = line.detectTemplatesBatch(frames, cls, m, p);
        std::printf("run %s %d '%s'\n", run, ok ? 1 : 0, line.lastError().c_str());
        if (!m.empty()) dump(run, m[0], p[0]);
        std::printf("selected %s pass %ld fail %ld checks %ld\n", run, PostProcessor::times().depth_selected_pass, PostProcessor::times().depth_selected_fail,
                    PostProcessor::times().depth_checks);
    };
    batch("mode0");
    line.setDepthStatistic(1);
    line.setGpuDepthSelect(false);
    batch("sorted_host");
    line.setGpuDepthSelect(true);
    batch("sorted_gpu");

    {   // the one-class form: translated copies on the host, as PoseDetection::detectBatch hands them over
        std::vector<std::vector<uint8_t>> cb(NF);
        std::vector<std::vector<uint16_t>> db(NF);
        std::vector<std::vector<Image>> fr = make_frames(0, 0);
        for (int k = 0; k < NF; ++k) {
            translate_u8c3(reinterpret_cast<const uint8_t*>(bgr.data()), W, H, ox, oy, cb[k]);
            translate_u16(depth[k].data(), W, H, ox, oy, db[k]);
            fr[k][0].data = cb[k].data(); fr[k][1].data = db[k].data();
        }
        std::vector<std::vector<lm_match_t>> m1;
        std::vector<std::vector<std::vector<ObjectPose>>> p1;
        const bool ok = line.detectTemplateBatch(fr, 0, m1, p1);
        std::printf("run sorted_one %d '%s'\n", ok ? 1 : 0, line.lastError().c_str());
        dump("sorted_one", m1, p1);
    }
    {   // streamed: two batches in flight, collected in order
        std::vector<std::vector<Image>> b0(frames.begin(), frames.begin() + 3), b1(frames.begin() + 3, frames.end());
        std::vector<std::vector<std::vector<lm_match_t>>> m0, m1;
        std::vector<std::vector<std::vector<std::vector<ObjectPose>>>> p0, p1;
        const bool g0 = line.detectTemplatesBatchBegin(b0, cls), g1 = line.detectTemplatesBatchBegin(b1, cls);
        // the two slot sets with a batch in flight refuse detectTemplatesSlots; the free one serves it (the frame an earlier run left in its first
        // slot) and leaves the batches in flight as they are
        for (int s = 0; s < HighLevelLineMOD::kBatchSets; ++s) {
            std::vector<std::vector<std::vector<lm_match_t>>> mr;
            std::vector<std::vector<std::vector<std::vector<ObjectPose>>>> pr;
            const bool served = line.detectTemplatesSlots(s * HighLevelLineMOD::kBatchSlots, 1, cls, mr, pr);
            std::printf("refused busy_set_%d %d '%s' in_flight %d\n", s, served ? 0 : 1, line.lastError().c_str(), line.batchesInFlight());
        }
        const bool e0 = line.detectTemplatesBatchEnd(m0, p0), e1 = line.detectTemplatesBatchEnd(m1, p1);
        std::printf("run stream %d %d %d %d '%s'\n", g0 ? 1 : 0, g1 ? 1 : 0, e0 ? 1 : 0, e1 ? 1 : 0, line.lastError().c_str());
        if (!m0.empty()) dump("stream0", m0[0], p0[0]);
        if (!m1.empty()) dump("stream1", m1[0], p1[0]);
    }

    // ---- the frames as a camera pipeline leaves them: in device memory, ingested into slot set 1 with the shift in the ingest's opts
    const int first = HighLevelLineMOD::kBatchSlots;
    const size_t cbytes = (size_t)W * H * 3, dbytes = (size_t)W * H * 2;
    void* dev = nullptr;
    if (lm_device_alloc((cbytes + dbytes) * NF, &dev) != LM_OK) { std::printf("lm_device_alloc failed: %s\n", lm_last_error()); return 1; }
    std::vector<lm_image_desc> col(NF), dep(NF);
    std::vector<lm_ingest_opts> opts(NF);
    for (int k = 0; k < NF; ++k) {
        char* c = static_cast<char*>(dev) + (size_t)k * (cbytes + dbytes);
        if (lm_device_copy(c, bgr.data(), cbytes, 0) != LM_OK || lm_device_copy(c + cbytes, depth[k].data(), dbytes, 0) != LM_OK) { std::printf("lm_device_copy failed: %s\n", lm_last_error()); return 1; }
        std::memset(&col[k], 0, sizeof(lm_image_desc)); std::memset(&dep[k], 0, sizeof(lm_image_desc));
        col[k].data = c; col[k].row_stride = (int64_t)W * 3; col[k].width = W; col[k].height = H; col[k].format = LM_PIX_BGR8;
        dep[k].data = c + cbytes; dep[k].row_stride = (int64_t)W * 2; dep[k].width = W; dep[k].height = H; dep[k].format = LM_PIX_DEPTH_U16; dep[k].scale = 1.0f;
        opts[k].flip_x = 0; opts[k].shift_x = ox; opts[k].shift_y = oy;
    }
    auto ingest = [&] {
        if (lm_ingest_frames(line.handle(), first, NF, col.data(), dep.data(), opts.data(), nullptr) != LM_OK) { std::printf("lm_ingest_frames failed: %s\n", lm_last_error()); return false; }
        return true;
    };
    if (!ingest()) return 1;
    {
        PostProcessor::resetTimes();
        const bool ok = line.detectTemplatesSlots(first, NF, cls, m, p);
        std::printf("run slots %d '%s'\n", ok ? 1 : 0, line.lastError().c_str());
        if (!m.empty()) dump("slots", m[0], p[0]);
        std::printf("selected slots pass %ld fail %ld checks %ld\n", PostProcessor::times().depth_selected_pass, PostProcessor::times().depth_selected_fail,
                    PostProcessor::times().depth_checks);
    }
    {   // PoseDetection on top: detectBatch (which shifts by the camera's principal point itself) against detectBatchSlots
        const std::vector<std::string> names{"lagergehaeuse.ply"};
        std::vector<std::vector<Image>> plain = make_frames(0, 0);
        std::vector<std::vector<std::vector<ObjectPose>>> a, b;
        const bool oka = pd.detectBatch(plain, names, 2, a);
        std::printf("run pd_batch %d '%s'\n", oka ? 1 : 0, pd.lastError().c_str());
        if (!ingest()) return 1;
        const bool okb = pd.detectBatchSlots(first, NF, names, 2, b);
        std::printf("run pd_slots %d '%s'\n", okb ? 1 : 0, pd.lastError().c_str());
        for (size_t i = 0; !a.empty() && i < a[0].size(); ++i) for (size_t k = 0; k < a[0][i].size(); ++k) print_pose("final", "pd_batch", i, 0, k, a[0][i][k]);
        for (size_t i = 0; !b.empty() && i < b[0].size(); ++i) for (size_t k = 0; k < b[0][i].size(); ++k) print_pose("final", "pd_slots", i, 0, k, b[0][i][k]);
    }
    // ---- refusals of detectTemplatesSlots, each with its reason
    {
        std::vector<std::vector<std::vector<lm_match_t>>> mr;
        std::vector<std::vector<std::vector<std::vector<ObjectPose>>>> pr;
        bool r = line.detectTemplatesSlots(first + 6, 4, cls, mr, pr);
        std::printf("refused crosses_set %d '%s'\n", r ? 0 : 1, line.lastError().c_str());
        r = line.detectTemplatesSlots(first, 0, cls, mr, pr);
        std::printf("refused no_frames %d '%s'\n", r ? 0 : 1, line.lastError().c_str());
        line.setDepthStatistic(0);
        r = line.detectTemplatesSlots(first, NF, cls, mr, pr);
        std::printf("refused reference_statistic %d '%s'\n", r ? 0 : 1, line.lastError().c_str());
        line.setDepthStatistic(1);
        line.setGpuColorCheck(false);
        r = line.detectTemplatesSlots(first, NF, cls, mr, pr);
        std::printf("refused host_colour_check %d '%s'\n", r ? 0 : 1, line.lastError().c_str());
        line.setGpuColorCheck(true);
        // ... and none of them left anything behind: the same call goes through again
        r = line.detectTemplatesSlots(first, NF, cls, mr, pr);
        std::printf("run slots_again %d '%s' in_flight %d\n", r ? 1 : 0, line.lastError().c_str(), line.batchesInFlight());
        if (!mr.empty()) dump("slots_again", mr[0], pr[0]);
    }
    lm_device_free(dev);
    return 0;
}
