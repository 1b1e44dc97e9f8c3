// Test driver of the shipped mode through the facade (tests/test_gpu_keep_depth_facade.py): the reference's own settings
// file -- `only use color modality: 1`, `use depth improvement: 1`, threshold 80 -- plus `depth statistic: 1` (and, second mode, `use icp: 1`),
// read with readSettings, which turns `keep depth on device` on.  Templates of the mesh are made on the GPU; the frames are the golden frame
// and three copies with the scene moved along the optical axis.
//   keep_depth_facade <settings.yml> <mesh.bin: nv nf | xyz | faces | normals> <bgr.raw> <depth.raw> <statistic | icp>
// statistic: "pose <run> <frame> <group> <k> ..." (%.9g) for
//   detect         PoseDetection::detect frame by frame (the groups of HighLevelLineMOD::getObjectPoses)
//   batch          detectTemplatesBatch; "selected batch pass <n> fail <n> checks <n>" = depth checks decided on a GPU-selected value
//   stream0/1      the streamed Begin / End, two batches in flight
//   slots_up       detectTemplatesSlots on frames put into slot set 1 with lm_upload_frame
//   slots_in       ... and ingested there from device memory with lm_ingest_frames
// icp: "final <run> <frame> <k> ..." for detect (frame by frame), batch (the class-list detectBatch) and slots (detectBatchSlots on ingested frames).
// Both: "settings ...", "detector modalities <n> keeps_depth <n>", "run <run> <ok> '<lastError>'".
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

static void dump_groups(const std::string& run, size_t frame, const std::vector<std::vector<ObjectPose>>& groups) {
    for (size_t g = 0; g < groups.size(); ++g)
        for (size_t k = 0; k < groups[g].size(); ++k) print_pose("pose", run, frame, g, k, groups[g][k]);
}

static void dump(const std::string& run, const std::vector<std::vector<std::vector<ObjectPose>>>& poses, size_t first = 0) {
    for (size_t i = 0; i < poses.size(); ++i) dump_groups(run, first + i, poses[i]);
}

static void dump_matches(const std::string& run, size_t frame, const std::vector<lm_match_t>& m) {
    uint64_t hsh = 1469598103934665603ull;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(m.data());
    for (size_t k = 0; k < m.size() * sizeof(lm_match_t); ++k) { hsh ^= b[k]; hsh *= 1099511628211ull; }
    std::printf("matches %s %zu %zu %016llx\n", run.c_str(), frame, m.size(), (unsigned long long)hsh);
}

static void dump_final(const std::string& run, size_t frame, const std::vector<ObjectPose>& poses) {
    for (size_t k = 0; k < poses.size(); ++k) print_pose("final", run, frame, 0, k, poses[k]);
}

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const bool icp_mode = std::string(argv[5]) == "icp";
    CameraParameters cam;
    TemplateGenerationSettings ts;
    if (!readSettings(argv[1], cam, ts)) { std::printf("settings file not read\n"); return 3; }
    std::printf("settings colourOnly %d depthImprovement %d threshold %g statistic %d icp %d keep %d\n", ts.onlyUseColorModality ? 1 : 0, ts.useDepthImprovement ? 1 : 0,
                (double)ts.detectorThreshold, ts.depthStatistic, ts.useIcp ? 1 : 0, ts.keepDepthOnDevice ? 1 : 0);
    ts.modelFolder = "no-such-folder/";      // the model is handed in below
    std::vector<char> mb = slurp(argv[2]);
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
    const int W = cam.videoWidth, H = cam.videoHeight, NF = 4;
    const int ox = (int)(-cam.cx + W / 2), oy = (int)(-cam.cy + H / 2);      // (the file's principal point is the centre: no shift)
    PoseDetection pd(cam, ts);
    HighLevelLineMOD& line = *pd.lineMod();
    std::printf("detector modalities %d keeps_depth %d facade %d\n", lm_num_modalities(line.handle()), lm_keeps_depth(line.handle()), line.keepsDepthOnDevice() ? 1 : 0);
    SoftRender render(cam);
    SymmetryProperties sym;
    sym.rotationallySymmetrical = true; sym.planesOfSymmetry = Vec3{1, 1, 1};
    GeneratorSettings gs;
    gs.startDistance = 550; gs.endDistance = 700; gs.stepSize = 50; gs.subdivisions = 3;
    std::printf("templates %d\n", generate_templates_gpu(line, render, mesh, "lagergehaeuse.ply", sym, gs));
    double lo[3] = {0, 0, 0}, hi[3] = {255, 150, 255};   // models/lagergehaeuse.yml
    line.setColorRange(0, lo, hi);
    pd.refreshClassIds();
    if (icp_mode && (!pd.icpRefiner() || !pd.icpRefiner()->setModel(0, mesh))) { std::printf("no icp model\n"); return 3; }
    std::vector<char> bgr = slurp(argv[3]), depth0 = slurp(argv[4]);
    if (bgr.size() != (size_t)W * H * 3 || depth0.size() != (size_t)W * H * 2) return 3;
    // frame k: the golden frame with every measured depth moved by dz[k] mm -- the depth checks of the copies pass and fail elsewhere
    const int dz[NF] = {0, 45, -45, 90};
    std::vector<std::vector<uint16_t>> depth(NF, std::vector<uint16_t>((size_t)W * H));
    for (int k = 0; k < NF; ++k)
        for (size_t i = 0; i < (size_t)W * H; ++i) {
            const uint16_t d = reinterpret_cast<const uint16_t*>(depth0.data())[i];
            depth[k][i] = d > 1 ? (uint16_t)((int)d + dz[k]) : d;
        }
    auto images = [&](int k) {
        std::vector<Image> im(2);
        im[0].data = bgr.data(); im[0].width = W; im[0].height = H;
        im[1].data = depth[(size_t)k].data(); im[1].width = W; im[1].height = H; im[1].type = 1;
        return im;
    };
    const std::string name = "lagergehaeuse.ply";
    const std::vector<std::string> names{name};
    const std::vector<uint16_t> cls{0};
    const uint16_t N_OBJECTS = 4;
    const int first = HighLevelLineMOD::kBatchSlots;
    const size_t cbytes = (size_t)W * H * 3, dbytes = (size_t)W * H * 2;
    void* dev = nullptr;
    if (lm_device_alloc((cbytes + dbytes) * NF, &dev) != LM_OK) { std::printf("lm_device_alloc failed: %s\n", lm_last_error()); return 1; }
    std::vector<lm_image_desc> col(NF), dep(NF);
    std::vector<lm_ingest_opts> opts(NF);
    for (int k = 0; k < NF; ++k) {
        char* c = static_cast<char*>(dev) + (size_t)k * (cbytes + dbytes);
        if (lm_device_copy(c, bgr.data(), cbytes, 0) != LM_OK || lm_device_copy(c + cbytes, depth[(size_t)k].data(), dbytes, 0) != LM_OK) { std::printf("lm_device_copy failed: %s\n", lm_last_error()); return 1; }
        std::memset(&col[k], 0, sizeof(lm_image_desc)); std::memset(&dep[k], 0, sizeof(lm_image_desc));
        col[k].data = c; col[k].row_stride = (int64_t)W * 3; col[k].width = W; col[k].height = H; col[k].format = LM_PIX_BGR8;
        dep[k].data = c + cbytes; dep[k].row_stride = (int64_t)W * 2; dep[k].width = W; dep[k].height = H; dep[k].format = LM_PIX_DEPTH_U16; dep[k].scale = 1.0f;
        std::memset(&opts[k], 0, sizeof(lm_ingest_opts));
        opts[k].shift_x = ox; opts[k].shift_y = oy;
    }
    auto ingest = [&] {
        if (lm_ingest_frames(line.handle(), first, NF, col.data(), dep.data(), opts.data(), nullptr) != LM_OK) { std::printf("lm_ingest_frames failed: %s\n", lm_last_error()); return false; }
        return true;
    };

    if (!icp_mode) {
        // ---- detect() frame by frame: the reference's call
        for (int k = 0; k < NF; ++k) {
            std::vector<Image> im = images(k);
            std::vector<ObjectPose> out;
            pd.detect(im, name, N_OBJECTS, out, true);
            std::printf("run detect_%d %d '%s'\n", k, pd.lastError().empty() ? 1 : 0, pd.lastError().c_str());
            dump_groups("detect", (size_t)k, line.getObjectPoses());
            dump_matches("detect", (size_t)k, line.getMatches());
        }
        std::vector<std::vector<Image>> frames;
        for (int k = 0; k < NF; ++k) frames.push_back(images(k));
        for (auto& fr : frames) for (Image& im : fr) { im.shift_x = ox; im.shift_y = oy; }
        std::vector<std::vector<std::vector<lm_match_t>>> m;
        std::vector<std::vector<std::vector<std::vector<ObjectPose>>>> p;
        {
            PostProcessor::resetTimes();
            const bool ok = line.detectTemplatesBatch(frames, cls, m, p);
            std::printf("run batch %d '%s'\n", ok ? 1 : 0, line.lastError().c_str());
            if (!p.empty()) dump("batch", p[0]);
            std::printf("selected batch pass %ld fail %ld checks %ld\n", PostProcessor::times().depth_selected_pass, PostProcessor::times().depth_selected_fail,
                        PostProcessor::times().depth_checks);
        }
        {   // streamed: two batches in flight, collected in order
            std::vector<std::vector<Image>> b0(frames.begin(), frames.begin() + 3), b1(frames.begin() + 3, frames.end());
            std::vector<std::vector<std::vector<lm_match_t>>> m0, m1;
            std::vector<std::vector<std::vector<std::vector<ObjectPose>>>> p0, p1;
            const bool g0 = line.detectTemplatesBatchBegin(b0, cls), g1 = line.detectTemplatesBatchBegin(b1, cls);
            const int in_flight = line.batchesInFlight();
            const bool e0 = line.detectTemplatesBatchEnd(m0, p0), e1 = line.detectTemplatesBatchEnd(m1, p1);
            std::printf("run stream %d %d %d %d in_flight %d '%s'\n", g0 ? 1 : 0, g1 ? 1 : 0, e0 ? 1 : 0, e1 ? 1 : 0, in_flight, line.lastError().c_str());
            if (!p0.empty()) dump("stream", p0[0]);
            if (!p1.empty()) dump("stream", p1[0], 3);
        }
        {   // frames the caller put into the slots: uploaded from host memory ...
            bool up = true;
            for (int k = 0; k < NF; ++k)
                up = up && lm_upload_frame_shifted(line.handle(), first + k, reinterpret_cast<const uint8_t*>(bgr.data()), 0, depth[(size_t)k].data(), 0, ox, oy) == LM_OK;
            if (!up) std::printf("lm_upload_frame_shifted failed: %s\n", lm_last_error());
            PostProcessor::resetTimes();
            const bool ok = up && line.detectTemplatesSlots(first, NF, cls, m, p);
            std::printf("run slots_up %d '%s'\n", ok ? 1 : 0, line.lastError().c_str());
            if (!p.empty()) dump("slots_up", p[0]);
            std::printf("selected slots_up pass %ld fail %ld checks %ld\n", PostProcessor::times().depth_selected_pass, PostProcessor::times().depth_selected_fail,
                        PostProcessor::times().depth_checks);
        }
        {   // ... and ingested from device memory
            const bool ok = ingest() && line.detectTemplatesSlots(first, NF, cls, m, p);
            std::printf("run slots_in %d '%s'\n", ok ? 1 : 0, line.lastError().c_str());
            if (!p.empty()) dump("slots_in", p[0]);
        }
        {   // a match gate with a depth range: served from the kept depth frame, on the colour modality.  Frame 0 (the part at its own distance)
            // and frame 3 (the scene 90 mm further away: most of it leaves the range), through detect() and through the batch form
            MatchGate gate;
            gate.useDepthRange = true; gate.zmin = 600; gate.zmax = 700; gate.grow = 8;
            pd.setMatchGate(gate);
            for (int k : {0, 3}) {
                std::vector<Image> im = images(k);
                std::vector<ObjectPose> out;
                pd.detect(im, name, N_OBJECTS, out, true);
                std::printf("run gate_detect_%d %d '%s'\n", k, pd.lastError().empty() ? 1 : 0, pd.lastError().c_str());
                dump_matches("gate_detect", (size_t)k, line.getMatches());
                dump_groups("gate_detect", (size_t)k, line.getObjectPoses());
            }
            std::vector<std::vector<Image>> two{frames[0], frames[3]};
            const bool ok = line.detectTemplatesBatch(two, cls, m, p);
            std::printf("run gate_batch %d '%s'\n", ok ? 1 : 0, line.lastError().c_str());
            for (size_t i = 0; !m.empty() && i < m[0].size(); ++i) dump_matches("gate_batch", i == 0 ? 0 : 3, m[0][i]);
            for (size_t i = 0; !p.empty() && i < p[0].size(); ++i) dump_groups("gate_batch", i == 0 ? 0 : 3, p[0][i]);
            pd.clearMatchGate();
            // the same gate on the same settings without the frame on the device: refused by the library, as before
            TemplateGenerationSettings tn = ts;
            tn.keepDepthOnDevice = false;
            PoseDetection pn(cam, tn);
            pn.setMatchGate(gate);
            std::vector<Image> im = images(0);
            const bool found = pn.lineMod()->detectTemplate(im, 0);
            std::printf("refused gate_without_depth_frame %d '%s'\n", !found && !pn.lineMod()->lastError().empty() ? 1 : 0, pn.lineMod()->lastError().c_str());
        }
        {   // a frame that came without depth: the depth selection names the slot, and nothing stays in flight
            const bool up = lm_upload_frame(line.handle(), first + 1, reinterpret_cast<const uint8_t*>(bgr.data()), 0, nullptr, 0) == LM_OK;
            if (up) (void)line.detectTemplatesSlots(first, NF, cls, m, p);
            size_t poses = 0;
            for (const auto& fr : p.empty() ? std::vector<std::vector<std::vector<ObjectPose>>>() : p[0]) for (const auto& g : fr) poses += g.size();
            // (loud, never a silent switch of implementation: without the selected values the batch has no poses, and lastError() says why)
            std::printf("refused no_depth_in_slot %d '%s' poses %zu in_flight %d\n", up && !line.lastError().empty() ? 1 : 0, line.lastError().c_str(), poses, line.batchesInFlight());
        }
    } else {
        for (int k = 0; k < NF; ++k) {
            std::vector<Image> im = images(k);
            std::vector<ObjectPose> out;
            pd.detect(im, name, N_OBJECTS, out, true);
            std::printf("run detect_%d %d '%s'\n", k, pd.lastError().empty() ? 1 : 0, pd.lastError().c_str());
            size_t groups = 0;
            for (const auto& g : line.getObjectPoses()) groups += !g.empty();
            std::printf("groups %d %zu %zu\n", k, groups, out.size());
            dump_final("detect", (size_t)k, out);
        }
        {
            std::vector<std::vector<Image>> fr;
            for (int k = 0; k < NF; ++k) fr.push_back(images(k));
            std::vector<std::vector<std::vector<ObjectPose>>> out;
            const bool ok = pd.detectBatch(fr, names, N_OBJECTS, out);
            std::printf("run batch %d '%s'\n", ok ? 1 : 0, pd.lastError().c_str());
            for (size_t i = 0; !out.empty() && i < out[0].size(); ++i) dump_final("batch", i, out[0][i]);
        }
        {
            std::vector<std::vector<std::vector<ObjectPose>>> out;
            const bool ok = ingest() && pd.detectBatchSlots(first, NF, names, N_OBJECTS, out);
            std::printf("run slots %d '%s'\n", ok ? 1 : 0, pd.lastError().c_str());
            for (size_t i = 0; !out.empty() && i < out[0].size(); ++i) dump_final("slots", i, out[0][i]);
        }
    }
    lm_device_free(dev);
    return 0;
}
