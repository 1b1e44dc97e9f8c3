// Test driver of "use icp" in PoseDetection's batch, stream and slot forms (tests/test_gpu_icp_batch_facade.py): an
// RGB-D PoseDetection with "use icp", a principal point off centre (the shift is (-12, +10)), the sorted depth statistic, templates of the
// mesh made on the GPU and the ICP model set after them.  Frames: the golden frame, a copy with the scene moved 45 mm along the optical
// axis, and a copy with the part pushed 150 mm back (every pixel the first final pose renders goes 150 mm behind it, as icp_facade.cpp
// builds it).  Prints "final <form> <frame> <k> ..." with %.9g for four forms -- detect() frame by frame, the class-list detectBatch, two
// batches in flight through Begin / End, detectBatchSlots on the frames ingested from device memory -- "groups <frame> <non-empty groups>
// <accepted>" for detect(), "run <form> <ok> '<lastError>'" and "refused <what> <refused> '<lastError>'".
//   icp_batch_facade <mesh.bin: nv nf | xyz | faces | normals> <bgr.raw> <depth.raw> <threshold> <step size>
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

static void print_final(const char* form, size_t frame, const std::vector<ObjectPose>& poses) {
    for (size_t k = 0; k < poses.size(); ++k) {
        const ObjectPose& p = poses[k];
        std::printf("final %s %zu %zu t %.9g %.9g %.9g q %.9g %.9g %.9g %.9g bb %d %d %d %d\n", form, frame, k, p.translation.x, p.translation.y,
                    p.translation.z, p.quaternions.w, p.quaternions.x, p.quaternions.y, p.quaternions.z, p.boundingBox.x, p.boundingBox.y,
                    p.boundingBox.width, p.boundingBox.height);
    }
}

int main(int argc, char** argv) {
    if (argc < 6) return 2;
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
    const int W = 640, H = 480, NF = 3;
    const uint16_t N_OBJECTS = 4;
    CameraParameters cam;   // linemod_settings.yml with the principal point moved off centre: the shift is (-12, +10)
    cam.fx = 1044.87f; cam.fy = 1045.69141f; cam.cx = 332; cam.cy = 230; cam.videoWidth = W; cam.videoHeight = H;
    const int ox = (int)(-cam.cx + W / 2), oy = (int)(-cam.cy + H / 2);
    TemplateGenerationSettings ts;
    ts.onlyUseColorModality = false;
    ts.detectorThreshold = (float)std::atof(argv[4]);
    ts.stepSize = (uint16_t)std::atoi(argv[5]);
    ts.numberWantedPoses = 2;
    ts.useIcp = true;
    ts.icpSubsamplingFactor = 2;
    ts.modelFolder = "no-such-folder/";   // the model is handed in below
    PoseDetection pd(cam, ts);
    HighLevelLineMOD& line = *pd.lineMod();
    line.setDepthStatistic(1);
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
    if (!pd.icpRefiner() || !pd.icpRefiner()->setModel(0, mesh)) { std::printf("no icp model\n"); return 3; }      // after the generator: it renders from mesh 0
    std::vector<char> bgr = slurp(argv[2]), depth0 = slurp(argv[3]);
    if (bgr.size() != (size_t)W * H * 3 || depth0.size() != (size_t)W * H * 2) return 3;
    const uint16_t* d0 = reinterpret_cast<const uint16_t*>(depth0.data());
    std::vector<std::vector<uint16_t>> depth(NF, std::vector<uint16_t>(d0, d0 + (size_t)W * H));
    for (size_t i = 0; i < (size_t)W * H; ++i) depth[1][i] = d0[i] > 1 ? (uint16_t)(d0[i] + 45) : d0[i];
    const std::string name = "lagergehaeuse.ply";
    const std::vector<std::string> names{name};
    auto images = [&](int k) {
        std::vector<Image> im(2);
        im[0].data = bgr.data(); im[0].width = W; im[0].height = H;
        im[1].data = depth[(size_t)k].data(); im[1].width = W; im[1].height = H; im[1].type = 1;
        return im;
    };
    {   // frame 2: the part pushed 150 mm back.  The pose detect() ends with on the golden frame (or, if the check rejects every group, the
        // first unrefined pose) lives in the shifted frame: render it there, move those pixels, and translate the frame back
        std::vector<Image> im = images(0);
        std::vector<ObjectPose> out;
        pd.detect(im, name, 1, out, true);
        std::vector<std::vector<ObjectPose>> groups = line.getObjectPoses();
        ObjectPose pose;
        bool have = !out.empty();
        if (have) pose = out[0];
        for (size_t g = 0; g < groups.size() && !have; ++g) if (!groups[g].empty()) { pose = groups[g][0]; have = true; }
        if (!have) { std::printf("no pose on the golden frame\n"); return 0; }
        std::vector<uint16_t> shifted, rd;
        std::vector<uint8_t> rb;
        translate_u16(d0, W, H, ox, oy, shifted);
        const Mat4 view = icp_view_matrix(pose);
        render.render_view(mesh, view.m, rb, rd);
        size_t moved = 0;
        for (size_t i = 0; i < shifted.size(); ++i) if (rd[i] > 1) { shifted[i] = (uint16_t)(rd[i] + 150); ++moved; }
        translate_u16(shifted.data(), W, H, -ox, -oy, depth[2]);
        std::printf("pushed back %zu pixels\n", moved);
    }

    // ---- form 1: detect() frame by frame
    for (int k = 0; k < NF; ++k) {
        std::vector<Image> im = images(k);
        std::vector<ObjectPose> out;
        pd.detect(im, name, N_OBJECTS, out, true);
        std::printf("run detect_%d %d '%s'\n", k, pd.lastError().empty() ? 1 : 0, pd.lastError().c_str());
        size_t groups = 0;
        for (const auto& g : line.getObjectPoses()) groups += !g.empty();
        std::printf("groups %d %zu %zu\n", k, groups, out.size());
        print_final("detect", (size_t)k, out);
    }
    // ---- form 2: the class-list detectBatch
    {
        std::vector<std::vector<Image>> fr;
        for (int k = 0; k < NF; ++k) fr.push_back(images(k));
        std::vector<std::vector<std::vector<ObjectPose>>> out;
        const bool ok = pd.detectBatch(fr, names, N_OBJECTS, out);
        std::printf("run batch %d '%s'\n", ok ? 1 : 0, pd.lastError().c_str());
        for (size_t i = 0; !out.empty() && i < out[0].size(); ++i) print_final("batch", i, out[0][i]);
    }
    // ---- form 3: two batches in flight (frames 0 .. 1 and frame 2), collected in order
    {
        std::vector<std::vector<Image>> b0{images(0), images(1)}, b1{images(2)};
        std::vector<std::vector<std::vector<ObjectPose>>> o0, o1;
        const bool g0 = pd.detectBatchBegin(b0, names), g1 = pd.detectBatchBegin(b1, names);
        const bool e0 = pd.detectBatchEnd(N_OBJECTS, o0);
        const std::string err0 = pd.lastError();
        const bool e1 = pd.detectBatchEnd(N_OBJECTS, o1);
        std::printf("run stream %d %d %d %d '%s' '%s'\n", g0 ? 1 : 0, g1 ? 1 : 0, e0 ? 1 : 0, e1 ? 1 : 0, err0.c_str(), pd.lastError().c_str());
        for (size_t i = 0; !o0.empty() && i < o0[0].size(); ++i) print_final("stream", i, o0[0][i]);
        for (size_t i = 0; !o1.empty() && i < o1[0].size(); ++i) print_final("stream", 2 + i, o1[0][i]);
    }
    // ---- form 4: the same frames in device memory, ingested into slot set 1 with the shift in the ingest's opts
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
        opts[k].flip_x = 0; opts[k].shift_x = ox; opts[k].shift_y = oy;
    }
    if (lm_ingest_frames(line.handle(), first, NF, col.data(), dep.data(), opts.data(), nullptr) != LM_OK) { std::printf("lm_ingest_frames failed: %s\n", lm_last_error()); return 1; }
    {
        std::vector<std::vector<std::vector<ObjectPose>>> out;
        const bool ok = pd.detectBatchSlots(first, NF, names, N_OBJECTS, out);
        std::printf("run slots %d '%s'\n", ok ? 1 : 0, pd.lastError().c_str());
        for (size_t i = 0; !out.empty() && i < out[0].size(); ++i) print_final("slots", i, out[0][i]);
    }
    // ---- refusals, each with its reason
    {
        std::vector<std::vector<Image>> fr{images(0)};
        std::vector<std::vector<ObjectPose>> one;
        bool r = pd.detectBatch(fr, name, 1, one);      // the single-class form runs no ICP branch
        std::printf("refused single_class %d '%s'\n", r ? 0 : 1, pd.lastError().c_str());
        std::vector<std::vector<std::vector<ObjectPose>>> out;
        line.setGpuColorCheck(false);
        r = pd.detectBatch(fr, names, 1, out);
        std::printf("refused host_colour_check_batch %d '%s'\n", r ? 0 : 1, pd.lastError().c_str());
        r = pd.detectBatchSlots(first, NF, names, 1, out);
        std::printf("refused host_colour_check_slots %d '%s'\n", r ? 0 : 1, pd.lastError().c_str());
        line.setGpuColorCheck(true);
        r = pd.detectBatchSlots(first + 6, 4, names, 1, out);
        std::printf("refused crosses_set %d '%s'\n", r ? 0 : 1, pd.lastError().c_str());
        r = pd.detectBatchSlots(first, NF, std::vector<std::string>{"no-such-class"}, 1, out);
        std::printf("refused unknown_class %d '%s'\n", r ? 0 : 1, pd.lastError().c_str());
        // ... and none of them left anything behind
        r = pd.detectBatchSlots(first, NF, names, N_OBJECTS, out);
        std::printf("run slots_again %d '%s' in_flight %d\n", r ? 1 : 0, pd.lastError().c_str(), line.batchesInFlight());
        for (size_t i = 0; !out.empty() && i < out[0].size(); ++i) print_final("slots_again", i, out[0][i]);
    }
    {   // a colour-only detector keeps no depth frame in its slots
        TemplateGenerationSettings tc = ts;
        tc.onlyUseColorModality = true;
        PoseDetection pc(cam, tc);
        std::vector<std::vector<Image>> fr{images(0)};
        std::vector<std::vector<std::vector<ObjectPose>>> out;
        bool r = pc.detectBatch(fr, names, 1, out);
        std::printf("refused colour_only_batch %d '%s'\n", r ? 0 : 1, pc.lastError().c_str());
        r = pc.detectBatchSlots(0, 1, names, 1, out);
        std::printf("refused colour_only_slots %d '%s'\n", r ? 0 : 1, pc.lastError().c_str());
    }
    lm_device_free(dev);
    return 0;
}
