// Template generation on the GPU against the host generator: one bank made with generate_templates (SoftRender + addTemplate per
// viewpoint) and one with generate_templates_gpu, in separate HighLevelLineMODs; prints every difference.
// usage: template_gen <mesh.bin> <W> <H> <color_only> <scale> <angleStart> <angleStop> <angleStep> gen <start> <end> <step> <subdiv> <rotsym> <px> <py> <pz>
//        template_gen <mesh.bin> <W> <H> <color_only> <scale> <angleStart> <angleStop> <angleStep> views <n_views> <radius>
//   gen: the two generators over radii start..end; views: the first n_views viewpoints of the subdivision-1 sphere at `radius`, as a loop
//   of addTemplate against one addTemplatesRendered.  Both write their files (writeLinemod) into ./host and ./gpu.
// Prints "templates <host> <gpu>", "diff records <n>", "host_s <s>", "gpu_s <s>", "error host '<..>' gpu '<..>'", and the
// markers "== host" / "== gpu" before each generator's output (its ERROR lines).  LM_GEN_SKIP_HOST=1: the GPU generator alone (timing).
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../line-mod-pipeline_amd/host/HighLevelLinemod.h"
#include "../../line-mod-pipeline_amd/host/PostProcess.h"
#include "../../line-mod-pipeline_amd/host/TemplateGenerator.h"

using namespace lmamd;

static int diff_banks(lm_detector* a, lm_detector* b) {
    int diffs = 0;
    const int M = lm_num_modalities(a), L = lm_pyramid_levels(a);
    if (lm_num_classes(a) != lm_num_classes(b)) return 1;
    std::vector<lm_feature> fa(4096), fb(4096);
    for (int c = 0; c < lm_num_classes(a); ++c) {
        if (std::strcmp(lm_class_id(a, c), lm_class_id(b, c)) || lm_class_num_templates(a, c) != lm_class_num_templates(b, c)) { ++diffs; continue; }
        for (int t = 0; t < lm_class_num_templates(a, c); ++t)
            for (int l = 0; l < L; ++l)
                for (int m = 0; m < M; ++m) {
                    int wa, ha, na, wb, hb, nb;
                    lm_get_template(a, c, t, l, m, &wa, &ha, fa.data(), &na);
                    lm_get_template(b, c, t, l, m, &wb, &hb, fb.data(), &nb);
                    if (wa != wb || ha != hb || na != nb || std::memcmp(fa.data(), fb.data(), sizeof(lm_feature) * (size_t)na)) {
                        if (diffs < 5) std::printf("record differs: template %d level %d modality %d\n", t, l, m);
                        ++diffs;
                    }
                }
    }
    return diffs;
}

int main(int argc, char** argv) {
    if (argc < 11) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> mb((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(mb.data());
    const uint32_t nv = hdr[0], nf = hdr[1];
    const float* v = reinterpret_cast<const float*>(mb.data() + 8);
    const int32_t* fi = reinterpret_cast<const int32_t*>(mb.data() + 8 + (size_t)nv * 12);
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    const bool color_only = std::atoi(argv[4]) != 0;
    float sc[3] = {1, 1, 1};
    std::sscanf(argv[5], "%f,%f,%f", &sc[0], &sc[1], &sc[2]);
    Mesh mesh;
    mesh.vertices.resize(nv);
    for (uint32_t i = 0; i < nv; ++i) mesh.vertices[i] = Vec3{v[3 * i] * sc[0], v[3 * i + 1] * sc[1], v[3 * i + 2] * sc[2]};
    mesh.indices.assign(fi, fi + (size_t)nf * 3);
    CameraParameters cam;   // the shipped camera, scaled with the frame; templates are rendered with the principal point centred
    cam.fx = 1044.87f * (float)W / 640.f; cam.fy = 1045.69141f * (float)W / 640.f; cam.cx = (float)(W / 2); cam.cy = (float)(H / 2);
    cam.videoWidth = (uint16_t)W; cam.videoHeight = (uint16_t)H;
    TemplateGenerationSettings ts;
    ts.onlyUseColorModality = color_only;
    ts.angleStart = (int16_t)std::atoi(argv[6]); ts.angleStop = (int16_t)std::atoi(argv[7]); ts.angleStep = (int16_t)std::atoi(argv[8]);
    const std::string mode = argv[9];
    SoftRender render(cam);
    HighLevelLineMOD host(cam, ts), gpu(cam, ts);
    const char* name = "lagergehaeuse.ply";
    int nh = 0, ng = 0;
    double th = 0, tg = 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    if (mode == "gen" && argc >= 18) {
        GeneratorSettings gs;
        gs.startDistance = (uint16_t)std::atoi(argv[10]); gs.endDistance = (uint16_t)std::atoi(argv[11]); gs.stepSize = (uint16_t)std::atoi(argv[12]);
        gs.subdivisions = (uint8_t)std::atoi(argv[13]);
        SymmetryProperties sym;
        sym.rotationallySymmetrical = std::atoi(argv[14]) != 0;
        sym.planesOfSymmetry = Vec3{(float)std::atof(argv[15]), (float)std::atof(argv[16]), (float)std::atof(argv[17])};
        const char* skip = std::getenv("LM_GEN_SKIP_HOST");
        std::printf("== host\n"); std::fflush(stdout);
        auto t0 = now();
        if (!(skip && std::string(skip) == "1")) nh = generate_templates(host, render, mesh, name, sym, gs);
        th = std::chrono::duration<double>(now() - t0).count();
        std::printf("== gpu\n"); std::fflush(stdout);
        t0 = now();
        ng = generate_templates_gpu(gpu, render, mesh, name, sym, gs);
        tg = std::chrono::duration<double>(now() - t0).count();
    } else if (mode == "views" && argc >= 12) {
        CameraViewPoints cams;
        cams.createCameraViewPoints((float)std::atof(argv[11]), 1);
        std::vector<Vec3> views(cams.getVertices().begin(), cams.getVertices().begin() + std::atoi(argv[10]));
        std::vector<uint8_t> bgr;
        std::vector<uint16_t> depth;
        std::printf("== host\n"); std::fflush(stdout);
        auto t0 = now();
        for (const Vec3& c : views) {
            render.render(mesh, c, bgr, depth);
            std::vector<Image> imgs(2);
            imgs[0].data = bgr.data(); imgs[0].width = W; imgs[0].height = H; imgs[0].type = 0;
            imgs[1].data = depth.data(); imgs[1].width = W; imgs[1].height = H; imgs[1].type = 1;
            host.addTemplate(imgs, name, c);
        }
        host.pushBackTemplates();
        nh = (int)host.getNumTemplates();
        th = std::chrono::duration<double>(now() - t0).count();
        std::printf("== gpu\n"); std::fflush(stdout);
        t0 = now();
        if (!gpu.addTemplatesRendered(render, mesh, name, views)) std::printf("refused: %s\n", gpu.lastError().c_str());
        gpu.pushBackTemplates();
        ng = (int)gpu.getNumTemplates();
        tg = std::chrono::duration<double>(now() - t0).count();
    } else {
        return 2;
    }
    std::fflush(stdout);
    std::printf("== end\n");
    std::printf("templates %d %d\n", nh, ng);
    std::printf("diff records %d\n", diff_banks(host.handle(), gpu.handle()));
    std::printf("host_s %.3f\ngpu_s %.3f\n", th, tg);
    std::printf("error host '%s' gpu '%s'\n", host.lastError().c_str(), gpu.lastError().c_str());
    mkdir("host", 0755); mkdir("gpu", 0755);
    if (chdir("host") != 0) return 3;
    host.writeLinemod();
    if (chdir("../gpu") != 0) return 3;
    gpu.writeLinemod();
    return 0;
}
