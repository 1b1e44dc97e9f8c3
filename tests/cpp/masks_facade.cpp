// Test driver for the facade's mask overloads (HighLevelLineMOD::detectTemplate with in_masks, PoseDetection::detect with masks).
//   masks_facade match <color_only 0|1> <bgr.raw> <depth.raw> <color_mask.raw | -> <depth_mask.raw | -> <threshold>
//       run from a directory holding linemod_templates.yml.gz: readLinemod, detectTemplate(imgs, 0, masks), prints the raw match list.
//   masks_facade pose <mesh.bin> <bgr.raw> <depth.raw> <shift_x> <margin>
//       renders templates of the mesh (colour only, threshold 80), builds a PoseDetection whose principal point shifts the frame by
//       (shift_x, 0), detects once without masks, then with a mask (camera coordinates) that covers the first pose's box grown by
//       `margin` pixels, then with its complement.  Prints the first pose of the first two runs ("pose <run> ..." or "none <run>"),
//       the box, and every final pose of the complement run (up to 10 objects; the frame holds weaker detections elsewhere) and of
//       the complement displaced the way a mask translated in the wrong direction would be.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "../../line-mod-pipeline_amd/host/HighLevelLinemod.h"
#include "../../line-mod-pipeline_amd/host/PoseDetection.h"
#include "../../line-mod-pipeline_amd/host/PostProcess.h"
#include "../../line-mod-pipeline_amd/host/TemplateGenerator.h"

using namespace lmamd;

static std::vector<char> slurp(const char* p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static Image view(const void* data, int type) {
    Image im;
    im.data = data; im.width = 640; im.height = 480; im.type = type;
    return im;
}

static int run_match(int argc, char** argv) {
    if (argc < 8) return 2;
    CameraParameters cam;
    cam.fx = 1044.87f; cam.fy = 1045.69141f; cam.cx = 320; cam.cy = 240; cam.videoWidth = 640; cam.videoHeight = 480;
    TemplateGenerationSettings ts;
    ts.onlyUseColorModality = std::atoi(argv[2]) != 0;
    ts.detectorThreshold = (float)std::atof(argv[7]);
    HighLevelLineMOD line(cam, ts);
    line.readLinemod();
    std::vector<char> bgr = slurp(argv[3]), depth = slurp(argv[4]);
    std::vector<char> cm = std::strcmp(argv[5], "-") ? slurp(argv[5]) : std::vector<char>();
    std::vector<char> dm = std::strcmp(argv[6], "-") ? slurp(argv[6]) : std::vector<char>();
    if (bgr.size() != 640u * 480 * 3 || depth.size() != 640u * 480 * 2) return 3;
    if ((!cm.empty() && cm.size() != 640u * 480) || (!dm.empty() && dm.size() != 640u * 480)) return 3;
    std::vector<Image> imgs = {view(bgr.data(), 0), view(depth.data(), 1)};
    std::vector<Image> masks = {view(cm.empty() ? nullptr : cm.data(), 2), view(dm.empty() ? nullptr : dm.data(), 2)};
    bool found = line.detectTemplate(imgs, 0, masks);
    std::printf("found %d error '%s'\n", found ? 1 : 0, line.lastError().c_str());
    for (const lm_match_t& m : line.getMatches())
        std::printf("match %d %d %.9g %d %d\n", m.x, m.y, m.similarity, m.template_id, m.class_idx);
    return 0;
}

static void print_poses(const char* run, const std::vector<ObjectPose>& poses, size_t n) {
    if (poses.empty()) { std::printf("none %s\n", run); return; }
    for (size_t i = 0; i < poses.size() && i < n; ++i) {
        const ObjectPose& p = poses[i];
        std::printf("pose %s t %.4f %.4f %.4f q %.6f %.6f %.6f %.6f bb %d %d %d %d\n", run, p.translation.x, p.translation.y, p.translation.z,
                    p.quaternions.w, p.quaternions.x, p.quaternions.y, p.quaternions.z, p.boundingBox.x, p.boundingBox.y, p.boundingBox.width,
                    p.boundingBox.height);
    }
}

static int run_pose(int argc, char** argv) {
    if (argc < 7) return 2;
    std::vector<char> mb = slurp(argv[2]);
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(mb.data());
    uint32_t nv = hdr[0], nf = hdr[1];
    const float* v = reinterpret_cast<const float*>(mb.data() + 8);
    const int32_t* f = reinterpret_cast<const int32_t*>(mb.data() + 8 + (size_t)nv * 12);
    Mesh mesh;
    mesh.vertices.resize(nv);
    for (uint32_t i = 0; i < nv; ++i) mesh.vertices[i] = Vec3{v[3 * i], v[3 * i + 1], v[3 * i + 2]};
    mesh.indices.assign(f, f + (size_t)nf * 3);
    const int shift_x = std::atoi(argv[5]), margin = std::atoi(argv[6]);

    CameraParameters cam;   // linemod_settings.yml, with the principal point moved: PoseDetection translates by (w/2 - cx, h/2 - cy)
    cam.fx = 1044.87f; cam.fy = 1045.69141f; cam.cx = (float)(320 - shift_x); cam.cy = 240; cam.videoWidth = 640; cam.videoHeight = 480;
    TemplateGenerationSettings ts;
    ts.onlyUseColorModality = true;
    ts.detectorThreshold = 80.0f;
    PoseDetection pd(cam, ts);
    SoftRender render(cam);
    SymmetryProperties sym;   // models/lagergehaeuse.yml
    sym.rotationallySymmetrical = true; sym.planesOfSymmetry = Vec3{1, 1, 1};
    GeneratorSettings gs;
    gs.startDistance = 550; gs.endDistance = 700; gs.stepSize = 50; gs.subdivisions = 3;
    int n = generate_templates(*pd.lineMod(), render, mesh, "lagergehaeuse.ply", sym, gs);
    std::printf("templates %d\n", n);
    double lo[3] = {0, 0, 0}, hi[3] = {255, 150, 255};
    pd.lineMod()->setColorRange(0, lo, hi);
    pd.refreshClassIds();

    std::vector<char> bgr = slurp(argv[3]), depth = slurp(argv[4]);
    std::vector<Image> imgs = {view(bgr.data(), 0), view(depth.data(), 1)};
    std::vector<ObjectPose> out;
    pd.detect(imgs, "lagergehaeuse.ply", 1, out, true);
    const std::vector<ObjectPose> plain = pd.getFinalObjectPoses();
    print_poses("plain", plain, 1);
    if (plain.empty()) return 0;
    // the first pose's box lies in the TRANSLATED frame: camera coordinates are (x - shift_x, y)
    const Rect bb = plain[0].boundingBox;
    const int x0 = std::max(bb.x - shift_x - margin, 0), x1 = std::min(bb.x + bb.width - shift_x + margin, 640);
    const int y0 = std::max(bb.y - margin, 0), y1 = std::min(bb.y + bb.height + margin, 480);
    std::vector<uint8_t> cover(640 * 480, 0), exclude(640 * 480, 255);
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) { cover[(size_t)y * 640 + x] = 255; exclude[(size_t)y * 640 + x] = 0; }
    std::printf("box %d %d %d %d\n", x0, y0, x1, y1);
    out.clear();
    pd.detect(imgs, {view(cover.data(), 2)}, "lagergehaeuse.ply", 1, out, true);
    print_poses("cover", pd.getFinalObjectPoses(), 1);
    out.clear();
    pd.detect(imgs, {view(exclude.data(), 2)}, "lagergehaeuse.ply", 10, out, true);
    print_poses("exclude", pd.getFinalObjectPoses(), 10);
    // the sensitivity of the check above: the same complement displaced by -2 shift_x, where a mask translated the wrong way lands
    std::vector<uint8_t> misplaced(640 * 480, 255);
    for (int y = y0; y < y1; ++y)
        for (int x = std::max(x0 - 2 * shift_x, 0); x < std::min(x1 - 2 * shift_x, 640); ++x) misplaced[(size_t)y * 640 + x] = 0;
    out.clear();
    pd.detect(imgs, {view(misplaced.data(), 2)}, "lagergehaeuse.ply", 10, out, true);
    print_poses("misplaced", pd.getFinalObjectPoses(), 10);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "match")) return run_match(argc, argv);
    if (!std::strcmp(argv[1], "pose")) return run_pose(argc, argv);
    return 2;
}
