// Test driver for the facade's match gate (HighLevelLineMOD::setMatchGate / PoseDetection::setMatchGate): an RGB-D PoseDetection with
// templates of the mesh made on the GPU, a gate of a depth range, grow 8 and the class's colour range, and the same frame through
// detect(), detectBatch and the streamed form; then, with the gate cleared, detect() with the gate's mask built on the host (mask.raw)
// passed through the masks overload, and detect() without anything.
//   match_gate_facade <mesh.bin: nv nf | xyz | faces> <bgr.raw> <depth.raw> <mask.raw> <zmin> <zmax> <threshold> <objects>
// Prints "pose <run> <k> ..." per final pose, or "none <run>".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../line-mod-pipeline_amd/host/PoseDetection.h"

using namespace lmamd;

static std::vector<char> slurp(const char* p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void print_poses(const std::string& run, const std::vector<ObjectPose>& poses) {
    if (poses.empty()) { std::printf("none %s\n", run.c_str()); return; }
    for (size_t i = 0; i < poses.size(); ++i) {
        const ObjectPose& p = poses[i];
        std::printf("pose %s %zu t %.9g %.9g %.9g q %.9g %.9g %.9g %.9g bb %d %d %d %d\n", run.c_str(), i, p.translation.x, p.translation.y,
                    p.translation.z, p.quaternions.w, p.quaternions.x, p.quaternions.y, p.quaternions.z, p.boundingBox.x, p.boundingBox.y,
                    p.boundingBox.width, p.boundingBox.height);
    }
}

int main(int argc, char** argv) {
    if (argc < 9) return 2;
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
    const uint16_t objects = (uint16_t)std::atoi(argv[8]);
    CameraParameters cam;   // linemod_settings.yml: cx = w / 2, cy = h / 2, so camera coordinates are the detector's
    cam.fx = 1044.87f; cam.fy = 1045.69141f; cam.cx = 320; cam.cy = 240; cam.videoWidth = W; cam.videoHeight = H;
    TemplateGenerationSettings ts;
    ts.onlyUseColorModality = false;          // (a depth gate needs the depth frame on the device)
    ts.detectorThreshold = (float)std::atof(argv[7]);
    ts.modelFolder = "no-such-folder/";
    PoseDetection pd(cam, ts);
    SoftRender render(cam);
    SymmetryProperties sym;
    sym.rotationallySymmetrical = true; sym.planesOfSymmetry = Vec3{1, 1, 1};
    GeneratorSettings gs;
    gs.startDistance = 550; gs.endDistance = 700; gs.stepSize = 50; gs.subdivisions = 3;
    std::printf("templates %d\n", generate_templates_gpu(*pd.lineMod(), render, mesh, "lagergehaeuse.ply", sym, gs));
    double lo[3] = {0, 0, 0}, hi[3] = {255, 150, 255};   // models/lagergehaeuse.yml
    pd.lineMod()->setColorRange(0, lo, hi);
    pd.refreshClassIds();
    std::vector<char> bgr = slurp(argv[2]), depth = slurp(argv[3]), mask = slurp(argv[4]);
    if (bgr.size() != (size_t)W * H * 3 || depth.size() != (size_t)W * H * 2 || mask.size() != (size_t)W * H) return 3;
    std::vector<Image> imgs(2);
    imgs[0].data = bgr.data(); imgs[0].width = W; imgs[0].height = H;
    imgs[1].data = depth.data(); imgs[1].width = W; imgs[1].height = H; imgs[1].type = 1;
    const std::string cls = "lagergehaeuse.ply";
    std::vector<ObjectPose> out;

    MatchGate gate;
    gate.useDepthRange = true; gate.zmin = std::atoi(argv[5]); gate.zmax = std::atoi(argv[6]);
    gate.grow = 8;
    gate.useClassColorRange = true;
    pd.setMatchGate(gate);
    pd.detect(imgs, cls, objects, out, true);
    std::printf("error detect '%s'\n", pd.lineMod()->lastError().c_str());
    print_poses("detect", pd.getFinalObjectPoses());
    pd.detect(imgs, cls, objects, out, true);                    // (again: the slot keeps its rule, nothing is set anew)
    print_poses("detect_again", pd.getFinalObjectPoses());

    std::vector<std::vector<Image>> frames{imgs, imgs, imgs};
    std::vector<std::vector<ObjectPose>> bout;
    const bool bok = pd.detectBatch(frames, cls, objects, bout);
    std::printf("batch %d '%s'\n", bok ? 1 : 0, pd.lastError().c_str());
    for (size_t i = 0; i < bout.size(); ++i) print_poses("batch" + std::to_string(i), bout[i]);

    // streamed: two batches in flight, collected in order
    std::vector<std::string> names{cls};
    std::vector<std::vector<Image>> b0{imgs, imgs}, b1{imgs};
    std::vector<std::vector<std::vector<ObjectPose>>> s0, s1;
    const bool ok0 = pd.detectBatchBegin(b0, names), ok1 = pd.detectBatchBegin(b1, names);
    const bool e0 = pd.detectBatchEnd(objects, s0), e1 = pd.detectBatchEnd(objects, s1);
    std::printf("stream %d %d %d %d '%s'\n", ok0 ? 1 : 0, ok1 ? 1 : 0, e0 ? 1 : 0, e1 ? 1 : 0, pd.lastError().c_str());
    if (!s0.empty()) for (size_t i = 0; i < s0[0].size(); ++i) print_poses("stream0_" + std::to_string(i), s0[0][i]);
    if (!s1.empty()) for (size_t i = 0; i < s1[0].size(); ++i) print_poses("stream1_" + std::to_string(i), s1[0][i]);

    // the same mask built on the host, through the masks overload (colour and depth modality), with the gate cleared
    pd.clearMatchGate();
    std::vector<Image> masks(2);
    for (Image& m : masks) { m.data = mask.data(); m.width = W; m.height = H; m.type = 2; }
    pd.detect(imgs, masks, cls, objects, out, true);
    print_poses("masked", pd.getFinalObjectPoses());
    pd.detect(imgs, cls, objects, out, true);
    print_poses("plain", pd.getFinalObjectPoses());
    std::printf("matches plain %zu\n", pd.lineMod()->getMatches().size());

    // a gate the library refuses fails the call with the reason
    gate.grow = 17;
    pd.setMatchGate(gate);
    pd.detect(imgs, cls, objects, out, true);
    std::printf("refused '%s' poses %zu\n", pd.lineMod()->lastError().c_str(), pd.getFinalObjectPoses().size());
    return 0;
}
