// readSettings' "use icp" / "icp subsampling factor" and load_ply_ascii's per-vertex normals (no GPU needed).
// usage: icp_settings <linemod_settings.yml> <model.ply>
#include <cstdio>

#include "../../line-mod-pipeline_amd/host/HighLevelLinemod.h"
#include "../../line-mod-pipeline_amd/host/TemplateGenerator.h"

using namespace lmamd;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    CameraParameters cam;
    TemplateGenerationSettings ts;
    std::printf("defaults useIcp %d step %d\n", ts.useIcp ? 1 : 0, (int)ts.icpSubsamplingFactor);
    const bool ok = readSettings(argv[1], cam, ts);
    std::printf("read %d useIcp %d step %d\n", ok ? 1 : 0, ts.useIcp ? 1 : 0, (int)ts.icpSubsamplingFactor);
    Mesh m;
    std::string err;
    const bool pl = load_ply_ascii(argv[2], m, &err);
    std::printf("ply %d vertices %zu faces %zu normals %zu\n", pl ? 1 : 0, m.vertices.size(), m.indices.size() / 3, m.normals.size());
    for (size_t i = 0; i < m.normals.size(); ++i)
        std::printf("v %.6f %.6f %.6f n %.6f %.6f %.6f\n", m.vertices[i].x, m.vertices[i].y, m.vertices[i].z, m.normals[i].x, m.normals[i].y, m.normals[i].z);
    return 0;
}
