// Host references of the template generator's stages for tests/test_gpu_template_gen.py:
//   gen_stages render <mesh.bin> <W> <H> <scale> <x> <y> <z> [<x> <y> <z> ...]
//     per camera position: view_proj.bin (16 floats, SoftRender::view_proj) and SoftRender::render's colour channel 0 + depth
//     (cov_<k>.raw W*H bytes, depth_<k>.raw W*H uint16), appended as view_proj_<k>.bin
//   gen_stages rotate <in8.raw> <in16.raw> <W> <H> <angle> ...: warp_rotate_u8 (one channel) / warp_rotate_u16 -> rot8_<k>.raw, rot16_<k>.raw
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../line-mod-pipeline_amd/host/TemplateGenerator.h"

using namespace lmamd;

template <typename T>
static void save(const std::string& path, const std::vector<T>& v) {
    std::ofstream o(path, std::ios::binary);
    o.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}
template <typename T>
static std::vector<T> load(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(b.size() / sizeof(T));
    std::memcpy(v.data(), b.data(), v.size() * sizeof(T));
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "render" && argc >= 9) {
        std::vector<char> mb = load<char>(argv[2]);
        const uint32_t* hdr = reinterpret_cast<const uint32_t*>(mb.data());
        const float* v = reinterpret_cast<const float*>(mb.data() + 8);
        const int32_t* fi = reinterpret_cast<const int32_t*>(mb.data() + 8 + (size_t)hdr[0] * 12);
        const int W = std::atoi(argv[3]), H = std::atoi(argv[4]);
        const float s = (float)std::atof(argv[5]);
        Mesh mesh;
        for (uint32_t i = 0; i < hdr[0]; ++i) mesh.vertices.push_back(Vec3{v[3 * i] * s, v[3 * i + 1] * s, v[3 * i + 2] * s});
        mesh.indices.assign(fi, fi + (size_t)hdr[1] * 3);
        CameraParameters cam;
        cam.fx = 1044.87f * (float)W / 640.f; cam.fy = 1045.69141f * (float)W / 640.f; cam.cx = (float)(W / 2); cam.cy = (float)(H / 2);
        cam.videoWidth = (uint16_t)W; cam.videoHeight = (uint16_t)H;
        SoftRender r(cam);
        for (int k = 0; 6 + 3 * k + 2 < argc; ++k) {
            const Vec3 c{(float)std::atof(argv[6 + 3 * k]), (float)std::atof(argv[7 + 3 * k]), (float)std::atof(argv[8 + 3 * k])};
            std::vector<float> vp(16);
            r.view_proj(c, vp.data());
            std::vector<uint8_t> bgr, cov((size_t)W * H);
            std::vector<uint16_t> depth;
            r.render(mesh, c, bgr, depth);
            for (size_t i = 0; i < cov.size(); ++i) cov[i] = bgr[3 * i];
            save("view_proj_" + std::to_string(k) + ".bin", vp);
            save("cov_" + std::to_string(k) + ".raw", cov);
            save("depth_" + std::to_string(k) + ".raw", depth);
        }
        return 0;
    }
    if (mode == "rotate" && argc >= 7) {
        const std::vector<uint8_t> a = load<uint8_t>(argv[2]);
        const std::vector<uint16_t> b = load<uint16_t>(argv[3]);
        const int W = std::atoi(argv[4]), H = std::atoi(argv[5]);
        for (int k = 0; 6 + k < argc; ++k) {
            std::vector<uint8_t> o8;
            std::vector<uint16_t> o16;
            warp_rotate_u8(a.data(), W, H, 1, (float)std::atof(argv[6 + k]), o8);
            warp_rotate_u16(b.data(), W, H, (float)std::atof(argv[6 + k]), o16);
            save("rot8_" + std::to_string(k) + ".raw", o8);
            save("rot16_" + std::to_string(k) + ".raw", o16);
        }
        return 0;
    }
    return 2;
}
