// register_host.cpp -- csrc/lm_register.h on the host: lmr::project, the function k_register_scatter calls per raw depth pixel, over the
// records of a file, and lmr::build_rays.  Built by tests/test_register_cpu.py with g++ -ffp-contract=off, plain and under ASan / UBSan,
// and compared there with tests/register_reference.py.  No GPU, nothing loaded into Python.
//   register_host project IN OUT    IN: 21 floats (R row-major, t, fx, fy, cx, cy, k1, k2, p1, p2, k3), then records of 3 floats (rx, ry, t)
//                                   OUT: per record int32 dropped, float u, float v, uint32 m
//   register_host rays OUT w h fx fy cx cy k1 k2 p1 p2 k3       OUT: 2 * w * h floats
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lm_register.h"

static std::vector<unsigned char> read_all(const char* path) {
    std::vector<unsigned char> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    unsigned char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "project")) {
        const std::vector<unsigned char> in = read_all(argv[2]);
        if (in.size() < 21 * sizeof(float) || (in.size() - 21 * sizeof(float)) % (3 * sizeof(float))) { std::fprintf(stderr, "bad input size\n"); return 2; }
        float head[21];
        std::memcpy(head, in.data(), sizeof(head));
        lmr::Rig g;
        std::memcpy(g.r, head, sizeof(g.r));
        std::memcpy(g.t, head + 9, sizeof(g.t));
        g.fx = head[12]; g.fy = head[13]; g.cx = head[14]; g.cy = head[15];
        g.k1 = head[16]; g.k2 = head[17]; g.p1 = head[18]; g.p2 = head[19]; g.k3 = head[20];
        const size_t n = (in.size() - sizeof(head)) / (3 * sizeof(float));
        FILE* out = std::fopen(argv[3], "wb");
        if (!out) return 2;
        for (size_t k = 0; k < n; ++k) {
            float rec[3];
            std::memcpy(rec, in.data() + sizeof(head) + k * sizeof(rec), sizeof(rec));
            const lmr::Hit h = lmr::project(g, rec[0], rec[1], rec[2]);
            const int32_t dropped = h.dropped;
            std::fwrite(&dropped, 4, 1, out); std::fwrite(&h.u, 4, 1, out); std::fwrite(&h.v, 4, 1, out); std::fwrite(&h.m, 4, 1, out);
        }
        std::fclose(out);
        std::printf("OK %zu\n", n);
        return 0;
    }
    if (argc == 14 && !std::strcmp(argv[1], "rays")) {
        const int w = std::atoi(argv[3]), h = std::atoi(argv[4]);
        if (w <= 0 || h <= 0) return 2;
        double p[9];
        for (int k = 0; k < 9; ++k) p[k] = std::strtod(argv[5 + k], nullptr);
        std::vector<float> rays(2 * (size_t)w * (size_t)h);
        lmr::build_rays(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], w, h, rays.data());
        FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 2;
        std::fwrite(rays.data(), sizeof(float), rays.size(), out);
        std::fclose(out);
        std::printf("OK %zu\n", rays.size());
        return 0;
    }
    std::fprintf(stderr, "usage: register_host project IN OUT | register_host rays OUT w h fx fy cx cy k1 k2 p1 p2 k3\n");
    return 2;
}
