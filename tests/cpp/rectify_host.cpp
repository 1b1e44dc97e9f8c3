// rectify_host.cpp -- csrc/lm_rectify.h on the host: lmq::build_map and lmq::quant, and lmq::colour_pixel / lmq::depth_pixel -- the functions
// k_rectify calls per output pixel -- with a memory read that dereferences the address, over a source that ENDS where its malloc block
// ends.  Built by tests/test_rectify_cpu.py with g++ -ffp-contract=off, plain and under ASan / UBSan, and compared there with
// tests/rectify_reference.py.  No GPU, nothing loaded into Python.
//   rectify_host map OUT sw sh iw ih  fx fy cx cy k1 k2 p1 p2 k3  fx' fy' cx' cy'     OUT: 2 * iw * ih int32
//   rectify_host table IN OUT sw sh iw ih                                              IN: 2 * iw * ih floats (sx, sy)
//   rectify_host quant IN OUT n                                                        IN: doubles, OUT: int32
//   rectify_host pixels IN OUT       IN: 10 int64 (kind, swap_rb, matrix, width, height, row_stride, plane_stride, offset, nbytes, npairs), one
//                                    double (scale), nbytes source bytes, npairs * 2 int32 (qx, qy).  The source is copied to the last nbytes
//                                    of a block of offset + nbytes bytes.  OUT: per pair one uint32, B | G << 8 | R << 16 or the depth
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lm_rectify.h"

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

static int write_all(const char* path, const void* p, size_t bytes) {
    FILE* out = std::fopen(path, "wb");
    if (!out) return 2;
    std::fwrite(p, 1, bytes, out);
    std::fclose(out);
    return 0;
}

// the kernel's loads, on the host: typed reads at the address itself (a misaligned u16 / u32 read is UBSan's to report)
struct HostLd {
    lmq::u32 b8(lmq::addr_t p) const { return *reinterpret_cast<const uint8_t*>(p); }
    lmq::u32 b16(lmq::addr_t p) const { return *reinterpret_cast<const uint16_t*>(p); }
    lmq::u32 b32(lmq::addr_t p) const { return *reinterpret_cast<const uint32_t*>(p); }
};

int main(int argc, char** argv) {
    if (argc == 20 && !std::strcmp(argv[1], "map")) {
        double p[13];
        for (int k = 0; k < 13; ++k) p[k] = std::strtod(argv[7 + k], nullptr);
        const lmq::Cam s = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], std::atoi(argv[3]), std::atoi(argv[4])};
        const lmq::Cam d = {p[9], p[10], p[11], p[12], 0, 0, 0, 0, 0, std::atoi(argv[5]), std::atoi(argv[6])};
        if (s.width <= 0 || s.height <= 0 || d.width <= 0 || d.height <= 0) return 2;
        std::vector<int32_t> map(2 * (size_t)d.width * (size_t)d.height);
        lmq::build_map(s, d, nullptr, map.data());
        if (write_all(argv[2], map.data(), map.size() * 4)) return 2;
        std::printf("OK %zu\n", map.size());
        return 0;
    }
    if (argc == 8 && !std::strcmp(argv[1], "table")) {
        const std::vector<unsigned char> in = read_all(argv[2]);
        lmq::Cam s = {}, d = {};
        s.width = std::atoi(argv[4]); s.height = std::atoi(argv[5]); d.width = std::atoi(argv[6]); d.height = std::atoi(argv[7]);
        if (d.width <= 0 || d.height <= 0 || in.size() != 8 * (size_t)d.width * (size_t)d.height) { std::fprintf(stderr, "bad input size\n"); return 2; }
        std::vector<float> table(in.size() / 4);
        std::memcpy(table.data(), in.data(), in.size());
        std::vector<int32_t> map(table.size());
        lmq::build_map(s, d, table.data(), map.data());
        if (write_all(argv[3], map.data(), map.size() * 4)) return 2;
        std::printf("OK %zu\n", map.size());
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "quant")) {
        const std::vector<unsigned char> in = read_all(argv[2]);
        std::vector<double> s(in.size() / 8);
        std::memcpy(s.data(), in.data(), s.size() * 8);
        std::vector<int32_t> q(s.size());
        for (size_t k = 0; k < s.size(); ++k) q[k] = lmq::quant(s[k], std::atoi(argv[4]));
        if (write_all(argv[3], q.data(), q.size() * 4)) return 2;
        std::printf("OK %zu\n", q.size());
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "pixels")) {
        const std::vector<unsigned char> in = read_all(argv[2]);
        int64_t hd[10];
        double scale;
        if (in.size() < sizeof(hd) + 8) { std::fprintf(stderr, "bad input size\n"); return 2; }
        std::memcpy(hd, in.data(), sizeof(hd));
        std::memcpy(&scale, in.data() + sizeof(hd), 8);
        const size_t offset = (size_t)hd[7], nbytes = (size_t)hd[8], npairs = (size_t)hd[9], head = sizeof(hd) + 8;
        if (in.size() != head + nbytes + npairs * 8) { std::fprintf(stderr, "bad input size\n"); return 2; }
        unsigned char* block = static_cast<unsigned char*>(std::malloc(offset + nbytes));      // the source ends where the block ends
        if (!block) return 2;
        std::memcpy(block + offset, in.data() + head, nbytes);
        lmq::Src s;
        s.data = (lmq::addr_t)reinterpret_cast<uintptr_t>(block + offset);
        s.kind = (int)hd[0]; s.swap_rb = (int)hd[1]; s.matrix = (int)hd[2]; s.width = (int)hd[3]; s.height = (int)hd[4];
        s.row_stride = hd[5]; s.plane_stride = hd[6]; s.scale = (float)scale;
        s.dwords = s.kind == LMQ_PX4 && s.data % 4 == 0 && s.row_stride % 4 == 0;      // as the library sets it
        std::vector<int32_t> q(2 * npairs);
        std::memcpy(q.data(), in.data() + head + nbytes, npairs * 8);
        std::vector<uint32_t> out(npairs);
        const bool depth = s.kind == LMQ_U16 || s.kind == LMQ_F32;
        for (size_t k = 0; k < npairs; ++k)
            out[k] = depth ? lmq::depth_pixel(s, q[2 * k], q[2 * k + 1], HostLd()) : lmq::colour_pixel_any(s, q[2 * k], q[2 * k + 1], HostLd());
        std::free(block);
        if (write_all(argv[3], out.data(), out.size() * 4)) return 2;
        std::printf("OK %zu\n", npairs);
        return 0;
    }
    std::fprintf(stderr, "usage: rectify_host map | table | quant | pixels ...\n");
    return 2;
}
