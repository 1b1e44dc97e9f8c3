// rectify_reduce_host.cpp -- csrc/lm_rectify_reduce.h on the host: lmy::colour_pixel (lm_rectify.h's blend of four converted taps at an
// ideal pixel's map entry, under lm_reduce.h's box), lmy::depth_nearest / lmy::depth_min_valid, with a memory read that dereferences the
// address, over a source that ENDS where its malloc block ends.  Built by tests/test_rectify_reduce_cpu.py with g++ -ffp-contract=off,
// plain and under ASan / UBSan, and compared there with the composition of tests/rectify_reference.py and tests/reduce_reference.py.
// No GPU, nothing loaded into Python.
//   rectify_reduce_host image IN OUT
//       IN: 18 int64 (kind, swap_rb, matrix, source width, source height, row_stride, plane_stride, offset, nbytes, num_x, den_x, num_y,
//       den_y, mode, pipeline, ideal width, ideal height, 0), one double (scale), with pipeline != 0: 13 int32 (black, gain[3], ccm[9])
//       and 4096 tone bytes, then the map (2 * ideal width * ideal height int32: qx, qy) and nbytes source bytes.  The source is copied
//       to the last nbytes of a block of offset + nbytes bytes, the map into a block of exactly its size.
//       mode 0: colour, 1: depth NEAREST, 2: depth MIN_VALID.
//       OUT: the whole reduced ideal image, one uint32 per pixel (B | G << 8 | R << 16, or the depth)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lm_rectify_reduce.h"

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

// the kernel's loads, on the host: typed reads at the address itself (a misaligned u16 / u32 read is UBSan's to report)
struct HostLd {
    lmy::u32 b8(lmi::addr_t p) const { return *reinterpret_cast<const uint8_t*>(p); }
    lmy::u32 b16(lmi::addr_t p) const { return *reinterpret_cast<const uint16_t*>(p); }
    lmy::u32 b32(lmi::addr_t p) const { return *reinterpret_cast<const uint32_t*>(p); }
};
struct HostTone {
    const unsigned char* t;
    lmy::u32 operator()(lmy::u32 i) const { return i < 4096u ? t[i] : (std::abort(), 0u); }
};

static int image(const char* in_path, const char* out_path) {
    const std::vector<unsigned char> in = read_all(in_path);
    int64_t hd[18];
    double scale;
    size_t head = sizeof(hd) + 8;
    if (in.size() < head) { std::fprintf(stderr, "bad input size\n"); return 2; }
    std::memcpy(hd, in.data(), sizeof(hd));
    std::memcpy(&scale, in.data() + sizeof(hd), 8);
    lmi::RawPipe pipe = lmi::RawPipe();
    std::vector<unsigned char> tone(4096, 0);
    if (hd[14]) {
        int32_t p[13];
        if (in.size() < head + sizeof(p) + 4096) { std::fprintf(stderr, "bad input size\n"); return 2; }
        std::memcpy(p, in.data() + head, sizeof(p));
        pipe.black = p[0];
        for (int k = 0; k < 3; ++k) pipe.gain[k] = (lmy::u32)p[1 + k];
        for (int k = 0; k < 9; ++k) pipe.ccm[k] = p[4 + k];
        std::memcpy(tone.data(), in.data() + head + sizeof(p), 4096);
        head += sizeof(p) + 4096;
    }
    const size_t offset = (size_t)hd[7], nbytes = (size_t)hd[8];
    const int mw = (int)hd[15], mh = (int)hd[16];
    if (mw < 1 || mh < 1) return 2;
    const size_t map_bytes = 2 * (size_t)mw * (size_t)mh * sizeof(int32_t);
    if (in.size() != head + map_bytes + nbytes) { std::fprintf(stderr, "bad input size\n"); return 2; }
    int32_t* map = static_cast<int32_t*>(std::malloc(map_bytes));                          // the map ends where its block ends
    unsigned char* block = static_cast<unsigned char*>(std::malloc(offset + nbytes));      // the source ends where the block ends
    if (!map || !block) return 2;
    std::memcpy(map, in.data() + head, map_bytes);
    std::memcpy(block + offset, in.data() + head + map_bytes, nbytes);
    lmq::Src s;
    s.data = (lmi::addr_t)reinterpret_cast<uintptr_t>(block + offset);
    s.kind = (int)hd[0]; s.swap_rb = (int)hd[1]; s.matrix = (int)hd[2]; s.width = (int)hd[3]; s.height = (int)hd[4];
    s.row_stride = hd[5]; s.plane_stride = hd[6]; s.scale = (float)scale;
    s.dwords = s.kind == LMQ_PX4 && s.data % 4 == 0 && s.row_stride % 4 == 0;      // as the library sets it
    const lmx::Ratio r = {(int)hd[9], (int)hd[10], (int)hd[11], (int)hd[12]};
    const int mode = (int)hd[13];
    const lmy::Map m = {map, mw, mh};
    const int rw = lmx::reduced_size(mw, r.num_x, r.den_x), rh = lmx::reduced_size(mh, r.num_y, r.den_y);
    std::vector<uint32_t> out((size_t)rw * (size_t)rh);
    const HostTone ht = {tone.data()};
    for (int Y = 0; Y < rh; ++Y)
        for (int X = 0; X < rw; ++X)
            out[(size_t)Y * rw + X] = mode == 0 ? lmy::colour_pixel(s, pipe, m, r, X, Y, HostLd(), ht)
                                    : mode == 1 ? lmy::depth_nearest(s, m, r, X, Y, HostLd()) : lmy::depth_min_valid(s, m, r, X, Y, HostLd());
    std::free(block);
    std::free(map);
    FILE* f = std::fopen(out_path, "wb");
    if (!f) return 2;
    std::fwrite(out.data(), 4, out.size(), f);
    std::fclose(f);
    std::printf("OK %d %d\n", rw, rh);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "image")) return image(argv[2], argv[3]);
    std::fprintf(stderr, "usage: rectify_reduce_host image IN OUT\n");
    return 2;
}
