// color_check_dump.cpp -- the host colour check (PostProcess.cpp: bgr2hsv_inrange, convex_hull, hull_counts) on cases read from a binary
// file, results on stdout, for tests/test_color_check_cpu.py to compare with tests/color_check_reference.py.  No GPU, no library.
//   file: int32 mode
//   mode 1 (masks):  int64 npix, int32 nranges, nranges x (3 lower + 3 upper) doubles, npix x 3 bytes BGR
//                    -> stdout (binary): per range npix mask bits, least significant bit first, (npix + 7) / 8 bytes
//   mode 2 (counts): int32 w, int32 h, w x h bytes colour mask (0 / non-zero), int32 ncases, per case int32 npts, ox, oy, npts x (x, y) int32
//                    -> stdout (text): per case one line "nv in_hull in_both x0 y0 x1 y1 .." (hull of the points, then placed at (ox, oy))
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../line-mod-pipeline_amd/host/PostProcess.h"

namespace {
template <typename T>
bool rd(FILE* f, T* v, size_t n = 1) { return std::fread(v, sizeof(T), n, f) == n; }
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: color_check_dump <cases file>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t mode = 0;
    if (!rd(f, &mode)) return 3;
    if (mode == 1) {
        int64_t npix = 0; int32_t nr = 0;
        if (!rd(f, &npix) || !rd(f, &nr) || npix <= 0 || npix > (1 << 26) || nr < 0 || nr > 4096) return 3;
        std::vector<double> rg((size_t)nr * 6);
        std::vector<uint8_t> bgr((size_t)npix * 3), mask, bits((size_t)(npix + 7) / 8);
        if (!rd(f, rg.data(), rg.size()) || !rd(f, bgr.data(), bgr.size())) return 3;
        for (int r = 0; r < nr; ++r) {
            lmamd::bgr2hsv_inrange(bgr.data(), (int)npix, 1, 0, &rg[(size_t)r * 6], &rg[(size_t)r * 6 + 3], mask);
            std::fill(bits.begin(), bits.end(), 0);
            for (int64_t i = 0; i < npix; ++i) if (mask[(size_t)i]) bits[(size_t)(i >> 3)] |= (uint8_t)(1u << (i & 7));
            if (std::fwrite(bits.data(), 1, bits.size(), stdout) != bits.size()) return 4;
        }
    } else if (mode == 2) {
        int32_t w = 0, h = 0, nc = 0;
        if (!rd(f, &w) || !rd(f, &h) || w <= 0 || h <= 0 || (int64_t)w * h > (1 << 26)) return 3;
        std::vector<uint8_t> mask((size_t)w * h);
        if (!rd(f, mask.data(), mask.size()) || !rd(f, &nc) || nc < 0) return 3;
        for (int c = 0; c < nc; ++c) {
            int32_t hd[3];
            if (!rd(f, hd, 3) || hd[0] < 0 || hd[0] > (1 << 20)) return 3;
            std::vector<int32_t> xy((size_t)hd[0] * 2);
            if (!rd(f, xy.data(), xy.size())) return 3;
            std::vector<lmamd::Pt> pts;
            for (int i = 0; i < hd[0]; ++i) pts.push_back(lmamd::Pt{xy[2 * (size_t)i], xy[2 * (size_t)i + 1]});
            std::vector<lmamd::Pt> hull = lmamd::convex_hull(pts);
            std::vector<lmamd::Pt> placed = hull;
            for (lmamd::Pt& p : placed) { p.x += hd[1]; p.y += hd[2]; }
            long in_hull = 0, in_both = 0;
            lmamd::hull_counts(placed, mask.data(), w, h, &in_hull, &in_both);
            std::printf("%zu %ld %ld", hull.size(), in_hull, in_both);
            for (const lmamd::Pt& p : hull) std::printf(" %d %d", p.x, p.y);
            std::printf("\n");
        }
    } else {
        return 3;
    }
    std::fclose(f);
    return 0;
}
