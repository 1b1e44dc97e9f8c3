// Host driver of the depth check's sorted order statistic (tests/test_depth_select_cpu.py): median_mat_sorted of host/PostProcess.cpp and the
// bin-choosing step of csrc/lm_depth_select.h -- the one k_depth_select calls -- on the cases of a file.
//   depth_select_host <cases.bin>
// cases.bin: int32 n_cases; per case int32 {w, h, bb.x, bb.y, bb.width, bb.height, position, shift_x, shift_y}, then w * h uint16 depths.
// Prints per case "<sorted> <radix flat> <radix two-level> <reference element>":
//   sorted     median_mat_sorted
//   radix      the two-pass radix select at rank n / position on the crop as median_mat clips it (histograms built here, the bins chosen by
//              lm_select_bin over 256 bins / by lm_select_bin256), 65535 for an empty crop
//   reference  median_mat: v[n / position] after std::nth_element(v, v + n / 4) of this library
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../line-mod-pipeline_amd/csrc/lm_depth_select.h"
#include "../../line-mod-pipeline_amd/host/PostProcess.h"

using namespace lmamd;

// the crop's values t, the translation applied as the slot holds it (zeros shifted in)
static std::vector<uint16_t> crop_values(const std::vector<uint16_t>& d, int w, int h, Rect bb, int sx, int sy) {
    std::vector<uint16_t> t;
    const long long x0 = std::max(bb.x, 0), y0 = std::max(bb.y, 0);
    const long long x1 = std::min<long long>((long long)bb.x + bb.width, w), y1 = std::min<long long>((long long)bb.y + bb.height, h);
    for (long long y = y0; y < y1; ++y)
        for (long long x = x0; x < x1; ++x) {
            const long long ux = x - sx, uy = y - sy;
            const uint16_t v = (ux >= 0 && ux < w && uy >= 0 && uy < h) ? d[(size_t)uy * (size_t)w + (size_t)ux] : (uint16_t)0;
            t.push_back(v <= 1 ? (uint16_t)65535 : v);
        }
    return t;
}

static int radix_select(const std::vector<uint16_t>& t, uint32_t rank, bool two_level) {
    if (t.empty()) return 65535;
    std::vector<uint32_t> hist(LM_SEL_BINS, 0), coarse(LM_SEL_COARSE, 0);
    auto choose = [&](uint32_t r) {
        std::fill(coarse.begin(), coarse.end(), 0u);
        for (int b = 0; b < LM_SEL_BINS; ++b) coarse[(size_t)(b / (LM_SEL_BINS / LM_SEL_COARSE))] += hist[(size_t)b];
        return two_level ? lm_select_bin256(hist.data(), coarse.data(), r) : lm_select_bin(hist.data(), LM_SEL_BINS, r);
    };
    for (uint16_t v : t) hist[(size_t)(v >> 8)] += 1;
    const LmSelBin hi = choose(rank);
    std::fill(hist.begin(), hist.end(), 0u);
    for (uint16_t v : t) if ((v >> 8) == hi.bin) hist[(size_t)(v & 255)] += 1;
    const LmSelBin lo = choose(hi.rank);
    return (hi.bin << 8) | lo.bin;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    int32_t n_cases = 0;
    if (!f.read(reinterpret_cast<char*>(&n_cases), 4)) return 3;
    for (int32_t c = 0; c < n_cases; ++c) {
        int32_t hd[9];
        if (!f.read(reinterpret_cast<char*>(hd), sizeof(hd))) return 3;
        const int w = hd[0], h = hd[1];
        std::vector<uint16_t> d((size_t)w * (size_t)h);
        if (!d.empty() && !f.read(reinterpret_cast<char*>(d.data()), (std::streamsize)(d.size() * 2))) return 3;
        const Rect bb{hd[2], hd[3], hd[4], hd[5]};
        const uint8_t position = (uint8_t)hd[6];
        const uint16_t sorted = median_mat_sorted(d.data(), w, h, bb, position, hd[7], hd[8]);
        const uint16_t ref = median_mat(d.data(), w, h, bb, position, hd[7], hd[8]);
        const std::vector<uint16_t> t = crop_values(d, w, h, bb, hd[7], hd[8]);
        const uint32_t rank = position ? (uint32_t)(t.size() / position) : 0u;
        const int flat = position ? radix_select(t, rank, false) : 65535, two = position ? radix_select(t, rank, true) : 65535;
        std::printf("%d %d %d %d\n", (int)sorted, flat, two, (int)ref);
    }
    // then int32 n_hist; per histogram uint32 rank and 256 uint32 counts: "<bin> <rank left> <bin> <rank left>" of the flat and the two-level form
    int32_t n_hist = 0;
    if (!f.read(reinterpret_cast<char*>(&n_hist), 4)) return 0;
    for (int32_t c = 0; c < n_hist; ++c) {
        uint32_t rank = 0, hist[LM_SEL_BINS], coarse[LM_SEL_COARSE] = {};
        if (!f.read(reinterpret_cast<char*>(&rank), 4) || !f.read(reinterpret_cast<char*>(hist), sizeof(hist))) return 3;
        for (int b = 0; b < LM_SEL_BINS; ++b) coarse[b / (LM_SEL_BINS / LM_SEL_COARSE)] += hist[b];
        const LmSelBin a = lm_select_bin(hist, LM_SEL_BINS, rank), b2 = lm_select_bin256(hist, coarse, rank);
        std::printf("%d %u %d %u\n", a.bin, a.rank, b2.bin, b2.rank);
    }
    return 0;
}
