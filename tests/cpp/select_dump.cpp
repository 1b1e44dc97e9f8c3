// select_dump -- the host yardstick of the feature selection: lmh::select_color / lmh::select_depth of csrc/lm_extract.cpp on candidate
// lists read from stdin, the selected features to stdout.  tests/test_select_cpu.py compares tests/select_reference.py with it.
// Input, per list: "modality n want area_bits", then n lines "x y label score_bits" (floats as the decimal value of their 32 bits).
// Output, per list: the number of features (-1: fewer candidates than wanted), then one line "x y label" per feature.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lm_extract.h"

static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

int main() {
    int modality, want;
    long n;
    unsigned area_bits;
    while (std::scanf("%d %ld %d %u", &modality, &n, &want, &area_bits) == 4) {
        std::vector<lmh::Candidate> cands((size_t)n);
        int per_label[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (long k = 0; k < n; ++k) {
            int x, y, label;
            unsigned bits;
            if (std::scanf("%d %d %d %u", &x, &y, &label, &bits) != 4 || label < 0 || label > 7) return 2;
            cands[(size_t)k] = lmh::Candidate{{x, y, label}, from_bits(bits)};
            ++per_label[label];
        }
        lmh::Template t;
        const bool ok = modality == 0 ? lmh::select_color(cands, (size_t)want, t)
                                      : lmh::select_depth(cands, per_label, from_bits(area_bits), (size_t)want, t);
        if (!ok) { std::printf("-1\n"); continue; }
        std::printf("%zu\n", t.features.size());
        for (const lm_feature& f : t.features) std::printf("%d %d %d\n", f.x, f.y, f.label);
    }
    return 0;
}
