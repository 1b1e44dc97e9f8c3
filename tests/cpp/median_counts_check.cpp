// The word arithmetic of k_dmedian's counting median (lm_median_counts.h) on the CPU, exhaustively.  Built with g++ from this file alone
// (tests/test_median_counts_cpu.py, also under ASan / UBSan); no GPU.
//   flags   for every counter position, all 16 x 11 pairs (A, B) of a window's two partial counts -- A <= 15: three rows of five pixels,
//           B <= 10: two rows -- against A + B >= 13, with the seven other counters at every combination of their extremes (A: 0 / 15,
//           B: 0 / 10, and the two mixed pairs), so that a carry or a borrow between counters would show
//   words   the nine ranks' codes and cumulative words; sums of words stay what the kernel's bounds say; the label of every flag count
//   median  random 5 x 5 windows of ranks through the kernel's whole chain (words, horizontal sums, A and B, flags, label) against the
//           sorted window's middle element
// usage: median_counts_check          prints OK and the number of checks, or the cases that differ
#include "lm_median_counts.h"

#include <algorithm>
#include <cstdio>

namespace {

int g_bad = 0;
long g_checks = 0;
void expect(bool ok, const char* what, unsigned a, unsigned b, unsigned c, unsigned d) {
    ++g_checks;
    if (!ok && ++g_bad <= 20) printf("%s: %u %u %#x %#x\n", what, a, b, c, d);
}

uint32_t label_of_rank(uint32_t rank) { return rank ? 1u << (rank - 1) : 0u; }     // ranks 0..8 -> 0, 1, 2, 4, ..., 128

void check_flags() {
    // the other counters' (A, B): both extremes of each and the mixed pairs
    const uint32_t NA[4] = {0, 15, 0, 15}, NB[4] = {0, 10, 10, 0};
    for (int pos = 0; pos < 8; ++pos)
        for (uint32_t a = 0; a <= 15; ++a)
            for (uint32_t b = 0; b <= 10; ++b)
                for (int n = 0; n < 4; ++n) {
                    uint32_t A = 0, B = 0;
                    for (int k = 0; k < 8; ++k) {
                        A |= (k == pos ? a : NA[n]) << (4 * k);
                        B |= (k == pos ? b : NB[n]) << (4 * k);
                    }
                    const uint32_t f = lm_mc_flags(A, B);
                    expect((f & ~0x88888888u) == 0, "flag word has bits outside the counters' top bits", a, b, A, f);
                    expect((((f >> (4 * pos + 3)) & 1u) != 0) == (a + b >= 13), "flag of the counter under test", a, b, A, f);
                    for (int k = 0; k < 8; ++k)
                        if (k != pos) expect((((f >> (4 * k + 3)) & 1u) != 0) == (NA[n] + NB[n] >= 13), "flag of a neighbouring counter", a, b, A, f);
                    // the kernel's entry: the bias already added to B
                    expect(lm_mc_flags_biased(A, B + LM_MC_BIAS) == f, "biased entry", a, b, A, f);
                }
}

void check_words() {
    for (uint32_t rank = 0; rank <= 8; ++rank) {
        const uint32_t code = lm_mc_rank_code(rank), w = lm_mc_word(code);
        expect(code < 32, "code is a shift count", rank, code, w, 0);
        expect(rank != 0 || code == 0, "rank 0 (an invalid pixel's zero byte) has the code 0", rank, code, w, 0);
        for (uint32_t k = 0; k < 8; ++k)      // counter k: the pixels of rank <= 7 - k
            expect(((w >> (4 * k)) & 15u) == (rank <= 7 - k ? 1u : 0u), "cumulative word", rank, k, w, code);
        for (uint32_t r2 = 0; r2 < rank; ++r2) expect(lm_mc_rank_code(r2) != code, "codes differ", rank, r2, code, 0);
        // 25 pixels of one rank: five per row sum, fifteen in A, ten in B -- the bounds the carry-free forms rest on
        const uint32_t h = 5 * w, A = 3 * h, B = 2 * h;
        for (uint32_t k = 0; k < 8; ++k) {
            expect(((h >> (4 * k)) & 15u) == (rank <= 7 - k ? 5u : 0u), "row sum of five", rank, k, h, 0);
            expect(((A >> (4 * k)) & 15u) == (rank <= 7 - k ? 15u : 0u), "A of fifteen", rank, k, A, 0);
            expect(((B >> (4 * k)) & 15u) == (rank <= 7 - k ? 10u : 0u), "B of ten", rank, k, B, 0);
        }
        expect(lm_mc_label(lm_mc_flags(A, B)) == label_of_rank(rank), "median of 25 equal pixels", rank, code, A, B);
    }
    // n flags, wherever they sit, give 128 >> n
    for (uint32_t m = 0; m < 256; ++m) {
        uint32_t f = 0;
        for (int k = 0; k < 8; ++k) f |= ((m >> k) & 1u) << (4 * k + 3);
        expect(lm_mc_label(f) == (128u >> __builtin_popcount(m)), "label of a flag word", m, f, 0, 0);
    }
}

void check_median() {
    uint32_t s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    for (int it = 0; it < 200000; ++it) {
        // windows of few distinct ranks (what a depth image gives) and of any
        const uint32_t lo = rnd() % 9, span = it % 3 == 0 ? 9 : 1 + rnd() % 3;
        uint32_t r[25], h[5];
        for (int y = 0; y < 5; ++y) {
            h[y] = 0;
            for (int x = 0; x < 5; ++x) { r[5 * y + x] = (lo + rnd() % span) % 9; h[y] += lm_mc_word(lm_mc_rank_code(r[5 * y + x])); }
        }
        const uint32_t A = h[0] + h[1] + h[2], B = h[3] + h[4];
        std::sort(r, r + 25);
        expect(lm_mc_label(lm_mc_flags(A, B)) == label_of_rank(r[12]), "median of a window", r[12], (unsigned)it, A, B);
    }
}

}  // namespace

int main() {
    check_flags();
    check_words();
    check_median();
    if (g_bad) { printf("FAIL: %d of %ld checks\n", g_bad, g_checks); return 1; }
    printf("OK %ld checks\n", g_checks);
    return 0;
}
