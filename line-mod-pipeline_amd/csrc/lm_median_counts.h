// lm_median_counts.h -- the word arithmetic of k_dmedian's counting median (lm_dev_depth.h, a5 streaming form), as functions the host can
// run too: tests/cpp/median_counts_check.cpp checks them exhaustively with g++, no GPU.
//
// The nine labels 0 < 1 < 2 < 4 < ... < 128 are ranks 0..8.  A 32-bit word holds eight 4-bit counters; counter k counts the pixels of
// rank <= 7 - k (CUMULATIVE counts: rank 8 is in none of them, and the counters never increase with k).  The 5 x 5 median is the lowest
// rank whose counter reaches 13 of the 25 pixels, rank 8 if none does.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LM_MC_FN __host__ __device__ __forceinline__
#else
#define LM_MC_FN inline
#endif

// k_dnormal's RANK CODE of a label (ensure_luts writes the table): 4 rank for ranks 0..7, 29 for rank 8.
LM_MC_FN uint32_t lm_mc_rank_code(uint32_t rank) { return rank < 8u ? 4u * rank : 29u; }

// A pixel's cumulative word from its rank code, ONE shift: 0x11111111 >> 4 rank has a one in the counters 0 .. 7 - rank, and the shift
// by 29 pushes the last one (bit 28) out: rank 8 counts nowhere, without a test.  (Counting towards the top -- 0x11111111 << 4 rank --
// has no such shift below 32: its empty word would need a second and a third operation per pixel.)
LM_MC_FN uint32_t lm_mc_word(uint32_t code) { return 0x11111111u >> (code & 31u); }

// The five row sums of a window (each the sum of five pixels' words: counters <= 5) are never added up: 25 does not fit a counter.
// A = the first three rows' sum (counters <= 15), B = the last two rows' (<= 10).  Per counter,
//     A + B >= 13  <=>  A + (B + 3) >= 16  <=>  floor((A + B + 3) / 2) >= 8,
// and the floor average of two counter words needs no carry between counters: (x & y) + (((x ^ y) >> 1) & 0x77777777) is exact per
// counter, at most (15 + 13) / 2 = 14.  Bit 3 of a counter of the average is the verdict.
// (the + 3 costs nothing in the kernel: it rides in the three-operand add that forms B)
#define LM_MC_BIAS 0x33333333u
LM_MC_FN uint32_t lm_mc_flags_biased(uint32_t A, uint32_t B3) {      // B3 = B + LM_MC_BIAS
    return ((A & B3) + (((A ^ B3) >> 1) & 0x77777777u)) & 0x88888888u;
}
LM_MC_FN uint32_t lm_mc_flags(uint32_t A, uint32_t B) { return lm_mc_flags_biased(A, B + LM_MC_BIAS); }

// The counters never increase with k, so the ranks that reached 13 are exactly those from the median rank up (counters 0 .. 7 - median):
// with n flags set the median rank is 8 - n and its label (1 << rank) >> 1 = 128 >> n  (n = 0..8 -> 128, 64, ..., 1, 0).
LM_MC_FN uint32_t lm_mc_label(uint32_t flags) { return 128u >> (uint32_t)__builtin_popcount(flags); }
