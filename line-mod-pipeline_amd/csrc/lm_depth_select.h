// lm_depth_select.h -- the bin-choosing step of the depth check's sorted order statistic (k_depth_select, lm_k_depth_select.hip; DESIGN.md
// section 20), shared by the kernel and the host (tests/cpp/depth_select_host.cpp runs it against a sort).
//
// The statistic of rank k of a crop is the element at 0-based index k of the ascending sort of t = (d <= 1) ? 65535 : d.  A radix select over
// the 16-bit key finds it from two histograms: of the high bytes, then of the low bytes of the values whose high byte is the chosen one.
// Each time the bin that holds the rank is the first whose running count exceeds it; the rank inside that bin is the rank less the counts
// of the bins below.  Counts are 32-bit: a crop is at most a frame, far below 2^32 pixels.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LM_SEL_HD __host__ __device__
#else
#define LM_SEL_HD
#endif

#define LM_SEL_BINS 256          // bins of a pass: one byte of the key
#define LM_SEL_COARSE 16         // the kernel's bin search goes through 16 sums of 16 bins each

struct LmSelBin { int bin; uint32_t rank; };      // the chosen bin, and the rank among that bin's elements

// The bin of hist[0 .. nbins) that holds the element of 0-based rank `rank` in bin order, and the rank left inside it.  rank must be below
// the histogram's total; when it is not (never from a checked query), the last bin comes back with the rank that is left over.
LM_SEL_HD inline LmSelBin lm_select_bin(const uint32_t* hist, int nbins, uint32_t rank) {
    LmSelBin r;
    r.bin = nbins - 1; r.rank = rank;
    for (int b = 0; b < nbins; ++b) {
        const uint32_t c = hist[b];
        if (r.rank < c) { r.bin = b; return r; }
        if (b + 1 < nbins) r.rank -= c;
    }
    return r;
}

// The same over 256 bins in two steps of 16, as the kernel walks them: coarse[c] = hist[16 c] + .. + hist[16 c + 15].  Equal to
// lm_select_bin(hist, 256, rank) for every rank below the total.
LM_SEL_HD inline LmSelBin lm_select_bin256(const uint32_t* hist, const uint32_t* coarse, uint32_t rank) {
    const LmSelBin c = lm_select_bin(coarse, LM_SEL_COARSE, rank);
    LmSelBin f = lm_select_bin(hist + c.bin * (LM_SEL_BINS / LM_SEL_COARSE), LM_SEL_BINS / LM_SEL_COARSE, c.rank);
    f.bin += c.bin * (LM_SEL_BINS / LM_SEL_COARSE);
    return f;
}
