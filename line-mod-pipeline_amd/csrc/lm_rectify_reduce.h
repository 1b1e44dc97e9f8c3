// lm_rectify_reduce.h -- the rule of the rectified AND reduced ingest (lm_k_rectify_reduce.hip; written out in
// include/linemod_hip.h) as functions the host can run too.  It is the composition of two rules that exist, and this header holds no
// arithmetic of its own: a pixel of the rectified image Rc / Rd of the IDEAL geometry is lm_rectify.h's blend of four converted taps /
// nearest source pixel at that ideal pixel's map entry (RcAt, RdAt), and the reduced pixel is lm_reduce.h's box / depth rule over those
// pixels (lmx::box, lmx::nearest, lmx::min_valid).  Rc and Rd are never stored: every pixel of them is formed where the box needs it.
// The memory read and the tone table's read are parameters, so tests/cpp/rectify_reduce_host.cpp drives exactly the kernel's loads with
// g++ under ASan / UBSan over sources that end where their allocation ends.  A load is issued only for a tap inside the source.  No GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "lm_reduce.h"

namespace lmy {

typedef lmi::u32 u32;

// the detector's map: (qx, qy) of ideal pixel (i, j) at q[2 (j mw + i)], q[2 (j mw + i) + 1]; every entry lies in [-64, 32 n + 32] (lmq::quant)
struct Map { const int32_t* q; int mw, mh; };

// Rc at the map entry (qx, qy), B | G << 8 | R << 16.  KIND is one of lm_rectify.h's tap kinds, or LM_INGEST_BAYER_RGGB for the four 8-bit
// Bayer kinds, or LM_INGEST_RAW for the raw kinds: the three functions k_rectify's kernels call
template <int KIND, class Ld, class Tone>
LMI_FN u32 ideal_pixel(const lmq::Src& s, const lmi::RawPipe& p, int qx, int qy, Ld ld, Tone tone) {
    if constexpr (KIND == LM_INGEST_RAW) return lmq::colour_pixel_raw(s, p, qx, qy, ld, tone);
    else if constexpr (KIND == LM_INGEST_BAYER_RGGB) return lmq::colour_pixel_bayer(s, qx, qy, ld);
    else return lmq::colour_pixel<KIND>(s, qx, qy, ld);
}

// Rc(i, j) and Rd(i, j) of the whole ideal geometry, 0 outside it (the box and the depth rules never ask there)
template <int KIND, class Ld, class Tone>
struct RcAt {
    const lmq::Src& s; const lmi::RawPipe& p; Map m; Ld ld; Tone tone;
    LMI_FN u32 operator()(int i, int j) const {
        if (i < 0 || i >= m.mw || j < 0 || j >= m.mh) return 0u;
        const size_t at = 2 * ((size_t)j * (size_t)m.mw + (size_t)i);
        return ideal_pixel<KIND>(s, p, m.q[at], m.q[at + 1], ld, tone);
    }
};
template <class Ld>
struct RdAt {
    const lmq::Src& s; Map m; Ld ld;
    LMI_FN u32 operator()(int i, int j) const {
        if (i < 0 || i >= m.mw || j < 0 || j >= m.mh) return 0u;
        const size_t at = 2 * ((size_t)j * (size_t)m.mw + (size_t)i);
        return lmq::depth_pixel(s, m.q[at], m.q[at + 1], ld);
    }
};

// Reduced colour pixel (X, Y) of the reduced ideal geometry: the box over Rc
template <int KIND, class Ld, class Tone>
LMI_FN u32 colour_pixel_of(const lmq::Src& s, const lmi::RawPipe& p, const Map& m, const lmx::Ratio& r, int X, int Y, Ld ld, Tone tone) {
    const RcAt<KIND, Ld, Tone> at = {s, p, m, ld, tone};
    return lmx::box(r, X, Y, at);
}

// the kind switch: one branch per reduced pixel, uniform over the image
template <class Ld, class Tone>
LMI_FN u32 colour_pixel(const lmq::Src& s, const lmi::RawPipe& p, const Map& m, const lmx::Ratio& r, int X, int Y, Ld ld, Tone tone) {
    switch (s.kind) {
    case LMQ_PX3: return colour_pixel_of<LMQ_PX3>(s, p, m, r, X, Y, ld, tone);
    case LMQ_PX4: return colour_pixel_of<LMQ_PX4>(s, p, m, r, X, Y, ld, tone);
    case LMQ_PLANAR: return colour_pixel_of<LMQ_PLANAR>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_GRAY8: return colour_pixel_of<LM_INGEST_GRAY8>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_NV12: return colour_pixel_of<LM_INGEST_NV12>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_NV21: return colour_pixel_of<LM_INGEST_NV21>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_YUY2: return colour_pixel_of<LM_INGEST_YUY2>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_UYVY: return colour_pixel_of<LM_INGEST_UYVY>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 0: return colour_pixel_of<LM_INGEST_FLOAT + 0>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 1: return colour_pixel_of<LM_INGEST_FLOAT + 1>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 2: return colour_pixel_of<LM_INGEST_FLOAT + 2>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 3: return colour_pixel_of<LM_INGEST_FLOAT + 3>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 4: return colour_pixel_of<LM_INGEST_FLOAT + 4>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 5: return colour_pixel_of<LM_INGEST_FLOAT + 5>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 6: return colour_pixel_of<LM_INGEST_FLOAT + 6>(s, p, m, r, X, Y, ld, tone);
    case LM_INGEST_FLOAT + 7: return colour_pixel_of<LM_INGEST_FLOAT + 7>(s, p, m, r, X, Y, ld, tone);
    default: return s.kind >= LM_INGEST_RAW ? colour_pixel_of<LM_INGEST_RAW>(s, p, m, r, X, Y, ld, tone) : colour_pixel_of<LM_INGEST_BAYER_RGGB>(s, p, m, r, X, Y, ld, tone);
    }
}

// Reduced depth pixel (X, Y): the reduction's depth rule over Rd
template <class Ld>
LMI_FN u32 depth_nearest(const lmq::Src& s, const Map& m, const lmx::Ratio& r, int X, int Y, Ld ld) {
    const RdAt<Ld> at = {s, m, ld};
    return lmx::nearest(r, X, Y, at);
}
template <class Ld>
LMI_FN u32 depth_min_valid(const lmq::Src& s, const Map& m, const lmx::Ratio& r, int X, int Y, Ld ld) {
    const RdAt<Ld> at = {s, m, ld};
    return lmx::min_valid(r, X, Y, at);
}

}  // namespace lmy
