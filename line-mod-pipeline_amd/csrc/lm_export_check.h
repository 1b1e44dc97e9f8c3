// lm_export_check.h -- what the host hands k_export about a frame's destination (LmExportImage), and the checks that turn a caller's
// lm_image_desc / lm_draw_prim into it or into a refusal (lm_export_check.cpp; lm_export_frames).  Plain C++, no
// HIP, like lm_ingest_check.h: tests/cpp/export_host.cpp drives it with g++ under ASan / UBSan, and every refusal is pinned without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "../../include/linemod_hip.h"

// how a destination pixel lies in memory: the public LM_PIX_* format minus the channel order
enum { LM_EXPORT_PX3 = 0, LM_EXPORT_PX4 = 1, LM_EXPORT_PLANAR = 2, LM_EXPORT_NV12 = 3 };
// One frame of a call as k_export reads it
struct LmExportImage {
    uint8_t* data;                      // DEVICE pointer to surface pixel (0, 0)
    long long row_stride, plane_stride; // bytes (plane_stride: between the planes of LM_EXPORT_PLANAR, from the Y to the chroma plane of NV12)
    int crop_x, crop_y;                 // the window's top-left corner in the surface (validated: the window lies inside it)
    int kind, swap_rb;                  // swap_rb: the destination's channels are R, G, B
    int matrix;                         // NV12: the row of lmw::fwd_coef
    int flip_x, shift_x, shift_y;       // the ingest options to undo; |shift_x| <= w, |shift_y| <= h (clamped by the host)
    int es;                             // 0: an 8-bit destination; 4 / 2: a float one, binary32 / binary16 elements (k_export_float's frame)
    float scale;                        // float destinations: channel value c is written as (float)c * scale
};

namespace lmc {

enum { EXPORT_MAX_PRIMS = 65536 };

// The call's pointers and counts: a null dst, n_slots <= 0, null prims with n_prims > 0, n_prims > EXPORT_MAX_PRIMS
std::string check_export_counts(bool dst_null, int n_slots, bool prims_null, size_t n_prims);
// The frame itself: at most 8192 x 8192, the width a multiple of 16.  Returns the refusal, or an empty string.
std::string check_export_frame(int w, int h);
// Destination `im` of frame `frame` for a w x h window -> *out (flip_x, shift_x, shift_y are left 0: the caller's).
std::string check_export_image(int w, int h, const lm_image_desc& im, int frame, LmExportImage* out);
// Two destination windows of one call that overlap in memory: byte ranges per plane, compared by first and last byte (conservative: two
// windows side by side in one surface are refused too).
std::string check_export_overlap(int w, int h, const LmExportImage* images, int n);
// Primitive k of a call over n_frames frames
std::string check_export_prim(const lm_draw_prim& p, size_t k, int n_frames);

}  // namespace lmc
