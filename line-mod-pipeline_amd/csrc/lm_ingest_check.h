// lm_ingest_check.h -- what the host hands k_ingest / k_register / k_rectify about a frame's images (LmIngestImage, LmIngestDesc), and the
// one check that turns a caller's lm_image_desc into it (lm_ingest_check.cpp).  Plain C++, no HIP: the check is arithmetic on a struct, so
// tests/cpp/ingest_check_host.cpp drives it with g++ under ASan / UBSan, and every refusal is pinned without a GPU.
#pragma once
#include <stdint.h>
#include <string>

#include "../../include/linemod_hip.h"
#include "lm_ingest_yuv.h"
#include "lm_ingest_bayer.h"
#include "lm_ingest_raw.h"
#include "lm_ingest_float.h"

// ---- device-resident frames in the producer's format -> the slots (lm_k_ingest.hip)
// One image of one frame as k_ingest reads it: kind = how a pixel lies in memory (the public LM_PIX_* format minus the channel order),
// swap_rb = the source's channels are R, G, B.  aligned: every 16-pixel span a lane reads starts on a 16-byte boundary (the fast path).
// The grey and YUV kinds of a colour image (LM_INGEST_GRAY8 = 5 .. LM_INGEST_UYVY = 9; the kind carries the chroma order and the byte order
// inside the macropixel) are lm_ingest_yuv.h's: frames with such a colour image are k_ingest_yuv's.  The raw Bayer kinds
// (LM_INGEST_BAYER_RGGB = 10 .. LM_INGEST_BAYER_BGGR = 13) are lm_ingest_bayer.h's and k_ingest_bayer's; all others are k_ingest's
// (lm_ingest_family).  The kinds from LM_INGEST_RAW = 14 on (storage and pattern: lm_ingest_raw.h) are k_ingest_raw's: the high-bit raw
// formats, and an 8-bit Bayer image while a raw pipeline is set (lmc::process_bayer8).  The kinds from LM_INGEST_FLOAT = 128 on (element
// and shape: lm_ingest_float.h) are k_ingest_float's: the float colour formats, converted with `scale`.
enum { LM_INGEST_PX3 = 0, LM_INGEST_PX4 = 1, LM_INGEST_PLANAR = 2, LM_INGEST_U16 = 3, LM_INGEST_F32 = 4 };
struct LmIngestImage {
    const uint8_t* data;                // DEVICE pointer to source pixel (0, 0)
    long long row_stride, plane_stride; // bytes (plane_stride: between the planes of LM_INGEST_PLANAR, from the Y to the chroma plane of NV12 / NV21)
    int crop_x, crop_y;                 // the window's top-left corner in the source (validated: the window lies inside it)
    int kind, swap_rb, aligned;
    int src_w, src_h;                   // the source's size: a Bayer source reflects at its own edges, wherever the window lies
    float scale;                        // LM_INGEST_F32: millimetres per unit; the float colour kinds: to_u8's factor
};
struct LmIngestDesc {
    LmIngestImage colour, depth;
    int flip_x, shift_x, shift_y;       // |shift_x| <= w, |shift_y| <= h (clamped by the host)
    int matrix;                         // YUV colour image: the row of lmi::yuv_coef (0 BT.601 limited, 1 BT.709 limited, 2 BT.601 full, 3 BT.709 full)
};

namespace lmc {

// What the routes of an image differ in: lm_ingest_frames (plain), lm_ingest_frames_rectified / lm_stage_rectify (rectified), the raw
// depth image of lm_ingest_frames_registered / lm_stage_register_depth (raw_depth) and lm_ingest_frames_reduced / lm_stage_reduce (reduced).  Everything else of the check is shared.
enum Role { COLOUR, DEPTH, RAW_DEPTH };             // the `who` words; DEPTH and RAW_DEPTH take the depth formats alone, COLOUR the others
enum AlignedRule { SPANS, DWORD, NEVER };           // LmIngestImage::aligned: lmi::spans_aligned / a 4-byte pixel read as one dword / 0
struct Geometry {
    Role role;
    int win_w, win_h;               // the window: the detector's frame
    const char* source_name; int source_w, source_h;    // the camera whose size the source must have; nullptr: any size
    const char* bound_name; int bound_w, bound_h;       // the geometry the window must lie in; nullptr: the source itself, in OpenCV's sentence
    const char* row_name; int row_w;                    // a row stride covers row_w pixels: a "window", "source" or "raw" row
    bool whole;                     // the stage hooks: no window, crop 0
    const char* prefix;             // in front of the size, window and row refusals ("rectification: " or nothing)
    AlignedRule aligned;
    int num_x, den_x, num_y, den_y; // the reduced route (den_x != 0): the bound is the image's OWN reduced geometry, ((width den_x) / num_x) x ((height den_y) / num_y)
};
Geometry plain(const lm_config& c, Role role);
Geometry rectified(const lm_config& c, const lm_rectification_desc& rect, Role role, bool whole);
Geometry raw_depth(const lm_config& c, const lm_registration_desc& reg, bool whole);
// lm_ingest_frames_reduced / lm_stage_reduce (red: as check_reduction left it).  An image whose apply bit is clear takes the plain geometry
// (the stage hook: the whole source, ratio 1 / 1).
Geometry reduced(const lm_config& c, const lm_reduction_desc& red, Role role, bool whole);
// lm_ingest_frames_rectified_reduced / lm_stage_rectify_reduce: the rectified route's check of the source (the source camera's size, a
// source row) with the window placed in the REDUCED IDEAL geometry, ((ideal.width den_x) / num_x) x ((ideal.height den_y) / num_y); an
// image whose apply bit is clear takes the rectified geometry as it is.
Geometry rectified_reduced(const lm_config& c, const lm_rectification_desc& rect, const lm_reduction_desc& red, Role role, bool whole);

// lm_set_reduction's and lm_reduced_camera's check of a caller's reduction -> *out with the fractions in lowest terms.  Returns the
// refusal ("reduction: ..."), or an empty string.
std::string check_reduction(const lm_reduction_desc& in, lm_reduction_desc* out);

// "Is there a depth plane" in the slots of a detector with this configuration: depth is a modality, or LM_FLAG_KEEP_DEPTH
inline bool keeps_depth(const lm_config& c) { return c.num_modalities == 2 || (c.flags & LM_FLAG_KEEP_DEPTH) != 0; }

// What an lm_ingest_frames* call does with its depth descriptors, decided on the host before any descriptor is read.
//   registered: the call's depth images are RAW depth images for the registration (lm_ingest_frames_registered, depth_route
//   LM_RECTIFY_DEPTH_REGISTERED); depth_given: the caller passed a depth descriptor array.
// A detector that keeps no depth ignores the descriptors of every route but the registered one, which it refuses (the returned
// sentence; empty: no refusal).  One whose depth is a modality requires them, and so does the registered route (depth_required: without
// them the call is a "bad argument"); a colour-only detector that keeps depth takes them if they are there.  *takes_depth = the call
// reads the descriptors and writes the slots' depth planes.
inline bool depth_required(const lm_config& c, bool registered) { return keeps_depth(c) && (registered || c.num_modalities == 2); }
std::string check_depth_call(const lm_config& c, bool registered, bool depth_given, bool* takes_depth);
// Image `im` of frame `frame` against g -> *out and, where matrix is not null, the image's row of lmi::yuv_coef.  o: the frame's options,
// shifts already clamped (the SPANS rule reads flip_x and shift_x).  Returns the refusal, or an empty string: the image is good.
std::string check_image(const Geometry& g, const lm_image_desc& im, int frame, const lm_ingest_opts& o, LmIngestImage* out, int* matrix);

// While a raw pipeline is set (lm_set_raw_processing), an 8-bit Bayer image that check_image has passed takes the raw kind of its
// pattern, N = 8 (and the general load path); any other image is left as it is.
void process_bayer8(LmIngestImage* im);

}  // namespace lmc
