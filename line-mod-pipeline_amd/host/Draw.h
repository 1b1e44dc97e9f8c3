// Draw.h -- the reference pipeline's drawing as primitive lists for lm_export_frames (include/linemod_hip.h):
//     HighLevelLineMOD::drawResponse          (HighLevelLinemod.cpp:545-: a circle per feature of the best template)     -> drawResponse
//     PoseDetection::drawCoordinateSystem     (PoseDetection.cpp:162-190: the pose's three axes as lines of thickness 2)  -> drawAxes
// and a bounding box.  The builders only append lm_draw_prim records -- nothing is drawn here; one lm_export_frames call composites
// the list onto the resident frames on the GPU and writes them in the consumer's format (PoseDetection::exportResults).  Primitives
// live in FRAME coordinates, where matches and poses live: behind the principal-point shift.  Parity with cv::circle / cv::line is not
// claimed (the header has the rule).  Header-only, like HighLevelLinemodIcp.h.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "HighLevelLinemod.h"
#include "PostProcess.h"

namespace lmamd {

inline lm_draw_prim drawPrim(int kind, int frame, int x0, int y0, int x1, int y1, int thickness, uint8_t b, uint8_t g, uint8_t r, uint8_t a = 255) {
    lm_draw_prim p;
    p.kind = kind; p.frame = frame; p.x0 = x0; p.y0 = y0; p.x1 = x1; p.y1 = y1; p.thickness = thickness;
    p.b = b; p.g = g; p.r = r; p.a = a;
    return p;
}

// the outline of in_rect, inclusive corners (x, y) .. (x + width - 1, y + height - 1)
inline void drawBox(const Rect& in_rect, uint8_t b, uint8_t g, uint8_t r, int in_thickness, int in_frame, std::vector<lm_draw_prim>& out) {
    out.push_back(drawPrim(LM_DRAW_BOX, in_frame, in_rect.x, in_rect.y, in_rect.x + in_rect.width - 1, in_rect.y + in_rect.height - 1, in_thickness, b, g, r));
}

// drawCoordinateSystem: the pose's origin and the tips of its three axes (in_length model units along x, y, z), projected with
// (fx, fy, width / 2, height / 2) -- the camera of the shifted frame -- in double precision and rounded half-to-even, as segments of
// thickness 2 from the origin: x red (0, 0, 255), y green, z blue.  An axis with an endpoint at Z <= 0 or outside the coordinate bound
// [-8192, 8191] is left out.  in_rotation: 3 x 3 row-major, model -> camera.
inline void drawAxes(const double in_rotation[9], const double in_translation[3], double fx, double fy, int in_width, int in_height, double in_length,
                     int in_frame, std::vector<lm_draw_prim>& out) {
    int px[4][2];
    bool ok[4];
    for (int k = 0; k < 4; ++k) {
        double P[3];
        for (int r = 0; r < 3; ++r) P[r] = (k == 0 ? 0.0 : in_length * in_rotation[3 * r + (k - 1)]) + in_translation[r];
        ok[k] = P[2] > 0.0;
        if (!ok[k]) continue;
        const double u = std::nearbyint(fx * P[0] / P[2] + in_width / 2.0), v = std::nearbyint(fy * P[1] / P[2] + in_height / 2.0);
        ok[k] = u >= -8192.0 && u <= 8191.0 && v >= -8192.0 && v <= 8191.0;
        if (ok[k]) { px[k][0] = (int)u; px[k][1] = (int)v; }
    }
    const uint8_t bgr[3][3] = {{0, 0, 255}, {0, 255, 0}, {255, 0, 0}};
    for (int k = 0; k < 3; ++k)
        if (ok[0] && ok[k + 1]) out.push_back(drawPrim(LM_DRAW_SEGMENT, in_frame, px[0][0], px[0][1], px[k + 1][0], px[k + 1][1], 2, bgr[k][0], bgr[k][1], bgr[k][2]));
}

// the rotation of an ObjectPose, row-major, model -> camera (fromGLM2CV(toMat3(quaternions)))
inline void poseRotation(const ObjectPose& in_pose, double out[9]) {
    const Mat4 m = toMat4(in_pose.quaternions);   // column-major: m[col][row]
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[3 * r + c] = m.m[c][r];
}

inline void drawAxes(const ObjectPose& in_pose, const CameraParameters& in_cam, float in_length, int in_frame, std::vector<lm_draw_prim>& out) {
    double R[9];
    poseRotation(in_pose, R);
    const double t[3] = {in_pose.translation.x, in_pose.translation.y, in_pose.translation.z};
    drawAxes(R, t, in_cam.fx, in_cam.fy, in_cam.videoWidth, in_cam.videoHeight, in_length, in_frame, out);
}

// drawResponse: one ring of radius T / 2 (in_T <= 0: the detector's T(0)), thickness 1, per level-0 feature of the match's template at
// (f.x + match.x, f.y + match.y) -- blue (255, 0, 0) for the colour modality, green (0, 255, 0) for the depth modality.  false (out_error)
// when the template cannot be read.
inline bool drawResponse(lm_detector* in_detector, const lm_match_t& in_match, int in_frame, int in_T, std::vector<lm_draw_prim>& out,
                         std::string* out_error = nullptr) {
    const int radius = (in_T > 0 ? in_T : lm_get_T(in_detector, 0)) / 2;
    const uint8_t bgr[2][3] = {{255, 0, 0}, {0, 255, 0}};
    for (int m = 0; m < lm_num_modalities(in_detector) && m < 2; ++m) {
        int w = 0, h = 0, n = 0;
        if (lm_get_template(in_detector, in_match.class_idx, in_match.template_id, 0, m, &w, &h, nullptr, &n) != LM_OK) {
            if (out_error) *out_error = lm_last_error();
            return false;
        }
        std::vector<lm_feature> f((size_t)std::max(n, 1));
        if (lm_get_template(in_detector, in_match.class_idx, in_match.template_id, 0, m, &w, &h, f.data(), &n) != LM_OK) {
            if (out_error) *out_error = lm_last_error();
            return false;
        }
        for (int k = 0; k < n; ++k)
            out.push_back(drawPrim(LM_DRAW_RING, in_frame, f[(size_t)k].x + in_match.x, f[(size_t)k].y + in_match.y, radius, 0, 1, bgr[m][0], bgr[m][1], bgr[m][2]));
    }
    return true;
}

}  // namespace lmamd
