// HighLevelLinemodIcp.h -- the reference pipeline's ICP refinement class (HighLevelLinemodIcp.cpp:3-137) over the C ABI: the scene
// cloud and the rounds of ICP run on the GPU (lm_icp_set_model / lm_stage_icp_refine_host), and so does the
// best-pose check (estimateBestMatchGpu / meanDepthDifferencesGpu over lm_stage_icp_verify_host: the GPU rasteriser draws what SoftRender
// draws bit for bit, the sums are integers, so the means are those of the host check to the last bit).  estimateBestMatch and
// meanDepthDifference, the same check on the host with SoftRender, stay as the yardstick.  Header-only (like GroupWaves.h):
// PoseDetection.cpp uses it, and a program built from the host sources as before (HighLevelLinemod, PostProcess, TemplateGenerator,
// PoseDetection) links without another source file.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "HighLevelLinemod.h"
#include "PostProcess.h"
#include "TemplateGenerator.h"

namespace lmamd {

class HighLevelLinemodIcp {
public:
    // ICP(in_iteration, in_tolerance, in_rejectionScale, in_numIterations) and the model files (modelFolder + file, PLY with normals) of
    // the detector's classes in class-index order; an empty file list loads nothing (setModel hands meshes in instead).
    HighLevelLinemodIcp(lm_detector* in_detector, uint16_t in_iteration, float in_tolerance, float in_rejectionScale, uint16_t in_numIterations,
                        uint16_t in_sampleStep, std::vector<std::string> in_modelFiles, std::string in_modFolder);

    // loadModels for one class: rows 0, step, 2 step, ... of the mesh's vertices with their normals.  false (lastError) without normals.
    // Also keeps the mesh resident as render mesh in_modelNumber (lm_set_render_mesh) for the GPU check: the class index, the convention
    // of Benchmark::loadModel, and the same mesh.  Render meshes are shared by index across the detector: addTemplatesRendered renders
    // from index 0, so generate banks before setModel, or call setModel again afterwards.
    bool setModel(uint16_t in_modelNumber, const Mesh& in_mesh);
    // Keeps the frame and the bbox of the next registerToScene.  in_depth is the principal-point-shifted depth image (the frame the
    // match ran on); the intrinsics used are (fx, fy, width / 2, height / 2) -- DESIGN.md section 9's choice.  The bbox is clipped to
    // the frame (cv::rectangle on the mask does the same in the reference).
    void prepareDepthForIcp(const uint16_t* in_depth, int in_width, int in_height, const CameraParameters& in_cam, const Rect& in_bb);
    // Refines every pose in place (lm_stage_icp_refine_host).  false (lastError) when the refinement could not run; a scene cloud of
    // fewer than 6 points leaves the poses as they were and is not an error here.
    bool registerToScene(std::vector<ObjectPose>& in_poses, uint16_t in_modelNumber);
    // :93-137: render every pose, mask = render > 1 and scene > 600 eroded 3x3 twice, mean |scene - render| over the mask (0 if empty)
    // truncated to uint16; pose i is kept if (mean < best && mean != 0) || i == 0; true (and in_bestPose) when the kept mean <= 35.
    bool estimateBestMatch(const uint16_t* in_depthImg, const std::vector<ObjectPose>& in_poses, const SoftRender& in_render,
                           uint16_t in_modelIndice, uint16_t& in_bestPose);
    // the mean of estimateBestMatch for one pose (exposed for tests)
    double meanDepthDifference(const uint16_t* in_depthImg, const ObjectPose& in_pose, const SoftRender& in_render, uint16_t in_modelIndice);
    // The same two on the GPU (lm_stage_icp_verify_host): every pose of the group in one call, rendered as resident render mesh
    // in_modelIndice under in_render.view_proj_of(icp_view_matrix(pose)).  in_depth is in_width x in_height (estimateBestMatchGpu: the
    // renderer's size).  The means and the verdict are those of the host forms.  false with lastError() when the call fails;
    // estimateBestMatchGpu also returns false, with lastError() empty, when the group is rejected.
    bool meanDepthDifferencesGpu(const uint16_t* in_depthImg, int in_width, int in_height, const std::vector<ObjectPose>& in_poses,
                                 const SoftRender& in_render, uint16_t in_modelIndice, std::vector<double>& out_means);
    bool estimateBestMatchGpu(const uint16_t* in_depthImg, const std::vector<ObjectPose>& in_poses, const SoftRender& in_render,
                              uint16_t in_modelIndice, uint16_t& in_bestPose);
    // The batch forms, for frames resident in the detector's slots (the principal-point-shifted frames a batch was matched on; DESIGN.md
    // section 21).  A group: its frame's slot, its class, its poses and the bbox of its first pose.
    struct SlotGroup { int slot = 0; uint16_t modelNumber = 0; Rect boundingBox; std::vector<ObjectPose>* poses = nullptr; };
    // One lm_icp_refine_slots call for all groups; every bbox is clipped to the in_width x in_height frame as prepareDepthForIcp clips it.
    // out_status[g]: LM_OK (the poses are refined in place), LM_ERR_INVALID (a scene cloud of fewer than 6 points: the poses stay, as
    // registerToScene leaves them) or LM_ERR_OVERFLOW.  false (lastError) only when the call itself is refused or fails.
    bool registerToSceneSlots(std::vector<SlotGroup>& in_groups, int in_width, int in_height, const CameraParameters& in_cam,
                              std::vector<int32_t>& out_status);
    // One lm_icp_verify call for all poses of all groups, rendered under icp_view_matrix as meanDepthDifferencesGpu renders them:
    // out_means[g][k] for pose k of group g.
    bool meanDepthDifferencesSlots(const std::vector<SlotGroup>& in_groups, const SoftRender& in_render, std::vector<std::vector<double>>& out_means);
    // :106-131 on the means alone: pose i is kept if (mean < best && mean != 0) || i == 0, the kept mean truncated to uint16; true (and
    // in_bestPose) when it is <= correctEstimateTreshold.  An empty list is rejected.
    static bool selectBestMatch(const std::vector<double>& in_means, uint16_t& in_bestPose);
    const std::string& lastError() const { return error; }

    static constexpr uint16_t correctEstimateTreshold = 35;
    static constexpr int sceneMinDepth = 600;   // :113: scene > 600

private:
    lm_detector* det;
    lm_icp_params params{};
    std::vector<Mesh> meshes;      // by class index: the renderer's meshes
    std::vector<uint16_t> depth;   // prepareDepthForIcp's frame
    int width = 0, height = 0;
    CameraParameters cam;
    Rect bb;
    std::string error;
};

// The camera-frame pose of an ObjectPose (fromGLM2CV(toMat3(quaternions)) | translation), 4x4 row-major, and back (updatePosition).
inline void pose_to_matrix(const ObjectPose& p, double out[16]) {
    const Mat4 m = toMat4(p.quaternions);   // column-major: m[col][row]
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[4 * r + c] = m.m[c][r];
    out[3] = p.translation.x; out[7] = p.translation.y; out[11] = p.translation.z;
    out[12] = 0; out[13] = 0; out[14] = 0; out[15] = 1;
}

inline void matrix_to_pose(const double m[16], ObjectPose& p) {
    Mat4 g;
    std::memset(g.m, 0, sizeof(g.m));
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) g.m[c][r] = (float)m[4 * r + c];
    g.m[3][3] = 1.f;
    p.quaternions = toQuat(g);
    p.translation = Vec3{(float)m[3], (float)m[7], (float)m[11]};
}

inline HighLevelLinemodIcp::HighLevelLinemodIcp(lm_detector* in_detector, uint16_t in_iteration, float in_tolerance, float in_rejectionScale,
                                         uint16_t in_numIterations, uint16_t in_sampleStep, std::vector<std::string> in_modelFiles,
                                         std::string in_modFolder)
    : det(in_detector) {
    params.step = std::max<int>(in_sampleStep, 1);
    params.iterations = in_iteration;
    params.tolerance = in_tolerance;
    params.rejection_scale = in_rejectionScale;
    params.levels = in_numIterations;
    params.max_points = 0;
    for (size_t k = 0; k < in_modelFiles.size(); ++k) {   // loadModels (:24-37)
        Mesh m;
        std::string e;
        if (!load_ply_ascii(in_modFolder + in_modelFiles[k], m, &e)) { error = e; continue; }
        setModel((uint16_t)k, m);
    }
}

inline bool HighLevelLinemodIcp::setModel(uint16_t k, const Mesh& mesh) {
    if (mesh.normals.size() != mesh.vertices.size() || mesh.vertices.empty()) { error = "the ICP model needs per-vertex normals"; return false; }
    std::vector<float> xyzn(mesh.vertices.size() * 6);
    for (size_t i = 0; i < mesh.vertices.size(); ++i) {
        float* r = &xyzn[6 * i];
        r[0] = mesh.vertices[i].x; r[1] = mesh.vertices[i].y; r[2] = mesh.vertices[i].z;
        r[3] = mesh.normals[i].x; r[4] = mesh.normals[i].y; r[5] = mesh.normals[i].z;
    }
    if (lm_icp_set_model(det, k, xyzn.data(), (int)mesh.vertices.size(), params.step) != LM_OK) { error = lm_last_error(); return false; }
    if (meshes.size() <= k) meshes.resize((size_t)k + 1);
    meshes[k] = mesh;
    // (last: a class index beyond LM_MAX_RENDER_MESHES keeps its ICP model and the host check, and fails here)
    std::vector<float> xyz(mesh.vertices.size() * 3);
    for (size_t i = 0; i < mesh.vertices.size(); ++i) {
        xyz[3 * i] = mesh.vertices[i].x; xyz[3 * i + 1] = mesh.vertices[i].y; xyz[3 * i + 2] = mesh.vertices[i].z;
    }
    if (lm_set_render_mesh(det, k, xyz.data(), (int)mesh.vertices.size(), mesh.indices.data(), (int)mesh.indices.size()) != LM_OK) {
        error = lm_last_error();
        return false;
    }
    return true;
}

inline void HighLevelLinemodIcp::prepareDepthForIcp(const uint16_t* in_depth, int w, int h, const CameraParameters& in_cam, const Rect& in_bb) {
    depth.assign(in_depth, in_depth + (size_t)w * h);
    width = w; height = h;
    cam = in_cam;
    const int x0 = std::max(in_bb.x, 0), y0 = std::max(in_bb.y, 0);
    const int x1 = std::min(in_bb.x + in_bb.width, w), y1 = std::min(in_bb.y + in_bb.height, h);
    bb = Rect{x0, y0, std::max(x1 - x0, 0), std::max(y1 - y0, 0)};
}

inline bool HighLevelLinemodIcp::registerToScene(std::vector<ObjectPose>& in_poses, uint16_t in_modelNumber) {
    error.clear();
    if (in_poses.empty()) return true;
    if (depth.empty()) { error = "prepareDepthForIcp first"; return false; }
    std::vector<double> P(16 * in_poses.size());
    for (size_t i = 0; i < in_poses.size(); ++i) pose_to_matrix(in_poses[i], &P[16 * i]);
    lm_icp_query q{};
    q.x = bb.x; q.y = bb.y; q.width = bb.width; q.height = bb.height;
    q.class_idx = in_modelNumber;
    q.first_pose = 0; q.num_poses = (int)in_poses.size();
    q.fx = cam.fx; q.fy = cam.fy; q.cx = 0.5 * width; q.cy = 0.5 * height;
    const int rc = lm_stage_icp_refine_host(det, depth.data(), &q, 1, &params, P.data());
    if (rc != LM_OK) {
        const std::string e = lm_last_error();
        if (rc == LM_ERR_INVALID && e.find("fewer than 6") != std::string::npos) return true;   // the rule's own stop: poses unchanged
        error = e;
        return false;
    }
    for (size_t i = 0; i < in_poses.size(); ++i) {
        ObjectPose& p = in_poses[i];
        matrix_to_pose(&P[16 * i], p);
    }
    return true;
}

// glm::eulerAngles / glm::qua<float>(vec3) as the reference's estimateBestMatch uses them (:99-101)
inline void icp_euler_angles(const Quat& q, float e[3]) {
    const float y = 2.f * (q.y * q.z + q.w * q.x), x = q.w * q.w - q.x * q.x - q.y * q.y + q.z * q.z;
    e[0] = (std::fabs(x) < 1e-12f && std::fabs(y) < 1e-12f) ? 2.f * std::atan2(q.x, q.w) : std::atan2(y, x);
    float s = -2.f * (q.x * q.z - q.w * q.y);
    s = s < -1.f ? -1.f : (s > 1.f ? 1.f : s);
    e[1] = std::asin(s);
    e[2] = std::atan2(2.f * (q.x * q.y + q.w * q.z), q.w * q.w + q.x * q.x - q.y * q.y - q.z * q.z);
}
inline Quat icp_quat_from_euler(const float e[3]) {
    const float cx = std::cos(e[0] * 0.5f), cy = std::cos(e[1] * 0.5f), cz = std::cos(e[2] * 0.5f);
    const float sx = std::sin(e[0] * 0.5f), sy = std::sin(e[1] * 0.5f), sz = std::sin(e[2] * 0.5f);
    Quat q;
    q.w = cx * cy * cz + sx * sy * sz;
    q.x = sx * cy * cz - cx * sy * sz;
    q.y = cx * sy * cz + sx * cy * sz;
    q.z = cx * cy * sz - sx * sy * cz;
    return q;
}

// 3x3 erosion of a 0/1 mask; pixels outside the image count as set (cv::erode's default border: the border does not erode)
inline void icp_erode3(std::vector<uint8_t>& m, int w, int h) {
    std::vector<uint8_t> o(m.size());
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            uint8_t v = 1;
            for (int dy = -1; dy <= 1 && v; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int yy = y + dy, xx = x + dx;
                    if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
                    if (!m[(size_t)yy * w + xx]) { v = 0; break; }
                }
            o[(size_t)y * w + x] = v;
        }
    m.swap(o);
}

// The view matrix estimateBestMatch renders a pose with (:99-104): euler angles (x + pi, -y, -z), pi a float, and the translation
// (t.x, -t.y, -t.z).  (Not Benchmark::calculateViewMat, which subtracts a double pi.)
inline Mat4 icp_view_matrix(const ObjectPose& pose) {
    float e[3];
    icp_euler_angles(pose.quaternions, e);
    const float f[3] = {e[0] + 3.14159265358979323846f, -e[1], -e[2]};
    Mat4 view = toMat4(icp_quat_from_euler(f));
    view.m[3][0] = pose.translation.x; view.m[3][1] = -pose.translation.y; view.m[3][2] = -pose.translation.z; view.m[3][3] = 1.0f;
    return view;
}

inline double HighLevelLinemodIcp::meanDepthDifference(const uint16_t* scene, const ObjectPose& pose, const SoftRender& render, uint16_t k) {
    if (k >= meshes.size()) return 0.0;
    const Mat4 view = icp_view_matrix(pose);
    std::vector<uint8_t> bgr;
    std::vector<uint16_t> rd;
    render.render_view(meshes[k], view.m, bgr, rd);
    const int w = render.width, h = render.height;
    std::vector<uint8_t> mask((size_t)w * h);
    for (size_t i = 0; i < mask.size(); ++i) mask[i] = rd[i] > 1 && scene[i] > sceneMinDepth;
    icp_erode3(mask, w, h);
    icp_erode3(mask, w, h);
    double sum = 0;
    long n = 0;
    for (size_t i = 0; i < mask.size(); ++i)
        if (mask[i]) { sum += std::abs((int)scene[i] - (int)rd[i]); ++n; }
    return n ? sum / (double)n : 0.0;
}

inline bool HighLevelLinemodIcp::selectBestMatch(const std::vector<double>& in_means, uint16_t& in_bestPose) {
    uint16_t bestMean = 0, bestPose = 0;
    for (size_t i = 0; i < in_means.size(); ++i) {
        const double mean = in_means[i];
        if ((mean < bestMean && mean != 0) || i == 0) {
            bestPose = (uint16_t)i;
            bestMean = (uint16_t)mean;
        }
    }
    if (bestMean <= correctEstimateTreshold && !in_means.empty()) {
        in_bestPose = bestPose;
        return true;
    }
    return false;
}

inline bool HighLevelLinemodIcp::estimateBestMatch(const uint16_t* in_depthImg, const std::vector<ObjectPose>& in_poses, const SoftRender& in_render,
                                            uint16_t in_modelIndice, uint16_t& in_bestPose) {
    std::vector<double> means(in_poses.size());
    for (size_t i = 0; i < in_poses.size(); ++i) means[i] = meanDepthDifference(in_depthImg, in_poses[i], in_render, in_modelIndice);
    return selectBestMatch(means, in_bestPose);
}

inline bool HighLevelLinemodIcp::meanDepthDifferencesGpu(const uint16_t* in_depthImg, int in_width, int in_height, const std::vector<ObjectPose>& in_poses,
                                                  const SoftRender& in_render, uint16_t in_modelIndice, std::vector<double>& out_means) {
    error.clear();
    out_means.assign(in_poses.size(), 0.0);
    if (in_poses.empty()) return true;
    std::vector<lm_icp_verify_query> q(in_poses.size());
    for (size_t i = 0; i < q.size(); ++i) {
        q[i].frame = 0;
        q[i].mesh_idx = in_modelIndice;
        const Mat4 view = icp_view_matrix(in_poses[i]);
        in_render.view_proj_of(view.m, q[i].view_proj);
    }
    std::vector<lm_icp_verify_result> r(q.size());
    if (lm_stage_icp_verify_host(det, in_depthImg, 1, in_width, in_height, q.data(), (int)q.size(), sceneMinDepth, r.data()) != LM_OK) {
        error = lm_last_error();
        return false;
    }
    for (size_t i = 0; i < r.size(); ++i) out_means[i] = r[i].mean;
    return true;
}

inline bool HighLevelLinemodIcp::registerToSceneSlots(std::vector<SlotGroup>& in_groups, int w, int h, const CameraParameters& in_cam,
                                                      std::vector<int32_t>& out_status) {
    error.clear();
    out_status.assign(in_groups.size(), LM_OK);
    if (in_groups.empty()) return true;
    std::vector<int32_t> slots(in_groups.size());
    std::vector<lm_icp_query> q(in_groups.size());
    std::vector<double> P;
    for (size_t g = 0; g < in_groups.size(); ++g) {
        const SlotGroup& e = in_groups[g];
        const int x0 = std::max(e.boundingBox.x, 0), y0 = std::max(e.boundingBox.y, 0);
        const int x1 = std::min(e.boundingBox.x + e.boundingBox.width, w), y1 = std::min(e.boundingBox.y + e.boundingBox.height, h);
        slots[g] = e.slot;
        q[g] = lm_icp_query{};
        q[g].x = x0; q[g].y = y0; q[g].width = std::max(x1 - x0, 0); q[g].height = std::max(y1 - y0, 0);
        q[g].class_idx = e.modelNumber;
        q[g].first_pose = (int)(P.size() / 16); q[g].num_poses = (int)e.poses->size();
        q[g].fx = in_cam.fx; q[g].fy = in_cam.fy; q[g].cx = 0.5 * w; q[g].cy = 0.5 * h;
        P.resize(P.size() + 16 * e.poses->size());
        for (size_t i = 0; i < e.poses->size(); ++i) pose_to_matrix((*e.poses)[i], &P[16 * ((size_t)q[g].first_pose + i)]);
    }
    if (P.empty()) P.resize(16);      // (groups without poses: the call still wants a pose array)
    std::vector<int32_t> status(in_groups.size(), -1);
    const int rc = lm_icp_refine_slots(det, slots.data(), q.data(), (int)q.size(), &params, P.data(), status.data());
    if (rc != LM_OK && status[0] == -1) { error = lm_last_error(); return false; }      // refused: the statuses are untouched
    if (rc == LM_ERR_HIP) { error = lm_last_error(); return false; }
    out_status = status;
    for (size_t g = 0; g < in_groups.size(); ++g) {
        if (status[g] != LM_OK) continue;
        for (size_t i = 0; i < in_groups[g].poses->size(); ++i) matrix_to_pose(&P[16 * ((size_t)q[g].first_pose + i)], (*in_groups[g].poses)[i]);
    }
    return true;
}

inline bool HighLevelLinemodIcp::meanDepthDifferencesSlots(const std::vector<SlotGroup>& in_groups, const SoftRender& in_render,
                                                           std::vector<std::vector<double>>& out_means) {
    error.clear();
    out_means.assign(in_groups.size(), std::vector<double>());
    std::vector<lm_icp_verify_query> q;
    for (const SlotGroup& e : in_groups)
        for (const ObjectPose& p : *e.poses) {
            lm_icp_verify_query v{};
            v.frame = e.slot;
            v.mesh_idx = e.modelNumber;
            const Mat4 view = icp_view_matrix(p);
            in_render.view_proj_of(view.m, v.view_proj);
            q.push_back(v);
        }
    if (q.empty()) return true;
    std::vector<lm_icp_verify_result> r(q.size());
    if (lm_icp_verify(det, q.data(), (int)q.size(), sceneMinDepth, r.data()) != LM_OK) { error = lm_last_error(); return false; }
    size_t k = 0;
    for (size_t g = 0; g < in_groups.size(); ++g)
        for (size_t i = 0; i < in_groups[g].poses->size(); ++i) out_means[g].push_back(r[k++].mean);
    return true;
}

inline bool HighLevelLinemodIcp::estimateBestMatchGpu(const uint16_t* in_depthImg, const std::vector<ObjectPose>& in_poses, const SoftRender& in_render,
                                               uint16_t in_modelIndice, uint16_t& in_bestPose) {
    std::vector<double> means;
    if (!meanDepthDifferencesGpu(in_depthImg, in_render.width, in_render.height, in_poses, in_render, in_modelIndice, means)) return false;
    return selectBestMatch(means, in_bestPose);
}

}  // namespace lmamd
