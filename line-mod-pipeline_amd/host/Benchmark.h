// Benchmark.h -- the reference pipeline's accuracy harness (Benchmark.cpp:11-245, utility.cpp:99-127) over the C ABI: the Hodan error
// (calculateErrorHodan), ADD (calculateErrorLM) and ADD-S (calculateErrorLMAmbigous) run on the GPU (lm_pose_error_vsd /
// lm_pose_error_add), the ground-truth readers on the host.  Header-only (like HighLevelLinemodIcp.h): a program
// built from the host sources as before (HighLevelLinemod, PostProcess, TemplateGenerator, PoseDetection) links without another file.
// The renders are those of SoftRender (projection) under the reference's calculateViewMat, drawn by the GPU rasteriser, which draws what
// SoftRender::render_view draws bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "HighLevelLinemod.h"
#include "PostProcess.h"
#include "TemplateGenerator.h"

namespace lmamd {

// glm::eulerAngles(q) = (pitch, yaw, roll) and glm::qua<float>(vec3 eulerAngles)  (glm/gtc/quaternion.inl), in float
inline Vec3 glm_euler_angles(const Quat& q) {
    const float y = 2.f * (q.y * q.z + q.w * q.x), x = q.w * q.w - q.x * q.x - q.y * q.y + q.z * q.z;
    Vec3 e;
    e.x = (std::fabs(x) < 1e-12f && std::fabs(y) < 1e-12f) ? 2.f * std::atan2(q.x, q.w) : std::atan2(y, x);
    float s = -2.f * (q.x * q.z - q.w * q.y);
    s = s < -1.f ? -1.f : (s > 1.f ? 1.f : s);
    e.y = std::asin(s);
    e.z = std::atan2(2.f * (q.x * q.y + q.w * q.z), q.w * q.w + q.x * q.x - q.y * q.y - q.z * q.z);
    return e;
}
inline Quat glm_quat_from_euler(const Vec3& e) {
    const float cx = std::cos(e.x * 0.5f), cy = std::cos(e.y * 0.5f), cz = std::cos(e.z * 0.5f);
    const float sx = std::sin(e.x * 0.5f), sy = std::sin(e.y * 0.5f), sz = std::sin(e.z * 0.5f);
    Quat q;
    q.w = cx * cy * cz + sx * sy * sz;
    q.x = sx * cy * cz - cx * sy * sz;
    q.y = cx * sy * cz + sx * cy * sz;
    q.z = cx * cy * sz - sx * sy * cz;
    return q;
}

// Benchmark::calculateViewMat (:165-170): euler angles (x - pi, -y, -z), pi in double as M_PI, and the translation (t.x, -t.y, -t.z)
// as OpenglRender::renderDepthToFrontBuff(indice, rotMat, traVec) sets it.  (Not the +pi of HighLevelLinemodIcp's render.)
inline Mat4 benchmark_view_mat(const ObjectPose& p) {
    const Vec3 e = glm_euler_angles(p.quaternions);
    Mat4 v = toMat4(glm_quat_from_euler(Vec3{(float)((double)e.x - 3.14159265358979323846), -e.y, -e.z}));
    v.m[3][0] = p.translation.x; v.m[3][1] = -p.translation.y; v.m[3][2] = -p.translation.z; v.m[3][3] = 1.0f;
    return v;
}

// glm::toMat3(q), row-major (fromGLM2CV)
inline void pose_rotation_rows(const Quat& q, float R[9]) {
    const Mat4 m = toMat4(q);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = m.m[c][r];
}

// One (frame, estimate, ground truth) triple of Benchmark::evaluate.
struct BenchmarkQuery {
    int frame = 0;
    ObjectPose estimate, groundTruth;
    uint16_t modelIndex = 0;
};

class Benchmark {
public:
    // det: the detector whose GPU evaluates (lm_pose_error_*); cam: the SoftRender camera of the renders
    Benchmark(lm_detector* in_detector, const CameraParameters& in_cam) : det(in_detector), render(in_cam) {}

    // loadModel (:77-82): the model of ADD / ADD-S.  Keeps the mesh resident as render mesh in_meshIndex (lm_set_render_mesh), which is
    // also the model index calculateErrorHodan renders.  ADD reads every vertex, ADD-S every subsampleStep-th (subsamplingModel).
    bool loadModel(const Mesh& in_mesh, uint16_t in_meshIndex = 0) {
        std::vector<float> xyz(in_mesh.vertices.size() * 3);
        for (size_t i = 0; i < in_mesh.vertices.size(); ++i) {
            xyz[3 * i] = in_mesh.vertices[i].x; xyz[3 * i + 1] = in_mesh.vertices[i].y; xyz[3 * i + 2] = in_mesh.vertices[i].z;
        }
        if (lm_set_render_mesh(det, in_meshIndex, xyz.data(), (int)in_mesh.vertices.size(), in_mesh.indices.data(), (int)in_mesh.indices.size()) != LM_OK)
            return setError(lm_last_error());
        modelIndex = in_meshIndex;
        return true;
    }
    bool loadModel(const std::string& in_modelLocation, uint16_t in_meshIndex = 0) {
        Mesh m;
        std::string err;
        if (!load_ply_ascii(in_modelLocation, m, &err)) return setError("cannot read the model " + in_modelLocation + ": " + err);
        return loadModel(m, in_meshIndex);
    }

    // :18-38: the ground truth pose<imageCounter>.yml of groundTruthFolder against in_estimatePose on the (principal-point-shifted)
    // depth image; counts a correct pose below 0.3.  NaN, with lastError(), when the ground truth cannot be read or the call fails.
    float calculateErrorHodan(const uint16_t* in_depthImg, int in_width, int in_height, const ObjectPose& in_estimatePose, uint16_t in_modelIndice) {
        ObjectPose gt;
        if (!readGroundTruthPose(groundTruthFolder + "pose" + std::to_string(imageCounter) + ".yml", gt)) return nan();
        std::vector<lm_vsd_result> r;
        if (!evaluate(in_depthImg, 1, in_width, in_height, {BenchmarkQuery{0, in_estimatePose, gt, in_modelIndice}}, r)) return nan();
        last = r[0];
        if (r[0].error < 0.3f) hodanCounter++;
        return r[0].error;
    }
    // :40-75 and :84-131 (ground truth tra<imageCounter>.tra / rot<imageCounter>.rot of linemodFolder); a mean <= objectDiameter counts
    float calculateErrorLM(const ObjectPose& in_estimate) { return errorLM(in_estimate, false); }
    float calculateErrorLMAmbigous(const ObjectPose& in_estimate) { return errorLM(in_estimate, true); }

    // :11-16
    void increaseImgCounter() {
        imageCounter++;
        std::printf("Hodan Score: %g Counter: %d            \n", hodanScore(), imageCounter);
    }
    float hodanScore() const { return (float)hodanCounter * 100 / (float)imageCounter; }
    float lmScore() const { return (float)lineCounter * 100 / (float)imageCounter; }

    // Batched Hodan errors: frames = n_frames depth images (w x h), one result per query (the counters are not touched).
    bool evaluate(const uint16_t* in_frames, int in_nFrames, int in_width, int in_height, const std::vector<BenchmarkQuery>& in_queries,
                  std::vector<lm_vsd_result>& out) {
        std::vector<lm_vsd_query> q(in_queries.size());
        for (size_t k = 0; k < q.size(); ++k) {
            q[k].frame = in_queries[k].frame;
            q[k].mesh_idx = in_queries[k].modelIndex;
            viewProj(in_queries[k].groundTruth, q[k].view_proj_gt);
            viewProj(in_queries[k].estimate, q[k].view_proj_est);
        }
        out.assign(q.size(), lm_vsd_result{});
        if (lm_pose_error_vsd(det, in_frames, in_nFrames, in_width, in_height, q.data(), (int)q.size(), visibilityThreshold, errorThreshold,
                              out.data()) != LM_OK)
            return setError(lm_last_error());
        return true;
    }
    // Batched ADD (symmetric false, every vertex) / ADD-S (every subsampleStep-th vertex) of the loaded model: one mean per query.
    bool evaluateLM(const std::vector<BenchmarkQuery>& in_queries, bool in_symmetric, std::vector<float>& out) {
        std::vector<lm_add_query> q(in_queries.size());
        for (size_t k = 0; k < q.size(); ++k) {
            const BenchmarkQuery& b = in_queries[k];
            pose_rotation_rows(b.groundTruth.quaternions, q[k].R_gt);
            pose_rotation_rows(b.estimate.quaternions, q[k].R_est);
            q[k].t_gt[0] = b.groundTruth.translation.x; q[k].t_gt[1] = b.groundTruth.translation.y; q[k].t_gt[2] = b.groundTruth.translation.z;
            q[k].t_est[0] = b.estimate.translation.x; q[k].t_est[1] = b.estimate.translation.y; q[k].t_est[2] = b.estimate.translation.z;
        }
        out.assign(q.size(), 0.f);
        if (lm_pose_error_add(det, modelIndex, in_symmetric ? (int)subsampleStep : 1, in_symmetric ? 1 : 0, q.data(), (int)q.size(), out.data(),
                              nullptr) != LM_OK)
            return setError(lm_last_error());
        return true;
    }

    // projection * calculateViewMat(pose) (Mat4 order): what the GPU renders a pose with
    void viewProj(const ObjectPose& in_pose, float out[16]) const {
        const Mat4 v = benchmark_view_mat(in_pose);
        render.view_proj_of(v.m, out);
    }

    // :180-194: rotMat (!!opencv-matrix, 3 x 3) and position of a cv::FileStorage file; the quaternion is toQuat(rotMat)
    bool readGroundTruthPose(const std::string& in_path, ObjectPose& out) {
        double R[9], t[3];
        size_t n = 0;
        if (lm_yaml_numbers(in_path.c_str(), "rotMat", R, 9, &n) != LM_OK || n != 9) return setError("ground truth " + in_path + ": " + lm_last_error());
        if (lm_yaml_numbers(in_path.c_str(), "position", t, 3, &n) != LM_OK || n != 3) return setError("ground truth " + in_path + ": " + lm_last_error());
        Mat4 m;
        std::memset(m.m, 0, sizeof(m.m));
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) m.m[c][r] = (float)R[3 * r + c];
        m.m[3][3] = 1.f;
        out.quaternions = toQuat(m);
        out.translation = Vec3{(float)t[0], (float)t[1], (float)t[2]};
        return true;
    }
    // :196-245: two numbers skipped in each file, the translation x 10 (cm -> mm), quat_cast of the rotation, then the euler
    // adjustment (x - pi / 2, y, z), pi in double as M_PI
    bool readGroundTruthLinemodDataset(const std::string& in_traPath, const std::string& in_rotPath, ObjectPose& out) {
        std::ifstream ft(in_traPath), fr(in_rotPath);
        if (!ft.is_open()) return setError("cannot open the ground truth translation " + in_traPath);
        if (!fr.is_open()) return setError("cannot open the ground truth rotation " + in_rotPath);
        double skip;
        float t[3];
        if (!(ft >> skip >> skip >> t[0] >> t[1] >> t[2])) return setError("ground truth translation " + in_traPath + ": fewer than 5 numbers");
        double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, v;
        int cnt = 0;
        if (!(fr >> skip >> skip)) return setError("ground truth rotation " + in_rotPath + ": fewer than 2 numbers");
        while (cnt < 9 && fr >> v) R[cnt++] = v;
        if (cnt < 9) return setError("ground truth rotation " + in_rotPath + ": fewer than 9 matrix entries");
        Mat4 m;
        std::memset(m.m, 0, sizeof(m.m));
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) m.m[c][r] = (float)R[3 * r + c];
        m.m[3][3] = 1.f;
        const Vec3 e = glm_euler_angles(toQuat(m));
        out.quaternions = glm_quat_from_euler(Vec3{(float)((double)e.x - 3.14159265358979323846 / 2), e.y, e.z});
        out.translation = Vec3{t[0] * 10, t[1] * 10, t[2] * 10};
        return true;
    }
    // utility.cpp:99-127 loadDepthLineModDataset: int32 rows, int32 cols, then rows x cols uint16 samples
    bool loadDepthLineModDataset(const std::string& in_path, std::vector<uint16_t>& out, int& rows, int& cols) {
        std::ifstream f(in_path, std::ios::binary);
        if (!f.is_open()) return setError("cannot open the depth file " + in_path);
        int32_t hdr[2];
        if (!f.read(reinterpret_cast<char*>(hdr), sizeof(hdr)) || hdr[0] < 0 || hdr[1] < 0) return setError("depth file " + in_path + ": bad header");
        rows = hdr[0]; cols = hdr[1];
        out.assign((size_t)rows * cols, 0);
        if (!f.read(reinterpret_cast<char*>(out.data()), (std::streamsize)(out.size() * sizeof(uint16_t))))
            return setError("depth file " + in_path + ": fewer samples than rows x cols");
        return true;
    }

    const std::string& lastError() const { return error; }
    const lm_vsd_result& lastCounts() const { return last; }   // the counts of the last calculateErrorHodan

    std::string groundTruthFolder = "benchmark/";          // pose<N>.yml (readGroundTruthPose)
    std::string linemodFolder = "benchmarkLINEMOD/";       // tra<N>.tra, rot<N>.rot (readGroundTruthLinemodDataset)
    int32_t imageCounter = 0, hodanCounter = 0, lineCounter = 0;
    uint32_t subsampleStep = 40;
    int32_t visibilityThreshold = 15;   // delta, mm (BOP)
    int32_t errorThreshold = 20;        // tau, mm (BOP)
    // The reference's header calls this the object's diameter in cm, but calculateErrorLM compares it with a mean distance in mm (the
    // vertices and translations are mm): kept as the reference has it, 21, compared with the mm mean.
    float objectDiameter = 21;

private:
    lm_detector* det;
    SoftRender render;
    uint16_t modelIndex = 0;
    lm_vsd_result last{};
    std::string error;

    bool setError(const std::string& e) { error = e; return false; }
    static float nan() { return std::numeric_limits<float>::quiet_NaN(); }
    float errorLM(const ObjectPose& in_estimate, bool in_symmetric) {
        ObjectPose gt;
        const std::string n = std::to_string(imageCounter);
        if (!readGroundTruthLinemodDataset(linemodFolder + "tra" + n + ".tra", linemodFolder + "rot" + n + ".rot", gt)) return nan();
        std::vector<float> mean;
        if (!evaluateLM({BenchmarkQuery{0, in_estimate, gt, modelIndex}}, in_symmetric, mean)) return nan();
        if (mean[0] <= objectDiameter) lineCounter++;
        return mean[0];
    }
};

}  // namespace lmamd
