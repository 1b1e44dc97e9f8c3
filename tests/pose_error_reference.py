"""numpy restatement of the reference's Benchmark.cpp: the Hodan error's pixel rules (calculateVisibilityMasks, calculateErrorHodan on
CV_16U data), ADD / ADD-S per vertex under DESIGN.md section 11's float32 contract, the means, the view matrix (calculateViewMat) and
the ground-truth readers (readGroundTruthPose, readGroundTruthLinemodDataset, utility.cpp's loadDepthLineModDataset)."""
import math
import re

import numpy as np

F = np.float32


def vsd_masks(gt, est, scene, delta=15, tau=20):
    """The seven masks of calculateVisibilityMasks / calculateErrorHodan on uint16 images: saturating subtractions, occluded where
    render - scene > delta, rendered where render > 1, the `gtVisibility & estimateDepthRender` quirk, |gt - est| <= tau."""
    g, e, d = (np.asarray(a, np.int64) for a in (gt, est, scene))
    rg, re_ = g > 1, e > 1
    vg = rg & ~(np.maximum(g - d, 0) > delta)
    ve = (re_ & ~(np.maximum(e - d, 0) > delta)) | (vg & (e != 0))
    inter = vg & ve
    within = inter & (np.abs(g - e) <= tau)
    return rg, re_, vg, ve, inter, vg | ve, within


# (gt, est, scene) -> the seven counts at delta 15, tau 20; each row pins one edge of the rules
EDGE_CASES = [
    ("render 0", (0, 0, 0), (0, 0, 0, 0, 0, 0, 0)),
    ("render 1 is not rendered", (1, 1, 1000), (0, 0, 0, 0, 0, 0, 0)),
    ("render 2 is rendered", (2, 2, 1000), (1, 1, 1, 1, 1, 1, 1)),
    ("render - scene 15 is visible", (1015, 1015, 1000), (1, 1, 1, 1, 1, 1, 1)),
    ("render - scene 16 is occluded", (1016, 1016, 1000), (1, 1, 0, 0, 0, 0, 0)),
    ("|gt - est| 20 is within", (1000, 1020, 1010), (1, 1, 1, 1, 1, 1, 1)),
    ("|gt - est| 21 is not", (1000, 1021, 1010), (1, 1, 1, 1, 1, 1, 0)),
    ("scene 0 occludes a render", (500, 500, 0), (1, 1, 0, 0, 0, 0, 0)),
    ("scene 0 under a render of 15", (15, 15, 0), (1, 1, 1, 1, 1, 1, 1)),
    ("gt & est quirk: occluded estimate", (1000, 1100, 1000), (1, 1, 1, 1, 1, 1, 0)),
    ("gt & est quirk: estimate render 1", (1000, 1, 1000), (1, 0, 1, 1, 1, 1, 0)),
    ("estimate alone visible", (0, 1000, 1000), (0, 1, 0, 1, 0, 1, 0)),
    ("saturation: render below the scene", (10, 40000, 65535), (1, 1, 1, 1, 1, 1, 0)),
]


def vsd_counts(gt, est, scene, delta=15, tau=20):
    """(counts in lm_vsd_result order, error as float32: 1 - within / union, NaN for an empty union)"""
    c = [int(m.sum()) for m in vsd_masks(gt, est, scene, delta, tau)]
    with np.errstate(invalid="ignore", divide="ignore"):
        err = F(1) - F(c[6]) / F(c[5])
    return c, err


def transform(R, t, v):
    """R v + t in float32, row-major R, left to right: ((R0 x + R1 y) + R2 z) + t"""
    R = np.asarray(R, F).reshape(9)
    t = np.asarray(t, F).reshape(3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([R[3 * r] * x + R[3 * r + 1] * y + R[3 * r + 2] * z + t[r] for r in range(3)], axis=1)


def sq_len(a, b):
    d = a - b
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def add_per_vertex(vertices, step, R_gt, t_gt, R_est, t_est):
    v = np.asarray(vertices, F)[::step]
    return np.sqrt(sq_len(transform(R_gt, t_gt, v), transform(R_est, t_est, v)))


def adds_per_vertex(vertices, step, R_gt, t_gt, R_est, t_est, block=512):
    """For each GT vertex the smallest distance to any estimate vertex, never above the reference's start 999999."""
    v = np.asarray(vertices, F)[::step]
    g, e = transform(R_gt, t_gt, v), transform(R_est, t_est, v)
    out = np.empty(len(g), F)
    for i in range(0, len(g), block):
        s = sq_len(g[i:i + block, None, :], e[None, :, :])
        with np.errstate(invalid="ignore"):
            m = np.sqrt(np.nanmin(np.where(np.isnan(s), np.inf, s), axis=1))
        out[i:i + block] = np.where(m < F(999999), m, F(999999))
    return out


def mean_of(per_vertex):
    """sum(difference)[0] / numVertices: a double sum, divided, returned as float"""
    return F(np.sum(per_vertex.astype(np.float64)) / len(per_vertex))


# ---- poses and the view matrix (float32, glm's formulas)
def quat_to_mat3(q):
    """glm::mat3_cast of (w, x, y, z), row-major"""
    w, x, y, z = (F(c) for c in q)
    one, two = F(1), F(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], F)


def euler_angles(q):
    w, x, y, z = (float(c) for c in q)
    yy, xx = 2 * (y * z + w * x), w * w - x * x - y * y + z * z
    ex = 2 * math.atan2(x, w) if abs(xx) < 1e-12 and abs(yy) < 1e-12 else math.atan2(yy, xx)
    ey = math.asin(max(-1.0, min(1.0, -2 * (x * z - w * y))))
    ez = math.atan2(2 * (x * y + w * z), w * w + x * x - y * y - z * z)
    return ex, ey, ez


def quat_from_euler(e):
    cx, cy, cz = (math.cos(a * 0.5) for a in e)
    sx, sy, sz = (math.sin(a * 0.5) for a in e)
    return (cx * cy * cz + sx * sy * sz, sx * cy * cz - cx * sy * sz, cx * sy * cz + sx * cy * sz, cx * cy * sz - sx * sy * cz)


def view_mat(q, t):
    """calculateViewMat + renderDepthToFrontBuff's translation: row-major 4x4 of rotation(euler (x - pi, -y, -z)), (t.x, -t.y, -t.z)"""
    ex, ey, ez = euler_angles(q)
    V = np.eye(4, dtype=F)
    V[:3, :3] = quat_to_mat3(quat_from_euler((ex - math.pi, -ey, -ez)))
    V[:3, 3] = [t[0], -t[1], -t[2]]
    return V


def projection(fy=1045.69141, w=640, h=480):
    """SoftRender's glm::perspective(2 atan(h / 2 fy), w / h, 100, 10000), row-major"""
    fovy = 2 * math.atan(h / (2 * fy))
    t = math.tan(fovy / 2)
    P = np.zeros((4, 4), F)
    P[0, 0], P[1, 1] = 1 / ((w / h) * t), 1 / t
    P[2, 2], P[2, 3], P[3, 2] = -(10100.0) / 9900.0, -(2 * 10000.0 * 100.0) / 9900.0, -1
    return P


def view_proj_mat4(P, V):
    """projection * view as the 16 floats of Mat4 (column-major: m[col][row])"""
    return (P.astype(np.float64) @ V.astype(np.float64)).astype(F).T.reshape(16)


# ---- readers
def read_pose_yml(path):
    """readGroundTruthPose: rotMat (!!opencv-matrix data, row-major) and position"""
    text = open(path).read()
    data = re.search(r"rotMat:.*?data:\s*\[(.*?)\]", text, re.S).group(1)
    pos = re.search(r"position:\s*\[(.*?)\]", text, re.S).group(1)
    return np.array([float(v) for v in data.replace("\n", " ").split(",")]).reshape(3, 3), np.array([float(v) for v in pos.split(",")])


def read_linemod_tra_rot(tra_path, rot_path):
    """readGroundTruthLinemodDataset: (rotation matrix before the euler adjustment, adjusted euler angles' source, translation x 10)"""
    tn = open(tra_path).read().split()
    rn = open(rot_path).read().split()
    t = np.array([F(v) for v in tn[2:5]], F) * F(10)
    R = np.array([float(v) for v in rn[2:11]]).reshape(3, 3)
    return R, t


def load_dpt(path):
    """loadDepthLineModDataset: int32 rows, int32 cols, rows x cols uint16"""
    raw = open(path, "rb").read()
    rows, cols = np.frombuffer(raw[:8], np.int32)
    return np.frombuffer(raw[8:8 + 2 * rows * cols], np.uint16).reshape(rows, cols)


def mat3_to_quat(M):
    """quat_cast of a row-major rotation matrix: (w, x, y, z)"""
    m = np.asarray(M, np.float64)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        return (0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s)
    i = int(np.argmax([m[0, 0], m[1, 1], m[2, 2]]))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(1.0 + m[i, i] - m[j, j] - m[k, k]) * 2
    q = [0.0] * 4
    q[0] = (m[k, j] - m[j, k]) / s
    q[1 + i] = 0.25 * s
    q[1 + j] = (m[j, i] + m[i, j]) / s
    q[1 + k] = (m[k, i] + m[i, k]) / s
    return tuple(q)


def linemod_quat(R):
    """readGroundTruthLinemodDataset's rotation: quat_cast, eulerAngles, then (x - pi / 2, y, z) back to a quaternion"""
    ex, ey, ez = euler_angles(mat3_to_quat(R))
    return quat_from_euler((ex - math.pi / 2, ey, ez))
