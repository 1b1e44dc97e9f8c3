"""numpy restatement of the ICP pose refinement contract: the scene cloud of prepareDepthForIcp, the model
cloud of loadModels and ICP(iterations, tolerance, rejection_scale, levels)::registerModelToScene.  float32 exactly where the
contract says float (scene positions, neighbour distances of the normals, the 1-NN distances fed to the median), float64
everywhere else.  Test infrastructure only: the product runs this on the GPU (csrc/lm_k_icp.hip)."""
from dataclasses import dataclass

import numpy as np

MAD_SCALE = 1.48257968
FVAL_START = 9999999999.0


@dataclass(frozen=True)
class Rules:
    """The contract's selection and tie rules.  The defaults are the contract; the other values exist so that a
    test can show that flipping one rule moves the result by more than the GPU tests' tolerance (tests/test_icp_cpu.py)."""
    median: str = "lower"          # "lower": element (m - 1) // 2 of the sorted distances; "upper": element m // 2
    threshold: str = "<"           # rejection: keep d < thr; "<=" keeps d == thr too
    picky_tie: str = "lower"       # picky step: equal d on one dst point goes to the lower src index; "higher"
    nn_tie: str = "lower"          # 1-NN: equal distance goes to the lower dst index; "higher"
    knn_tie: str = "lower"         # 12-NN of the normals: equal distance goes to the lower index; "higher"


CONTRACT = Rules()


def box_blur3(depth):
    """3x3 box blur of a uint16 frame, border REFLECT_101, (sum + 4) // 9 per pixel."""
    d = np.pad(depth.astype(np.int64), 1, mode="reflect")     # numpy 'reflect' = OpenCV BORDER_REFLECT_101
    h, w = depth.shape
    s = sum(d[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return (s + 4) // 9


def scene_points(depth, K, bbox, step):
    """Steps 1-4 of the scene cloud: float32 (n, 3) positions in the bbox's row-major order, filtered and subsampled."""
    fx, fy, cx, cy = (np.float32(k) for k in K)
    x0, y0, bw, bh = bbox
    z = box_blur3(depth)[y0:y0 + bh, x0:x0 + bw].astype(np.float32)
    v, u = np.mgrid[y0:y0 + bh, x0:x0 + bw]
    u = u.astype(np.float32)
    v = v.astype(np.float32)
    x = ((u - cx) / fx) * z
    y = ((v - cy) / fy) * z
    x[z == 0] = 0
    y[z == 0] = 0
    pts = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)
    mean = pts[:, 2].astype(np.float64).sum() / len(pts)
    pts = pts[~(np.abs(pts[:, 2].astype(np.float64) - mean) > 300.0)]
    return subsample(pts, step)


def subsample(rows, step):
    """Rows 0, step, 2 step, ... up to len(rows) // step rows (samplePCUniform / loadModels)."""
    n = len(rows) // step
    return rows[:n * step:step][:n] if n else rows[:0]


def knn12(pts, k=12, chunk=512, rules=CONTRACT):
    """Indices of each point's k nearest neighbours (itself included) by float32 squared distance, ties to the lower index
    (rules.knn_tie); and the k-th and (k+1)-th distances."""
    n = len(pts)
    kk = min(k, n)
    idx = np.zeros((n, kk), np.int64)
    dk = np.zeros(n, np.float32)
    dk1 = np.full(n, np.inf, np.float32)
    for a in range(0, n, chunk):
        p = pts[a:a + chunk]
        dx = pts[None, :, 0] - p[:, None, 0]
        dy = pts[None, :, 1] - p[:, None, 1]
        dz = pts[None, :, 2] - p[:, None, 2]
        d = dx * dx + dy * dy + dz * dz
        m = min(kk + 1, n)
        kth = np.partition(d, m - 1, axis=1)[:, m - 1]
        for r in range(len(p)):
            cand = np.nonzero(d[r] <= kth[r])[0]
            key = cand if rules.knn_tie == "lower" else -cand
            order = cand[np.lexsort((key, d[r, cand]))]
            idx[a + r] = order[:kk]
            dk[a + r] = d[r, order[kk - 1]]
            if len(order) > kk:
                dk1[a + r] = d[r, order[kk]]
    return idx, dk, dk1


def normals(pts, k=12, rules=CONTRACT):
    """Smallest-eigenvalue eigenvector of the mean-centred (float64) covariance of each point's k nearest neighbours, oriented
    towards the camera (n . p <= 0)."""
    idx, dk, dk1 = knn12(pts, k, rules=rules)
    P = pts.astype(np.float64)[idx]                       # (n, k, 3)
    c = P - P.mean(1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", c, c)
    _, vec = np.linalg.eigh(cov)
    nrm = vec[:, :, 0]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    flip = (nrm * pts.astype(np.float64)).sum(1) > 0
    nrm[flip] *= -1
    return nrm, dk, dk1


def scene_cloud(depth, K, bbox, step, rules=CONTRACT):
    """prepareDepthForIcp: (n, 6) float32 [x y z nx ny nz]."""
    pts = scene_points(depth, K, bbox, step)
    if len(pts) == 0:
        return np.zeros((0, 6), np.float32)
    nrm, _, _ = normals(pts, rules=rules)
    return np.concatenate([pts, nrm.astype(np.float32)], 1)


def cv_round(x):
    return int(np.rint(x))                                # half to even, like cvRound


def level_schedule(n, levels=8, iterations=6, tolerance=0.1):
    """(level, s, maxIt, iterations that can run) from the coarsest level down.  fval_perc starts at 0, so the loop condition
    !(fval_perc < 1 + TolP && fval_perc > 1 - TolP) holds only while TolP <= 1: levels with TolP > 1 never iterate."""
    out = []
    for level in range(levels - 1, -1, -1):
        num = max(cv_round(n / float(1 << level)), 1)     # (choice) at least one sample
        s = cv_round(n / float(num))
        tolp = tolerance * (level + 1) ** 2
        max_it = cv_round(iterations / float(level + 1))
        out.append((level, s, max_it, max_it if tolp <= 1.0 else 0, tolp))   # (level, s, maxIt, rounds, TolP)
    return out


def transform(M, X):
    """M (4x4) applied to (n, 6) rows: positions rotated and translated, normals rotated.  Explicit left-to-right sums."""
    R, t = M[:3, :3], M[:3, 3]
    out = np.empty_like(X)
    for r in range(3):
        out[:, r] = R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1] + R[r, 2] * X[:, 2] + t[r]
        out[:, 3 + r] = R[r, 0] * X[:, 3] + R[r, 1] * X[:, 4] + R[r, 2] * X[:, 5]
    return out


def euler_pose(x):
    rx, ry, rz = x[:3]
    cx_, sx = np.cos(rx), np.sin(rx)
    cy_, sy = np.cos(ry), np.sin(ry)
    cz, sz = np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]])
    Ry = np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rz @ Ry @ Rx
    M[:3, 3] = x[3:]
    return M


def lower_median(v, rules=CONTRACT):
    s = np.sort(v, kind="stable")
    return s[(len(s) - 1) // 2 if rules.median == "lower" else len(s) // 2]


def nearest(moved, dstp, rules=CONTRACT):
    """1-NN of each moved point among dstp by float64 squared distance, ties to the lower index (rules.nn_tie); distances returned
    as float32."""
    idx = np.zeros(len(moved), np.int64)
    dd = np.zeros(len(moved))
    for a in range(0, len(moved), 1024):
        m = moved[a:a + 1024]
        dx = m[:, None, 0] - dstp[None, :, 0]
        dy = m[:, None, 1] - dstp[None, :, 1]
        dz = m[:, None, 2] - dstp[None, :, 2]
        d = dx * dx + dy * dy + dz * dz
        if rules.nn_tie == "lower":
            j = np.argmin(d, axis=1)                      # first minimum = lower index
        else:
            j = d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)
        idx[a:a + 1024] = j
        dd[a:a + 1024] = d[np.arange(len(m)), j]
    return idx, dd.astype(np.float32)


def select_pairs(d, nn, rejection_scale, rules=CONTRACT):
    """Rejection by the lower median and the MAD, then the picky step: per dst point the smallest d, ties to the lower src index.
    Returns (src indices, dst indices) in ascending src order."""
    med = lower_median(d, rules)
    mad = lower_median(np.abs(d - med), rules)
    thr = float(rejection_scale) * MAD_SCALE * float(mad) + float(med)
    d64 = d.astype(np.float64)
    keep = np.nonzero(d64 < thr if rules.threshold == "<" else d64 <= thr)[0]
    best = {}
    for i in keep:                                        # ascending src index: a later equal d never replaces (picky_tie "lower")
        j = int(nn[i])
        if j not in best or d[i] < d[best[j]] or (rules.picky_tie == "higher" and d[i] == d[best[j]]):
            best[j] = i
    src = np.array(sorted(best.values()), np.int64)
    return src, nn[src]


def point_to_plane(S, D):
    """Least squares of [s x n, n] x = (d - s) . n over the pairs (s from srcL, n the dst normal); None when singular."""
    s, n, d = S[:, :3], D[:, 3:], D[:, :3]
    A = np.concatenate([np.cross(s, n), n], 1)
    b = ((d - s) * n).sum(1)
    try:
        x = np.linalg.solve(A.T @ A, A.T @ b)
    except np.linalg.LinAlgError:
        return None
    return None if np.isnan(x).any() else x


def icp_register(model, scene, P, iterations=6, tolerance=0.1, rejection_scale=2.5, levels=8, trace=None, rules=CONTRACT):
    """registerModelToScene for one pose P (4x4): returns the refined 4x4.  model, scene: (n, 6) float32.  trace, if a list,
    receives (level, iterations run) per level.  rules: the selection and tie rules (the contract's by default)."""
    P = np.asarray(P, np.float64)
    src = transform(P, model.astype(np.float64))
    dst = scene.astype(np.float64).copy()
    n = len(src)
    mean_avg = 0.5 * (src[:, :3].mean(0) + dst[:, :3].mean(0))
    src[:, :3] -= mean_avg
    dst[:, :3] -= mean_avg
    scale = n / (0.5 * (np.linalg.norm(src[:, :3], axis=1).sum() + np.linalg.norm(dst[:, :3], axis=1).sum()))
    src[:, :3] *= scale
    dst[:, :3] *= scale
    pose = np.eye(4)
    for level, s, max_it, runs, tolp in level_schedule(n, levels, iterations, tolerance):
        srcL = subsample(transform(pose, src), s)
        dstL = subsample(dst, s)
        posex = np.eye(4)
        fval_old, fval_perc, it = FVAL_START, 0.0, 0
        moved = srcL
        if len(srcL) < 6 or len(dstL) < 6:               # fewer than 6 pairs possible: the first round would stop the level
            runs = 0
        while runs and not (fval_perc < 1 + tolp and fval_perc > 1 - tolp) and it < max_it:
            nn, d = nearest(moved[:, :3], dstL[:, :3], rules)
            si, di = select_pairs(d, nn, rejection_scale, rules)
            if len(si) < 6:
                break
            x = point_to_plane(srcL[si], dstL[di])
            if x is None:
                break
            posex = euler_pose(x)
            moved = transform(posex, srcL)
            fval = np.sqrt(((srcL[si] - dstL[di]) ** 2).sum()) / len(moved)
            fval_perc = fval / fval_old
            fval_old = fval
            it += 1
        if trace is not None:
            trace.append((level, it))
        pose = posex @ pose
    R, t = pose[:3, :3], pose[:3, 3] / scale + mean_avg - pose[:3, :3] @ mean_avg
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R, t
    return out @ P


def rotation_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1)))


def render_depth(vertices, faces, pose, K, w, h):
    """Minimal z-buffer of a triangle mesh (mm, pinhole K = (fx, fy, cx, cy)): uint16 depth, 0 where empty.  Test scenes only."""
    fx, fy, cx, cy = K
    V = vertices.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
    uv = np.stack([V[:, 0] / V[:, 2] * fx + cx, V[:, 1] / V[:, 2] * fy + cy], 1)
    zb = np.full((h, w), np.inf)
    for f in faces:
        a, b, c = uv[f]
        za, zb_, zc = V[f, 2]
        lo = np.floor(np.minimum(np.minimum(a, b), c)).astype(int)
        hi = np.ceil(np.maximum(np.maximum(a, b), c)).astype(int)
        x0, y0 = max(lo[0], 0), max(lo[1], 0)
        x1, y1 = min(hi[0], w - 1), min(hi[1], h - 1)
        if x0 > x1 or y0 > y1:
            continue
        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        px, py = xx + 0.5, yy + 0.5
        den = (b[1] - c[1]) * (a[0] - c[0]) + (c[0] - b[0]) * (a[1] - c[1])
        if abs(den) < 1e-12:
            continue
        l0 = ((b[1] - c[1]) * (px - c[0]) + (c[0] - b[0]) * (py - c[1])) / den
        l1 = ((c[1] - a[1]) * (px - c[0]) + (a[0] - c[0]) * (py - c[1])) / den
        l2 = 1 - l0 - l1
        inside = (l0 >= 0) & (l1 >= 0) & (l2 >= 0)
        if not inside.any():
            continue
        z = 1.0 / (l0 / za + l1 / zb_ + l2 / zc)
        sub = zb[y0:y1 + 1, x0:x1 + 1]
        upd = inside & (z < sub)
        sub[upd] = z[upd]
    out = np.where(np.isfinite(zb), np.rint(zb), 0)
    return out.astype(np.uint16)
