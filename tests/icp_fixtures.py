"""Inputs for the ICP rule tests (tests/test_icp_cpu.py without a GPU, tests/test_gpu_icp.py on one): dyadic depth frames whose
neighbour distances are exact in float32, so that 12-NN ties are real on both sides; a model made from a scene cloud so that round
one sees one exact distance on every pair; a near scene with holes; and the frame0 cases that pin the median and the picky tie."""
import os

import numpy as np

import icp_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
K0 = (1044.87, 1045.69141, 320.0, 240.0)       # linemod_settings.yml
W, H = 640, 480

# fx = fy = 1024 and an integer principal point: x = ((u - cx) / 1024) z is a multiple of 2^-10 for an integer z, exact in float32
K_DYADIC = (1024.0, 1024.0, 320.0, 240.0)
DYADIC_BBOX = (290, 216, 60, 48)


def dyadic_depth(kind):
    """A 640 x 480 frame of terraces at 1024 + 2k mm.  "steps": vertical steps every 5 columns; "ridge": a stepped ridge, with
    alternating bands of rows; "box": a box 4 mm proud of a banded plane.  The blur mixes the terraces into ramps two pixels wide:
    neighbourhoods that are not planar and that tie."""
    v, u = np.mgrid[0:H, 0:W]
    z = np.full((H, W), 1024, np.int64)
    if kind == "steps":
        z += 2 * ((u // 5) % 3)
    elif kind == "ridge":
        z += 2 * np.minimum(np.abs(u - 320) // 3, 3) + 2 * ((v // 7) % 2)
    elif kind == "box":
        z += np.where((np.abs(u - 320) < 9) & (np.abs(v - 240) < 7), -4, 0) + 2 * ((v // 6) % 2)
    else:
        raise ValueError(kind)
    return z.astype(np.uint16)


def candidate_distances_exact(pts, k=12):
    """True when every pair that can enter a point's k-NN list or tie its (k+1)-th entry (exact float64 distance at most the
    (k+1)-th smallest) has a float32 squared distance equal to the float64 one, and every other pair's float32 distance stays above
    it.  Then no rounding or contraction of the float arithmetic can reorder or untie the neighbour lists."""
    p64 = pts.astype(np.float64)
    n = len(pts)
    kk = min(k, n - 1)
    for a in range(0, n, 512):
        q, q64 = pts[a:a + 512], p64[a:a + 512]
        d32 = (pts[None, :, 0] - q[:, None, 0]) ** 2 + (pts[None, :, 1] - q[:, None, 1]) ** 2 + (pts[None, :, 2] - q[:, None, 2]) ** 2
        d64 = ((p64[None, :, 0] - q64[:, None, 0]) ** 2 + (p64[None, :, 1] - q64[:, None, 1]) ** 2
               + (p64[None, :, 2] - q64[:, None, 2]) ** 2)
        kth = np.partition(d64, kk, axis=1)[:, kk:kk + 1]
        near = d64 <= kth
        if (d32[near].astype(np.float64) != d64[near]).any():
            return False
        if (np.broadcast_to(kth, d64.shape)[~near] >= d32[~near]).any():
            return False
    return True


def eigen_gap_clear(pts, k=12, rel=1e-6):
    """Points whose neighbourhood covariance has its smallest eigenvalue clearly apart from the next: the normal is defined, and any
    eigen-solver agrees on it to rounding."""
    idx, _, _ = R.knn12(pts, k)
    P = pts.astype(np.float64)[idx]
    c = P - P.mean(1, keepdims=True)
    lam = np.linalg.eigvalsh(np.einsum("nki,nkj->nij", c, c))
    return lam[:, 1] - lam[:, 0] > rel * np.maximum(lam[:, 2], 1e-300)


def shifted_model(scene, t):
    """Model rows = the scene's rows moved by t mm along z (exact for the dyadic scenes: z is an integer).  With the identity pose,
    every point's 1-NN is its own scene point (the rows are more than 2 t apart) at one and the same float distance: the median is
    that distance, the MAD is 0 and the rejection threshold equals every d."""
    m = scene.astype(np.float32).copy()
    m[:, 2] += np.float32(t)
    return m


def near_depth():
    """A near frame (mean z of the bbox under 300 mm) with holes: the holes' interior pixels stay 0 after the blur and, being within
    300 mm of the mean, become duplicate (0, 0, 0) points; each hole gives more than 12 of them."""
    v, u = np.mgrid[0:H, 0:W]
    z = 240 + ((u // 4) % 3) + 2 * ((v // 5) % 2) + (np.abs(u - 300) // 7)
    z = z.astype(np.int64)
    for (x0, y0) in [(262, 222), (300, 236), (331, 250)]:
        z[y0:y0 + 9, x0:x0 + 8] = 0
    return z.astype(np.uint16)


NEAR_BBOX = (258, 218, 84, 44)


def frame0():
    f = np.load(os.path.join(GOLDEN, "frame0.npz"))
    return f["bgr"], f["depth"]


def mesh_model():
    m = np.load(os.path.join(GOLDEN, "lagergehaeuse.npz"))
    xyzn = np.load(os.path.join(GOLDEN, "lagergehaeuse_normals.npz"))["xyzn"]
    U, _, Vt = np.linalg.svd(m["gt_rotation"])
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = U @ Vt, m["gt_position"]
    return m["vertices"], m["faces"], xyzn, G


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    M = np.eye(4)
    M[i, i] = M[j, j] = c
    M[i, j], M[j, i] = -s, s
    return M


def perturbed(G, axis, deg, dt):
    P = G @ rot(axis, deg)
    P[:3, 3] += dt
    return P


def frame0_rule_cases(G):
    """frame0 cases whose refined pose moves by far more than the GPU tolerance when one rule of the reference is flipped (checked in
    tests/test_icp_cpu.py).  The model is the mesh cloud at model_step: it has rows at one position with different normals, so two
    src rows tie exactly on d and the picky winner changes fval, hence where a level stops.  (name, bbox, model_step, pose, params,
    the rule it pins as a Rules override)."""
    P1 = perturbed(G, 0, 3, [4, -6, 10])
    return [
        ("median", (292, 262, 60, 60), 8, P1, dict(tolerance=0.01, rejection_scale=0.05), dict(median="upper")),
        ("picky_a", (292, 262, 60, 60), 2, G, dict(tolerance=0.001, rejection_scale=0.5, iterations=10), dict(picky_tie="higher")),
        ("picky_b", (300, 250, 60, 60), 8, G, dict(tolerance=0.001, rejection_scale=0.5, iterations=10), dict(picky_tie="higher")),
        ("picky_c", (300, 250, 60, 60), 2, G, dict(tolerance=0.01, rejection_scale=2.5, levels=3), dict(picky_tie="higher")),
    ]


# the dyadic threshold case: the identity pose, the "box" scene at step 2, its rows moved by THRESHOLD_SHIFT mm as the model
THRESHOLD_SHIFT = 0.25
THRESHOLD_PARAMS = [dict(), dict(levels=1, iterations=1), dict(levels=3, iterations=10, tolerance=0.01), dict(levels=8, tolerance=0.001,
                                                                                                         rejection_scale=0.05)]


def pose_diff(a, b):
    return R.rotation_angle(a[:3, :3], b[:3, :3]), float(np.abs(a[:3, 3] - b[:3, 3]).max())
