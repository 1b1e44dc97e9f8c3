"""Pose-error evaluation on the GPU: lm_stage_vsd_counts / lm_pose_error_vsd against the numpy restatement of
Benchmark.cpp's pixel rules (tests/pose_error_reference.py) on crafted images and on renders of frame0's ground truth, batches equal to
single calls, ADD / ADD-S per vertex bit for bit and their means within 1 ulp, and the error paths."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_error_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 480


def _mesh():
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    return g


def _det(lm):
    g = _mesh()
    d = lm.Detector(color_only=True, width=W, height=H)
    d.set_render_mesh(0, g["vertices"], g["faces"])
    return d, g


def _fields(r):
    return [int(r[k]) for k in ("rendered_gt", "rendered_est", "visible_gt", "visible_est", "intersection", "combination", "within_tau")]


def _same_error(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes()


EDGES = R.EDGE_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("name,px,expected", EDGES, ids=[e[0] for e in EDGES])
def test_vsd_counts_edges(lm, name, px, expected):
    d = lm.Detector(color_only=True, width=64, height=64)
    try:
        g, e, s = (np.full((3, 5), v, np.uint16) for v in px)
        g[0, 0] = e[0, 0] = s[0, 0] = 0          # one background pixel beside them changes nothing
        r = d.vsd_counts(g, e, s, 15, 20)
        exp = [14 * v for v in expected]
        assert _fields(r) == exp, (name, _fields(r), exp)
        c, err = R.vsd_counts(g, e, s, 15, 20)
        assert c == exp
        assert _same_error(r["error"], err)
        if exp[5] == 0:
            assert np.isnan(r["error"])
        else:
            assert r["error"] == np.float32(1) - np.float32(exp[6]) / np.float32(exp[5])
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(480, 640), (17, 33), (1, 1), (961, 1281)])
def test_vsd_counts_random_images(lm, shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    base = rng.integers(0, 3000, shape)
    g = np.clip(base + rng.integers(-30, 30, shape), 0, 65535).astype(np.uint16)
    e = np.clip(base + rng.integers(-30, 30, shape), 0, 65535).astype(np.uint16)
    s = np.clip(base + rng.integers(-30, 30, shape), 0, 65535).astype(np.uint16)
    for a in (g, e, s):
        a[rng.random(shape) < 0.1] = rng.choice([0, 1, 2], 1)[0]
    d = lm.Detector(color_only=True, width=64, height=64)
    try:
        for delta, tau in ((15, 20), (0, 0), (3, 7)):
            r = d.vsd_counts(g, e, s, delta, tau)
            c, err = R.vsd_counts(g, e, s, delta, tau)
            assert _fields(r) == c and _same_error(r["error"], err), (delta, tau)
    finally:
        d.close()


def _axis_quat(axis, deg):
    a = np.radians(deg) / 2
    v = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return (np.cos(a), *(np.sin(a) * v))


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return (w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
            w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2)


def _poses(g):
    """(name, quaternion, translation) of the GT and perturbed estimates"""
    qg = R.mat3_to_quat(g["gt_rotation"])
    tg = np.asarray(g["gt_position"], np.float64)
    return qg, tg, [
        ("identical", qg, tg),
        ("shifted 4 mm", qg, tg + [4, 0, 0]),
        ("deeper 30 mm", qg, tg + [0, 0, 30]),
        ("turned 10 deg", _qmul(qg, _axis_quat([0, 1, 0], 10)), tg),
        ("partly out of frame", qg, tg + [187, 0, 0]),
        ("wholly out of frame", qg, tg + [2000, 0, 0]),
        ("behind the camera", qg, tg * [1, 1, -1]),
    ]


def _vp(q, t):
    return R.view_proj_mat4(R.projection(), R.view_mat(q, t))


@pytest.mark.gpu
def test_pose_error_vsd_on_frame0_renders(lm, frame0):
    _, depth = frame0
    d, g = _det(lm)
    try:
        qg, tg, poses = _poses(g)
        vg = _vp(qg, tg)
        _, dg = d.render(0, vg, W, H)
        assert (dg > 1).sum() > 1000
        ves = [_vp(q, t) for _, q, t in poses]
        res = d.pose_error_vsd(depth, 0, 0, [vg] * len(ves), ves)
        for (name, _, _), ve, r in zip(poses, ves, res):
            _, de = d.render(0, ve, W, H)
            c, err = R.vsd_counts(dg, de, depth)
            assert _fields(r) == c, (name, _fields(r), c)
            assert _same_error(r["error"], err), (name, r["error"], err)
        byname = {p[0]: r for p, r in zip(poses, res)}
        assert byname["identical"]["combination"] > 0 and byname["identical"]["error"] == 0.0
        assert byname["shifted 4 mm"]["error"] > 0.0
        assert byname["behind the camera"]["rendered_est"] == 0
        assert byname["wholly out of frame"]["rendered_est"] == 0
        assert 0 < byname["partly out of frame"]["rendered_est"] < byname["identical"]["rendered_est"]
        # nothing rendered at all and the scene empty: the reference's 0 / 0
        r0 = d.pose_error_vsd(depth, 0, 0, ves[-1], ves[-1])[0]
        assert _fields(r0) == [0] * 7 and np.isnan(r0["error"])
    finally:
        d.close()


@pytest.mark.gpu
def test_pose_error_vsd_batch_equals_single_calls(lm, frame0):
    _, depth = frame0
    frames = np.stack([depth, np.roll(depth, 7, axis=1), np.zeros_like(depth)])
    d, g = _det(lm)
    try:
        qg, tg, _ = _poses(g)
        rng = np.random.default_rng(5)
        n = 150                                   # three chunks of at most 64 queries
        vg, ve, fr = [], [], []
        for k in range(n):
            q = _qmul(qg, _axis_quat(rng.normal(size=3), rng.uniform(0, 25)))
            vg.append(_vp(qg, tg + rng.normal(0, 3, 3)))
            ve.append(_vp(q, tg + rng.normal(0, 15, 3)))
            fr.append(int(rng.integers(0, 3)))
        batch = d.pose_error_vsd(frames, fr, 0, vg, ve)
        for k in range(n):
            one = d.pose_error_vsd(frames[fr[k]], 0, 0, vg[k], ve[k])[0]
            assert batch[k].tobytes() == one.tobytes(), k
        k = int(np.argmax(batch["combination"]))
        _, dgk = d.render(0, vg[k], W, H)
        _, dek = d.render(0, ve[k], W, H)
        assert _fields(batch[k]) == R.vsd_counts(dgk, dek, frames[fr[k]])[0]
    finally:
        d.close()


def _rand_rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return R.quat_to_mat3(q)


@pytest.mark.gpu
@pytest.mark.parametrize("step", [1, 40, 14136])
def test_pose_error_add_and_adds_bit_exact(lm, step):
    d, g = _det(lm)
    try:
        rng = np.random.default_rng(step)
        v = g["vertices"]
        Rg = np.stack([_rand_rot(rng) for _ in range(3)])
        Re = np.stack([_rand_rot(rng) for _ in range(3)])
        tg = rng.normal(0, 100, (3, 3)).astype(np.float32) + [0, 0, 600]
        te = tg + rng.normal(0, 10, (3, 3)).astype(np.float32)
        Re[0], te[0] = Rg[0], tg[0]               # identical poses: 0 everywhere
        for symmetric in (False, True):
            mean, pv = d.pose_error_add(0, Rg, tg, Re, te, step=step, symmetric=symmetric, per_vertex=True)
            nq = 1 if (symmetric and step == 1) else 3   # the numpy all-pairs search at step 1 is the slow part: one query
            for k in range(nq):
                f = R.adds_per_vertex if symmetric else R.add_per_vertex
                ref = f(v, step, Rg[k], tg[k], Re[k], te[k])
                assert pv[k].shape == ref.shape
                assert pv[k].tobytes() == ref.tobytes(), (symmetric, k, np.flatnonzero(pv[k] != ref)[:5])
                m = R.mean_of(ref)
                assert abs(int(mean[k].view(np.int32)) - int(m.view(np.int32))) <= 1, (mean[k], m)
            assert mean[0] == 0.0
    finally:
        d.close()


@pytest.mark.gpu
def test_adds_is_small_on_a_symmetric_mesh(lm):
    # a box centred on the z axis: a 180 degree turn about z maps its vertices onto each other
    xs, ys, zs = np.meshgrid(np.linspace(-40, 40, 9), np.linspace(-20, 20, 5), np.linspace(-10, 10, 3), indexing="ij")
    v = np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1).astype(np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    d = lm.Detector(color_only=True, width=64, height=64)
    try:
        d.set_render_mesh(2, v, faces)
        Rg = np.eye(3, dtype=np.float32)
        Re = np.diag([-1, -1, 1]).astype(np.float32)
        t = np.array([5, -3, 700], np.float32)
        add = d.pose_error_add(2, Rg, t, Re, t, symmetric=False)[0]
        adds = d.pose_error_add(2, Rg, t, Re, t, symmetric=True)[0]
        assert add > 20 and adds < 1e-3, (add, adds)
    finally:
        d.close()


@pytest.mark.gpu
def test_pose_error_error_paths(lm, frame0):
    _, depth = frame0
    d, g = _det(lm)
    lib = lm.load_library()
    try:
        vp = np.eye(4, dtype=np.float32).reshape(16)
        eye = np.eye(3, dtype=np.float32)
        t = np.zeros(3, np.float32)
        for bad_mesh in (-1, 16, 3):              # out of range, out of range, never set
            with pytest.raises(lm.LinemodError) as e:
                d.pose_error_vsd(depth, 0, bad_mesh, vp, vp)
            assert e.value.code == lm.LM_ERR_INVALID
            with pytest.raises(lm.LinemodError) as e:
                d.pose_error_add(bad_mesh, eye, t, eye, t)
            assert e.value.code == lm.LM_ERR_INVALID
        for bad_frame in (-1, 1):
            with pytest.raises(lm.LinemodError) as e:
                d.pose_error_vsd(depth, bad_frame, 0, vp, vp)
            assert e.value.code == lm.LM_ERR_INVALID
        with pytest.raises(lm.LinemodError) as e:
            d.pose_error_add(0, eye, t, eye, t, step=0)
        assert e.value.code == lm.LM_ERR_INVALID
        q = (lm.VsdQuery * 1)()
        res = np.zeros(1, lm.VSD_RESULT_DTYPE)
        dp = depth.ctypes.data_as(C.c_void_p)
        rp = res.ctypes.data_as(C.c_void_p)
        assert lib.lm_pose_error_vsd(d.h, dp, 1, 0, H, q, 1, 15, 20, rp) == lm.LM_ERR_INVALID       # bad size
        assert lib.lm_pose_error_vsd(d.h, dp, 1, W, -1, q, 1, 15, 20, rp) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_vsd(d.h, dp, 0, W, H, q, 1, 15, 20, rp) == lm.LM_ERR_INVALID       # no frames
        assert lib.lm_pose_error_vsd(d.h, None, 1, W, H, q, 1, 15, 20, rp) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_vsd(d.h, dp, 1, W, H, None, 1, 15, 20, rp) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_vsd(d.h, dp, 1, W, H, q, 1, 15, 20, None) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_vsd(None, dp, 1, W, H, q, 1, 15, 20, rp) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_vsd(d.h, dp, 1, W, H, q, -1, 15, 20, rp) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_vsd(d.h, None, 0, 0, 0, None, 0, 15, 20, None) == lm.LM_OK          # n = 0: nothing
        mean = np.zeros(1, np.float32)
        mp = mean.ctypes.data_as(C.c_void_p)
        aq = np.zeros(1, lm.ADD_QUERY_DTYPE)
        ap = aq.ctypes.data_as(C.c_void_p)
        assert lib.lm_pose_error_add(d.h, 0, 1, 0, None, 1, mp, None) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_add(d.h, 0, 1, 0, ap, 1, None, None) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_add(None, 0, 1, 0, ap, 1, mp, None) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_add(d.h, 0, -3, 1, ap, 1, mp, None) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_add(d.h, 0, 1, 1, None, 0, None, None) == lm.LM_OK
        img = np.zeros((4, 4), np.uint16)
        ip = img.ctypes.data_as(C.c_void_p)
        assert lib.lm_stage_vsd_counts(d.h, ip, ip, None, 4, 4, 15, 20, rp) == lm.LM_ERR_INVALID
        assert lib.lm_stage_vsd_counts(d.h, ip, ip, ip, 0, 4, 15, 20, rp) == lm.LM_ERR_INVALID
        assert lib.lm_stage_vsd_counts(d.h, ip, ip, ip, 4, 4, 15, 20, None) == lm.LM_ERR_INVALID
        # the detector still matches after all of it
        assert d.pose_error_add(0, eye, t, eye, t, step=40)[0] == 0.0
    finally:
        d.close()
