"""CPU tests of the pose-error evaluation: the numpy restatement's pixel rules against hodan_pose0.cpp's loop on
hand-made images, the readers of host/Benchmark.h (tests/cpp/benchmark_readers.cpp) against numpy on files written here, and the
binding's entry points (argument errors first, no silent fallback without a device)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_error_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "line-mod-pipeline_amd", "host")


def hodan_loop(dg, de, din, delta=15, tau=20):
    """tests/cpp/hodan_pose0.cpp's per-pixel loop, transcribed line by line"""
    n_gt = n_est = inter = uni = good = px_gt = px_est = 0
    for g, e, d in zip(dg.ravel().tolist(), de.ravel().tolist(), din.ravel().tolist()):
        px_gt += g > 1
        px_est += e > 1
        g_occl = (g - d if g > d else 0) > delta
        vg = (g > 1) and not g_occl
        e_occl = (e - d if e > d else 0) > delta
        ve = (e > 1) and not e_occl
        if vg and e != 0:
            ve = True
        n_gt += vg
        n_est += ve
        inter += vg and ve
        uni += vg or ve
        ad = g - e if g > e else e - g
        good += (vg and ve) and not (ad > tau)
    return [px_gt, px_est, n_gt, n_est, inter, uni, good]


@pytest.mark.parametrize("name,px,expected", R.EDGE_CASES, ids=[e[0] for e in R.EDGE_CASES])
def test_restatement_edges_match_hodan_loop(name, px, expected):
    g, e, s = (np.full((2, 3), v, np.uint16) for v in px)
    c, err = R.vsd_counts(g, e, s)
    assert c == [6 * v for v in expected] == hodan_loop(g, e, s), name
    assert np.isnan(err) if c[5] == 0 else err == np.float32(1) - np.float32(c[6]) / np.float32(c[5])


def test_restatement_matches_hodan_loop_on_random_images():
    rng = np.random.default_rng(11)
    base = rng.integers(0, 2000, (40, 50))
    g, e, s = (np.clip(base + rng.integers(-30, 30, base.shape), 0, 65535).astype(np.uint16) for _ in range(3))
    for a in (g, e, s):
        a[rng.random(base.shape) < 0.15] = 0
    for delta, tau in ((15, 20), (0, 0), (5, 40)):
        assert R.vsd_counts(g, e, s, delta, tau)[0] == hodan_loop(g, e, s, delta, tau)


def test_add_restatement_contract():
    """The per-vertex expression is float32 throughout; ADD-S never exceeds the reference's 999999 start."""
    v = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.float32)
    Rm = np.eye(3, dtype=np.float32)
    d = R.add_per_vertex(v, 1, Rm, [0, 0, 0], Rm, [3, 4, 0])
    assert d.dtype == np.float32 and np.array_equal(d, np.float32([5, 5, 5]))
    assert np.array_equal(R.adds_per_vertex(v, 1, Rm, [0, 0, 0], Rm, [2e6, 0, 0]), np.float32([999999] * 3))
    assert R.mean_of(np.float32([1, 2, 4])) == np.float32(7 / 3)


@pytest.fixture(scope="module")
def readers_exe(lm, tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("readers")
    exe = str(d / "benchmark_readers")
    libdir = os.path.dirname(lm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "benchmark_readers.cpp"),
                           os.path.join(HOST, "HighLevelLinemod.cpp"), os.path.join(HOST, "PostProcess.cpp"),
                           os.path.join(HOST, "TemplateGenerator.cpp"), "-L" + libdir, "-llinemod_hip", "-lpthread", "-Wl,-rpath," + libdir])
    return exe


def _nums(line, tag):
    parts = line.split()
    i = parts.index(tag)
    return np.array([float(v) for v in parts[i + 1:i + 4 if tag == "t" else i + 5]])


def test_readers_match_numpy(readers_exe, tmp_path):
    shutil.copy(os.path.join(ROOT, "tests", "golden", "reference_data", "pose0.yml"), tmp_path / "pose0.yml")
    rot = [0.36, -0.48, 0.8, 0.8, 0.6, 0.0, -0.48, 0.64, 0.6]
    with open(tmp_path / "tra0.tra", "w") as f:
        f.write("1 3\n 2.5\n-1.25\n 61.3\n")
    with open(tmp_path / "rot0.rot", "w") as f:
        f.write("3 3\n" + "\n".join(" ".join("%.6f" % v for v in rot[3 * r:3 * r + 3]) for r in range(3)) + "\n")
    depth = np.arange(7 * 5, dtype=np.uint16).reshape(7, 5) * 997
    with open(tmp_path / "depth0.dpt", "wb") as f:
        f.write(np.array([7, 5], np.int32).tobytes() + depth.tobytes())
    r = subprocess.run([readers_exe, "pose0.yml", "tra0.tra", "rot0.rot", "depth0.dpt"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {l.split(" q ")[0] if " q " in l else " ".join(l.split()[:2]) if l.startswith("missing") else l.split()[0]: l
           for l in r.stdout.splitlines()}
    # pose0.yml: the quaternion of rotMat, position as written
    Rp, tp = R.read_pose_yml(tmp_path / "pose0.yml")
    q = _nums(out["pose"], "q")
    qn = np.array(R.mat3_to_quat(Rp.astype(np.float32)))
    assert np.allclose(q * np.sign(q[0]), qn * np.sign(qn[0]), atol=2e-6)
    assert np.array_equal(_nums(out["pose"], "t").astype(np.float32), tp.astype(np.float32))
    # the view-projection of the pose: SoftRender's projection times calculateViewMat (x - pi, -y, -z; t.x, -t.y, -t.z)
    vp = np.array([float(v) for v in out["viewproj"].split()[1:]])
    vn = R.view_proj_mat4(R.projection(), R.view_mat(qn, tp))
    assert np.allclose(vp, vn, rtol=1e-5, atol=1e-4), (vp, vn)
    # LINEMOD: two numbers skipped in each file, translation x 10, the euler adjustment x - pi / 2
    Rl, tl = R.read_linemod_tra_rot(tmp_path / "tra0.tra", tmp_path / "rot0.rot")
    assert np.array_equal(_nums(out["linemod"], "t").astype(np.float32), tl) and np.array_equal(tl, np.float32([25, -12.5, 613]))
    ql = _nums(out["linemod"], "q")
    qe = np.array(R.linemod_quat(Rl))
    assert np.allclose(ql * np.sign(ql[0]), qe * np.sign(qe[0]), atol=2e-6), (ql, qe)
    qraw = np.array(R.mat3_to_quat(Rl))
    assert not np.allclose(np.abs(ql), np.abs(qraw), atol=1e-3)     # the adjustment is applied
    # .dpt: int32 rows, int32 cols, uint16 samples
    dn = R.load_dpt(tmp_path / "depth0.dpt")
    assert np.array_equal(dn, depth)
    assert out["dpt"].split()[1:] == ["7", "5", str(int(depth.sum())), str(int(depth.flat[0])), str(int(depth.flat[-1]))]
    # missing files are errors, not zeros
    for key in ("missing pose", "missing tra", "missing rot"):
        assert " error '" in out[key] and "no_such_dir" in out[key], out[key]
    assert out["missing dpt"].startswith("missing dpt 0 'cannot open")


def test_binding_declares_pose_error_entry_points(lm):
    lib = lm.load_library()
    for n in ("lm_pose_error_vsd", "lm_pose_error_add", "lm_stage_vsd_counts"):
        assert n in lm.EXPORTS and getattr(lib, n).argtypes is not None
    assert b"0.7" in lib.lm_version()
    assert lm.VSD_RESULT_DTYPE.itemsize == 32 and lm.ADD_QUERY_DTYPE.itemsize == 96 and C.sizeof(lm.VsdQuery) == 136


def test_pose_error_argument_errors_come_first(lm):
    """Argument errors are LM_ERR_INVALID with or without a device; without one the calls fail with LM_ERR_NO_DEVICE (no fallback)."""
    lib = lm.load_library()
    cfg = lm.default_config(color_only=True)
    h = C.c_void_p()
    assert lib.lm_create(C.byref(cfg), C.byref(h)) == lm.LM_OK
    try:
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        img = np.zeros((4, 4), np.uint16)
        res = np.zeros(1, lm.VSD_RESULT_DTYPE)
        q = (lm.VsdQuery * 1)()
        mean = np.zeros(1, np.float32)
        aq = np.zeros(1, lm.ADD_QUERY_DTYPE)
        assert lib.lm_stage_vsd_counts(h, p(img), p(img), None, 4, 4, 15, 20, p(res)) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_vsd(h, p(img), 1, 0, 4, q, 1, 15, 20, p(res)) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_add(h, 0, 0, 0, p(aq), 1, p(mean), None) == lm.LM_ERR_INVALID
        assert lib.lm_pose_error_vsd(h, None, 0, 0, 0, None, 0, 15, 20, None) == lm.LM_OK
        rc = lib.lm_stage_vsd_counts(h, p(img), p(img), p(img), 4, 4, 15, 20, p(res))
        assert rc in (lm.LM_OK, lm.LM_ERR_NO_DEVICE)
        if rc == lm.LM_ERR_NO_DEVICE:
            assert lib.lm_pose_error_add(h, 0, 1, 0, p(aq), 1, p(mean), None) == lm.LM_ERR_NO_DEVICE
    finally:
        lib.lm_destroy(h)
