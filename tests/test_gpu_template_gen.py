"""Template-bank generation on the GPU: generate_templates_gpu / lm_add_templates_rendered make the host
generator's bank bit for bit -- template count and order, every lm_get_template record, every TemplatePose (linemod_tempPosFile.bin),
the decompressed linemod_templates.yml.gz, the "ERROR::Cant create Template" lines and lastError().  The stage hooks match
SoftRender::render and warp_rotate_* byte for byte; the error paths return codes."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "line-mod-pipeline_amd", "host")


def _mesh(tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(np.array([len(g["vertices"]), len(g["faces"])], np.uint32).tobytes())
        fh.write(g["vertices"].astype(np.float32).tobytes())
        fh.write(g["faces"].astype(np.int32).tobytes())
    return g


def _exe(lm, tmp_path, name):
    exe = str(tmp_path / name)
    libdir = os.path.dirname(lm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", name + ".cpp"),
                           os.path.join(HOST, "HighLevelLinemod.cpp"), os.path.join(HOST, "PostProcess.cpp"),
                           os.path.join(HOST, "TemplateGenerator.cpp"), "-L" + libdir, "-llinemod_hip", "-lpthread", "-Wl,-rpath," + libdir])
    return exe


def run_compare(lm, tmp_path, args, timeout=1500):
    _mesh(tmp_path)
    exe = _exe(lm, tmp_path, "template_gen")
    r = subprocess.run([exe, "mesh.bin"] + [str(a) for a in args], cwd=tmp_path, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    host_part = out.split("== host\n")[1].split("== gpu\n")[0]
    gpu_part = out.split("== gpu\n")[1].split("== end\n")[0]
    res = dict(l.split(" ", 1) for l in out.split("== end\n")[1].splitlines() if " " in l)
    nh, ng = (int(v) for v in res["templates"].split())
    print(res)
    assert nh == ng and nh > 0
    assert res["diff"] == "records 0", res
    err = res["error"]
    assert err.split("' gpu '")[0] == "host '" + err.split("' gpu '")[1].rstrip("'"), err
    n_err = host_part.count("ERROR::Cant create Template")
    assert gpu_part.count("ERROR::Cant create Template") == n_err
    for f in ("linemod_tempPosFile.bin",):
        a = open(tmp_path / "host" / f, "rb").read()
        b = open(tmp_path / "gpu" / f, "rb").read()
        assert len(a) == len(b) and a == b, f
    ya = gzip.open(tmp_path / "host" / "linemod_templates.yml.gz").read()
    yb = gzip.open(tmp_path / "gpu" / "linemod_templates.yml.gz").read()
    assert ya == yb
    return nh, n_err, float(res["host_s"]), float(res["gpu_s"])


@pytest.mark.gpu
def test_shipped_colour_only_bank(lm, tmp_path):
    """Case 1: the shipped settings (colour only, 640x480, lagergehaeuse with its symmetry), two radii."""
    n, _, th, tg = run_compare(lm, tmp_path, [640, 480, 1, "1,1,1", -45, 45, 10, "gen", 500, 550, 50, 3, 1, 1, 1, 1])
    print("case 1: %d templates, host %.1f/s, gpu %.1f/s" % (n, n / th, n / tg))


@pytest.mark.gpu
def test_rgbd_1280x960_scaled_mesh(lm, tmp_path):
    """Case 2: 1280x960 RGB-D, config5_e2e's anisotropically scaled mesh, rendered centred."""
    n, _, th, tg = run_compare(lm, tmp_path, [1280, 960, 0, "1.35,1,0.8", -30, 30, 30, "gen", 600, 650, 50, 3, 1, 1, 1, 1])
    print("case 2: %d templates, host %.1f/s, gpu %.1f/s" % (n, n / th, n / tg))


@pytest.mark.gpu
@pytest.mark.parametrize("color_only,scale,partial", [(1, "0.45,0.45,0.45", True), (0, "0.6,0.6,0.6", True), (0, "0.8,0.8,0.8", False)])
def test_failure_part_way_through_a_viewpoint(lm, tmp_path, color_only, scale, partial):
    """Case 3: a small model far away -- extraction fails at some angle of some viewpoints: that viewpoint keeps its earlier angles,
    drops the rest, and generation goes on with the next viewpoint."""
    n, n_err, _, _ = run_compare(lm, tmp_path, [640, 480, color_only, scale, -45, 45, 10, "gen", 1000, 1200, 200, 3, 1, 1, 1, 1])
    print("case 3 (%s, %s): %d templates, %d failing viewpoints" % (color_only, scale, n, n_err))
    assert n_err > 0
    if partial:   # 10 angles per viewpoint: some failing viewpoint kept its first angles (measured: 144 and 134 templates)
        assert n % 10 != 0


@pytest.mark.gpu
@pytest.mark.parametrize("views,a0,a1,step", [(1, 0, 0, 1), (4, -25, 25, 10), (5, -20, 20, 10)])
def test_chunk_boundaries(lm, tmp_path, views, a0, a1, step):
    """Case 4: views x angles = 1, one chunk of the facade's 24 slots, one chunk + 1."""
    run_compare(lm, tmp_path, [640, 480, 1, "1,1,1", a0, a1, step, "views", views, 600])


@pytest.mark.gpu
@pytest.mark.parametrize("color_only", [1, 0])
def test_part_cut_by_the_frame_border(lm, tmp_path, color_only):
    """Near views whose part crosses the frame edge: the border of the rotated mask stays un-eroded (addTemplate's erode), the
    rim / interior replicate the border (shrink_mask)."""
    run_compare(lm, tmp_path, [640, 480, color_only, "4,4,4", -10, 10, 10, "views", 6, 420])


CAMS = [(0, 0, 600), (250, 300, 500), (0, 600, 0.0), (120, -40, 260), (400, 0, 0)]   # centred, oblique, straight down (the nudge), very near, side


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,scale", [(640, 480, 1.0), (1280, 960, 1.0), (641, 479, 2.5)])
def test_render_hook_matches_softrender(lm, tmp_path, w, h, scale):
    """lm_stage_render against SoftRender::render (render_view): byte-equal coverage and depth, with views where the part is partly
    outside the frame (scale 2.5) and very near."""
    g = _mesh(tmp_path)
    exe = _exe(lm, tmp_path, "gen_stages")
    subprocess.check_call([exe, "render", "mesh.bin", str(w), str(h), str(scale)] + [str(c) for cam in CAMS for c in cam], cwd=tmp_path)
    det = lm.Detector(color_only=True)      # (the hook renders at any size)
    det.set_render_mesh(0, g["vertices"].astype(np.float32) * np.float32(scale), g["faces"])
    covered = 0
    for k in range(len(CAMS)):
        vp = np.fromfile(tmp_path / ("view_proj_%d.bin" % k), np.float32)
        cov_ref = np.fromfile(tmp_path / ("cov_%d.raw" % k), np.uint8).reshape(h, w)
        dep_ref = np.fromfile(tmp_path / ("depth_%d.raw" % k), np.uint16).reshape(h, w)
        cov, dep = det.render(0, vp, w, h)
        assert np.array_equal(cov, cov_ref), (k, int((cov != cov_ref).sum()))
        assert np.array_equal(dep, dep_ref), (k, int((dep != dep_ref).sum()))
        covered += int(cov.any())
    assert covered >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(640, 480), (641, 481), (96, 77)])
def test_rotate_hook_matches_warp_rotate(lm, tmp_path, w, h):
    """lm_stage_rotate against warp_rotate_u8 / warp_rotate_u16 for several angles, both parities of the frame size."""
    _mesh(tmp_path)
    exe = _exe(lm, tmp_path, "gen_stages")
    rng = np.random.default_rng(w * h)
    a = rng.integers(0, 256, (h, w)).astype(np.uint8)
    b = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    b[rng.random((h, w)) < 0.3] = 0
    a.tofile(tmp_path / "in8.raw")
    b.tofile(tmp_path / "in16.raw")
    angles = [-45, -35, -7, 0, 3, 10, 45, 90, 137]
    subprocess.check_call([exe, "rotate", "in8.raw", "in16.raw", str(w), str(h)] + [str(x) for x in angles], cwd=tmp_path)
    det = lm.Detector(color_only=True, width=640, height=480)
    for k, ang in enumerate(angles):
        o8, o16 = det.rotate(a, b, ang)
        r8 = np.fromfile(tmp_path / ("rot8_%d.raw" % k), np.uint8).reshape(h, w)
        r16 = np.fromfile(tmp_path / ("rot16_%d.raw" % k), np.uint16).reshape(h, w)
        assert np.array_equal(o8, r8), (ang, int((o8 != r8).sum()))
        assert np.array_equal(o16, r16), (ang, int((o16 != r16).sum()))


def _vp_centre(radius=600.0):
    # projection * lookAt((0, 0, r), 0, +y) of the shipped 640x480 camera, as SoftRender builds it (column-major)
    f = 1.0 / np.tan(np.arctan(480 / (2 * 1045.69141)))
    P = np.zeros((4, 4), np.float64)
    P[0, 0] = f / (640 / 480); P[1, 1] = f; P[2, 2] = -10100 / 9900; P[2, 3] = -1; P[3, 2] = -2 * 1e6 / 9900
    V = np.eye(4); V[3, 2] = -radius
    return (V @ P).astype(np.float32).ravel()   # m[c][r] = (P V)[r][c]


@pytest.mark.gpu
def test_error_paths(lm):
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    det = lm.Detector(color_only=True, width=640, height=480)
    lib = det.lib
    v = np.ascontiguousarray(g["vertices"], np.float32)
    f = np.ascontiguousarray(g["faces"], np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.lm_set_render_mesh(det.h, 0, p(v), 0, p(f), f.size) == lm.LM_ERR_INVALID          # empty mesh
    assert lib.lm_set_render_mesh(det.h, 0, p(v), len(v), p(f), 0) == lm.LM_ERR_INVALID
    bad = f.copy(); bad[5] = len(v)
    assert lib.lm_set_render_mesh(det.h, 0, p(v), len(v), p(bad), bad.size) == lm.LM_ERR_INVALID   # index beyond the vertices
    assert lib.lm_set_render_mesh(det.h, 16, p(v), len(v), p(f), f.size) == lm.LM_ERR_INVALID       # LM_MAX_RENDER_MESHES
    det.set_render_mesh(0, v, f)
    vp = _vp_centre()
    angles = np.array([-10, 0, 10], np.float32)
    ids = np.zeros(3, np.int32); bbs = np.zeros((3, 4), np.int32); crops = np.zeros(640 * 480 * 3, np.uint16); offs = np.zeros(4, np.uint64)
    call = lambda mesh, nv, cap: lib.lm_add_templates_rendered(det.h, b"x", mesh, p(vp), nv, p(angles), 3, p(ids), p(bbs), p(crops), cap, p(offs))
    assert call(0, 0, crops.size) == lm.LM_ERR_INVALID                                             # zero views
    assert call(1, 1, crops.size) == lm.LM_ERR_INVALID                                             # no mesh under index 1
    assert call(-1, 1, crops.size) == lm.LM_ERR_INVALID
    assert call(0, 1, 10) == lm.LM_ERR_OVERFLOW                                                    # capacity too small: nothing added
    assert lib.lm_num_templates(det.h) == 0
    assert (ids == -1).all() and int(offs[3]) > 10
    assert call(0, 1, crops.size) == lm.LM_OK
    assert (ids >= 0).all() and lib.lm_num_templates(det.h) == 3
    # a busy lane refuses
    bgr = np.zeros((480, 640, 3), np.uint8)
    assert lib.lm_upload_frame(det.h, 0, p(bgr), 0, None, 0) == lm.LM_OK
    assert lib.lm_match_begin(det.h, 0, 0, 1, 80.0, 0) == lm.LM_OK
    assert call(0, 1, crops.size) == lm.LM_ERR_INVALID
    assert lib.lm_stage_render(det.h, 0, p(vp), 640, 480, p(np.zeros(640 * 480, np.uint8)), p(np.zeros(640 * 480, np.uint16))) == lm.LM_ERR_INVALID
    out = np.zeros(4096, lm.MATCH_DTYPE)
    counts = np.zeros(1, np.int32)
    assert lib.lm_match_end(det.h, 0, p(out), 4096, p(counts)) in (lm.LM_OK, lm.LM_ERR_OVERFLOW)
    assert lib.lm_num_templates(det.h) == 3


@pytest.mark.gpu
def test_binding_add_templates_rendered_crops(lm):
    """Detector.add_templates_rendered: ids in view-major order, crops of the bboxes' size."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    det = lm.Detector(color_only=True, width=640, height=480)
    det.set_render_mesh(3, g["vertices"], g["faces"])
    ids, bbs, crops = det.add_templates_rendered("part", 3, np.stack([_vp_centre(600), _vp_centre(700)]), [-10, 10])
    assert ids.shape == (2, 2) and list(ids.ravel()) == [0, 1, 2, 3]
    for k, c in enumerate(crops):
        x, y, w, h = bbs.reshape(-1, 4)[k]
        assert c.shape == (h, w) and (c > 0).any()


@pytest.mark.gpu
@pytest.mark.skipif(os.environ.get("LM_CONFIG5_FULL") != "1", reason="opt-in: the full config-5 bank (24 300 templates), LM_CONFIG5_FULL=1")
def test_config5_full_bank(lm, tmp_path):
    """BASELINE config 5's bank: 162 viewpoints x 5 radii x 10 angles at 1280x960 RGB-D, per class; here the first class, bank for bank."""
    n, _, th, tg = run_compare(lm, tmp_path, [1280, 960, 0, "1,1,1", -45, 45, 10, "gen", 600, 800, 50, 2, 0, 0, 0, 0], timeout=7200)
    print("config 5 class 0: %d templates, host %.1f s, gpu %.1f s" % (n, th, tg))
