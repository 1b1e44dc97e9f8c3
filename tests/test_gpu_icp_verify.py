"""The best-pose check of the ICP branch on the GPU (lm_k_verify.hip) against the numpy restatement of
estimateBestMatch's mean depth difference (tests/icp_verify_reference.py): count and integer sum exactly on crafted images and on
renders of the shipped mesh, batches equal to single calls, the slot form equal to the host form, and the error paths."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_verify_reference as V  # noqa: E402
import pose_error_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 480
THR = 80.0
SIZES = [(1, 1), (5, 3), (64, 16), (65, 17), (70, 37)]      # (w, h): one pixel, below a tile, a tile's 60 columns crossed, two tile rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det(lm):
    d = lm.Detector(color_only=True, width=64, height=64)
    yield d
    d.close()


def _check(det, render, scene, scene_min=600):
    got = det.icp_verify_counts(render, scene, scene_min)
    exp = V.verify(render, scene, scene_min)
    assert got[:2] == exp[:2], (got, exp)
    assert got[2] == exp[2]                                     # the same quotient of the same integers
    return got


def _full(w=70, h=37, render=1000, scene=1010):
    return np.full((h, w), render, np.uint16), np.full((h, w), scene, np.uint16)


@pytest.mark.parametrize("render,scene,valid", [(0, 1000, False), (1, 1000, False), (2, 1000, True), (1000, 600, False), (1000, 601, True)])
def test_threshold_edges(det, render, scene, valid):
    r, s = _full(render=render, scene=scene)
    got = _check(det, r, s)
    assert got[0] == (70 * 37 if valid else 0)
    assert got[1] == (70 * 37 * abs(scene - render) if valid else 0)


def test_scene_min_is_an_argument(det):
    r, s = _full(scene=700)
    assert _check(det, r, s, 699)[0] == 70 * 37
    assert _check(det, r, s, 700)[0] == 0


def test_blocks_and_holes(det):
    w, h = 70, 37
    r, s = _full()
    assert _check(det, r, s) == (w * h, 10 * w * h, 10.0)       # a full frame: the border does not erode, corner pixels survive
    for (x, y), lost in (((35, 18), 25), ((0, 0), 9), ((w - 1, h - 1), 9), ((w - 1, 0), 9), ((0, h - 1), 9), ((59, 15), 25), ((60, 16), 25)):
        r, s = _full()
        s[y, x] = 0
        assert _check(det, r, s)[0] == w * h - lost, (x, y)
        r, s = _full()
        r[y, x] = 0
        assert _check(det, r, s)[0] == w * h - lost, (x, y)
    for bw, bh, count in ((5, 5, 1), (4, 5, 0), (5, 4, 0), (6, 5, 2), (7, 7, 9)):
        for x0, y0 in ((30, 10), (57, 13), (58, 14)):            # inside a tile, and across the tiles' corner at (60, 16)
            r, s = _full(render=0)
            r[y0:y0 + bh, x0:x0 + bw] = 1000
            assert _check(det, r, s)[0] == count, (bw, bh, x0, y0)
    # a set block on the border keeps what a block in the interior loses: the outside counts as set
    r, s = _full(render=0)
    r[:3, :3] = 1000
    assert _check(det, r, s)[0] == 1
    r, s = _full(render=0)
    r[-3:, -4:] = 1000
    assert _check(det, r, s)[0] == 2


@pytest.mark.parametrize("w,h", SIZES + [(121, 33), (640, 480)])
def test_random_images(det, w, h):
    rng = np.random.default_rng(100 * w + h)
    for unset in (0.1, 0.01):
        base = rng.integers(650, 3000, (h, w))
        r = np.clip(base + rng.integers(-40, 40, (h, w)), 0, 65535).astype(np.uint16)    # above the scene and below it
        s = np.clip(base + rng.integers(-40, 40, (h, w)), 0, 65535).astype(np.uint16)
        r[rng.random((h, w)) < unset / 2] = rng.choice([0, 1])
        s[rng.random((h, w)) < unset / 2] = rng.choice([0, 600])
        got = _check(det, r, s)
        if (w, h) == (640, 480):
            assert got[0] > 1000
    r = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    s = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    _check(det, r, s)
    _check(det, np.maximum(r, 2), np.maximum(s, 601))            # everything valid: count w * h
    _check(det, s, r, 0)


def test_absolute_difference_both_ways(det):
    r, s = _full(render=1500, scene=1000)
    assert _check(det, r, s) == (70 * 37, 500 * 70 * 37, 500.0)
    r, s = _full(render=1000, scene=1500)
    assert _check(det, r, s) == (70 * 37, 500 * 70 * 37, 500.0)
    r, s = _full(render=65535, scene=601)
    assert _check(det, r, s)[1] == 64934 * 70 * 37


def test_total_needs_64_bits(det):
    r, s = _full(640, 480, render=2, scene=65535)
    got = _check(det, r, s)
    assert got == (307200, 20131737600, 65533.0)
    assert got[1] > 2 ** 32


def test_empty_mask(det):
    r, s = _full(render=0)
    assert _check(det, r, s) == (0, 0, 0.0)
    r, s = _full()
    r[::4, ::4] = 0                                              # every 5x5 window has a hole
    assert _check(det, r, s) == (0, 0, 0.0)


# ---- the rendered path
def _axis_quat(axis, deg):
    a = np.radians(deg) / 2
    v = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return (np.cos(a), *(np.sin(a) * v))


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return (w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
            w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2)


@pytest.fixture(scope="module")
def mesh():
    return np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))


def _view_projs(g, w=W, h=H, fy=1045.69141):
    qg = R.mat3_to_quat(g["gt_rotation"])
    tg = np.asarray(g["gt_position"], np.float64)
    poses = [("gt", qg, tg), ("deeper 100 mm", qg, tg + [0, 0, 100]), ("turned 4 deg", _qmul(qg, _axis_quat([0, 1, 0], 4)), tg),
             ("out of frame", qg, tg + [3000, 0, 0]), ("deeper 40 mm", qg, tg + [0, 0, 40])]
    P = R.projection(fy, w, h)
    return [p[0] for p in poses], np.stack([R.view_proj_mat4(P, R.view_mat(q, t)) for _, q, t in poses])


@pytest.fixture(scope="module")
def rendered(lm, mesh):
    """One detector with the shipped mesh resident, the five poses' view-projections at 640 x 480 and the renders the reference reads."""
    d = lm.Detector(color_only=False)
    d.set_render_mesh(0, mesh["vertices"], mesh["faces"])
    names, vps = _view_projs(mesh)
    renders = [d.render(0, vp, W, H)[1] for vp in vps]
    yield d, names, vps, renders
    d.close()


def test_rendered_poses_against_frame0(rendered, frame0):
    d, names, vps, renders = rendered
    _, depth = frame0
    assert (renders[0] > 1).sum() > 1000 and (renders[3] > 1).sum() == 0
    count, total, mean = d.icp_verify(depth, 0, 0, vps)
    for k, name in enumerate(names):
        exp = V.verify(renders[k], depth)
        assert (int(count[k]), int(total[k])) == exp[:2], (name, count[k], total[k], exp)
        assert mean[k] == exp[2]
    print("rendered poses:", names, count, total, mean)
    assert count[0] > 500 and count[3] == 0 and mean[3] == 0.0
    # The host check (SoftRender + meanDepthDifference, run on the CPU) gives for this fixture: GT 4670 pixels, mean 46.83 -- frame0's
    # depth lies some 45 mm behind lagergehaeuse.npz's ground truth, so the rule rejects the GT pose itself; 100 mm deeper 3299
    # pixels, mean 51.10 (rejected); 40 mm deeper 4043 pixels, mean 14.61 (accepted).
    # (Exactness is the comparison above.  Here 1 mm of room: this test's view matrices are built in numpy, the host's in float, and a
    # differently rounded matrix can move silhouette pixels, a fraction of a percent of the mask.)
    for k, host_mean in ((0, 46.83), (1, 51.10), (4, 14.61)):
        assert abs(float(mean[k]) - host_mean) < 1.0, (names[k], mean[k])
    assert [V.select_best([m])[0] for m in (mean[0], mean[1], mean[4])] == [False, False, True]
    assert V.select_best([mean[0], mean[1], mean[3], mean[4]]) == (True, 3)     # as a group: the out-of-frame pose's 0 is skipped


def test_small_render_against_a_scene_made_from_it(lm, mesh):
    w, h = 160, 120
    d = lm.Detector(color_only=True, width=64, height=64)
    try:
        d.set_render_mesh(3, mesh["vertices"], mesh["faces"])
        names, vps = _view_projs(mesh, w, h, 1045.69141 / 4)
        rng = np.random.default_rng(3)
        base = d.render(3, vps[0], w, h)[1]
        assert (base > 1).sum() > 300
        scene = np.where(base > 1, base + 150, 900).astype(np.uint16)     # (the part stands at about 600 mm: + 150 clears scene_min)
        scene[rng.random((h, w)) < 0.01] = 0
        count, total, mean = d.icp_verify(scene, 0, 3, vps)
        for k, name in enumerate(names):
            exp = V.verify(d.render(3, vps[k], w, h)[1], scene)
            assert (int(count[k]), int(total[k]), mean[k]) == exp, (name, exp)
        assert count[0] > 0 and mean[0] == 150.0
    finally:
        d.close()


def test_70_queries_over_two_frames_equal_single_calls(rendered, frame0):
    """Crosses the 64-query chunk; the frames alternate, so a chunk holds both."""
    d, names, vps, renders = rendered
    _, depth = frame0
    other = np.where(renders[0] > 1, renders[0] + 150, depth).astype(np.uint16)
    frames = np.stack([depth, other])
    singles = {}
    for f in range(2):
        for k in range(3):
            c, t, m = d.icp_verify(frames[f], 0, 0, vps[k][None])
            singles[f, k] = (int(c[0]), int(t[0]), float(m[0]))
            assert singles[f, k] == V.verify(renders[k], frames[f])
    fr = [(i * 7 + i // 3) % 2 for i in range(70)]
    ks = [(i * 5) % 3 for i in range(70)]
    count, total, mean = d.icp_verify(frames, fr, 0, vps[ks])
    for i in range(70):
        assert (int(count[i]), int(total[i]), float(mean[i])) == singles[fr[i], ks[i]], i
    assert singles[1, 0][0] > 500 and singles[1, 0][2] == 150.0


def test_slot_form_equals_host_form_and_leaves_other_lanes_alone(lm, rendered, frame0, golden0):
    d, names, vps, renders = rendered
    bgr, depth = frame0
    other = np.where(renders[0] > 1, renders[0] + 150, depth).astype(np.uint16)
    d.add_class("lagergehaeuse.ply", golden0["rgbd_descs"], golden0["rgbd_features"])
    exp_list = d.match(bgr, depth, THR, class_idx=0)
    assert len(exp_list) > 0
    d.upload_frame(0, bgr, depth)
    d.upload_frame(1, bgr, other)
    d.upload_frame(2, bgr, depth)
    d.upload_frame(3, bgr, depth)
    d.match_begin(1, 2, 1, THR, 0)
    d.match_begin(2, 3, 1, THR, 0)
    slots = [0, 1, 1, 0, 1, 0, 0, 1]
    ks = [0, 1, 2, 3, 0, 1, 2, 2]
    got = d.icp_verify(slots, None, 0, vps[ks])
    for lane, slot in ((1, 2), (2, 3)):
        out, counts = d.match_end(lane, n_slots=1)
        assert counts[0] == len(exp_list)
        assert out[0, :counts[0]].tobytes() == exp_list.tobytes()
    host = d.icp_verify(np.stack([depth, other]), slots, 0, vps[ks])
    for a, b in zip(got, host):
        assert np.array_equal(a, b)
    assert got[0][4] > 500 and got[2][4] == 150.0
    one = d.icp_verify(1, None, 0, vps[:1])                       # an integer slot for every query
    assert (one[0][0], one[1][0], one[2][0]) == (got[0][4], got[1][4], got[2][4])


def test_error_paths(lm, rendered, frame0):
    d, names, vps, renders = rendered
    _, depth = frame0
    with pytest.raises(lm.LinemodError) as e:                    # a mesh that is not resident
        d.icp_verify(depth, 0, 5, vps[:1])
    assert e.value.code == lm.LM_ERR_INVALID
    with pytest.raises(lm.LinemodError) as e:                    # a bad mesh index
        d.icp_verify(depth, 0, 99, vps[:1])
    assert e.value.code == lm.LM_ERR_INVALID
    with pytest.raises(lm.LinemodError) as e:                    # a bad frame index
        d.icp_verify(depth, 1, 0, vps[:1])
    assert e.value.code == lm.LM_ERR_INVALID
    for slot in (-1, 10 ** 6):                                   # a bad slot
        with pytest.raises(lm.LinemodError) as e:
            d.icp_verify(slot, None, 0, vps[:1])
        assert e.value.code == lm.LM_ERR_INVALID
    fresh = lm.Detector(color_only=False)
    try:
        fresh.set_render_mesh(0, np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[0, 1, 2]]))
        with pytest.raises(lm.LinemodError) as e:                # a slot without a frame
            fresh.icp_verify(0, None, 0, vps[:1])
        assert e.value.code == lm.LM_ERR_INVALID
    finally:
        fresh.close()
    colour = lm.Detector(color_only=True)
    try:
        colour.set_render_mesh(0, np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[0, 1, 2]]))
        colour.upload_frame(0, frame0[0])
        with pytest.raises(lm.LinemodError) as e:                # a colour-only detector keeps no depth frame
            colour.icp_verify(0, None, 0, vps[:1])
        assert e.value.code == lm.LM_ERR_INVALID and "colour-only" in str(e.value)
        c, t, m = colour.icp_verify(depth, 0, 0, vps[:1])        # ... the host form works on it
        assert c[0] == 0
    finally:
        colour.close()
    with pytest.raises(lm.LinemodError) as e:                    # w = 0
        d.icp_verify_counts(np.zeros((3, 0), np.uint16), np.zeros((3, 0), np.uint16))
    assert e.value.code == lm.LM_ERR_INVALID
    with pytest.raises(lm.LinemodError) as e:
        d.icp_verify(np.zeros((1, 3, 0), np.uint16), 0, 0, vps[:1])
    assert e.value.code == lm.LM_ERR_INVALID
    c, t, m = d.icp_verify(depth, 0, 0, np.zeros((0, 16), np.float32))    # n = 0 does nothing
    assert len(c) == len(t) == len(m) == 0
    c, t, m = d.icp_verify(0, None, 0, np.zeros((0, 16), np.float32))
    assert len(c) == 0
    c, t, m = d.icp_verify(depth, 0, 0, vps[:1])                 # the detector still works afterwards
    assert (int(c[0]), int(t[0])) == V.verify(renders[0], depth)[:2]
