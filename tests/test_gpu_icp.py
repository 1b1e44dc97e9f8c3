"""ICP pose refinement on the GPU (lm_k_icp.hip) against the numpy restatement of the contract (tests/icp_reference.py,
DESIGN.md section 9): scene clouds bit for bit, normals by tolerance, refined poses within 1e-4 rad and 0.01 mm."""
import os

import numpy as np
import pytest

import icp_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
K0 = (1044.87, 1045.69141, 320.0, 240.0)       # linemod_settings.yml
THR = 80.0

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mesh():
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


def assert_pose_close(got, exp):
    for a, b in zip(got.reshape(-1, 4, 4), exp.reshape(-1, 4, 4)):
        assert R.rotation_angle(a[:3, :3], b[:3, :3]) < 1e-4, (a, b)
        assert np.abs(a[:3, 3] - b[:3, 3]).max() < 0.01, (a[:3, 3], b[:3, 3])
        assert np.array_equal(a[3], [0, 0, 0, 1])


def assert_scene_equal(got, depth, K, bbox, step):
    pts = R.scene_points(depth, K, bbox, step)
    assert got.shape == (len(pts), 6)
    assert got[:, :3].tobytes() == pts.tobytes(), "scene positions differ from the reference"
    nrm, dk, dk1 = R.normals(pts)
    sure = dk1 > dk                                           # the 12th and 13th neighbour distances differ: the neighbour set is unique
    assert sure.mean() > 0.5
    dots = np.abs((got[:, 3:].astype(np.float64) * nrm).sum(1))
    assert (dots[sure] >= 1 - 1e-6).all(), np.sort(dots[sure])[:5]
    assert np.allclose(np.linalg.norm(got[:, 3:], axis=1), 1, atol=1e-6)


def scene_for_reference(d, depth, K, bbox, step):
    """The reference refines the GPU's own scene cloud: its positions are bit-identical to the reference's (checked above), its
    normals agree by tolerance where the neighbour set is unique, and where it is not (12th and 13th distances equal, or two
    nearly equal small eigenvalues) a different but equally valid normal would move the pose.  The ICP rounds are compared alone."""
    got = d.icp_scene_cloud(depth, bbox, K, step)
    assert got[:, :3].tobytes() == R.scene_points(depth, K, bbox, step).tobytes()
    return got


@pytest.mark.parametrize("bbox,step", [((266, 238, 112, 112), 2), ((250, 200, 90, 70), 3), ((0, 0, 64, 48), 2), ((576, 432, 64, 48), 1),
                                       ((300, 260, 41, 37), 2)])
def test_scene_cloud_frame0_bit_identical(lm, frame0, bbox, step):
    _, depth = frame0
    d = lm.Detector(color_only=False)
    got = d.icp_scene_cloud(depth, bbox, K0, step)
    assert_scene_equal(got, depth, K0, bbox, step)
    d.close()


def test_scene_cloud_off_centre_principal_point(lm, frame0):
    _, depth = frame0
    K = (1044.87, 1045.69141, 301.5, 251.25)
    d = lm.Detector(color_only=False)
    got = d.icp_scene_cloud(depth, (240, 220, 100, 90), K, 2)
    assert_scene_equal(got, depth, K, (240, 220, 100, 90), 2)
    d.close()


def test_refine_frame0_from_true_and_perturbed_poses(lm, frame0, mesh):
    """frame0 of the benchmark, slot path: the resident frame (unshifted: cx = w/2, cy = h/2 as shipped) and K' = (fx, fy, w/2, h/2)."""
    bgr, depth = frame0
    _, _, xyzn, G = mesh
    bbox = (262, 232, 120, 120)
    poses = np.stack([G, perturbed(G, 0, 3, [4, -6, 10]), perturbed(G, 1, -4, [-8, 5, 12])])
    d = lm.Detector(color_only=False)
    d.icp_set_model(0, xyzn, 2)
    d.upload_frame(0, bgr, depth)
    got = d.icp_refine(0, bbox, 0, poses, K0)
    scene = scene_for_reference(d, depth, K0, bbox, 2)
    model = R.subsample(xyzn, 2)
    exp = np.stack([R.icp_register(model, scene, P) for P in poses])
    assert_pose_close(got, exp)
    # the host-frame hook computes the same
    got2 = d.icp_refine(depth, bbox, 0, poses, K0)
    assert_pose_close(got2, exp)
    d.close()


def test_refine_rendered_scenes_several_queries_and_poses(lm, mesh):
    """Two synthetic frames (SoftRender-style z-buffer of the mesh) side by side in one depth image: two queries of two and three
    poses in one call; the second object's bbox is given in a frame whose principal point is off centre (host-frame hook)."""
    V, F, xyzn, G = mesh
    K = (1044.87, 1045.69141, 330.0, 236.0)
    G2 = G @ rot(2, 25)
    G2[:3, 3] += [-70, -40, 60]
    depth = np.maximum(R.render_depth(V, F, G, K, 640, 480), 0)
    d2 = R.render_depth(V, F, G2, K, 640, 480)
    depth = np.where((d2 > 0) & ((depth == 0) | (d2 < depth)), d2, depth).astype(np.uint16)
    boxes = []
    for P in (G, G2):
        one = R.render_depth(V, F, P, K, 640, 480)
        ys, xs = np.nonzero(one)
        boxes.append((int(xs.min()) - 6, int(ys.min()) - 6, int(xs.max() - xs.min()) + 13, int(ys.max() - ys.min()) + 13))
    poses = np.stack([perturbed(G, 2, 2, [3, 3, -8]), perturbed(G, 0, -2, [0, 6, 6]),
                      perturbed(G2, 1, 3, [5, 0, 5]), G2, perturbed(G2, 2, -3, [-4, 4, 0])])
    d = lm.Detector(color_only=False)
    d.icp_set_model(0, xyzn, 2)
    d.icp_set_model(3, xyzn, 4)
    got = d.icp_refine(depth, boxes, [0, 3], poses, K, counts=[2, 3])
    exp = []
    for q, (bb, st) in enumerate(zip(boxes, (2, 4))):
        scene = scene_for_reference(d, depth, K, bb, 2)
        model = R.subsample(xyzn, st)
        for P in poses[:2] if q == 0 else poses[2:]:
            exp.append(R.icp_register(model, scene, P))
    assert_pose_close(got, np.stack(exp))
    d.close()


def test_error_paths_return_codes(lm, frame0, mesh):
    bgr, depth = frame0
    _, _, xyzn, G = mesh
    d = lm.Detector(color_only=False)
    P = G[None]
    with pytest.raises(lm.LinemodError) as e:                       # class without a model
        d.icp_refine(depth, (262, 232, 120, 120), 0, P, K0)
    assert e.value.code == lm.LM_ERR_INVALID
    d.icp_set_model(0, xyzn, 2)
    for bb in [(262, 232, 0, 120), (600, 232, 120, 120), (-1, 0, 20, 20), (0, 470, 20, 20)]:
        with pytest.raises(lm.LinemodError) as e:                   # empty / out-of-frame bbox
            d.icp_refine(depth, bb, 0, P, K0)
        assert e.value.code == lm.LM_ERR_INVALID
        with pytest.raises(lm.LinemodError):
            d.icp_scene_cloud(depth, bb, K0, 2)
    with pytest.raises(lm.LinemodError) as e:                       # cloud over capacity
        d.icp_refine(depth, (262, 232, 120, 120), 0, P, K0, max_points=100)
    assert e.value.code == lm.LM_ERR_OVERFLOW
    with pytest.raises(lm.LinemodError) as e:
        d.icp_scene_cloud(depth, (262, 232, 120, 120), K0, 2, cap=10)
    assert e.value.code == lm.LM_ERR_OVERFLOW
    empty = np.zeros_like(depth)
    with pytest.raises(lm.LinemodError) as e:                       # a cloud of fewer than 6 points: the pose stays as it was
        d.icp_refine(empty, (100, 100, 2, 2), 0, P, K0)
    assert e.value.code == lm.LM_ERR_INVALID and "fewer than 6" in str(e.value)
    with pytest.raises(lm.LinemodError):                            # slot without a frame
        d.icp_refine(1, (262, 232, 120, 120), 0, P, K0)
    with pytest.raises(lm.LinemodError):
        d.icp_set_model(1, xyzn[:10], 2)
    # the detector still works afterwards
    got = d.icp_refine(depth, (262, 232, 120, 120), 0, P, K0)
    assert np.isfinite(got).all()
    d.close()


def test_refine_beside_three_lanes_keeps_match_lists(lm, frame0, golden0, mesh):
    """A refine of a resident slot runs on its own stream while three lanes match other slots: their lists equal lm_match's."""
    bgr, depth = frame0
    _, _, xyzn, G = mesh
    d = lm.Detector(color_only=False)
    d.add_class("lagergehaeuse.ply", golden0["rgbd_descs"], golden0["rgbd_features"])
    exp = d.match(bgr, depth, THR, class_idx=0)
    assert len(exp) > 0
    d.icp_set_model(0, xyzn, 2)
    for s in range(4):
        d.upload_frame(s, bgr, depth)
    for lane in range(3):
        d.match_begin(lane, 1 + lane, 1, THR, 0)
    got_pose = d.icp_refine(0, (262, 232, 120, 120), 0, G[None], K0)
    for lane in range(3):
        out, counts = d.match_end(lane, n_slots=1)
        assert counts[0] == len(exp)
        assert out[0, :counts[0]].tobytes() == exp.tobytes()
    alone = d.icp_refine(0, (262, 232, 120, 120), 0, G[None], K0)
    assert np.array_equal(got_pose, alone)
    d.close()


def test_refine_slot_reads_the_shifted_frame_with_centred_principal_point(lm, frame0, mesh):
    """Off-centre camera: PoseDetection uploads the frame translated by (w/2 - cx, h/2 - cy); lm_icp_refine on that slot reads it with
    K' = (fx, fy, w/2, h/2) and ignores the query's cx, cy.  Reference: the same translation of the depth frame, the scene cloud with
    K', the rounds on it."""
    bgr, depth = frame0
    _, _, xyzn, G = mesh
    K = (1044.87, 1045.69141, 301.0, 252.0)
    ox, oy = int(-K[2] + 320), int(-K[3] + 240)                     # (19, -12)
    shifted = np.zeros_like(depth)
    shifted[max(oy, 0):480 + min(oy, 0), max(ox, 0):640 + min(ox, 0)] = depth[max(-oy, 0):480 - max(oy, 0), max(-ox, 0):640 - max(ox, 0)]
    bbox = (262 + ox, 232 + oy, 120, 120)
    Kc = (K[0], K[1], 320.0, 240.0)
    poses = np.stack([G, perturbed(G, 2, 3, [5, 5, -6])])
    d = lm.Detector(color_only=False)
    d.icp_set_model(0, xyzn, 2)
    d.upload_frame_shifted(0, bgr, depth, ox, oy)
    got = d.icp_refine(0, bbox, 0, poses, K)
    scene = scene_for_reference(d, shifted, Kc, bbox, 2)
    model = R.subsample(xyzn, 2)
    exp = np.stack([R.icp_register(model, scene, P) for P in poses])
    assert_pose_close(got, exp)
    # the query's own (cx, cy) on the shifted frame would give another cloud and other poses
    other = R.scene_points(shifted, K, bbox, 2)
    assert other.tobytes() != scene[:, :3].tobytes()
    d.close()


# ---- the selection and tie rules of DESIGN.md section 9 on inputs where they decide the result (tests/icp_fixtures.py).  Each case
# that pins a rule is shown by tests/test_icp_cpu.py to move by at least 10x the tolerance here when that rule is flipped.
import icp_fixtures as F


def unit_dots(got, nrm):
    """|n . n_ref| with the GPU's float normal renormalised in double: its float rounding alone costs 1e-7 of the dot product."""
    g = got[:, 3:].astype(np.float64)
    return np.abs((g / np.linalg.norm(g, axis=1, keepdims=True) * nrm).sum(1))


def refine_vs_reference(d, depth, bbox, K, model, mstep, poses, step=2, **params):
    """GPU refine of a host frame against the reference run on the GPU's own scene cloud."""
    d.icp_set_model(0, model, mstep)
    got = d.icp_refine(depth, bbox, 0, poses, K, step=step, **params)
    scene = scene_for_reference(d, depth, K, bbox, step)
    m = R.subsample(model, mstep)
    exp = np.stack([R.icp_register(m, scene, P, **params) for P in poses])
    assert_pose_close(got, exp)
    return got, exp


@pytest.mark.parametrize("kind", ["steps", "ridge", "box"])
def test_normals_on_exact_ties_match_the_lower_index_rule(lm, kind):
    """Dyadic terraces: every candidate distance is exact in float32, so the 12-NN lists and their ties are the same on both sides;
    every normal with a clear eigen-gap, tied ones included, equals the reference's (12-NN ties to the lower index)."""
    depth = F.dyadic_depth(kind)
    d = lm.Detector(color_only=False)
    got = d.icp_scene_cloud(depth, F.DYADIC_BBOX, F.K_DYADIC, 1)
    pts = R.scene_points(depth, F.K_DYADIC, F.DYADIC_BBOX, 1)
    assert got[:, :3].tobytes() == pts.tobytes()
    assert F.candidate_distances_exact(pts)
    nrm, dk, dk1 = R.normals(pts)
    clear = F.eigen_gap_clear(pts)
    assert ((dk == dk1) & clear).sum() >= 300                 # tie-rich
    dots = unit_dots(got, nrm)
    assert (dots[clear] >= 1 - 1e-9).all(), np.sort(dots[clear])[:5]
    d.close()


@pytest.mark.parametrize("params", F.THRESHOLD_PARAMS, ids=lambda p: ",".join("%s=%s" % kv for kv in sorted(p.items())) or "shipped")
def test_rejection_threshold_is_strict_on_exact_ties(lm, params):
    """Model = the GPU's scene cloud moved 0.25 mm in z, identity pose: every round-one d is the same float, MAD = 0 and the threshold
    equals d.  d < thr keeps no pair and every level stops, so the pose stays the identity; d <= thr would move it 0.25 mm."""
    depth = F.dyadic_depth("box")
    d = lm.Detector(color_only=False)
    scene = d.icp_scene_cloud(depth, F.DYADIC_BBOX, F.K_DYADIC, 2)
    model = F.shifted_model(scene, F.THRESHOLD_SHIFT)
    got, _ = refine_vs_reference(d, depth, F.DYADIC_BBOX, F.K_DYADIC, model, 1, np.eye(4)[None], **params)
    assert F.pose_diff(got[0], np.eye(4)) == (0.0, 0.0)
    d.close()


@pytest.mark.parametrize("case", range(4), ids=["median", "picky_a", "picky_b", "picky_c"])
def test_frame0_rule_cases(lm, case):
    """frame0 with the parameters that expose the lower median (tolerance 0.01, rejection scale 0.05) and the picky tie on duplicate
    model rows (tolerance 0.001 with 10 iterations, or levels 3)."""
    _, depth = F.frame0()
    _, _, xyzn, G = F.mesh_model()
    name, bbox, mstep, P, params, _ = F.frame0_rule_cases(G)[case]
    d = lm.Detector(color_only=False)
    refine_vs_reference(d, depth, bbox, K0, xyzn, mstep, P[None], **params)
    d.close()


@pytest.mark.parametrize("params", [dict(tolerance=0.01, rejection_scale=0.5, iterations=1, levels=8),
                                    dict(tolerance=0.001, rejection_scale=2.5, iterations=6, levels=3),
                                    dict(tolerance=0.01, rejection_scale=0.05, iterations=10, levels=1)],
                         ids=["it1-lv8", "it6-lv3", "it10-lv1"])
def test_frame0_parameter_sweep(lm, params):
    """Every level iterates (levels 3-7 included, k_icp_level_src with large strides and tiny nL) at the tolerances under 0.1."""
    _, depth = F.frame0()
    _, _, xyzn, G = F.mesh_model()
    poses = np.stack([G, F.perturbed(G, 1, -4, [-8, 5, 12])])
    d = lm.Detector(color_only=False)
    refine_vs_reference(d, depth, (292, 262, 60, 60), K0, xyzn, 8, poses, **params)
    d.close()


@pytest.mark.parametrize("bbox,step,n", [((316, 286, 3, 2), 1, 6), ((316, 286, 11, 2), 2, 11), ((316, 286, 4, 3), 1, 12),
                                         ((316, 286, 13, 2), 2, 13), ((270, 250, 17, 15), 1, 255), ((270, 250, 16, 16), 1, 256),
                                         ((270, 250, 5, 103), 2, 257)])
def test_scene_counts_around_the_tile(lm, bbox, step, n):
    """Scene clouds of 6 to 257 points: fewer than 12 neighbours, and one point either side of the 256-point tile of k_icp_normals."""
    _, depth = F.frame0()
    _, _, xyzn, G = F.mesh_model()
    d = lm.Detector(color_only=False)
    got = d.icp_scene_cloud(depth, bbox, K0, step)
    assert len(got) == n
    assert_scene_equal(got, depth, K0, bbox, step)
    poses = np.stack([G, F.perturbed(G, 2, 2, [3, -2, 4])])
    for params in (dict(), dict(tolerance=0.01, rejection_scale=0.5)):
        refine_vs_reference(d, depth, bbox, K0, xyzn, 8, poses, step=step, **params)
    d.close()


@pytest.mark.parametrize("bbox,step,chunks", [((292, 262, 60, 60), 2, 1), ((270, 240, 96, 64), 2, 2), ((160, 180, 320, 210), 10, 4)])
def test_nn_chunks_and_a_bbox_over_65536_pixels(lm, bbox, step, chunks):
    """dst counts of one, two and four 1-NN chunks (2048 dst points each); the last bbox has 67200 pixels, so k_icp_scan and the
    scatter see more than 256 blocks."""
    _, depth = F.frame0()
    _, _, xyzn, G = F.mesh_model()
    d = lm.Detector(color_only=False)
    scene = d.icp_scene_cloud(depth, bbox, K0, step)
    assert max(1, min(32, (len(scene) + 2047) // 2048)) == chunks           # lmk_icp_nn_chunks
    assert_scene_equal(scene, depth, K0, bbox, step)
    refine_vs_reference(d, depth, bbox, K0, xyzn, 8, F.perturbed(G, 0, 2, [3, 4, -5])[None], step=step, tolerance=0.01)
    d.close()


@pytest.fixture(scope="module")
def many_poses():
    """130 poses about the true one on a small frame0 bbox, and the reference's refinement of each (poses are independent)."""
    _, depth = F.frame0()
    _, _, xyzn, G = F.mesh_model()
    rng = np.random.default_rng(7)
    poses = np.stack([F.perturbed(G, int(rng.integers(3)), float(rng.uniform(-3, 3)), rng.uniform(-6, 6, 3)) for _ in range(130)])
    bbox = (300, 270, 40, 40)
    return depth, xyzn, bbox, poses


@pytest.mark.parametrize("np_", [1, 64, 65, 130])
def test_many_poses_in_one_query(lm, many_poses, np_):
    """k_icp_solve and k_icp_finish run 64-thread blocks: 65 and 130 poses are a second and a third block."""
    depth, xyzn, bbox, poses = many_poses
    d = lm.Detector(color_only=False)
    refine_vs_reference(d, depth, bbox, K0, xyzn, 16, poses[:np_])
    d.close()


def test_several_queries_with_uneven_pose_counts(lm, many_poses):
    depth, xyzn, _, poses = many_poses
    boxes = [(300, 270, 40, 40), (292, 262, 48, 36), (310, 280, 30, 30), (300, 270, 40, 40)]
    counts = [3, 0, 70, 1]
    d = lm.Detector(color_only=False)
    d.icp_set_model(0, xyzn, 16)
    d.icp_set_model(2, xyzn, 12)
    classes = [0, 2, 2, 0]
    got = d.icp_refine(depth, boxes, classes, poses[:74], K0, counts=counts)
    exp, first = [], 0
    for bb, c, n in zip(boxes, classes, counts):
        if n:
            scene = scene_for_reference(d, depth, K0, bb, 2)
            m = R.subsample(xyzn, 16 if c == 0 else 12)
            exp += [R.icp_register(m, scene, P) for P in poses[first:first + n]]
        first += n
    assert_pose_close(got, np.stack(exp))
    d.close()


def test_max_points_at_the_scene_count(lm):
    _, depth = F.frame0()
    _, _, xyzn, G = F.mesh_model()
    bbox = (292, 262, 60, 60)
    d = lm.Detector(color_only=False)
    d.icp_set_model(0, xyzn, 8)
    n = len(R.scene_points(depth, K0, bbox, 2))
    a = d.icp_refine(depth, bbox, 0, G[None], K0, max_points=n)
    assert np.array_equal(a, d.icp_refine(depth, bbox, 0, G[None], K0))
    with pytest.raises(lm.LinemodError) as e:
        d.icp_refine(depth, bbox, 0, G[None], K0, max_points=n - 1)
    assert e.value.code == lm.LM_ERR_OVERFLOW
    assert len(d.icp_scene_cloud(depth, bbox, K0, 2, cap=n)) == n
    with pytest.raises(lm.LinemodError) as e:
        d.icp_scene_cloud(depth, bbox, K0, 2, cap=n - 1)
    assert e.value.code == lm.LM_ERR_OVERFLOW
    d.close()


@pytest.mark.parametrize("step", [1, 2, 5])
@pytest.mark.parametrize("bbox", [(0, 0, 640, 40), (0, 440, 640, 40), (0, 0, 40, 480), (600, 0, 40, 480), (0, 0, 640, 120)])
def test_scene_positions_at_every_frame_edge(lm, bbox, step):
    """Bboxes on each frame edge (the blur's REFLECT_101 border) and one of 76800 pixels: positions bit for bit."""
    _, depth = F.frame0()
    d = lm.Detector(color_only=False)
    got = d.icp_scene_cloud(depth, bbox, K0, step)
    pts = R.scene_points(depth, K0, bbox, step)
    assert got.shape == (len(pts), 6) and got[:, :3].tobytes() == pts.tobytes()
    assert np.allclose(np.linalg.norm(got[:, 3:], axis=1), 1, atol=1e-6)
    d.close()


@pytest.mark.parametrize("step", [1, 2, 5])
def test_near_scene_with_holes(lm, step):
    """Mean z under 300 mm: the holes' pixels are kept as duplicate (0, 0, 0) points.  Positions bit for bit; every defined normal
    equals the reference's; a point whose 12 neighbours are all (0, 0, 0) has a zero covariance and gets (1, 0, 0) on both sides."""
    depth = F.near_depth()
    d = lm.Detector(color_only=False)
    got = d.icp_scene_cloud(depth, F.NEAR_BBOX, K0, step)
    pts = R.scene_points(depth, K0, F.NEAR_BBOX, step)
    assert got[:, :3].tobytes() == pts.tobytes()
    zero = (pts == 0).all(1)
    assert zero.sum() >= 13
    nrm, _, _ = R.normals(pts)
    idx, _, _ = R.knn12(pts)
    all_zero = zero[idx].all(1)
    assert all_zero.sum() > 0
    assert np.array_equal(got[all_zero, 3:], np.tile(np.float32([1, 0, 0]), (all_zero.sum(), 1)))
    assert np.array_equal(nrm[all_zero], np.tile([1.0, 0, 0], (all_zero.sum(), 1)))
    clear = F.eigen_gap_clear(pts)
    dots = unit_dots(got, nrm)
    assert (dots[clear] >= 1 - 1e-9).all(), np.sort(dots[clear])[:5]
    d.close()


def test_near_scene_duplicate_dst_points_across_a_chunk_boundary(lm):
    """The near scene at step 1 (3696 points, two 1-NN chunks) has (0, 0, 0) rows in both chunks; the model is the cloud moved by
    0.25 mm, so moved points near the origin tie between duplicate dst rows in both chunks."""
    depth = F.near_depth()
    d = lm.Detector(color_only=False)
    scene = d.icp_scene_cloud(depth, F.NEAR_BBOX, K0, 1)
    zero = np.nonzero((scene[:, :3] == 0).all(1))[0]
    chunk = (len(scene) + 1) // 2
    assert max(1, min(32, (len(scene) + 2047) // 2048)) == 2 and zero.min() < chunk <= zero.max()
    model = F.shifted_model(scene, F.THRESHOLD_SHIFT)
    P = np.eye(4)
    P[:3, 3] = [0.375, -0.25, 0.5]
    for params in (dict(), dict(tolerance=0.01, rejection_scale=0.5)):
        refine_vs_reference(d, depth, F.NEAR_BBOX, K0, model, 1, P[None], step=1, **params)
    d.close()


def test_fronto_parallel_plane_is_singular_on_both_sides(lm):
    """A flat scene at one depth: every normal is exactly (0, 0, -1), so three columns of the point-to-plane system are exactly zero.
    The GPU's elimination meets a zero pivot and gives NaN, numpy's solve reports a singular matrix: both end every level, and the
    pose comes back unchanged.  (A tilted, quantised plane is only badly conditioned; DESIGN.md section 9 leaves it open.)"""
    depth = np.full((480, 640), 1000, np.uint16)
    bbox = (290, 210, 60, 60)
    d = lm.Detector(color_only=False)
    scene = d.icp_scene_cloud(depth, bbox, K0, 2)
    assert np.array_equal(scene[:, 3:], np.tile(np.float32([0, 0, -1]), (len(scene), 1)))
    model = scene.copy()
    model[:, 2] += np.float32(0.125) * (np.arange(len(model)) % 5)
    P = np.eye(4)
    P[:3, 3] = [0.3, -0.2, 0.1]
    for params in (dict(), dict(tolerance=0.01, rejection_scale=0.5)):
        got, exp = refine_vs_reference(d, depth, bbox, K0, model, 1, P[None], **params)
        assert np.array_equal(got[0], P) and np.array_equal(exp[0], P)
    d.close()
