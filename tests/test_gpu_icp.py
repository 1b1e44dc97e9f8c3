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
