"""The ICP refinement batched across slots (lm_icp_refine_slots): queries on several slots' frames side by side in
the same launches -- against the numpy restatement of the contract (tests/icp_reference.py) within the project's tolerances, and byte
for byte against the same queries refined one at a time, in another order and in several chunks: a pose's arithmetic must not depend
on the company its query keeps.  Statuses, refusals, the lanes beside it, and lm_icp_verify over four slots in one call."""
import ctypes as C
import threading

import numpy as np
import pytest

import icp_fixtures as F
import icp_reference as R
from test_gpu_icp import THR, assert_pose_close, scene_for_reference

K0 = F.K0
pytestmark = pytest.mark.gpu

BOX_1712 = (292, 262, 60, 60)
BOX_13 = (316, 286, 13, 2)
BOX_2979 = (270, 240, 96, 64)
MANY_BOX = (300, 270, 40, 40)


def nn_chunks(n):
    return max(1, min(32, (n + 2047) // 2048))


def shifted(depth, ox, oy):
    out = np.zeros_like(depth)
    h, w = depth.shape
    out[max(oy, 0):h + min(oy, 0), max(ox, 0):w + min(ox, 0)] = depth[max(-oy, 0):h - max(oy, 0), max(-ox, 0):w - max(ox, 0)]
    return out


@pytest.fixture(scope="module")
def world(lm):
    """A detector with slots 0, 2 and 5 holding frame0, a rendered frame and frame0 shifted by (3, -2) pixels (slot 7: all zero); the five
    queries of the issue; the batch's result and the reference's."""
    bgr, depth = F.frame0()
    V, Fc, xyzn, G = F.mesh_model()
    G2 = G @ F.rot(2, 25)
    G2[:3, 3] += [-40, 20, 60]
    rendered = R.render_depth(V, Fc, G2, K0, F.W, F.H).astype(np.uint16)
    ys, xs = np.nonzero(rendered)
    box2 = (int(xs.min()) - 6, int(ys.min()) - 6, int(xs.max() - xs.min()) + 13, int(ys.max() - ys.min()) + 13)
    frames = {0: depth, 2: rendered, 5: shifted(depth, 3, -2), 7: np.zeros_like(depth)}
    d = lm.Detector(color_only=False, frame_slots=8)
    d.icp_set_model(0, xyzn, 8)
    d.icp_set_model(3, xyzn, 16)
    for s, f in frames.items():
        d.upload_frame(s, bgr, f)
    slots = [0, 2, 0, 5, 0]
    boxes = [BOX_1712, box2, BOX_13, BOX_2979, BOX_1712]
    classes = [0, 3, 0, 0, 0]
    counts = [2, 1, 1, 1, 0]
    poses = np.stack([F.perturbed(G, 0, 3, [4, -6, 10]), F.perturbed(G, 1, -4, [-8, 5, 12]), F.perturbed(G2, 2, 2, [3, 3, -8]),
                      F.perturbed(G, 2, 2, [3, -2, 4]), F.perturbed(G, 0, 2, [3, 4, -5])])
    got, status, rc = d.icp_refine_slots(slots, boxes, classes, poses, K0, counts=counts, return_status=True)
    scene_n = [len(d.icp_scene_cloud(frames[s], bb, K0, 2)) if n else 0 for s, bb, n in zip(slots, boxes, counts)]
    w = dict(scene_n=scene_n, lm=lm, d=d, frames=frames, slots=slots, boxes=boxes, classes=classes, counts=counts, poses=poses, got=got,
             status=status, rc=rc, xyzn=xyzn, G=G, bgr=bgr)
    yield w
    d.close()


def test_five_queries_over_three_slots_against_the_reference(world):
    w = world
    d, lm = w["d"], w["lm"]
    assert w["rc"] == lm.LM_OK and (w["status"] == lm.LM_OK).all()
    assert d.icp_batch_stats()[0] >= 1
    first, scenes, moved = 0, [], []
    for slot, bb, c, n in zip(w["slots"], w["boxes"], w["classes"], w["counts"]):
        if n:
            scene = scene_for_reference(d, w["frames"][slot], K0, bb, 2)        # positions bit-identical to the reference's, asserted there
            scenes.append(len(scene))
            model = R.subsample(w["xyzn"], 8 if c == 0 else 16)
            exp = np.stack([R.icp_register(model, scene, P) for P in w["poses"][first:first + n]])
            assert_pose_close(w["got"][first:first + n], exp)
            moved.append(not np.array_equal(w["got"][first:first + n], w["poses"][first:first + n]))
        first += n
    print("scene points", scenes, "moved", moved)
    assert moved[0] and sum(moved) >= 2              # (the 13-point query may well stop before its first step)
    assert scenes[0] == 1712 and scenes[2] == 13 and nn_chunks(scenes[0]) == 1 and nn_chunks(scenes[3]) == 2
    # a wrong slot would not go unnoticed: the same query on another slot's frame gives another pose
    other = d.icp_refine(0, BOX_2979, 0, w["poses"][4:5], K0)
    assert not np.array_equal(other[0], w["got"][4])


def company_cases(d, lm, slots, boxes, classes, counts, poses, batch):
    """The queries one at a time with lm_icp_refine on their slots, in reversed order in one call, and in several chunks: the same bytes."""
    first = np.concatenate([[0], np.cumsum(counts)])
    for k in range(len(slots)):
        if counts[k]:
            one = d.icp_refine(slots[k], boxes[k], classes[k], poses[first[k]:first[k + 1]], K0)
            assert one.tobytes() == batch[first[k]:first[k + 1]].tobytes(), "query %d alone differs from the batch" % k
    order = list(range(len(slots)))[::-1]
    rp = np.concatenate([poses[first[k]:first[k + 1]] for k in order])
    rev = d.icp_refine_slots([slots[k] for k in order], [boxes[k] for k in order], [classes[k] for k in order], rp, K0,
                             counts=[counts[k] for k in order])
    exp = np.concatenate([batch[first[k]:first[k + 1]] for k in order])
    assert rev.tobytes() == exp.tobytes(), "the reversed call differs from the batch"
    d.set_tuning(lm.TUNE_ICP_BATCH_MB, 1)
    try:
        small = d.icp_refine_slots(slots, boxes, classes, poses, K0, counts=counts)
        chunks = d.icp_batch_stats()[0]
    finally:
        d.set_tuning(lm.TUNE_ICP_BATCH_MB, 512)
    assert chunks > 1, "the smallest budget did not split the call"
    assert small.tobytes() == batch.tobytes(), "the call in %d chunks differs from the batch" % chunks


def test_company_does_not_matter(world):
    w = world
    company_cases(w["d"], w["lm"], w["slots"], w["boxes"], w["classes"], w["counts"], w["poses"], w["got"])


def test_company_does_not_matter_130_poses_in_9_queries_over_8_slots(lm):
    bgr, depth = F.frame0()
    _, _, xyzn, G = F.mesh_model()
    rng = np.random.default_rng(7)
    poses = np.stack([F.perturbed(G, int(rng.integers(3)), float(rng.uniform(-3, 3)), rng.uniform(-6, 6, 3)) for _ in range(130)])
    d = lm.Detector(color_only=False, frame_slots=8)
    d.icp_set_model(0, xyzn, 16)
    for s in range(8):
        d.upload_frame(s, bgr, depth)
    slots = [3, 0, 7, 1, 6, 2, 5, 4, 3]
    counts = [1, 64, 2, 30, 3, 17, 5, 7, 1]
    assert sum(counts) == 130
    boxes = [MANY_BOX] * 9
    batch = d.icp_refine_slots(slots, boxes, 0, poses, K0, counts=counts)
    assert d.icp_batch_stats()[0] == 1
    # every slot holds the same frame: one query of all 130 poses is the same work again
    assert d.icp_refine(0, MANY_BOX, 0, poses, K0).tobytes() == batch.tobytes()
    company_cases(d, lm, slots, boxes, [0] * 9, counts, poses, batch)
    d.close()


def test_statuses_per_query(world):
    w = world
    d, lm = w["d"], w["lm"]
    first = np.concatenate([[0], np.cumsum(w["counts"])])
    # an all-zero slot in the middle of the list, a bbox of four pixels: a cloud of fewer than 6 points (all of them (0, 0, 0))
    slots = w["slots"][:2] + [7] + w["slots"][2:]
    boxes = w["boxes"][:2] + [(100, 100, 2, 2)] + w["boxes"][2:]
    classes = w["classes"][:2] + [0] + w["classes"][2:]
    counts = w["counts"][:2] + [2] + w["counts"][2:]
    extra = np.stack([F.perturbed(w["G"], 1, 1, [1, 2, 3]), w["G"]])
    poses = np.concatenate([w["poses"][:3], extra, w["poses"][3:]])
    got, status, rc = d.icp_refine_slots(slots, boxes, classes, poses, K0, counts=counts, return_status=True)
    assert rc == lm.LM_ERR_INVALID and list(status) == [0, 0, lm.LM_ERR_INVALID, 0, 0, 0]
    msg = d.lib.lm_last_error().decode()
    assert "fewer than 6" in msg and "query 2" in msg
    assert got[3:5].tobytes() == extra.tobytes()
    assert np.concatenate([got[:3], got[5:]]).tobytes() == w["got"].tobytes()
    with pytest.raises(lm.LinemodError) as e:                        # without return_status the first such query raises
        d.icp_refine_slots(slots, boxes, classes, poses, K0, counts=counts)
    assert e.value.code == lm.LM_ERR_INVALID and "fewer than 6" in str(e.value)
    # a cloud over max_points while the others fit: the capacity is the second largest cloud's size
    cap = sorted(w["scene_n"])[-2]
    big = int(np.argmax(w["scene_n"]))
    assert w["scene_n"][big] > cap >= 1712
    over = [lm.LM_ERR_OVERFLOW if k == big else 0 for k in range(5)]
    got, status, rc = d.icp_refine_slots(w["slots"], w["boxes"], w["classes"], w["poses"], K0, counts=w["counts"], max_points=cap,
                                         return_status=True)
    assert rc == lm.LM_ERR_OVERFLOW and list(status) == over
    assert "query %d" % big in d.lib.lm_last_error().decode()
    for k in range(5):
        exp = w["poses"] if k == big else w["got"]
        assert got[first[k]:first[k + 1]].tobytes() == exp[first[k]:first[k + 1]].tobytes()
    # both in one call: the return value is the first non-OK code in query order
    big6 = big + (big >= 2)
    both = [lm.LM_ERR_INVALID if k == 2 else (lm.LM_ERR_OVERFLOW if k == big6 else 0) for k in range(6)]
    got, status, rc = d.icp_refine_slots(slots, boxes, classes, poses, K0, counts=counts, max_points=cap, return_status=True)
    assert list(status) == both and rc == both[min(2, big6)]
    got, status, rc = d.icp_refine_slots(slots[::-1], boxes[::-1], classes[::-1], poses, K0, counts=counts[::-1], max_points=cap,
                                         return_status=True)
    assert list(status) == both[::-1] and rc == both[::-1][min(5 - 2, 5 - big6)]
    # a status of NULL is accepted
    q, prm, sl = raw_call_args(lm, w["slots"], w["boxes"], w["classes"], w["counts"])
    P = w["poses"].copy()
    assert d.lib.lm_icp_refine_slots(d.h, sl.ctypes.data, q, len(w["slots"]), C.byref(prm), P.ctypes.data, None) == lm.LM_OK
    assert P.tobytes() == w["got"].tobytes()
    assert first[-1] == len(P)


def raw_call_args(lm, slots, boxes, classes, counts, camera=K0, **params):
    q = (lm.IcpQuery * max(len(slots), 1))()
    first = 0
    for k, (bb, c, n) in enumerate(zip(boxes, classes, counts)):
        q[k] = lm.IcpQuery(bb[0], bb[1], bb[2], bb[3], c, first, n, 0, *camera)
        first += n
    p = dict(step=2, iterations=6, tolerance=0.1, rejection_scale=2.5, levels=8, max_points=0)
    p.update(params)
    prm = lm.IcpParams(p["step"], p["iterations"], p["tolerance"], p["rejection_scale"], p["levels"], p["max_points"])
    return q, prm, np.asarray(slots, np.int32)


def test_refusals_leave_poses_and_status_untouched(world):
    w = world
    d, lm = w["d"], w["lm"]
    slots, boxes, classes, counts = w["slots"], w["boxes"], w["classes"], w["counts"]
    n = len(slots)

    def refused(det, slots_, boxes_, classes_, counts_, nq=None, null=None, camera=K0, what="", **params):
        q, prm, sl = raw_call_args(lm, slots_, boxes_, classes_, counts_, camera, **params)
        P = w["poses"].copy()
        status = np.full(n, 77, np.int32)
        args = dict(slots=sl.ctypes.data, q=q, prm=C.byref(prm), poses=P.ctypes.data)
        if null:
            args[null] = None
        rc = det.lib.lm_icp_refine_slots(det.h, args["slots"], args["q"], len(slots_) if nq is None else nq, args["prm"], args["poses"],
                                         status.ctypes.data)
        assert rc == lm.LM_ERR_INVALID, (what, rc)
        assert P.tobytes() == w["poses"].tobytes() and (status == 77).all(), what
        msg = det.lib.lm_last_error().decode()
        assert msg, what
        return msg

    def with_(lst, k, v):
        return lst[:k] + [v] + lst[k + 1:]

    for null in ("slots", "q", "prm", "poses"):
        refused(d, slots, boxes, classes, counts, null=null, what="null " + null)
    refused(d, slots, boxes, classes, counts, nq=-1, what="negative query count")
    for bad in (dict(step=0), dict(iterations=-1), dict(levels=0), dict(levels=31), dict(tolerance=-1.0), dict(rejection_scale=0.0),
                dict(max_points=-1)):
        assert "parameters" in refused(d, slots, boxes, classes, counts, what=str(bad), **bad)
    assert "slot" in refused(d, with_(slots, 3, 8), boxes, classes, counts, what="slot out of range")
    assert "slot" in refused(d, with_(slots, 3, -1), boxes, classes, counts, what="negative slot")
    assert "no frame" in refused(d, with_(slots, 1, 4), boxes, classes, counts, what="slot without a frame")
    for bb in [(262, 232, 0, 120), (262, 232, 120, -1), (600, 232, 120, 120), (-1, 0, 20, 20), (0, 470, 20, 20)]:
        assert "bbox" in refused(d, slots, with_(boxes, 2, bb), classes, counts, what=str(bb))
    assert "no ICP model" in refused(d, slots, boxes, with_(classes, 1, 2), counts, what="class without a model")
    assert "no ICP model" in refused(d, slots, boxes, with_(classes, 4, -1), counts, what="negative class")     # (a query without poses is checked too)
    assert "pose range" in refused(d, slots, boxes, classes, with_(counts, 0, -2), what="negative pose count")
    assert "intrinsics" in refused(d, slots, boxes, classes, counts, camera=(0.0, 1045.0, 320.0, 240.0), what="fx = 0")
    assert "intrinsics" in refused(d, slots, boxes, classes, counts, camera=(1044.0, float("nan"), 320.0, 240.0), what="fy = nan")
    colour = lm.Detector(color_only=True)
    try:
        colour.upload_frame(0, w["bgr"])
        assert "colour-only" in refused(colour, [0], [BOX_1712], [0], [1], what="colour-only detector")
    finally:
        colour.close()
    # an ICP call already in flight: while another thread's refinement runs, a call is refused for that reason.  The calls here are ones
    # that are refused anyway (step 0), so that none of them ever holds the claim itself; the library looks at the claim first.
    _, _, xyzn, G = F.mesh_model()
    busy = np.stack([F.perturbed(G, k % 3, 0.05 * k - 2.0, [1, -1, 2]) for k in range(96)])
    done = []
    t = threading.Thread(target=lambda: done.append(d.icp_refine_slots([0] * 4, [(262, 232, 120, 120)] * 4, 0, busy, K0, counts=[24] * 4)))
    hits = 0
    t.start()
    while t.is_alive():
        hits += "already in flight" in refused(d, slots, boxes, classes, counts, what="in flight", step=0)
    t.join()
    assert hits > 0 and len(done) == 1 and np.isfinite(done[0]).all()
    q, prm, sl = raw_call_args(lm, [0], [BOX_13], [0], [0])
    # no claim is left behind: n_queries == 0 is legal, and the batch still gives the same bytes
    assert d.lib.lm_icp_refine_slots(d.h, None, None, 0, C.byref(prm), None, None) == lm.LM_OK
    again = d.icp_refine_slots(slots, boxes, classes, w["poses"], K0, counts=counts)
    assert again.tobytes() == w["got"].tobytes()


def test_batch_refine_beside_three_lanes_keeps_match_lists(lm, frame0, golden0):
    """A batch refinement over three slots runs on its own stream while three lanes match other slots: their lists equal lm_match's."""
    bgr, depth = frame0
    _, _, xyzn, G = F.mesh_model()
    d = lm.Detector(color_only=False, frame_slots=8)
    d.add_class("lagergehaeuse.ply", golden0["rgbd_descs"], golden0["rgbd_features"])
    exp = d.match(bgr, depth, THR, class_idx=0)
    assert len(exp) > 0
    d.icp_set_model(0, xyzn, 8)
    for s in range(6):
        d.upload_frame(s, bgr, depth if s != 1 else shifted(depth, 3, -2))
    slots, boxes = [0, 1, 2], [BOX_1712, BOX_2979, BOX_13]
    poses = np.stack([F.perturbed(G, 0, 3, [4, -6, 10]), F.perturbed(G, 0, 2, [3, 4, -5]), F.perturbed(G, 2, 2, [3, -2, 4])])
    for lane in range(3):
        d.match_begin(lane, 3 + lane, 1, THR, 0)
    got = d.icp_refine_slots(slots, boxes, 0, poses, K0, counts=[1, 1, 1])
    for lane in range(3):
        out, counts = d.match_end(lane, n_slots=1)
        assert counts[0] == len(exp)
        assert out[0, :counts[0]].tobytes() == exp.tobytes()
    alone = d.icp_refine_slots(slots, boxes, 0, poses, K0, counts=[1, 1, 1])
    assert got.tobytes() == alone.tobytes() and not np.array_equal(got, poses)
    d.close()


def test_verify_over_four_slots_in_one_call_equals_the_per_slot_calls(lm, frame0):
    import test_gpu_icp_verify as TV
    bgr, depth = frame0
    m = np.load(F.GOLDEN + "/lagergehaeuse.npz")
    d = lm.Detector(color_only=False, frame_slots=8)
    d.set_render_mesh(0, m["vertices"], m["faces"])
    names, vps = TV._view_projs(m)
    render0 = d.render(0, vps[0], F.W, F.H)[1]
    frames = {1: depth, 3: np.where(render0 > 1, render0 + 150, depth).astype(np.uint16), 4: shifted(depth, 5, 3), 6: shifted(depth, -4, 2)}
    for s, f in frames.items():
        d.upload_frame(s, bgr, f)
    slots = [(1, 3, 4, 6)[(i * 3 + i // 4) % 4] for i in range(22)]
    ks = [(i * 2) % 5 for i in range(22)]
    count, total, mean = d.icp_verify(slots, None, 0, vps[ks])
    seen = set()
    for s in (1, 3, 4, 6):
        idx = [i for i in range(22) if slots[i] == s]
        c, t, mn = d.icp_verify(s, None, 0, vps[[ks[i] for i in idx]])
        hc, ht, hm = d.icp_verify(frames[s], 0, 0, vps[[ks[i] for i in idx]])
        for j, i in enumerate(idx):
            assert (int(count[i]), int(total[i]), float(mean[i])) == (int(c[j]), int(t[j]), float(mn[j])) == (int(hc[j]), int(ht[j]), float(hm[j]))
            seen.add((int(count[i]), int(total[i])))
    assert len(seen) > 6 and count.max() > 500
    d.close()
