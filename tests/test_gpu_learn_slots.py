"""Learning templates from resident frames (lm_add_templates_slots).  Every case uses two detectors of one
configuration: one learns the slots' frames with a single add_templates_slots call, the other with add_template per frame, from the
read_frame copies of the same slots and the same masks.  The template ids, the bounding boxes and get_template at every level and
modality must be equal -- no tolerance anywhere.  Small shapes: 80 x 80 and 160 x 80 with T = [5, 8], 100 x 80 with one level (a width
that is no multiple of 8: the fallback quantisers); frame0 at 640 x 480 also against the oracle's addTemplate."""
import ctypes as C

import numpy as np
import pytest

from conftest import crop_masks

pytestmark = pytest.mark.gpu


def make(lm, color_only, w, h, slots, **kw):
    return lm.Detector(color_only=color_only, width=w, height=h, frame_slots=slots, **kw)


def paint(frame, mask):
    """The object the mask outlines: inside the mask the colours are shifted by half the range and the surface comes 150 mm nearer, so
    the mask's rim lies on a strong edge (the colour features of a masked template are taken from the rim alone)."""
    bgr, depth = frame[0].copy(), frame[1].copy()
    if mask is not None:
        on = mask != 0
        bgr[on] = ((bgr[on].astype(np.int32) + 128) % 256).astype(np.uint8)
        depth[on] = np.where(depth[on] > 200, depth[on] - 150, depth[on])
    return bgr, depth


def assert_same_templates(a, b, ci, tids, name=""):
    L, M = a.pyramid_levels, a.num_modalities
    for tid in tids:
        for level in range(L):
            for mod in range(M):
                x, y = a.get_template(ci, tid, level, mod), b.get_template(ci, tid, level, mod)
                assert x[:2] == y[:2], "%s template %d level %d modality %d: size %r against %r" % (name, tid, level, mod, x[:2], y[:2])
                assert np.array_equal(x[2], y[2]), "%s template %d level %d modality %d: features differ" % (name, tid, level, mod)


def learn_both(lm, a, b, first_slot, slot_masks, host_masks, class_id="obj"):
    """a: one add_templates_slots call; b: add_template per slot from read_frame copies.  Returns (ids, bboxes) after comparing all."""
    ids, bbs = a.add_templates_slots(class_id, first_slot, slot_masks)
    return compare_with_add_template(a, b, first_slot, ids, bbs, host_masks, class_id)


def compare_with_add_template(a, b, first_slot, ids, bbs, host_masks, class_id="obj"):
    exp_ids = []
    for k, m in enumerate(host_masks):
        bgr, depth = a.read_frame(first_slot + k)
        tid, bb = b.add_template(class_id, bgr, depth, m)
        exp_ids.append(tid)
        assert int(ids[k]) == tid, "slot %d: id %d against %d" % (first_slot + k, int(ids[k]), tid)
        assert tuple(int(v) for v in bbs[k]) == tuple(bb), "slot %d: bbox" % (first_slot + k)
    assert a.num_templates() == b.num_templates()
    ci = a.find_class(class_id)
    if ci >= 0:
        assert_same_templates(a, b, ci, [t for t in exp_ids if t >= 0])
    return ids, bbs


@pytest.mark.parametrize("color_only", [False, True])
def test_frame0_eight_slots_and_oracle(lm, orc, frame0, color_only):
    bgr, depth = frame0
    dep = None if color_only else depth
    a, b = make(lm, color_only, 640, 480, 8), make(lm, color_only, 640, 480, 8)
    o = orc.Detector(color_only=color_only)
    masks = crop_masks(640, 480, 11, 8)
    for k in range(8):
        a.upload_frame(k, bgr, dep)
    ids, bbs = learn_both(lm, a, b, 0, masks, masks)
    added = [int(t) for t in ids if t >= 0]
    assert len(added) >= 3 and added == list(range(len(added)))
    for k, m in enumerate(masks):
        otid, obb = o.add_template("obj", bgr, dep, m)
        assert int(ids[k]) == otid and (otid < 0 or tuple(int(v) for v in bbs[k]) == tuple(obb))
    assert_same_templates(a, o, 0, added, "oracle")
    a.close(); b.close()


SMALL = [(80, 80, dict(T=[5, 8])), (160, 80, dict(T=[5, 8])), (100, 80, dict(T=[5], pyramid_levels=1))]


def small_masks(w, h):
    inside = np.zeros((h, w), np.uint8); inside[14:62, 12:w - 14] = 255
    border = np.zeros((h, w), np.uint8); border[0:50, 0:w * 2 // 3] = 255        # touches the top and the left border
    raw = np.zeros((h, w), np.uint8); raw[10:70, 8:w // 2] = 100; raw[10:70, w // 2:w - 8] = 200      # the rim rule works on raw bytes
    return [inside, border, raw, None]


@pytest.mark.parametrize("w,h,kw", SMALL, ids=["80x80", "160x80", "100x80_one_level"])
@pytest.mark.parametrize("color_only", [False, True], ids=["rgbd", "colour"])
def test_small_shapes_and_mask_kinds(lm, synth, color_only, w, h, kw):
    kw = dict(kw, num_features=20, **({} if color_only else dict(depth_num_features=20)))
    a, b = make(lm, color_only, w, h, 4, **kw), make(lm, color_only, w, h, 4, **kw)
    masks = small_masks(w, h)
    for k in range(4):
        bgr, depth = paint(synth.make_frame(w, h, seed=8800 + 7 * k + w, n_shapes=14), masks[k])
        a.upload_frame(k, bgr, None if color_only else depth)
    ids, _ = learn_both(lm, a, b, 0, masks, masks)
    assert (ids >= 0).sum() >= 3, ids
    a.close(); b.close()


def test_mask_sources(lm, synth):
    """A host pointer with a padded stride, a device pointer with a padded stride, and a rule (depth range, grow, rectangle), which must
    equal the same rule's stage_mask_rule output passed as a host mask."""
    w, h = 160, 80
    kw = dict(T=[5, 8], num_features=20, depth_num_features=20)
    a, b = make(lm, False, w, h, 3, **kw), make(lm, False, w, h, 3, **kw)
    m = np.zeros((h, w), np.uint8); m[8:70, 20:140] = 255
    frames = [paint(synth.make_frame(w, h, seed=8900 + k, n_shapes=14), m) for k in range(3)]
    # frame 2: the object alone lies inside the rule's depth range
    frames[2] = (frames[2][0], np.where(m != 0, np.clip(frames[2][1], 600, 900), 1150).astype(np.uint16))
    for k, f in enumerate(frames):
        a.upload_frame(k, *f)
    padded = np.full((h, w + 37), 255, np.uint8); padded[:, :w] = m              # the padding is set: reading it would change the mask
    host_view = padded[:, :w]
    assert host_view.strides == (w + 37, 1)
    dev = lm.DeviceBuffer(h * (w + 64))
    dev.upload(np.pad(m, ((0, 0), (0, 64)), constant_values=255))
    dev_view = dev.view(np.uint8, (h, w), strides=(w + 64, 1))
    rule = lm.make_mask_rule(1, depth_range=(500, 1000), grow=1, rect=(10, 5, 135, 70))
    staged = a.stage_mask_rule(frames[2][0], frames[2][1], lm.make_mask_rule(1, depth_range=(500, 1000), grow=1, rect=(10, 5, 135, 70)))
    assert (m != 0).sum() < (staged != 0).sum() < w * h and not np.array_equal(staged != 0, m != 0)
    ids, _ = learn_both(lm, a, b, 0, [host_view, dev_view, rule], [m, m, staged])
    assert (ids >= 0).all(), ids
    a.close(); b.close(); dev.close()


def test_failing_slot_in_the_middle(lm, synth):
    w, h = 80, 80
    kw = dict(T=[5, 8], num_features=20, depth_num_features=20)
    a, b = make(lm, False, w, h, 3, **kw), make(lm, False, w, h, 3, **kw)
    for k in range(3):
        a.upload_frame(k, *synth.make_frame(w, h, seed=9000 + k, n_shapes=14))
    tiny = np.zeros((h, w), np.uint8); tiny[30:33, 40:43] = 255
    ids, bbs = a.add_templates_slots("obj", 0, [None, tiny, None])       # returns normally: the failure is in the id and in lm_last_error
    assert b"not enough features" in lm.load_library().lm_last_error()
    assert ids.tolist() == [0, -1, 1] and bbs[1].tolist() == [0, 0, 0, 0]
    compare_with_add_template(a, b, 0, ids, bbs, [None, tiny, None])
    a.close(); b.close()


def test_slot_ranges(lm, synth):
    w, h, slots = 80, 80, 4
    kw = dict(T=[5, 8], num_features=20, depth_num_features=20)
    a, b = make(lm, False, w, h, slots, **kw), make(lm, False, w, h, slots, **kw)
    for k in range(slots):
        a.upload_frame(k, *synth.make_frame(w, h, seed=9100 + k, n_shapes=14))
    ids, _ = learn_both(lm, a, b, 2, [None, None], [None, None])              # first_slot > 0
    assert ids.tolist() == [0, 1]
    ids, _ = learn_both(lm, a, b, 0, [None] * slots, [None] * slots)          # n_slots == frame_slots
    assert ids.tolist() == [2, 3, 4, 5]
    before = a.num_templates()
    for first, n in ((0, slots + 1), (1, slots), (-1, 2), (slots, 1)):
        with pytest.raises(lm.LinemodError) as e:
            a.add_templates_slots("obj", first, [None] * n)
        assert e.value.code == lm.LM_ERR_INVALID
    assert a.num_templates() == before
    a.close(); b.close()


def test_ingest_learn_match(lm, frame0):
    """Frames ingested from device memory are learned where they lie and matched right after; the frames and a sticky rule survive.
    frame0 at 640 x 480 with the default configuration, the shape test_known_answer_via_gpu_add_template matches at."""
    bgr, depth = frame0
    w, h, n = 640, 480, 4
    a, b = make(lm, False, w, h, n), make(lm, False, w, h, n)
    dev = lm.DeviceBuffer(w * h * 5)
    dev.upload(bgr); dev.upload(depth, offset=w * h * 3)
    src = dict(colour=dev.view(np.uint8, (h, w, 3)), depth=dev.view(np.uint16, (h, w), offset=w * h * 3))
    a.ingest_frames(0, [src] * n)
    a.set_mask_rule(1, 1, modalities=3, depth_range=(1, 65535), grow=1)
    before = [a.read_frame(k) for k in range(n)]
    for k in range(n):
        assert np.array_equal(before[k][0], bgr) and np.array_equal(before[k][1], depth)
    masks = crop_masks(w, h, 11, 8)[:n]
    ids, bbs = learn_both(lm, a, b, 0, masks, masks)
    added = [k for k in range(n) if ids[k] >= 0]
    assert len(added) >= 2, ids
    for k in range(n):
        after = a.read_frame(k)
        assert after[0].tobytes() == before[k][0].tobytes() and after[1].tobytes() == before[k][1].tobytes()
    r = a.mask_rule(1)
    assert r is not None and (r.modalities, r.use_depth, r.zmin, r.zmax, r.grow) == (3, 1, 1, 65535, 1) and a.mask_rule(0) is None
    got = a.match_slot(0, 90.0)                       # no upload in between: the learned slot is matched as it is
    assert got.tobytes() == b.match(bgr, depth, 90.0).tobytes()
    T0 = a.get_T(0)
    for k in added:
        best = got[got["template_id"] == ids[k]]
        assert len(best) and best[0]["similarity"] == 100.0
        assert abs(int(best[0]["x"]) - int(bbs[k][0])) < T0 and abs(int(best[0]["y"]) - int(bbs[k][1])) < T0
    a.close(); b.close(); dev.close()


def test_refusals_leave_the_bank_alone(lm, synth):
    w, h, slots = 80, 80, 4
    kw = dict(T=[5, 8], num_features=20, depth_num_features=20)
    d = make(lm, False, w, h, slots, **kw)
    c = make(lm, True, w, h, slots, T=[5, 8], num_features=20)
    frames = [synth.make_frame(w, h, seed=9300 + k, n_shapes=14) for k in range(3)]
    for k, f in enumerate(frames):                      # slot 3 stays without a frame
        d.upload_frame(k, *f)
        c.upload_frame(k, f[0])
    ids, _ = d.add_templates_slots("obj", 0, [None])
    assert ids.tolist() == [0]
    lib, n0 = d.lib, d.num_templates()
    ids_buf, bb_buf = np.zeros(4, np.int32), np.zeros((4, 4), np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)

    def refused(call):
        with pytest.raises(lm.LinemodError) as e:
            call()
        assert e.value.code == lm.LM_ERR_INVALID, str(e.value)
        assert d.num_templates() == n0 and c.num_templates() == 0

    # null arguments, n_slots <= 0
    refused(lambda: d._check(lib.lm_add_templates_slots(d.h, None, 0, 1, None, p(ids_buf), p(bb_buf))))
    refused(lambda: d._check(lib.lm_add_templates_slots(d.h, b"obj", 0, 1, None, None, p(bb_buf))))
    refused(lambda: d._check(lib.lm_add_templates_slots(d.h, b"obj", 0, 1, None, p(ids_buf), None)))
    refused(lambda: d._check(lib.lm_add_templates_slots(d.h, b"obj", 0, 0, None, p(ids_buf), p(bb_buf))))
    refused(lambda: d.add_templates_slots("obj", 0, []))
    # a range outside the slots, a slot without a frame
    refused(lambda: d.add_templates_slots("obj", 3, [None, None]))
    refused(lambda: d.add_templates_slots("obj", 2, [None, None]))
    # rules lm_set_mask_rule would refuse: a depth gate on a colour-only detector, a rectangle outside the frame, grow out of range
    refused(lambda: c.add_templates_slots("obj", 0, [lm.make_mask_rule(1, depth_range=(500, 900))]))
    refused(lambda: d.add_templates_slots("obj", 0, [lm.make_mask_rule(1, rect=(40, 40, 60, 60))]))
    refused(lambda: d.add_templates_slots("obj", 0, [lm.make_mask_rule(1, depth_range=(500, 900), grow=17)]))
    # a lane with a match in flight
    d.match_begin(1, 1, 1, 80.0)
    refused(lambda: d.add_templates_slots("obj", 0, [None]))
    d.match_end(1, n_slots=1)
    # slots read by a colour check / by depth counts in flight
    m = np.zeros(1, lm.MATCH_DTYPE)                            # template 0 of class 0 at (10, 10): the check reads slot 0's frame
    m["x"], m["y"], m["similarity"] = 10, 10, 100.0
    sl = np.zeros(1, np.int32)
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(180, 255, 255)
    d._check(lib.lm_color_check_begin_slots(d.h, p(sl), lo, hi, p(m), 1))
    refused(lambda: d.add_templates_slots("obj", 0, [None]))
    ids, _ = d.add_templates_slots("obj", 1, [None])          # a slot the check does not read is learned
    assert ids.tolist() == [n0]
    n0 += 1
    cnt = np.zeros(1, np.int64)
    d._check(lib.lm_color_check_end(d.h, p(cnt), p(cnt.copy())))
    q = np.zeros(1, lm.DEPTH_QUERY_DTYPE)
    q[0] = (10, 10, 60, 50, 500, 900, 2, 0)
    d._check(lib.lm_depth_counts_begin(d.h, p(q), 1))
    refused(lambda: d.add_templates_slots("obj", 2, [None]))
    below = np.zeros(1, np.uint32)
    d._check(lib.lm_depth_counts_end(d.h, p(below), p(below.copy())))
    ids, _ = d.add_templates_slots("obj", 2, [None])
    assert ids.tolist() == [n0]
    d.close(); c.close()


def test_every_resource_is_released(lm, synth):
    w, h = 80, 80
    start = lm.live_resources()
    for cycle in range(2):
        d = make(lm, False, w, h, 2, T=[5, 8], num_features=20, depth_num_features=20)
        for k in range(2):
            d.upload_frame(k, *synth.make_frame(w, h, seed=9400 + k, n_shapes=14))
        m = np.zeros((h, w), np.uint8); m[5:75, 5:75] = 255
        ids, _ = d.add_templates_slots("obj", 0, [m, lm.make_mask_rule(1, depth_range=(1, 65535), hsv_range=([0, 0, 0], [180, 255, 255]))])
        assert (ids >= 0).any()
        assert all(x >= y for x, y in zip(lm.live_resources(), start)) and lm.live_resources() != start
        d.close()
        assert lm.live_resources() == start, (cycle, lm.live_resources(), start)
