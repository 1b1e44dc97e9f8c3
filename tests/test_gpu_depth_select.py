"""k_depth_select on the GPU (lm_depth_select_begin / _end) against the rule as numpy states it
(tests/depth_select_cases.py: numpy.sort(t.ravel())[k]), byte for byte: the crop shapes and pixel patterns at which the kernel can go
wrong, at the smallest geometry an RGB-D detector accepts (80 x 80); the counter width on a whole 640 x 480 frame of equal pixels; a list
beside depth counts and a colour check in flight; and every refusal with the words lm_last_error gives for it."""
import ctypes as C

import numpy as np
import pytest

import depth_select_cases as DS

pytestmark = pytest.mark.gpu

W, H = 80, 80
# (x, y, w, h) of the crops placed in every frame: 1 x 1, one row, one column, widths 7 / 8 / 9 (the 8-pixel piece's tail), n = 4 (k = 0),
# n = 5 (k = 1) as a row and as a column, n < 256 (idle threads), and one that ends at the frame's last column and last row
PLACES = [(3, 1, 1, 1), (5, 3, 37, 1), (1, 5, 1, 29), (4, 6, 7, 5), (13, 6, 8, 5), (23, 6, 9, 5), (34, 6, 2, 2), (38, 6, 5, 1), (45, 6, 1, 5),
          (4, 14, 11, 13), (47, 40, 33, 40)]
NAMES = sorted(DS.patterns(2, 2))


def frames_and_queries(lm):
    """One frame per pattern family (slot = its index; the LAST slot holds one too): every placed crop filled with the family's values for
    its shape, the rest of the frame random.  Queries: every placed crop at the depth check's rank, and the whole frame at several ranks."""
    rng = np.random.default_rng(11)
    frames, q = [], []
    for slot, name in enumerate(NAMES):
        f = rng.integers(0, 4000, (H, W)).astype(np.uint16)
        for (x, y, w, h) in PLACES:
            f[y:y + h, x:x + w] = DS.patterns(h, w, seed=slot)[name]
            q.append((x, y, x + w, y + h, (w * h) // 5, slot))
        for rank in (0, (W * H) // 5, W * H - 1):                       # more than one pass of the 256 threads over the crop
            q.append((0, 0, W, H, rank, slot))
        frames.append(f)
    return frames, np.array(q, lm.DEPTH_SELECT_QUERY_DTYPE)


def expect(frames, q):
    return np.array([DS.rule(frames[e["slot"]][e["y0"]:e["y1"], e["x0"]:e["x1"]], e["rank"]) for e in q], np.uint16)


@pytest.fixture(scope="module")
def rig(lm):
    frames, q = frames_and_queries(lm)
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=len(frames))
    bgr = np.zeros((H, W, 3), np.uint8)
    for slot, f in enumerate(frames):
        d.upload_frame(slot, bgr, f)
    yield d, frames, q, expect(frames, q)
    d.close()


def test_every_pattern_and_crop_shape_in_one_call(rig):
    """About 150 queries of one call over every slot, mixed sizes: each value equals the numpy rule's."""
    d, frames, q, exp = rig
    got = d.depth_select(q)
    assert got.dtype == np.uint16 and got.tobytes() == exp.tobytes(), [(tuple(e), int(g), int(x)) for e, g, x in zip(q, got, exp) if g != x][:10]
    # the families do what they are for: holes give 65535, the straddling pair lands on either side of the high-byte boundary
    per = len(PLACES) + 3
    for slot, name in enumerate(NAMES):
        vals = exp[slot * per: slot * per + len(PLACES)]
        if name == "holes":
            assert (vals == 65535).all()
        if name == "straddle_above":
            assert (vals == 0x0100).all()
        if name == "straddle_below":
            assert (vals == 0x00FF).all()
        if name == "first_bin":
            assert (vals < 256).all()
        if name == "last_bin":
            assert (vals[[1, 2, 9, 10]] >= 0xFF00).all()


def test_a_shorter_call_after_a_longer_one_and_an_empty_one(rig, lm):
    d, frames, q, exp = rig
    d.depth_select(q)
    idx = [len(q) - 1, 0, 17]
    got = d.depth_select(q[idx])
    assert got.tobytes() == exp[idx].tobytes()
    assert len(d.depth_select(np.zeros(0, lm.DEPTH_SELECT_QUERY_DTYPE))) == 0             # n == 0 is legal
    # empty crops of a non-empty list: 65535 whatever the rank holds
    e = np.array([(5, 5, 5, 9, 3, 0), (5, 5, 9, 5, -2, 1), (0, 0, 0, 0, 0, len(frames) - 1)], lm.DEPTH_SELECT_QUERY_DTYPE)
    assert (d.depth_select(e) == 65535).all()
    # every rank of one small crop: the whole sorted crop comes back
    x, y, w, h = PLACES[9]
    allr = np.array([(x, y, x + w, y + h, r, 3) for r in range(w * h)], lm.DEPTH_SELECT_QUERY_DTYPE)
    crop = frames[3][y:y + h, x:x + w]
    assert np.array_equal(d.depth_select(allr), np.sort(np.where(crop <= 1, 65535, crop).ravel()))


def test_whole_frame_of_equal_pixels_and_a_list_beside_counts_and_a_colour_check(lm, frame0, golden0):
    """640 x 480: a whole-frame crop of 307 200 equal pixels (a 16-bit counter would wrap), and on the golden frame a selection in flight
    beside depth counts and a colour check, each delivering what it delivers alone."""
    bgr, depth = frame0
    h, w = depth.shape
    d = lm.Detector(color_only=False, frame_slots=2)
    d.add_class("lagergehaeuse.ply", golden0["rgbd_descs"], golden0["rgbd_features"])
    d.upload_frame(0, bgr, np.full((h, w), 1234, np.uint16))
    d.upload_frame(1, bgr, depth)
    n = w * h
    q = np.array([(0, 0, w, h, r, 0) for r in (0, n // 5, 65535, 65536, n - 1)] + [(0, 0, w, h, n // 5, 1), (200, 150, 420, 330, (220 * 180) // 5, 1)],
                 lm.DEPTH_SELECT_QUERY_DTYPE)
    exp = np.array([1234] * 5 + [DS.rule(depth, n // 5), DS.rule(depth[150:330, 200:420], (220 * 180) // 5)], np.uint16)
    assert d.depth_select(q).tobytes() == exp.tobytes()
    # the three lists in flight at once
    m = np.zeros(3, lm.MATCH_DTYPE)
    m["x"], m["y"], m["similarity"], m["template_id"] = [260, 100, 300], [230, 60, 200], 90.0, [0, 1, 2]
    slots = np.array([1, 1, 0], np.int32)
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(255, 150, 255)
    alone_in, alone_both = d.color_check_counts_slots(slots, (0, 0, 0), (255, 150, 255), m)
    dq = np.array([(200, 150, 420, 330, 500, 900, 1, 0)], lm.DEPTH_QUERY_DTYPE)
    alone_below, alone_inside = d.depth_counts(dq)
    crop = depth[150:330, 200:420]
    t = np.where(crop <= 1, 65535, crop)
    assert (alone_below[0], alone_inside[0]) == ((t < 500).sum(), ((t >= 500) & (t <= 900)).sum())
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    d._check(d.lib.lm_color_check_begin_slots(d.h, vp(slots), lo, hi, vp(m), len(m)))
    d._check(d.lib.lm_depth_counts_begin(d.h, vp(dq), len(dq)))
    d.depth_select_begin(q)
    below, inside = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    d._check(d.lib.lm_depth_counts_end(d.h, vp(below), vp(inside)))
    gin, gboth = np.zeros(3, np.int64), np.zeros(3, np.int64)
    d._check(d.lib.lm_color_check_end(d.h, vp(gin), vp(gboth)))
    with pytest.raises(lm.LinemodError) as e:                   # the slots a selection in flight reads take no upload
        d.upload_frame(1, bgr, depth)
    assert "slot is read by a depth selection in flight: call lm_depth_select_end first" in str(e.value)
    got = d.depth_select_end()
    assert got.tobytes() == exp.tobytes()
    assert (below[0], inside[0]) == (alone_below[0], alone_inside[0])
    assert np.array_equal(gin, alone_in) and np.array_equal(gboth, alone_both) and gin.min() > 0
    d.upload_frame(1, bgr, depth)                               # ... and take one again afterwards
    d.close()


def test_refusals_name_their_cause(rig, lm):
    d, frames, q, exp = rig
    S = len(frames)
    one = lambda *e: np.array([e], lm.DEPTH_SELECT_QUERY_DTYPE)

    def refused(queries, words):
        with pytest.raises(lm.LinemodError) as e:
            d.depth_select(queries)
        assert e.value.code == lm.LM_ERR_INVALID and words in str(e.value), str(e.value)
        assert words in d.lib.lm_last_error().decode()

    refused(one(0, 0, 4, 4, 0, -1), "slot out of range")
    refused(one(0, 0, 4, 4, 0, S), "slot out of range")
    for crop in [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, W + 1, 4), (0, 0, 4, H + 1), (5, 0, 4, 4), (0, 5, 4, 4)]:
        refused(one(*crop, 0, 0), "crop outside the frame")
    refused(one(0, 0, 4, 4, -1, 0), "rank outside the crop")
    refused(one(0, 0, 4, 4, 16, 0), "rank outside the crop")
    bad_in_a_list = np.concatenate([q[:5], one(0, 0, 4, 4, 16, 0)])
    refused(bad_in_a_list, "query 5: rank outside the crop")
    # null arguments
    assert d.lib.lm_depth_select_begin(d.h, None, 1) == lm.LM_ERR_INVALID and b"null argument" in d.lib.lm_last_error()
    assert d.lib.lm_depth_select_begin(None, q.ctypes.data_as(C.c_void_p), 1) == lm.LM_ERR_INVALID
    assert d.lib.lm_depth_select_end(None, None) == lm.LM_ERR_INVALID
    # no list in flight; a list already in flight; a null value for a list of queries
    assert d.lib.lm_depth_select_end(d.h, None) == lm.LM_ERR_INVALID and b"no depth selection in flight" in d.lib.lm_last_error()
    d.depth_select_begin(q[:3])
    assert d.lib.lm_depth_select_begin(d.h, q.ctypes.data_as(C.c_void_p), 1) == lm.LM_ERR_INVALID
    assert b"a depth selection is in flight: call lm_depth_select_end first" in d.lib.lm_last_error()
    assert d.depth_select_end().tobytes() == exp[:3].tobytes()
    d.depth_select_begin(q[:3])
    assert d.lib.lm_depth_select_end(d.h, None) == lm.LM_ERR_INVALID and b"null argument" in d.lib.lm_last_error()
    # nothing above left anything behind
    assert d.depth_select(q).tobytes() == exp.tobytes()
    # a slot without a frame; a detector without a depth modality
    e = lm.Detector(color_only=False, width=W, height=H, frame_slots=2)
    e.upload_frame(0, np.zeros((H, W, 3), np.uint8), frames[0])
    with pytest.raises(lm.LinemodError) as ex:
        e.depth_select(one(0, 0, 4, 4, 0, 1))
    assert ex.value.code == lm.LM_ERR_INVALID and "no frame uploaded to slot 1" in str(ex.value)
    assert e.depth_select(one(0, 0, 4, 4, 0, 0))[0] == DS.rule(frames[0][:4, :4], 0)
    e.close()
    c = lm.Detector(color_only=True, width=W, height=H, frame_slots=2)
    c.upload_frame(0, np.zeros((H, W, 3), np.uint8))
    with pytest.raises(lm.LinemodError) as ex:
        c.depth_select(one(0, 0, 4, 4, 0, 0))
    assert ex.value.code == lm.LM_ERR_INVALID and "no depth modality" in str(ex.value)
    c.close()
