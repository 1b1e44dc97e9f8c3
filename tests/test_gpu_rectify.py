"""Lens rectification at ingest on the GPU (ABI 0.13 additive): lm_ingest_frames_rectified and lm_stage_rectify on a
160 x 80 RGB-D detector and a 64 x 32 colour-only one over 208 x 120 sources, compared byte for byte -- whole buffers, no tolerance, no
excluded pixel -- with tests/rectify_reference.py (the map and the pixel rule, written from the header) and with ingest_reference's crop,
mirror and shift of the rectified images.  Every source lies in a device allocation of exactly its size, so its last pixel is the
allocation's last byte."""
import ctypes as C

import numpy as np
import pytest

import rectify_reference as QR
import rectify_scenes as S
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

W, H, SW, SH = S.W, S.H, S.SW, S.SH
INVALID = 1
DEPTHS = {"u16": (S.depth_u16, 1.0), "f32": (S.depth_f32, 1000.0)}


def to_cam(lm, c):
    return lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])


class Stage:
    """The detectors, device copies of the sources (cached per format, padding and offset) and the references (computed once)."""

    def __init__(self, lm):
        self.lm = lm
        self.d = lm.Detector(color_only=False, width=W, height=H, frame_slots=6)
        self.mono = lm.Detector(color_only=True, width=S.MW, height=S.MH, T=[2, 8], frame_slots=2)
        self.bufs, self._dev, self._ref = [], {}, {}

    def put(self, host, fmt, pad=0, offset=0):
        """A device copy of a source array: rows `pad` bytes longer than their pixels, the data `offset` bytes into an allocation that
        ends with the image's last byte -> the view image_desc wants."""
        key = (id(host), fmt, pad, offset)
        if key in self._dev:
            return self._dev[key][0]
        planar = fmt.endswith("planar")
        data, rs = S.lay_out(host, pad, planar)
        buf = self.lm.DeviceBuffer(offset + len(data))
        buf.upload(data, offset)
        self.bufs.append(buf)
        item = host.dtype.itemsize
        if planar:
            strides = (host.shape[1] * rs, rs, 1)
        elif host.ndim == 3:
            strides = (rs, host.shape[2], 1)
        else:
            strides = (rs, item)
        view = buf.view(host.dtype.type, host.shape, offset, strides)
        self._dev[key] = (view, host)           # (the host array is kept: its id is the key)
        return view

    def ref(self, key, make):
        if key not in self._ref:
            self._ref[key] = make()
        return self._ref[key]

    def source(self, fmt):
        return self.ref(("src", fmt), lambda: S.source(fmt))

    def bgr(self, fmt):
        return self.ref(("bgr", fmt), lambda: QR.decode(self.source(fmt), fmt, S.flags(fmt)))

    def depth(self, dfmt):
        return self.ref(("depth", dfmt), lambda: DEPTHS[dfmt][0]())

    def rect(self, d, source, ideal, table=None):
        """Sets the rectification; the reference's map."""
        d.set_rectification(to_cam(self.lm, source), to_cam(self.lm, ideal), map=table)
        if table is not None:
            return QR.quant_table(table, source)
        key = ("map", tuple(sorted(source.items())), tuple(sorted(ideal.items())))
        return self.ref(key, lambda: QR.build_map(source, ideal))

    def close(self):
        self.d.close()
        self.mono.close()
        for b in self.bufs:
            b.close()


@pytest.fixture(scope="module")
def stage(lm):
    s = Stage(lm)
    yield s
    s.close()


def frame(stage, fmt, dfmt, crop=(0, 0), flip=False, shift=(0, 0), pad=0, offset=0, **more):
    """ingest_frames' dict of one frame."""
    f = dict(colour=stage.put(stage.source(fmt), fmt, pad, offset), crop=crop, flip_x=flip, shift=shift, **S.DESC[fmt], **more)
    if dfmt:
        item = 2 if dfmt == "u16" else 4
        f.update(depth=stage.put(stage.depth(dfmt), dfmt, pad * item, 0), depth_scale=DEPTHS[dfmt][1])
    return f


def expected(stage, qmap, fmt, dfmt, crop, flip, shift, w=W, h=H):
    Rc = stage.ref(("Rc", fmt, qmap.tobytes()), lambda: QR.rectify_colour(stage.bgr(fmt), qmap))
    exp_d = None
    if dfmt:
        Rd = stage.ref(("Rd", dfmt, qmap.tobytes()), lambda: QR.rectify_depth(stage.depth(dfmt), qmap, DEPTHS[dfmt][1]))
        exp_d = QR.slot_depth(Rd, w, h, crop, flip, shift)
    return QR.slot_colour(Rc, w, h, crop, flip, shift), exp_d


def check_slot(d, slot, exp_bgr, exp_depth, what):
    bgr, depth = d.read_frame(slot)
    assert np.array_equal(bgr, exp_bgr), "%s: colour differs at %d bytes" % (what, int((bgr != exp_bgr).sum()))
    if exp_depth is not None:
        assert np.array_equal(depth, exp_depth), "%s: depth differs at %d pixels" % (what, int((depth != exp_depth).sum()))


GEOMETRY = [((24, 20), False, (0, 0)), ((1, 3), True, (3, -2)), ((47, 39), False, (-5, 4)), ((48, 40), True, (-1, -7)), ((0, 0), False, (2, 9)),
            ((13, 1), True, (0, 0))]


@pytest.mark.parametrize("k", range(len(S.COLOUR_FORMATS)), ids=S.COLOUR_FORMATS)
def test_identity_equals_the_plain_ingest(stage, k):
    """Zero coefficients, the same K, the same size: the map is (32 i, 32 j), every blend has the weights (1024, 0, 0, 0), and the slot holds
    what lm_ingest_frames makes of the same descriptors.  No reference needed: the plumbing against the existing path."""
    d, fmt = stage.d, S.COLOUR_FORMATS[k]
    plain = S.source_cam(S.ZERO)
    stage.rect(d, plain, QR.pinhole_of(plain))
    for n in range(2):
        dfmt = ("u16", "f32")[(k + n) % 2]
        crop, flip, shift = GEOMETRY[(2 * k + n) % len(GEOMETRY)]
        f = frame(stage, fmt, dfmt, crop, flip, shift)
        d.ingest_frames(0, [f])
        d.ingest_frames(1, [dict(f, rectified=True)])
        a, b = d.read_frame(0), d.read_frame(1)
        assert a[0].any() and a[1].any()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "%s %s crop %s flip %s shift %s" % (fmt, dfmt, crop, flip, shift)


@pytest.mark.parametrize("k", range(len(S.COLOUR_FORMATS)), ids=S.COLOUR_FORMATS)
def test_brown_lens(stage, k):
    """k1 = -0.25 with p1, p2 and an ideal camera that sees beyond the source: odd crops (a window that starts on the second pixel and row
    of a chroma pair), mirror, shifts, unaligned data and strides, sources ending at their allocation's end."""
    d, fmt = stage.d, S.COLOUR_FORMATS[k]
    qmap = stage.rect(d, S.source_cam(), S.wide_ideal())
    win = qmap[3:3 + H, 1:1 + W]
    assert (win[:, :, 0] < -32).any() and (win[:, :, 1] < -32).any() and (qmap[:, :, 0] > 32 * SW).any() and (qmap[:, :, 1] > 32 * SH).any()
    assert ((qmap[:, :, 0] & 31) != 0).mean() > 0.5
    frames, exp = [], []
    for n, (crop, flip, shift) in enumerate(GEOMETRY[1:5]):
        dfmt = ("u16", "f32")[(k + n) % 2]
        frames.append(frame(stage, fmt, dfmt, crop, flip, shift, pad=(k + n) % 4, offset=(k + 3 * n + 1) % 4, rectified=True))
        exp.append(expected(stage, qmap, fmt, dfmt, crop, flip, shift))
    d.ingest_frames(0, frames)
    for s, ((crop, flip, shift), (eb, ed)) in enumerate(zip(GEOMETRY[1:5], exp)):
        assert (eb == 0).all(axis=2).sum() > 100 and eb.any()          # part of the window lies outside the source
        check_slot(d, s, eb, ed, "%s crop %s flip %s shift %s" % (fmt, crop, flip, shift))


def test_callers_map(stage):
    """A smooth warp with NaN, infinities, far-outside entries, exact ties and entries on the last row and column strewn in, on both
    detectors: rectification_map() is the reference's quantisation and the slots are the reference's images."""
    table = S.smooth_table(SW, SH)
    for d, w, h, cases in ((stage.d, W, H, [("bgr", "f32"), ("nv12", "u16")]), (stage.mono, S.MW, S.MH, [("rgba", None), ("uyvy", None)])):
        qmap = stage.rect(d, S.source_cam(), QR.pinhole_of(S.source_cam()), table)
        assert np.array_equal(d.rectification_map(), qmap)
        assert (qmap == -64).any() and (qmap[:, :, 0] == 32 * SW + 32).any() and (qmap[:, :, 0] == 32 * (SW - 1)).any() and (qmap[:, :, 1] == 32 * (SH - 1)).any()
        for s, (fmt, dfmt) in enumerate(cases):
            crop = (SW - w - s, SH - h - s)         # flush with the last row and column, and one off
            d.ingest_frames(s, [frame(stage, fmt, dfmt, crop, bool(s), (s, -s), pad=s, offset=s, rectified=True)])
            check_slot(d, s, *expected(stage, qmap, fmt, dfmt, crop, bool(s), (s, -s), w, h), what="caller's map %s" % fmt)


def test_one_call_many_frames(stage):
    """Five slots in two calls back to back (one per copy stream), every slot with another format, crop, mirror and shift, RGB-order and
    YUV sources mixed in one call; a slot outside the calls keeps its frame."""
    d = stage.d
    qmap = stage.rect(d, S.source_cam(), S.wide_ideal())
    rng = np.random.default_rng(9)
    keep = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 3000, (H, W)).astype(np.uint16))
    d.upload_frame(5, *keep)
    plan = [("bgra", "u16"), ("nv21", "f32"), ("rgb_planar", "u16"), ("yuy2", "f32"), ("gray", "u16")]
    frames = [frame(stage, fmt, dfmt, *GEOMETRY[n], pad=n % 4, offset=n % 4, rectified=True) for n, (fmt, dfmt) in enumerate(plan)]
    d.ingest_frames(0, frames[:3])
    d.ingest_frames(3, frames[3:])
    for n, (fmt, dfmt) in enumerate(plan):
        check_slot(d, n, *expected(stage, qmap, fmt, dfmt, *GEOMETRY[n]), what="slot %d (%s)" % (n, fmt))
    check_slot(d, 5, keep[0], keep[1], "the slot outside the calls")


@pytest.mark.parametrize("size", [(67, 45), (1, 1), (16, 1), (17, 3)], ids=lambda s: "%dx%d" % s)
def test_stage_hook_at_awkward_sizes(stage, size):
    """The whole rectified images at ideal geometries that are no multiple of anything: the kernel's row tails."""
    d = stage.d
    qmap = stage.rect(d, S.source_cam(), S.ideal_cam(*size))
    assert qmap.shape == (size[1], size[0], 2)
    for fmt, dfmt in (("bgr", "f32"), ("nv12", "u16"), ("rgba", "u16")):
        colour, depth = stage.put(stage.source(fmt), fmt, 1, 3), stage.put(stage.depth(dfmt), dfmt)
        Rc, Rd = QR.rectify_colour(stage.bgr(fmt), qmap), QR.rectify_depth(stage.depth(dfmt), qmap, DEPTHS[dfmt][1])
        for c_on, d_on in ((True, False), (False, True), (True, True)):
            got = d.stage_rectify(colour if c_on else None, depth if d_on else None, depth_scale=DEPTHS[dfmt][1], **S.DESC[fmt])
            assert (got[0] is None) == (not c_on) and (got[1] is None) == (not d_on)
            if c_on:
                assert np.array_equal(got[0], Rc), "%s at %s" % (fmt, size)
            if d_on:
                assert np.array_equal(got[1], Rd), "%s at %s" % (dfmt, size)


def test_rescale(stage):
    """An ideal geometry of another size (176 x 96): a pure rescale through the slots."""
    d = stage.d
    qmap = stage.rect(d, S.source_cam(S.ZERO), S.ideal_cam(176, 96))
    d.ingest_frames(0, [frame(stage, "rgb", "u16", (16, 16), True, (1, 1), rectified=True), frame(stage, "uyvy", "f32", (3, 5), rectified=True)])
    check_slot(d, 0, *expected(stage, qmap, "rgb", "u16", (16, 16), True, (1, 1)), what="rescale rgb")
    check_slot(d, 1, *expected(stage, qmap, "uyvy", "f32", (3, 5), False, (0, 0)), what="rescale uyvy")


def test_registered_route(stage):
    """REGISTERED: the depth plane is lm_ingest_frames_registered's for the same raw depth, the colour plane the rectified reference; refused
    when the registration's colour camera has another size than the ideal camera."""
    import register_scenes as RS
    lm, d = stage.lm, stage.d
    ideal = S.wide_ideal()
    qmap = stage.rect(d, S.source_cam(), ideal)
    dc = RS.depth_cam_a(RS.DIST)
    d.set_registration(to_cam(lm, dc), to_cam(lm, ideal), RS.ROT, RS.TRANS, splat=(1, 1))
    raw = stage.put(RS.scene_a(), "f32")
    crop = (23, 7)
    f = frame(stage, "nv12", None, crop, True, (2, -1), pad=1, offset=1)
    d.ingest_frames(0, [dict(f, depth=raw, register_depth=True)])
    d.ingest_frames(1, [dict(f, depth=raw, rectified=True, registered=True)])
    plain, both = d.read_frame(0), d.read_frame(1)
    assert (plain[1] != 0).sum() > 5000
    assert np.array_equal(both[1], plain[1]), "the registered depth plane differs"
    assert np.array_equal(both[0], expected(stage, qmap, "nv12", None, crop, True, (2, -1))[0]) and not np.array_equal(both[0], plain[0])
    stage.rect(d, S.source_cam(), S.ideal_cam(176, 96))
    with pytest.raises(lm.LinemodError) as e:
        d.ingest_frames(1, [dict(f, depth=raw, crop=(0, 0), rectified=True, registered=True)])
    assert e.value.code == INVALID and str(e.value).endswith("rectification: the registration's colour camera (208 x 120) is not the ideal camera (176 x 96)")
    d.set_registration(None, None, None, None)
    with pytest.raises(lm.LinemodError) as e:
        d.ingest_frames(1, [dict(f, depth=raw, crop=(0, 0), rectified=True, registered=True)])
    assert e.value.code == INVALID and str(e.value).endswith("no registration set: lm_set_registration first")
    assert np.array_equal(d.read_frame(1)[0], both[0])          # (the refusals enqueued nothing)


def test_it_is_an_upload_like_any_other(lm, orc, synth):
    """match_slot right after a rectified ingest, no explicit wait, equals record for record the match of the reference-rectified frame
    uploaded from the host; the bank is learned from that frame's crops."""
    RW, RH, THR = 320, 240, 75.0
    d = lm.Detector(color_only=False, width=RW, height=RH, frame_slots=2)
    bgr, depth = synth.make_frame(RW, RH, seed=501)
    source = QR.cam(RW, RH, 300.0, 300.0, 159.5, 119.5, (-0.12, 0.03, 0.002, -0.001, 0.0))
    ideal = QR.pinhole_of(source)
    qmap = QR.build_map(source, ideal)
    d.set_rectification(to_cam(lm, source), to_cam(lm, ideal))
    rb, rd = QR.rectify_colour(bgr, qmap), QR.rectify_depth(depth, qmap)
    assert not np.array_equal(rb, bgr) and (rd != 0).sum() > 1000
    o = orc.Detector(color_only=False)
    o.prepare(rb, rd)
    q = {(l, m): o.stage(0, l, m).reshape(RH >> l, RW >> l) for l in range(2) for m in range(2)}
    descs, feats, _ = synth.make_bank(40, 2, 2, seed=99, size_range=(48, 120), quantized=q, crop_fraction=0.3, frame_size=(RW, RH), T0=d.get_T(0))
    d.add_class("c", descs, feats)
    cb, db = lm.DeviceBuffer(bgr.nbytes), lm.DeviceBuffer(depth.nbytes)
    cb.upload(bgr)
    db.upload(depth)
    d.ingest_frame(1, cb.view(np.uint8, bgr.shape), db.view(np.uint16, depth.shape), rectified=True)
    m1 = d.match_slot(1, THR, 0)
    d.upload_frame(0, rb, rd)
    m0 = d.match_slot(0, THR, 0)
    assert len(m0) > 0
    assert_matches_equal(m1, m0)
    got = d.read_frame(1)
    assert np.array_equal(got[0], rb) and np.array_equal(got[1], rd)
    d.close()
    cb.close()
    db.close()


def test_set_ingest_set_another_ingest(stage):
    """The second call uses the second map, with no wait in between; clearing the rectification makes the rectified call refuse."""
    lm, d = stage.lm, stage.d
    f = frame(stage, "bgr", "u16", S.CROP, rectified=True)
    first = stage.rect(d, S.source_cam(), S.wide_ideal())
    d.ingest_frames(0, [f])
    second = stage.rect(d, S.source_cam((0.1, 0.0, -0.01, 0.02, 0.0)), S.ideal_cam())
    d.ingest_frames(1, [f])
    assert not np.array_equal(first, second)
    check_slot(d, 0, *expected(stage, first, "bgr", "u16", S.CROP, False, (0, 0)), what="the first map")
    check_slot(d, 1, *expected(stage, second, "bgr", "u16", S.CROP, False, (0, 0)), what="the second map")
    d.set_rectification(None)
    with pytest.raises(lm.LinemodError) as e:
        d.ingest_frames(1, [f])
    assert e.value.code == INVALID and str(e.value).endswith("rectification: no rectification set: lm_set_rectification first")
    with pytest.raises(lm.LinemodError) as e:
        d.stage_rectify(f["colour"])
    assert e.value.code == INVALID and str(e.value).endswith("rectification: no rectification set: lm_set_rectification first")
    check_slot(d, 1, *expected(stage, second, "bgr", "u16", S.CROP, False, (0, 0)), what="after the refusal")


def test_refusals(stage):
    """Every refusal of lm_ingest_frames_rectified with its words, before anything is enqueued: the slot holds what it held."""
    lm, d = stage.lm, stage.d
    lib = d.lib
    stage.rect(d, S.source_cam(), S.ideal_cam(176, 96))
    f = frame(stage, "bgr", "u16", (3, 5))
    good_c = lm.image_desc(f["colour"], crop=(3, 5))
    good_d = lm.image_desc(f["depth"], depth=True, crop=(3, 5))

    def call(edit_c=None, edit_d=None, first=3, route=0):
        ca, da = (lm.ImageDesc * 1)(), (lm.ImageDesc * 1)()
        for arr, base, edit in ((ca, good_c, edit_c), (da, good_d, edit_d)):
            C.memmove(C.byref(arr[0]), C.byref(base), C.sizeof(lm.ImageDesc))
            for name, value in (edit or {}).items():
                setattr(arr[0], name, value)
        rc = lib.lm_ingest_frames_rectified(d.h, first, 1, ca, da, None, route, None)
        return rc, (lib.lm_last_error().decode() if rc else "")

    assert call() == (0, "")
    before = d.read_frame(3)
    for route in (2, -1):
        assert call(route=route) == (INVALID, "rectification: unknown depth_route %d" % route)
    for who, key in (("colour", "edit_c"), ("depth", "edit_d")):
        for w_, h_ in ((207, 120), (208, 119), (176, 96)):
            assert call(**{key: {"width": w_, "height": h_}}) == \
                (INVALID, "rectification: %s image of frame 0: a %d x %d image is not the source camera (208 x 120)" % (who, w_, h_))
        for cx, cy in ((-1, 0), (0, -1), (176 - W + 1, 0), (0, 96 - H + 1), (1 << 30, 0)):
            assert call(**{key: {"crop_x": cx, "crop_y": cy}}) == \
                (INVALID, "rectification: %s image of frame 0: window %d x %d at (%d, %d) lies outside the 176 x 96 ideal geometry" % (who, W, H, cx, cy))
    assert call(edit_c={"row_stride": 3 * SW - 1}) == (INVALID, "rectification: colour image of frame 0: row_stride smaller than a source row")
    # lm_ingest_frames' own refusals, in its words
    assert call(edit_c={"format": lm.PIX_DEPTH_U16}) == (INVALID, "colour image of frame 0: LM_PIX_DEPTH_U16 is a depth format")
    assert call(edit_d={"format": lm.PIX_NV12}) == (INVALID, "depth image of frame 0: LM_PIX_NV12 is a colour format")
    assert call(edit_c={"format": 99}) == (INVALID, "colour image of frame 0: unknown pixel format 99")
    assert call(edit_c={"data": None}) == (INVALID, "colour image of frame 0: null data pointer")
    assert call(edit_d={"data": good_d.data + 1}) == (INVALID, "depth image of frame 0: data and row_stride of a u16 source must be multiples of 2")
    assert call(edit_d={"format": lm.PIX_DEPTH_F32, "scale": 0.0, "row_stride": 4 * SW}) == (INVALID, "depth image of frame 0: scale must be finite and positive")
    assert call(edit_c={"format": lm.PIX_NV12, "height": 119})[0] == INVALID
    assert call(first=6) == (INVALID, "slot out of range")
    d.upload_wait(3)
    after = d.read_frame(3)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_resources(lm):
    """A detector that rectified, on two copy streams, with two maps and through the stage hook, gives everything back."""
    start = lm.live_resources()
    for cycle in range(2):
        d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
        d.set_rectification(to_cam(lm, S.source_cam()), to_cam(lm, S.wide_ideal()))
        bgr, dep = S.source("bgr"), S.depth_u16()
        cb, db = lm.DeviceBuffer(bgr.nbytes), lm.DeviceBuffer(dep.nbytes)
        cb.upload(bgr)
        db.upload(dep)
        f = dict(colour=cb.view(np.uint8, bgr.shape), depth=db.view(np.uint16, dep.shape), crop=S.CROP, rectified=True)
        d.ingest_frames(0, [f])
        d.ingest_frames(1, [f])
        d.set_rectification(to_cam(lm, S.source_cam()), to_cam(lm, S.ideal_cam(176, 96)))
        d.ingest_frames(0, [dict(f, crop=(0, 0))] * 4)
        d.stage_rectify(f["colour"], f["depth"])
        d.upload_wait(-1)
        assert lm.live_resources()[0] > start[0] + 2
        steady = lm.live_resources()
        d.ingest_frames(0, [dict(f, crop=(0, 0))] * 4)
        d.upload_wait(-1)
        assert lm.live_resources() == steady, "a rectified ingest in the steady state created or released a resource"
        d.close()
        cb.close()
        db.close()
        assert lm.live_resources() == start, (cycle, lm.live_resources(), start)
