"""Area-averaged reduction at ingest on the GPU (ABI 0.13 additive): lm_ingest_frames_reduced and lm_stage_reduce on
the 64 x 32 colour-only detector and the 160 x 80 RGB-D one, compared byte for byte -- whole buffers, no tolerance, no excluded pixel --
with tests/reduce_reference.py (dense weight matrices from the interval definition; the depth rules as loops) and with ingest_reference's
crop, mirror and shift of the reduced images.  Sources are sized just above slot * ratio, so the reduced geometry exceeds the slot by two
or three pixels and a tail of source pixels stays unused; every source lies in a device allocation of exactly its size, so its last
pixel is the allocation's last byte."""
import numpy as np
import pytest

import rectify_reference as QR
import rectify_scenes as S
import reduce_reference as RR
import reduce_scenes as RS
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

W, H, MW, MH = RS.W, RS.H, RS.MW, RS.MH
INVALID = 1
NO_REDUCTION = "reduction: no reduction set: lm_set_reduction first"


def sides(slot_w, slot_h, r, fmt=None):
    """The source size for a slot and a ratio: R = slot + 3 x slot + 2 (or a pixel more where the format wants even sides)."""
    nx, dx, ny, dy = RR.ratio(r)
    w, h = RS.source_size(slot_w, (nx, dx), 3), RS.source_size(slot_h, (ny, dy), 2)
    if fmt and RS.even(fmt):
        w, h = w + (w & 1), h + (h & 1)
    return w, h


class Stage:
    """The detectors, device copies of the sources (cached per source, padding and offset) and the references (computed once)."""

    def __init__(self, lm):
        self.lm = lm
        self.d = lm.Detector(color_only=False, width=W, height=H, frame_slots=6)
        self.mono = lm.Detector(color_only=True, width=MW, height=MH, T=[2, 8], frame_slots=4)
        self.bufs, self._dev, self._ref = [], {}, {}

    def put(self, host, planar=False, pad=0, offset=0):
        """A device copy of a source array: rows `pad` bytes longer than their pixels, the data `offset` bytes into an allocation that
        ends with the image's last byte -> the view image_desc wants."""
        key = (id(host), pad, offset)
        if key in self._dev:
            return self._dev[key][0]
        data, rs = S.lay_out(host, pad, planar)
        buf = self.lm.DeviceBuffer(offset + len(data))
        buf.upload(data, offset)
        self.bufs.append(buf)
        if planar:
            strides = (host.shape[1] * rs, rs, 1)
        elif host.ndim == 3:
            strides = (rs, host.shape[2], 1)
        else:
            strides = (rs, host.dtype.itemsize)
        view = buf.view(host.dtype.type, host.shape, offset, strides)
        self._dev[key] = (view, host)           # (the host array is kept: its id is the key)
        return view

    def ref(self, key, make):
        if key not in self._ref:
            self._ref[key] = make()
        return self._ref[key]

    def colour(self, fmt, w, h):
        """(host array, decoded BGR)"""
        return self.ref(("src", fmt, w, h), lambda: RS.colour(fmt, w, h))

    def depth(self, dfmt, w, h):
        return self.ref(("depth", dfmt, w, h), lambda: RS.depth(dfmt, w, h))

    def reduced_colour(self, fmt, w, h, r):
        return self.ref(("Ac", fmt, w, h, RR.ratio(r)), lambda: RR.reduce_colour(self.colour(fmt, w, h)[1], r))

    def reduced_depth(self, dfmt, w, h, r, rule):
        host, scale = self.depth(dfmt, w, h)
        return self.ref(("Ad", dfmt, w, h, RR.ratio(r), rule), lambda: RR.reduce_depth(host, r, rule, scale))

    def pipeline(self, d, fmt):
        """The raw family runs under its pipeline; every other family with none set (an 8-bit Bayer source would go through it)."""
        if fmt.startswith("raw"):
            d.set_raw_processing(**RS.PIPE_FLOAT)
        else:
            d.set_raw_processing(None)

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


def colour_frame(stage, fmt, w, h, crop=(0, 0), flip=False, shift=(0, 0), pad=0, offset=0, **more):
    host = stage.colour(fmt, w, h)[0]
    return dict(colour=stage.put(host, fmt.endswith("planar"), pad, offset), crop=crop, flip_x=flip, shift=shift, reduced=True, **RS.desc(fmt, w), **more)


def check_slot(d, slot, exp_bgr, exp_depth, what):
    bgr, depth = d.read_frame(slot)
    assert np.array_equal(bgr, exp_bgr), "%s: colour differs at %d bytes" % (what, int((bgr != exp_bgr).sum()))
    if exp_depth is not None:
        assert np.array_equal(depth, exp_depth), "%s: depth differs at %d pixels" % (what, int((depth != exp_depth).sum()))


# crop inside the 3 x 2 pixels of slack, mirror, shifts of either sign and beyond the frame
GEOMETRY = [((0, 0), False, (0, 0)), ((3, 1), True, (3, -2)), ((1, 2), False, (-5, 4)), ((2, 0), True, (-1, -7)), ((3, 2), False, (2, 9)), ((1, 1), True, (0, 0)),
            ((2, 1), False, (MW + 5, 0)), ((0, 2), True, (-7, -(MH + 1)))]


@pytest.mark.parametrize("k", range(len(RS.RATIOS)), ids=[str(r).replace(" ", "") for r in RS.RATIOS])
def test_stage_and_ingest_equal_the_reference(stage, k):
    """Every ratio of the list across one format of each family on the 64 x 32 detector: lm_stage_reduce returns the reference's whole
    reduced image, and the slot holds its window at an odd crop, mirrored and shifted -- data pointer and row stride at changing byte
    alignments, the source ending with its allocation."""
    d, r = stage.mono, RS.RATIOS[k]
    d.set_reduction(r)
    for n, fmt in enumerate(RS.FAMILIES):
        w, h = sides(MW, MH, r, fmt)
        stage.pipeline(d, fmt)
        Ac = stage.reduced_colour(fmt, w, h, r)
        assert Ac.shape[1] >= MW + 3 and Ac.shape[0] >= MH + 2
        pad, offset = (k + n) % 4, (2 * k + n) % 4
        f = colour_frame(stage, fmt, w, h, pad=pad, offset=offset)
        got = d.stage_reduce(f["colour"], **RS.desc(fmt, w))[0]
        assert got.shape == Ac.shape and np.array_equal(got, Ac), "%s ratio %r: the stage hook differs at %d bytes" % (fmt, r, int((got != Ac).sum()))
        for g in range(2):
            crop, flip, shift = GEOMETRY[(3 * k + n + 4 * g) % len(GEOMETRY)]
            d.ingest_frames(g, [dict(f, crop=crop, flip_x=flip, shift=shift)])
            check_slot(d, g, RR.slot_colour(Ac, MW, MH, crop, flip, shift), None, "%s ratio %r crop %s flip %s shift %s" % (fmt, r, crop, flip, shift))
    d.set_raw_processing(None)


@pytest.mark.parametrize("rule", ["nearest", "min_valid"])
@pytest.mark.parametrize("apply", ["both", "colour", "depth"])
def test_rgbd_depth_rules_and_apply(stage, rule, apply):
    """The 160 x 80 RGB-D detector at 9/4 and (3/1, 9/4): both depth rules over u16 and f32 sources, and `apply` = both / colour only /
    depth only -- the image outside `apply` is at slot resolution and takes the plain ingest's window of its own crop."""
    d = stage.d
    for k, (r, cfmt, dfmt) in enumerate((((9, 4), "rgba", "u16"), (((3, 1), (9, 4)), "nv12", "f32"))):
        d.set_reduction(r, colour=apply != "depth", depth=apply != "colour", depth_rule=rule)
        cr = r if apply != "depth" else (1, 1)
        dr = r if apply != "colour" else (1, 1)
        cw, ch = sides(W, H, cr, cfmt)
        dw, dh = sides(W, H, dr)
        Ac, Ad = stage.reduced_colour(cfmt, cw, ch, cr), stage.reduced_depth(dfmt, dw, dh, dr, rule)
        dhost, scale = stage.depth(dfmt, dw, dh)
        if apply == "colour":
            assert np.array_equal(Ad, QR.rectify_depth(dhost, np.stack(np.meshgrid(32 * np.arange(dw), 32 * np.arange(dh)), axis=-1), scale))
        sc, sd = d.stage_reduce(colour_frame(stage, cfmt, cw, ch)["colour"], stage.put(dhost), depth_scale=scale, **RS.desc(cfmt, cw))
        assert np.array_equal(sc, Ac) and np.array_equal(sd, Ad), "stage hook, %s %s ratio %r" % (apply, rule, r)
        for g in range(2):
            crop, flip, shift = GEOMETRY[(k + 3 * g + 1) % 6]
            dcrop = (crop[0] ^ 1, crop[1])
            item = dhost.dtype.itemsize
            f = colour_frame(stage, cfmt, cw, ch, crop, flip, shift, pad=1 + g, offset=4 * g, depth=stage.put(dhost, pad=item * g), depth_crop=dcrop,
                             depth_scale=scale)
            d.ingest_frames(2 + g, [f])
            check_slot(d, 2 + g, RR.slot_colour(Ac, W, H, crop, flip, shift), RR.slot_depth(Ad, W, H, dcrop, flip, shift),
                       "%s %s ratio %r crop %s / %s flip %s shift %s" % (apply, rule, r, crop, dcrop, flip, shift))


def test_only_an_area_average_gives_these_bytes(stage):
    """A 1-pixel checkerboard of 0 / 255 reduced 2/1 is 128 everywhere ((510 + 2) / 4); 1-pixel vertical stripes reduced 3/1 are the
    reference's 85 / 170 pattern; the checkerboard reduced 3/1 is 142 / 113 (five or four bright pixels of nine).  The same sources through
    the rectifier with an ideal camera of a third of the focal length -- the only way to get the whole view into a slot without this route
    -- give none of the 3/1 patterns: its four taps sit on ONE source pixel there and return 0 or 255.  (At exactly 2/1 a bilinear tap at
    the pixel centre is the box filter, so the inequality is asserted at 3/1.)"""
    lm, d = stage.lm, stage.mono
    d.set_raw_processing(None)
    w, h = 3 * (MW + 3), 3 * (MH + 2)
    y, x = np.mgrid[0:h, 0:w]
    board = np.ascontiguousarray((255 * ((x + y) & 1)).astype(np.uint8)[:, :, None].repeat(3, 2))
    stripes = np.ascontiguousarray((255 * (x & 1)).astype(np.uint8)[:, :, None].repeat(3, 2))
    vb, vs = stage.put(board), stage.put(stripes)
    d.set_reduction((2, 1))
    got = d.stage_reduce(vb)[0]
    assert got.shape == (h // 2, w // 2, 3) and (got == 128).all()
    d.ingest_frames(0, [dict(colour=vb, crop=(5, 3), reduced=True)])
    assert (d.read_frame(0)[0] == 128).all()
    d.set_reduction((3, 1))
    exp_s, exp_b = RR.reduce_colour(stripes, (3, 1)), RR.reduce_colour(board, (3, 1))
    assert exp_s[0, :4, 0].tolist() == [85, 170, 85, 170] and exp_b[0, :2, 0].tolist() == [113, 142] and exp_b[1, 0, 0] == 142
    got_s, got_b = d.stage_reduce(vs)[0], d.stage_reduce(vb)[0]
    assert np.array_equal(got_s, exp_s) and np.array_equal(got_b, exp_b)
    d.ingest_frames(1, [dict(colour=vs, crop=(3, 2), flip_x=True, reduced=True)])
    check_slot(d, 1, RR.slot_colour(exp_s, MW, MH, (3, 2), True), None, "stripes 3/1")
    # the rectifier's bytes for the same whole view
    source = QR.cam(w, h, 120.0, 120.0, (w - 1) / 2.0, (h - 1) / 2.0)
    ideal = QR.cam(w // 3, h // 3, 40.0, 40.0, ((w - 1) / 2.0 + 0.5) / 3.0 - 0.5, ((h - 1) / 2.0 + 0.5) / 3.0 - 0.5)
    to = lambda c: lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])
    d.set_rectification(to(source), to(ideal))
    rect_s, rect_b = d.stage_rectify(vs)[0], d.stage_rectify(vb)[0]
    d.set_rectification(None)
    assert rect_s.shape == exp_s.shape
    assert not np.array_equal(rect_s, exp_s) and not np.array_equal(rect_b, exp_b)
    assert set(np.unique(rect_s).tolist()) <= {0, 255} and set(np.unique(exp_s).tolist()) == {85, 170}


@pytest.mark.parametrize("fmt", RS.FAMILIES)
def test_ratio_one_equals_the_plain_ingest(stage, fmt):
    """1 / 1: every span is one pixel of weight 1, and the slot holds what lm_ingest_frames makes of the same descriptors.  No reference
    needed: the plumbing against the existing path."""
    d = stage.d
    stage.pipeline(d, fmt)
    d.set_reduction((1, 1), depth_rule="min_valid")
    w, h = W + 12, H + 8
    for n, dfmt in enumerate(("u16", "f32")):
        dhost, scale = stage.depth(dfmt, w, h)
        crop, flip, shift = [((4, 2), False, (0, 0)), ((11, 7), True, (-3, 5))][n]
        f = colour_frame(stage, fmt, w, h, crop, flip, shift, depth=stage.put(dhost), depth_scale=scale)
        d.ingest_frames(0, [dict(f, reduced=False)])
        d.ingest_frames(1, [f])
        a, b = d.read_frame(0), d.read_frame(1)
        assert a[0].any() and a[1].any()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "%s %s crop %s flip %s shift %s" % (fmt, dfmt, crop, flip, shift)
    d.set_raw_processing(None)


def test_one_call_of_several_frames(stage):
    """One call of six frames with different formats and different source sizes equals the frames ingested one by one."""
    d = stage.d
    d.set_raw_processing(None)
    r = (9, 4)
    d.set_reduction(r, depth_rule="min_valid")
    frames, exp = [], []
    for n, fmt in enumerate(["bgr", "nv12", "rgba", "bayer_grbg", "yuy2", "bgr_planar"]):
        w, h = sides(W, H, r, fmt)
        w, h = w + 2 * n, h + 2 * (n % 3)          # every frame its own size
        dfmt = ("u16", "f32")[n % 2]
        dhost, scale = stage.depth(dfmt, w, h)
        crop, flip, shift = GEOMETRY[n % 6]
        frames.append(colour_frame(stage, fmt, w, h, crop, flip, shift, pad=n % 4, depth=stage.put(dhost), depth_scale=scale))
        exp.append((RR.slot_colour(stage.reduced_colour(fmt, w, h, r), W, H, crop, flip, shift),
                    RR.slot_depth(stage.reduced_depth(dfmt, w, h, r, "min_valid"), W, H, crop, flip, shift)))
    d.ingest_frames(0, frames)
    together = [d.read_frame(k) for k in range(6)]
    for k, f in enumerate(frames):
        d.ingest_frames(k, [f])
    for k in range(6):
        one = d.read_frame(k)
        assert np.array_equal(one[0], together[k][0]) and np.array_equal(one[1], together[k][1]), "frame %d" % k
        check_slot(d, k, exp[k][0], exp[k][1], "frame %d against the reference" % k)


def test_set_ingest_set_another_ingest(stage):
    """The second call uses the second ratio, with no wait in between; clearing the reduction makes the reduced calls refuse, and the
    refusal enqueues nothing."""
    lm, d = stage.lm, stage.mono
    d.set_raw_processing(None)
    w, h = sides(MW, MH, (3, 1))
    f = colour_frame(stage, "bgr", w, h, (1, 1))
    d.set_reduction((3, 1))
    d.ingest_frames(0, [f])
    d.set_reduction((9, 4))
    d.ingest_frames(1, [f])
    first, second = stage.reduced_colour("bgr", w, h, (3, 1)), stage.reduced_colour("bgr", w, h, (9, 4))
    check_slot(d, 0, RR.slot_colour(first, MW, MH, (1, 1)), None, "the first ratio")
    check_slot(d, 1, RR.slot_colour(second, MW, MH, (1, 1)), None, "the second ratio")
    d.set_reduction(None)
    with pytest.raises(lm.LinemodError) as e:
        d.ingest_frames(1, [f])
    assert e.value.code == INVALID and str(e.value).endswith(NO_REDUCTION)
    with pytest.raises(lm.LinemodError) as e:
        d.stage_reduce(f["colour"])
    assert e.value.code == INVALID and str(e.value).endswith(NO_REDUCTION)
    check_slot(d, 1, RR.slot_colour(second, MW, MH, (1, 1)), None, "after the refusal")


def test_refusals_through_the_library(stage):
    """The route's refusals on a live detector, before anything is enqueued: the slot holds what it held."""
    lm, d = stage.lm, stage.d
    d.set_raw_processing(None)
    d.set_reduction((9, 4))
    w, h = sides(W, H, (9, 4))
    dhost, scale = stage.depth("u16", w, h)
    f = colour_frame(stage, "bgr", w, h, (1, 1), depth=stage.put(dhost))
    d.ingest_frames(3, [f])
    before = d.read_frame(3)
    Rw, Rh = w * 4 // 9, h * 4 // 9

    def refused(words, **edit):
        with pytest.raises(lm.LinemodError) as e:
            d.ingest_frames(3, [dict(f, **edit)])
        assert e.value.code == INVALID and str(e.value).endswith(words), str(e.value)

    refused("reduction: colour image of frame 0: window %d x %d at (4, 0) lies outside the %d x %d reduced geometry of a %d x %d source" % (W, H, Rw, Rh, w, h),
            crop=(4, 0), depth_crop=(0, 0))
    refused("reduction: depth image of frame 0: window %d x %d at (0, 3) lies outside the %d x %d reduced geometry of a %d x %d source" % (W, H, Rw, Rh, w, h),
            crop=(0, 0), depth_crop=(0, 3))
    short = stage.lm.DeviceBuffer(3 * w * h)
    stage.bufs.append(short)
    refused("reduction: colour image of frame 0: row_stride smaller than a source row", colour=short.view(np.uint8, (h, w, 3), 0, (3 * w - 1, 3, 1)))
    with pytest.raises(lm.LinemodError) as e:
        d.ingest_frames(6, [f])
    assert e.value.code == INVALID and str(e.value).endswith("slot out of range")
    d.upload_wait(3)
    after = d.read_frame(3)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_it_is_an_upload_like_any_other(lm, orc, synth):
    """match_slot right after a reduced ingest, no explicit wait, equals record for record the match of the reference-reduced frame
    uploaded from the host; the bank is learned from that frame's crops."""
    RW, RH, THR = 320, 240, 75.0
    r = (9, 4)
    d = lm.Detector(color_only=False, width=RW, height=RH, frame_slots=2)
    bgr, depth = synth.make_frame(RW * 9 // 4 + 2, RH * 9 // 4 + 1, seed=501)
    d.set_reduction(r, depth_rule="min_valid")
    rb_whole, rd_whole = RR.reduce_colour(bgr, r), RR.reduce_depth(depth, r, "min_valid")
    rb, rd = RR.slot_colour(rb_whole, RW, RH), RR.slot_depth(rd_whole, RW, RH)
    assert rb.shape == (RH, RW, 3) and (rd != 0).sum() > 1000
    o = orc.Detector(color_only=False)
    o.prepare(rb, rd)
    q = {(l, m): o.stage(0, l, m).reshape(RH >> l, RW >> l) for l in range(2) for m in range(2)}
    descs, feats, _ = synth.make_bank(40, 2, 2, seed=99, size_range=(48, 120), quantized=q, crop_fraction=0.3, frame_size=(RW, RH), T0=d.get_T(0))
    d.add_class("c", descs, feats)
    cb, db = lm.DeviceBuffer(bgr.nbytes), lm.DeviceBuffer(depth.nbytes)
    cb.upload(bgr)
    db.upload(depth)
    d.ingest_frame(1, cb.view(np.uint8, bgr.shape), db.view(np.uint16, depth.shape), reduced=True)
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


def test_resources(lm):
    """A detector that reduced, on two copy streams, with two ratios and through the stage hook, gives everything back."""
    start = lm.live_resources()
    for cycle in range(2):
        d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
        d.set_reduction((9, 4))
        w, h = sides(W, H, (9, 4))
        (bgr, _), (dep, _) = RS.colour("bgr", w, h), RS.depth("u16", w, h)
        cb, db = lm.DeviceBuffer(bgr.nbytes), lm.DeviceBuffer(dep.nbytes)
        cb.upload(bgr)
        db.upload(dep)
        f = dict(colour=cb.view(np.uint8, bgr.shape), depth=db.view(np.uint16, dep.shape), crop=(1, 1), reduced=True)
        d.ingest_frames(0, [f])
        d.ingest_frames(1, [f])
        d.set_reduction((2, 1), depth_rule="min_valid")
        d.ingest_frames(0, [dict(f, crop=(0, 0))] * 4)
        d.stage_reduce(f["colour"], f["depth"])
        d.upload_wait(-1)
        assert lm.live_resources()[0] > start[0] + 2
        steady = lm.live_resources()
        d.ingest_frames(0, [dict(f, crop=(0, 0))] * 4)
        d.upload_wait(-1)
        assert lm.live_resources() == steady, "a reduced ingest in the steady state created or released a resource"
        d.close()
        cb.close()
        db.close()
        assert lm.live_resources() == start, "cycle %d: lm_destroy left %r, the baseline is %r" % (cycle, lm.live_resources(), start)
