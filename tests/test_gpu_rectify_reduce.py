"""Rectify and reduce in one ingest pass on the GPU (ABI 0.13 additive): lm_ingest_frames_rectified_reduced and
lm_stage_rectify_reduce on the 64 x 32 colour-only detector and the 160 x 80 RGB-D one, compared byte for byte -- whole buffers, no
tolerance, no excluded pixel -- with the composition of tests/rectify_reference.py and tests/reduce_reference.py
(tests/rectify_reduce_scenes.py) and with ingest_reference's crop, mirror and shift.  The source is rectify_scenes' 208 x 120 camera under
its barrel lens, the ideal camera sees more than the lens delivers, and every test with a lens first asserts on the reference map alone
that at least 40 pixels of its slot window have a footprint in which taps inside and outside the source meet.  Every source lies in a
device allocation of exactly its size, so its last pixel is the allocation's last byte."""
import numpy as np
import pytest

import rectify_reduce_scenes as X
import rectify_reference as QR
import rectify_scenes as S
import reduce_reference as RR
import reduce_scenes as RS
import register_reference as GR
import register_scenes as GS
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

W, H, MW, MH = RS.W, RS.H, RS.MW, RS.MH
SW, SH = S.SW, S.SH
INVALID = 1


def to_cam(lm, c):
    return lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])


class Stage:
    """The detectors, device copies of the sources (cached per source, padding and offset) and the references (computed once)."""

    def __init__(self, lm):
        self.lm = lm
        self.d = lm.Detector(color_only=False, width=W, height=H, frame_slots=6)
        self.mono = lm.Detector(color_only=True, width=MW, height=MH, T=[2, 8], frame_slots=4)
        self.bufs, self._dev = [], {}

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

    def colour(self, fmt):
        """(host array, decoded BGR) of the 208 x 120 source"""
        return X.cached(("gpu src", fmt), lambda: RS.colour(fmt, SW, SH))

    def depth(self, dfmt):
        return X.cached(("gpu depth", dfmt), lambda: RS.depth(dfmt, SW, SH))

    def lens(self, d, iw, ih, dist=S.LENS):
        """Sets the rectification of the scene; the reference's map."""
        source, ideal, qmap = X.lens_map(iw, ih, dist)
        d.set_rectification(to_cam(self.lm, source), to_cam(self.lm, ideal))
        return qmap

    def Ac(self, fmt, qmap, r):
        return X.cached(("Ac", fmt, qmap.shape, qmap[::7, ::5].tobytes(), RR.ratio(r)), lambda: X.reduced_colour(self.colour(fmt)[1], qmap, r))

    def Ad(self, dfmt, qmap, r, rule):
        host, scale = self.depth(dfmt)
        return X.cached(("Ad", dfmt, qmap.shape, qmap[::7, ::5].tobytes(), RR.ratio(r), rule), lambda: X.reduced_depth(host, qmap, r, rule, scale))

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


def colour_frame(stage, fmt, crop=(0, 0), flip=False, shift=(0, 0), pad=0, offset=0, **more):
    host = stage.colour(fmt)[0]
    return dict(colour=stage.put(host, fmt.endswith("planar"), pad, offset), crop=crop, flip_x=flip, shift=shift, rectify_reduce=True, **RS.desc(fmt, SW), **more)


def check_slot(d, slot, exp_bgr, exp_depth, what):
    bgr, depth = d.read_frame(slot)
    assert np.array_equal(bgr, exp_bgr), "%s: colour differs at %d bytes" % (what, int((bgr != exp_bgr).sum()))
    if exp_depth is not None:
        assert np.array_equal(depth, exp_depth), "%s: depth differs at %d pixels" % (what, int((depth != exp_depth).sum()))


# crop inside the 3 x 2 pixels of slack every scene has, mirror, shifts of either sign and beyond the frame
GEOMETRY = [((0, 0), False, (0, 0)), ((3, 1), True, (3, -2)), ((1, 2), False, (-5, 4)), ((2, 0), True, (-1, -7)), ((3, 2), False, (2, 9)), ((1, 1), True, (0, 0)),
            ((2, 1), False, (MW + 5, 0)), ((0, 2), True, (-7, -(MH + 1)))]


def test_the_listed_scenes_straddle_the_source():
    """The three scenes of the specification: taps inside and outside the source meet in at least 40 footprints of the slot window."""
    for (iw, ih), r, (sw, sh), crop in X.LENS_SCENES:
        assert X.ideal_sides(sw, sh, r) == (iw, ih)
        assert X.straddling(X.lens_map(iw, ih)[2], SW, SH, r, sw, sh, crop) >= 40


@pytest.mark.parametrize("k", range(len(RS.RATIOS)), ids=[str(r).replace(" ", "") for r in RS.RATIOS])
def test_stage_and_ingest_equal_the_reference(stage, k):
    """Every ratio of the list across one format of each family on the 64 x 32 detector under the barrel lens: lm_stage_rectify_reduce
    returns the composed reference's whole reduced ideal image, and the slot holds its window at an odd crop, mirrored and shifted -- data
    pointer and row stride at changing byte alignments, the source ending with its allocation.  8/1 runs the 16 x 4 tile, (3/1, 9/4) a
    mixed-axis one."""
    d, r = stage.mono, RS.RATIOS[k]
    iw, ih = X.ideal_sides(MW, MH, r)
    qmap = stage.lens(d, iw, ih)
    assert np.array_equal(d.rectification_map(), qmap)
    d.set_reduction(r)
    for n, fmt in enumerate(RS.FAMILIES):
        stage.pipeline(d, fmt)
        Ac = stage.Ac(fmt, qmap, r)
        assert Ac.shape[1] >= MW + 3 and Ac.shape[0] >= MH + 2
        pad, offset = (k + n) % 4, (2 * k + n) % 4
        f = colour_frame(stage, fmt, pad=pad, offset=offset)
        got = d.stage_rectify_reduce(f["colour"], **RS.desc(fmt, SW))[0]
        assert got.shape == Ac.shape and np.array_equal(got, Ac), "%s ratio %r: the stage hook differs at %d bytes" % (fmt, r, int((got != Ac).sum()))
        for g in range(2):
            crop, flip, shift = GEOMETRY[(3 * k + n + 4 * g) % len(GEOMETRY)]
            assert X.straddling(qmap, SW, SH, r, MW, MH, crop) >= 40
            d.ingest_frames(g, [dict(f, crop=crop, flip_x=flip, shift=shift)])
            check_slot(d, g, RR.slot_colour(Ac, MW, MH, crop, flip, shift), None, "%s ratio %r crop %s flip %s shift %s" % (fmt, r, crop, flip, shift))
    d.set_raw_processing(None)


@pytest.mark.parametrize("rule", ["nearest", "min_valid"])
@pytest.mark.parametrize("apply", ["both", "colour", "depth"])
def test_rgbd_depth_rules_and_apply(stage, rule, apply):
    """The 160 x 80 RGB-D detector in the 9/4 scene, DEPTH_ALIGNED: both depth rules over u16 and f32 sources, and `apply` = both /
    colour only / depth only -- the image outside `apply` takes the rectified rule alone, its crop in the 372 x 190 ideal geometry."""
    d = stage.d
    d.set_raw_processing(None)
    r = (9, 4)
    qmap = stage.lens(d, *X.ideal_sides(W, H, r))
    d.set_reduction(r, colour=apply != "depth", depth=apply != "colour", depth_rule=rule)
    cr = r if apply != "depth" else (1, 1)
    dr = r if apply != "colour" else (1, 1)
    for k, (cfmt, dfmt) in enumerate((("rgba", "u16"), ("nv12", "f32"))):
        Ac, Ad = stage.Ac(cfmt, qmap, cr), stage.Ad(dfmt, qmap, dr, rule)
        dhost, scale = stage.depth(dfmt)
        if apply == "colour":
            assert np.array_equal(Ad, QR.rectify_depth(dhost, qmap, scale))
        if apply == "depth":
            assert np.array_equal(Ac, QR.rectify_colour(stage.colour(cfmt)[1], qmap))
        sc, sd = d.stage_rectify_reduce(colour_frame(stage, cfmt)["colour"], stage.put(dhost), depth_scale=scale, **RS.desc(cfmt, SW))
        assert np.array_equal(sc, Ac) and np.array_equal(sd, Ad), "stage hook, %s %s" % (apply, rule)
        for g in range(2):
            crop, flip, shift = GEOMETRY[(k + 3 * g + 1) % 6]
            # an image at the ideal resolution: its window reaches from the corner, where the lens leaves the source, inwards
            ccrop = crop if apply != "depth" else (crop[0] + 1, crop[1] + 3)
            dcrop = (crop[0] ^ 1, crop[1]) if apply != "colour" else (Ad.shape[1] - W - crop[0], Ad.shape[0] - H - crop[1])
            assert X.straddling(qmap, SW, SH, cr, W, H, ccrop) >= 40
            item = dhost.dtype.itemsize
            f = colour_frame(stage, cfmt, ccrop, flip, shift, pad=1 + g, offset=4 * g, depth=stage.put(dhost, pad=item * g), depth_crop=dcrop, depth_scale=scale)
            d.ingest_frames(2 + g, [f])
            check_slot(d, 2 + g, RR.slot_colour(Ac, W, H, ccrop, flip, shift), RR.slot_depth(Ad, W, H, dcrop, flip, shift),
                       "%s %s crop %s / %s flip %s shift %s" % (apply, rule, ccrop, dcrop, flip, shift))


def registration_for(stage, d, r, splat=(1, 1)):
    """Sets the registration onto the colour image's geometry of this route: the ideal camera reduced by r, zero coefficients.  Returns
    (the colour camera as register_reference wants it, the detector's own ray table)."""
    source, ideal, _ = X.lens_map(*X.ideal_sides(W, H, (9, 4)))
    cc = stage.lm.reduced_camera(to_cam(stage.lm, ideal), r)
    d.set_registration(to_cam(stage.lm, GS.depth_cam_a(GS.DIST)), cc, GS.ROT, GS.TRANS, splat=splat)
    return GR.cam(cc.width, cc.height, cc.fx, cc.fy, cc.cx, cc.cy), d.registration_rays()


@pytest.mark.parametrize("apply", ["both", "depth"])
def test_registered_depth_beside_it(stage, apply):
    """DEPTH_REGISTERED: the depth plane equals, byte for byte, what lm_ingest_frames_registered leaves in another slot for the same raw
    depth, crop and options, and equals register_reference; the colour plane equals the composed reference.  The reduction's DEPTH bit
    and its depth rule change nothing of a registered depth; with the COLOUR bit clear the registration's colour camera is the ideal one."""
    lm, d = stage.lm, stage.d
    d.set_raw_processing(None)
    r = (9, 4)
    qmap = stage.lens(d, *X.ideal_sides(W, H, r))
    cr = r if apply == "both" else (1, 1)
    cc, rays = registration_for(stage, d, cr)
    Rg = X.cached(("Rg", apply), lambda: GR.register(GS.scene_a(), 1.0, rays, cc, GS.ROT, GS.TRANS, (1, 1)))
    raw = stage.put(GS.scene_a())
    Ac = stage.Ac("nv12", qmap, cr)
    crop = (3, 2) if apply == "both" else (106, 55)
    dcrop = (2, 1) if apply == "both" else (105, 54)
    planes = []
    for rule, depth_bit in (("nearest", True), ("min_valid", apply == "depth")):
        d.set_reduction(r, colour=apply == "both", depth=depth_bit or apply != "both", depth_rule=rule)
        f = colour_frame(stage, "nv12", crop, True, (2, -1), pad=1, offset=1, depth=raw, depth_crop=dcrop)
        d.ingest_frames(0, [dict(f, rectify_reduce=False, register_depth=True, crop=(24, 20))])          # (the plain colour window: only its depth plane is compared)
        d.ingest_frames(1, [dict(f, registered=True)])
        plain, both = d.read_frame(0), d.read_frame(1)
        assert (plain[1] != 0).sum() > 1000
        assert np.array_equal(both[1], plain[1]), "the registered depth plane differs from lm_ingest_frames_registered's"
        assert np.array_equal(both[1], GR_window(Rg, dcrop, True, (2, -1))), "the registered depth plane differs from the reference"
        assert np.array_equal(both[0], RR.slot_colour(Ac, W, H, crop, True, (2, -1)))
        planes.append(both[1])
    assert np.array_equal(planes[0], planes[1])
    # the registration's colour camera must have the size of the colour image's geometry in this route
    d.set_reduction(r, colour=apply != "both")
    with pytest.raises(lm.LinemodError) as e:
        d.ingest_frames(1, [dict(f, registered=True)])
    words = ("rectification: the registration's colour camera (165 x 84) is not the ideal camera (372 x 190)" if apply == "both" else
             "rectification: the registration's colour camera (372 x 190) is not the reduced ideal geometry (165 x 84)")
    assert e.value.code == INVALID and str(e.value).endswith(words), str(e.value)
    d.set_registration(None, None, None, None)
    with pytest.raises(lm.LinemodError) as e:
        d.ingest_frames(1, [dict(f, registered=True)])
    assert e.value.code == INVALID and str(e.value).endswith("no registration set: lm_set_registration first")
    assert np.array_equal(d.read_frame(1)[1], planes[1])          # (the refusals enqueued nothing)


def GR_window(Rg, crop, flip, shift):
    return RR.slot_depth(Rg, W, H, crop, flip, shift)


@pytest.mark.parametrize("fmt", RS.FAMILIES)
def test_identities_on_the_device(stage, fmt):
    """No reference needed, the plumbing against the existing paths: with an identity lens (zero coefficients, ideal = the source's
    pinhole) the slot holds what lm_ingest_frames_reduced makes of the same sources, slot for slot; at 1/1 it holds what
    lm_ingest_frames_rectified makes of them."""
    lm, d = stage.lm, stage.d
    stage.pipeline(d, fmt)
    source, ideal, _ = X.identity_map()
    d.set_rectification(to_cam(lm, source), to_cam(lm, ideal))
    d.set_reduction((5, 4), depth_rule="min_valid")           # 208 x 120 -> 166 x 96
    for n, dfmt in enumerate(("u16", "f32")):
        dhost, scale = stage.depth(dfmt)
        crop, flip, shift = [((4, 2), False, (0, 0)), ((5, 15), True, (-3, 5))][n]
        f = colour_frame(stage, fmt, crop, flip, shift, pad=n, depth=stage.put(dhost), depth_scale=scale)
        d.ingest_frames(2 * n, [dict(f, rectify_reduce=False, reduced=True)])
        d.ingest_frames(2 * n + 1, [f])
        a, b = d.read_frame(2 * n), d.read_frame(2 * n + 1)
        assert a[0].any() and a[1].any()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "identity lens: %s %s crop %s flip %s shift %s" % (fmt, dfmt, crop, flip, shift)
    qmap = stage.lens(d, SW, SH)
    d.set_reduction((1, 1))
    dhost, scale = stage.depth("f32")
    crop = (1, 2)
    assert X.straddling(qmap, SW, SH, (1, 1), W, H, crop) >= 40
    f = colour_frame(stage, fmt, crop, True, (2, -3), pad=3, depth=stage.put(dhost), depth_scale=scale)
    d.ingest_frames(4, [dict(f, rectify_reduce=False, rectified=True)])
    d.ingest_frames(5, [f])
    a, b = d.read_frame(4), d.read_frame(5)
    assert a[0].any() and a[1].any()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "1/1: %s" % fmt
    d.set_raw_processing(None)


def test_only_this_rule_gives_these_bytes(stage):
    """3/1 under the barrel lens: the slot equals the composition, and differs from lm_ingest_frames_rectified onto an ideal camera of a
    third of the focal length -- the only way to get the whole rectified view into a slot without this route, a four-tap gather that
    skips eight ideal pixels of nine -- on the same frame."""
    lm, d = stage.lm, stage.mono
    d.set_raw_processing(None)
    r = (3, 1)
    iw, ih = X.ideal_sides(MW, MH, r)
    source, ideal, _ = X.lens_map(iw, ih)
    qmap = stage.lens(d, iw, ih)
    d.set_reduction(r)
    crop = (2, 1)
    assert X.straddling(qmap, SW, SH, r, MW, MH, crop) >= 40
    f = colour_frame(stage, "bgr", crop)
    d.ingest_frames(0, [f])
    composed = RR.slot_colour(stage.Ac("bgr", qmap, r), MW, MH, crop)
    check_slot(d, 0, composed, None, "3/1 against the composition")
    third = QR.cam(iw // 3, ih // 3, ideal["fx"] / 3, ideal["fy"] / 3, (ideal["cx"] + 0.5) / 3 - 0.5, (ideal["cy"] + 0.5) / 3 - 0.5)
    d.set_rectification(to_cam(lm, source), to_cam(lm, third))
    d.ingest_frames(1, [dict(f, rectify_reduce=False, rectified=True)])
    gather = d.read_frame(1)[0]
    assert np.array_equal(gather, QR.slot_colour(QR.rectify_colour(stage.colour("bgr")[1], QR.build_map(source, third)), MW, MH, crop))
    assert int((gather != composed).sum()) > composed.size // 2
    assert np.array_equal(d.read_frame(0)[0], composed)


def test_one_call_of_six_frames_then_another_ratio(stage):
    """One call of six frames of different formats with a registered depth equals the frames ingested one by one and the references;
    then another ratio is set and the next call, with no wait in between, uses it."""
    lm, d = stage.lm, stage.d
    d.set_raw_processing(None)
    r = (9, 4)
    qmap = stage.lens(d, *X.ideal_sides(W, H, r))
    d.set_reduction(r, depth_rule="min_valid")
    cc, rays = registration_for(stage, d, r, splat=(2, 1))
    raws = [(GS.scene_a(), 1.0), (GS.scene_a(seed=8, far=100.0), 1.0)]
    Rg = [X.cached(("Rg six", n), lambda: GR.register(raws[n][0], raws[n][1], rays, cc, GS.ROT, GS.TRANS, (2, 1))) for n in range(2)]
    frames, exp = [], []
    for n, fmt in enumerate(["bgr", "nv12", "rgba", "bayer_grbg", "yuy2", "bgr_planar"]):
        crop, flip, shift = GEOMETRY[n % 6]
        dcrop = (crop[0] + 1, crop[1] ^ 1)
        frames.append(colour_frame(stage, fmt, crop, flip, shift, pad=n % 4, offset=n % 3, depth=stage.put(raws[n % 2][0], pad=4 * (n % 3)), depth_crop=dcrop,
                                   depth_scale=raws[n % 2][1], registered=True))
        exp.append((RR.slot_colour(stage.Ac(fmt, qmap, r), W, H, crop, flip, shift), RR.slot_depth(Rg[n % 2], W, H, dcrop, flip, shift)))
    d.ingest_frames(0, frames)
    together = [d.read_frame(k) for k in range(6)]
    for k, f in enumerate(frames):
        d.ingest_frames(k, [f])
    for k in range(6):
        one = d.read_frame(k)
        assert np.array_equal(one[0], together[k][0]) and np.array_equal(one[1], together[k][1]), "frame %d" % k
        check_slot(d, k, exp[k][0], exp[k][1], "frame %d against the references" % k)
    # another ratio, DEPTH_ALIGNED: (3/1, 9/4) of 372 x 190 is 124 x 84 -- narrower than the slot -- so 2/1: 186 x 95
    d.set_registration(None, None, None, None)
    d.set_reduction((2, 1), depth_rule="min_valid")
    dhost, scale = stage.depth("u16")
    f = colour_frame(stage, "yuy2", (11, 7), True, (1, 1), depth=stage.put(dhost), depth_crop=(12, 9))
    d.ingest_frames(0, [f])
    d.set_reduction((9, 4), depth_rule="nearest")
    d.ingest_frames(1, [dict(f, crop=(3, 2), depth_crop=(2, 2))])
    check_slot(d, 0, RR.slot_colour(stage.Ac("yuy2", qmap, (2, 1)), W, H, (11, 7), True, (1, 1)),
               RR.slot_depth(stage.Ad("u16", qmap, (2, 1), "min_valid"), W, H, (12, 9), True, (1, 1)), "the first ratio")
    check_slot(d, 1, RR.slot_colour(stage.Ac("yuy2", qmap, (9, 4)), W, H, (3, 2), True, (1, 1)),
               RR.slot_depth(stage.Ad("u16", qmap, (9, 4), "nearest"), W, H, (2, 2), True, (1, 1)), "the second ratio")


def test_both_grid_orders_give_the_same_bytes(stage):
    """LM_TUNE_RECTIFY_REDUCE_GRID: the frames of a call on the grid's fastest index, or its second -- four frames of three families in
    one call, both orders against the reference."""
    lm, d = stage.lm, stage.mono
    d.set_raw_processing(None)
    r = (16, 5)
    qmap = stage.lens(d, *X.ideal_sides(MW, MH, r))
    d.set_reduction(r)
    frames = [colour_frame(stage, fmt, *GEOMETRY[n], pad=n) for n, fmt in enumerate(["rgba", "nv12", "bayer_grbg", "bgr"])]
    try:
        for order in (1, 0):
            d.set_tuning(lm.TUNE_RECTIFY_REDUCE_GRID, order)
            d.ingest_frames(0, frames)
            for n, fmt in enumerate(["rgba", "nv12", "bayer_grbg", "bgr"]):
                check_slot(d, n, RR.slot_colour(stage.Ac(fmt, qmap, r), MW, MH, *GEOMETRY[n]), None, "grid order %d, frame %d" % (order, n))
            d.ingest_frames(0, [frames[3]] * 4)          # (the next order writes every slot anew)
    finally:
        d.set_tuning(lm.TUNE_RECTIFY_REDUCE_GRID, 0)


def test_refusals_through_the_library(stage):
    """The route's refusals on a live detector, before anything is enqueued: the slot holds what it held."""
    lm, d = stage.lm, stage.d
    d.set_raw_processing(None)
    r = (9, 4)
    stage.lens(d, *X.ideal_sides(W, H, r))
    d.set_reduction(r)
    dhost, scale = stage.depth("u16")
    f = colour_frame(stage, "bgr", (1, 1), depth=stage.put(dhost))
    d.ingest_frames(3, [f])
    before = d.read_frame(3)

    def refused(words, frames=None, slot=3, **edit):
        with pytest.raises(lm.LinemodError) as e:
            d.ingest_frames(slot, frames or [dict(f, **edit)])
        assert e.value.code == INVALID and str(e.value).endswith(words), str(e.value)

    refused("rectification: colour image of frame 0: window %d x %d at (6, 0) lies outside the 165 x 84 reduced ideal geometry" % (W, H), crop=(6, 0), depth_crop=(0, 0))
    refused("rectification: depth image of frame 0: window %d x %d at (0, 5) lies outside the 165 x 84 reduced ideal geometry" % (W, H), crop=(0, 0), depth_crop=(0, 5))
    small = lm.DeviceBuffer(3 * SW * SH)
    stage.bufs.append(small)
    refused("rectification: colour image of frame 0: a %d x %d image is not the source camera (%d x %d)" % (SW - 1, SH, SW, SH),
            colour=small.view(np.uint8, (SH, SW - 1, 3), 0, (3 * SW, 3, 1)))
    refused("rectification: colour image of frame 0: row_stride smaller than a source row", colour=small.view(np.uint8, (SH, SW, 3), 0, (3 * SW - 1, 3, 1)))
    refused("slot out of range", slot=6)
    assert d.lib.lm_ingest_frames_rectified_reduced(d.h, 3, 1, None, None, None, 9, None) == INVALID
    assert d.lib.lm_last_error().decode() == "rectification: unknown depth_route 9"
    refused("no registration set: lm_set_registration first", registered=True)
    d.set_reduction(r, depth=False)
    refused("rectification: depth image of frame 0: window %d x %d at (213, 0) lies outside the 372 x 190 ideal geometry" % (W, H), depth_crop=(213, 0))
    d.set_reduction(None)
    refused("reduction: no reduction set: lm_set_reduction first")
    with pytest.raises(lm.LinemodError) as e:
        d.stage_rectify_reduce(f["colour"])
    assert e.value.code == INVALID and str(e.value).endswith("reduction: no reduction set: lm_set_reduction first")
    d.set_reduction(r)
    d.set_rectification(None, None)
    refused("rectification: no rectification set: lm_set_rectification first")
    d.upload_wait(3)
    after = d.read_frame(3)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_it_is_an_upload_like_any_other(lm, orc, synth):
    """match_slot right after a rectified and reduced ingest, no explicit wait, equals record for record the match of the
    reference-composed frame uploaded from the host; the bank is learned from that frame's crops."""
    RW, RH, THR = 320, 240, 75.0
    r = (9, 4)
    d = lm.Detector(color_only=False, width=RW, height=RH, frame_slots=2)
    sw, sh = RW * 9 // 4 + 2, RH * 9 // 4 + 1
    bgr, depth = synth.make_frame(sw, sh, seed=501)
    source = QR.cam(sw, sh, 520.0, 521.0, (sw - 1) / 2.0 + 3.0, (sh - 1) / 2.0 - 2.0, (-0.12, 0.03, 0.001, -0.001, 0.0))
    ideal = QR.cam(sw, sh, 500.0, 500.0, (sw - 1) / 2.0, (sh - 1) / 2.0)
    qmap = QR.build_map(source, ideal)
    d.set_rectification(to_cam(lm, source), to_cam(lm, ideal))
    d.set_reduction(r, depth_rule="min_valid")
    rb, rd = RR.slot_colour(X.reduced_colour(bgr, qmap, r), RW, RH), RR.slot_depth(X.reduced_depth(depth, qmap, r, "min_valid"), RW, RH)
    assert rb.shape == (RH, RW, 3) and (rd != 0).sum() > 1000
    o = orc.Detector(color_only=False)
    o.prepare(rb, rd)
    q = {(l, m): o.stage(0, l, m).reshape(RH >> l, RW >> l) for l in range(2) for m in range(2)}
    descs, feats, _ = synth.make_bank(40, 2, 2, seed=99, size_range=(48, 120), quantized=q, crop_fraction=0.3, frame_size=(RW, RH), T0=d.get_T(0))
    d.add_class("c", descs, feats)
    cb, db = lm.DeviceBuffer(bgr.nbytes), lm.DeviceBuffer(depth.nbytes)
    cb.upload(bgr)
    db.upload(depth)
    d.ingest_frame(1, cb.view(np.uint8, bgr.shape), db.view(np.uint16, depth.shape), rectify_reduce=True)
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
    """A detector that rectified and reduced, on two copy streams, with two ratios, a registered depth and through the stage hook, gives
    everything back."""
    start = lm.live_resources()
    source, ideal, _ = X.lens_map(*X.ideal_sides(W, H, (9, 4)))
    for cycle in range(2):
        d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
        d.set_rectification(to_cam(lm, source), to_cam(lm, ideal))
        d.set_reduction((9, 4))
        (bgr, _), (dep, _) = RS.colour("bgr", SW, SH), RS.depth("u16", SW, SH)
        raw = np.ascontiguousarray(GS.scene_a())
        cb, db, rb = lm.DeviceBuffer(bgr.nbytes), lm.DeviceBuffer(dep.nbytes), lm.DeviceBuffer(raw.nbytes)
        cb.upload(bgr)
        db.upload(dep)
        rb.upload(raw)
        f = dict(colour=cb.view(np.uint8, bgr.shape), depth=db.view(np.uint16, dep.shape), crop=(1, 1), rectify_reduce=True)
        d.ingest_frames(0, [f])
        d.ingest_frames(1, [f])
        d.set_reduction((2, 1), depth_rule="min_valid")
        d.ingest_frames(0, [dict(f, crop=(0, 0))] * 4)
        d.stage_rectify_reduce(f["colour"], f["depth"])
        d.set_registration(to_cam(lm, GS.depth_cam_a()), lm.reduced_camera(to_cam(lm, ideal), (2, 1)), GS.ROT, GS.TRANS)
        g = dict(f, depth=rb.view(np.float32, raw.shape), registered=True)
        d.ingest_frames(0, [g] * 4)
        d.upload_wait(-1)
        assert lm.live_resources()[0] > start[0] + 2
        steady = lm.live_resources()
        d.ingest_frames(0, [dict(f, crop=(0, 0))] * 4)
        d.ingest_frames(0, [g] * 4)
        d.upload_wait(-1)
        assert lm.live_resources() == steady, "an ingest in the steady state created or released a resource"
        d.close()
        cb.close()
        db.close()
        rb.close()
        assert lm.live_resources() == start, "cycle %d: lm_destroy left %r, the baseline is %r" % (cycle, lm.live_resources(), start)
