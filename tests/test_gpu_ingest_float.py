"""The float colour sources of lm_ingest_frames on the GPU (0.13 additive, DESIGN.md section 13 "Float sources"): F32 and F16 sources in
device memory, interleaved with 3 or 4 channels, planar and grey -> the slots, compared byte for byte through read_frame with
tests/ingest_float_reference.py (a float32 multiply and np.rint over the whole source, then ingest_reference's crop, mirror and shift of
that image as BGR8).  The routes are checked differentially: a float source and, as LM_PIX_BGR8 through the same route, the image the
rule yields from it land in two slots that must be equal.  Equality is exact everywhere."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ingest_float_reference as FR
import ingest_reference as IR
import rectify_reduce_scenes as YS
import rectify_reference as QR
import rectify_scenes as S
import reduce_scenes as XS
import register_scenes as GS
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

SW, SH = 204, 98          # the sources of the sweep, as the other ingest suites': no multiple of 16
INVALID = 1
DETECTORS = [pytest.param(True, id="rgbd_160x80"), pytest.param(False, id="colour_48x32")]
NAMES = {FR.PIX_FLOAT | el | lay: name % tag for el, tag in ((0, "F32"), (0x10, "F16"))
         for lay, name in ((0, "BGR_%s"), (1, "RGB_%s"), (2, "BGRA_%s"), (3, "RGBA_%s"), (4, "BGR_%s_PLANAR"), (5, "RGB_%s_PLANAR"), (8, "GRAY_%s"))}


class Dev:
    """A FR.Source in a DeviceBuffer that ends where the source ends; `frame(**kw)` is ingest_frames' dict."""

    def __init__(self, lm, src):
        self.src = src
        self.buf = lm.DeviceBuffer(len(src.raw))
        self.buf.upload(src.raw)
        self.view = self.buf.view(src.dtype, src.host.shape, offset=src.offset, strides=src.strides())

    def frame(self, scale, **kw):
        return dict(colour=self.view, layout=self.src.layout, order=self.src.order, float_scale=scale, **kw)

    def close(self):
        self.buf.close()


def put(lm, bufs, host, strides=None):
    """A dense device copy of a host array -> the view image_desc wants."""
    host = np.ascontiguousarray(host)
    buf = lm.DeviceBuffer(host.nbytes)
    buf.upload(host)
    bufs.append(buf)
    return buf.view(host.dtype.type, host.shape)


def check_slot(d, slot, exp_bgr, what):
    bgr = d.read_frame(slot)[0]
    assert np.array_equal(bgr, exp_bgr), "%s: colour differs at %d bytes" % (what, int((bgr != exp_bgr).sum()))


@pytest.mark.parametrize("scale", [255.0, 2.0 ** 24])
def test_every_half(lm, scale):
    """One GRAY_F16 source whose pixel (x, y) holds the bit pattern 256 y + x: all 65536 halves through the kernel."""
    d = lm.Detector(color_only=True, width=256, height=256, T=[2, 8], frame_slots=1)
    bits = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    bufs = []
    view = put(lm, bufs, bits.view(np.float16))
    d.ingest_frame(0, view, layout="gray", float_scale=scale)
    g = FR.to_u8(FR.half_bits(bits), scale)
    check_slot(d, 0, np.stack([g, g, g], axis=-1), "every half at scale %r" % scale)
    if scale == 255.0:
        assert int(g.astype(np.int64).sum()) == 4569216 and len(np.unique(g)) == 256
    d.close()
    bufs[0].close()


@pytest.fixture(scope="module")
def sweep_sources(lm):
    """204 x 98 sources of all fourteen formats at every element multiple below 16 bytes, rows and planes one element longer than dense."""
    rng = np.random.default_rng(61)
    src = {(fmt, off): Dev(lm, FR.Source(fmt, SW, SH, rng, offset=off)) for fmt in FR.FORMATS for off in range(0, 16, 2 if fmt & 0x10 else 4)}
    # ties, negatives, values above 255, NaN and +-inf occur at every lane position of the first lane row of every format's offset-0 source
    for fmt in FR.FORMATS:
        h = src[fmt, 0].src.host.astype(np.float32)
        px = h if h.ndim == 2 else (h[0] if src[fmt, 0].src.layout == "chw" else h[:, :, 0])
        for test in (np.isnan, np.isposinf, np.isneginf, lambda v: v < 0, lambda v: v > 255, lambda v: (v > 0) & (v < 255) & (v % 1 == 0.5)):
            with np.errstate(invalid="ignore"):
                hit = test(px)
            assert all(hit[:, k::16].any() for k in range(16)), NAMES[fmt]
    dep = np.random.default_rng(62).integers(0, 65536, (SH, SW), dtype=np.uint16)
    dbuf = lm.DeviceBuffer(dep.nbytes)
    dbuf.upload(dep)
    yield src, (dbuf.view(np.uint16, dep.shape), dep)
    for s in src.values():
        s.close()
    dbuf.close()


@pytest.mark.parametrize("rgbd", DETECTORS)
@pytest.mark.parametrize("half", [0, 0x10], ids=["f32", "f16"])
def test_format_and_alignment_sweep(lm, sweep_sources, rgbd, half):
    """All seven layouts of the element x every offset x an odd crop and the far corner (the source ends where its allocation ends) x mirror x the shifts (0, 0), (7, -3) and one beyond
    the frame, at scale 1 and 0.5; four frames per call."""
    W, H = (160, 80) if rgbd else (48, 32)
    src, (dview, dhost) = sweep_sources
    d = lm.Detector(color_only=not rgbd, width=W, height=H, frame_slots=4)
    formats = [f for f in FR.FORMATS if f & 0x10 == half]
    offsets = range(0, 16, 2 if half else 4)
    geometry = list(itertools.product(offsets, ((3, 1), (SW - W, SH - H)), (False, True), ((0, 0), (7, -3), (W + 5, 0)), formats))
    pick = np.random.default_rng(63).integers(0, 2, len(geometry))
    cases = [(fmt, off, crop, flip, shift, (1.0, 0.5)[k]) for (off, crop, flip, shift, fmt), k in zip(geometry, pick)]
    cases += cases[:(-len(cases)) % 4]
    for i in range(0, len(cases), 4):
        group = cases[i:i + 4]
        d.ingest_frames(0, [src[fmt, off].frame(scale, depth=dview if rgbd else None, crop=crop, flip_x=flip, shift=shift) for fmt, off, crop, flip, shift, scale in group])
        for s, (fmt, off, crop, flip, shift, scale) in enumerate(group):
            exp = IR.colour(src[fmt, off].src.bgr(scale), W, H, crop=crop, flip_x=flip, shift=shift)
            check_slot(d, s, exp, "%s offset %d crop %s flip %s shift %s scale %s" % (NAMES[fmt], off, crop, flip, shift, scale))
            if rgbd and s == 0:
                assert np.array_equal(d.read_frame(s)[1], IR.depth(dhost, W, H, crop, 1.0, flip, shift))
    d.close()


def test_one_call_mixes_the_families(lm, sweep_sources):
    """BGR8, NV12, a raw format and two float frames in one call: every slot is right (each family's kernel takes its own frames), and the
    call launches each of the four families' kernels once.  A second call without float frames launches no float kernel
    (lm_debug_launch_counts: the launchers count where they launch)."""
    import ingest_yuv_reference as YR
    W, H = 48, 32
    src, _ = sweep_sources
    rng = np.random.default_rng(64)
    d = lm.Detector(color_only=True, width=W, height=H, T=[2, 8], frame_slots=6)
    bufs = []
    bgr = rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    nv = rng.integers(0, 256, (SH * 3 // 2, SW), dtype=np.uint8)
    mono = rng.integers(0, 1 << 12, (SH, SW), dtype=np.uint16)
    kw = dict(crop=(3, 1), flip_x=True, shift=(7, -3))
    a, b = src[0x2003, 4], src[0x2014, 6]
    frames = [dict(colour=put(lm, bufs, bgr), **kw), dict(colour=put(lm, bufs, nv), layout="nv12", **kw), a.frame(1.0, **kw),
              dict(colour=put(lm, bufs, mono), layout="mono", bits=12, **kw), b.frame(0.5, **kw)]
    c0 = lm.launch_counts()
    d.ingest_frames(0, frames)
    c1 = lm.launch_counts()
    assert {k: c1[k] - c0[k] for k in c0} == dict(rgb=1, yuv=1, bayer=0, raw=1, float=1, reduce_conv=0, export=0, export_float=0)
    m8 = (mono >> 4).astype(np.uint8)
    exp = [bgr, YR.yuv_to_bgr((nv[:SH], nv[SH:]), "nv12", ("bt601", "limited")), a.src.bgr(1.0), np.stack([m8, m8, m8], axis=-1), b.src.bgr(0.5)]
    for s, e in enumerate(exp):
        check_slot(d, s, IR.colour(e, W, H, crop=(3, 1), flip_x=True, shift=(7, -3)), "mixed call, slot %d" % s)
    # a call without float frames launches no float kernel; one with float frames alone launches nothing else
    d.ingest_frames(0, frames[:2])
    c2 = lm.launch_counts()
    assert {k: c2[k] - c1[k] for k in c1} == dict(rgb=1, yuv=1, bayer=0, raw=0, float=0, reduce_conv=0, export=0, export_float=0)
    d.ingest_frames(0, [frames[2], frames[4]])
    c3 = lm.launch_counts()
    assert {k: c3[k] - c2[k] for k in c2} == dict(rgb=0, yuv=0, bayer=0, raw=0, float=1, reduce_conv=0, export=0, export_float=0)
    d.close()
    for x in bufs:
        x.close()


# ---- the routes, differentially
ROUTE_FORMATS = [0x2001, 0x2014, 0x2008]          # one interleaved F32, one planar F16, one grey


def to_cam(lm, c):
    return lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])


@pytest.fixture(scope="module")
def route_sources(lm):
    """208 x 120 float sources (the rectify scenes' source camera) and, beside each, the BGR8 image the rule yields from the whole source."""
    rng = np.random.default_rng(65)
    out, bufs = {}, []
    for fmt in ROUTE_FORMATS:
        dev = Dev(lm, FR.Source(fmt, S.SW, S.SH, rng, offset=4, pad=1))
        out[fmt] = (dev, put(lm, bufs, dev.src.bgr(1.0)), dev.src.bgr(1.0))
    yield out
    for dev, _, _ in out.values():
        dev.close()
    for b in bufs:
        b.close()


@pytest.mark.parametrize("fmt", ROUTE_FORMATS, ids=lambda f: NAMES[f])
def test_routes_equal_the_bgr8_image_through_the_same_route(lm, route_sources, fmt):
    """Rectified, reduced and rectify-and-reduce on the colour-only 64 x 32 detector, window mirrored and shifted, and the three stage hooks."""
    dev, bgr_view, bgr = route_sources[fmt]
    d = lm.Detector(color_only=True, width=S.MW, height=S.MH, T=[2, 8], frame_slots=2)
    kw = dict(crop=(5, 3), flip_x=True, shift=(3, -2))
    d.set_rectification(to_cam(lm, S.source_cam()), to_cam(lm, S.ideal_cam(176, 96)))
    d.set_reduction((9, 4))
    for route in ("rectified", "reduced", "rectify_reduce"):
        c0 = lm.launch_counts()
        d.ingest_frames(0, [dev.frame(1.0, **kw, **{route: True})])
        c1 = lm.launch_counts()
        d.ingest_frames(1, [dict(colour=bgr_view, **kw, **{route: True})])
        c2 = lm.launch_counts()
        mine = "reduce_conv" if route == "reduced" else "float"
        assert {k: c1[k] - c0[k] for k in c0 if c1[k] != c0[k]} == {mine: 1} and {k: c2[k] - c1[k] for k in c1 if c2[k] != c1[k]} == {"rgb": 1}, route
        a, b = d.read_frame(0)[0], d.read_frame(1)[0]
        assert a.any() and len(np.unique(a)) > 100
        assert np.array_equal(a, b), "%s %s: %d bytes differ" % (NAMES[fmt], route, int((a != b).sum()))
    for hook in (d.stage_rectify, d.stage_reduce, d.stage_rectify_reduce):
        a = hook(dev.view, layout=dev.src.layout, order=dev.src.order, float_scale=1.0)[0]
        b = hook(bgr_view)[0]
        assert a.shape == b.shape and a.any() and np.array_equal(a, b), "%s %s" % (NAMES[fmt], hook.__name__)
    d.close()


@pytest.mark.parametrize("fmt", ROUTE_FORMATS, ids=lambda f: NAMES[f])
def test_registered_route_takes_float_colour(lm, route_sources, fmt):
    """The registered route's colour images are the plain ingest's: the float frame beside a raw depth image equals the BGR8 one."""
    dev, bgr_view, bgr = route_sources[fmt]
    d = lm.Detector(color_only=False, width=GS.W, height=GS.H, frame_slots=2)
    d.set_registration(to_cam(lm, GS.depth_cam_a(GS.DIST)), to_cam(lm, GS.colour_cam(GS.DIST)), GS.ROT, GS.TRANS, splat=(1, 1))
    bufs = []
    raw = put(lm, bufs, GS.scene_a())
    kw = dict(depth=raw, crop=GS.CROP, register_depth=True)
    d.ingest_frames(0, [dev.frame(1.0, **kw)])
    d.ingest_frames(1, [dict(colour=bgr_view, **kw)])
    a, b = d.read_frame(0), d.read_frame(1)
    assert np.array_equal(a[0], IR.colour(bgr, GS.W, GS.H, crop=GS.CROP)) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].any()
    d.close()
    bufs[0].close()


def test_match_after_a_float_ingest(lm, orc, synth):
    """match_slot after an RGB_F32_PLANAR ingest of frame / 255 at scale 255 returns the lists of the same frame uploaded as 8-bit, on the
    320 x 240 rig of the ingest suites."""
    W, H, THR = 320, 240, 75.0
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=2)
    bgr, depth = synth.make_frame(W, H, seed=500)
    o = orc.Detector(color_only=False)
    o.prepare(bgr, depth)
    q = {(l, m): o.stage(0, l, m).reshape(H >> l, W >> l) for l in range(2) for m in range(2)}
    descs, feats, _ = synth.make_bank(40, 2, 2, seed=99, size_range=(48, 120), quantized=q, crop_fraction=0.3, frame_size=(W, H), T0=d.get_T(0))
    d.add_class("c", descs, feats)
    tensor = np.ascontiguousarray(np.transpose(bgr[:, :, ::-1], (2, 0, 1))).astype(np.float32) / np.float32(255.0)       # torch's [3, H, W], RGB, 0 .. 1
    assert np.array_equal(FR.to_bgr(tensor, "chw", "rgb", 255.0), bgr)
    bufs = []
    d.upload_frame(0, bgr, depth)
    d.ingest_frame(1, put(lm, bufs, tensor), put(lm, bufs, depth), layout="chw", order="rgb", float_scale=255.0)
    got = d.read_frame(1)
    assert np.array_equal(got[0], bgr) and np.array_equal(got[1], depth)
    m0, m1 = d.match_slot(0, THR, 0), d.match_slot(1, THR, 0)
    assert len(m0) > 0
    assert_matches_equal(m1, m0)
    d.close()
    for b in bufs:
        b.close()


def test_refusals(lm, sweep_sources):
    """Every refusal the float formats add, through the library, with its words; nothing is enqueued: the slot holds what it held."""
    W, H = 160, 80
    src, (dview, dhost) = sweep_sources
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=2)
    planar, rgba = src[0x2004, 0], src[0x2013, 0]
    good_c = lm.image_desc(planar.view, layout="chw", float_scale=255.0)
    good_d = lm.image_desc(dview, depth=True)

    def call(edit_c=None, edit_d=None, first=1):
        ca, da = (lm.ImageDesc * 1)(), (lm.ImageDesc * 1)()
        for arr, g, edit in ((ca, good_c, edit_c), (da, good_d, edit_d)):
            C.memmove(C.byref(arr[0]), C.byref(g), C.sizeof(lm.ImageDesc))
            for name, value in (edit or {}).items():
                setattr(arr[0], name, value)
        rc = d.lib.lm_ingest_frames(d.h, first, 1, ca, da, None, None)
        return rc, (d.lib.lm_last_error().decode() if rc else "")

    c, dd = "colour image of frame 0: ", "depth image of frame 0: "
    d.ingest_frames(1, [rgba.frame(1.0, depth=dview)])
    before = d.read_frame(1)
    assert call(first=0) == (0, "")
    for bad in (0x2006, 0x2007, 0x2009, 0x2016, 0x2020, 0x2100, 0x2200, 0x3000):
        assert call({"format": bad}) == (INVALID, c + "unknown pixel format %d" % bad)
    for fmt, name in NAMES.items():
        assert call(edit_d={"format": fmt}) == (INVALID, dd + "LM_PIX_%s is a colour format" % name)
    assert call({"data": good_c.data + 2}) == (INVALID, c + "data and row_stride of a f32 source must be multiples of 4")
    assert call({"row_stride": good_c.row_stride + 2}) == (INVALID, c + "data and row_stride of a f32 source must be multiples of 4")
    assert call({"format": 0x2014, "data": good_c.data + 1}) == (INVALID, c + "data and row_stride of a f16 source must be multiples of 2")
    assert call({"plane_stride": good_c.plane_stride + 2}) == (INVALID, c + "plane_stride of a f32 source must be a multiple of 4")
    assert call({"format": 0x2014, "plane_stride": good_c.plane_stride + 1}) == (INVALID, c + "plane_stride of a f16 source must be a multiple of 2")
    assert call({"plane_stride": 0, "data": good_c.data + 2}) == (INVALID, c + "plane_stride must be positive")
    assert call({"row_stride": 4 * W - 4}) == (INVALID, c + "row_stride smaller than a window row")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call({"scale": bad}) == (INVALID, c + "scale must be finite and positive")
    after = d.read_frame(1)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    d.close()
