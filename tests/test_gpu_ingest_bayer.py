"""The raw Bayer source formats of lm_ingest_frames on the GPU (ABI 0.13 additive, DESIGN.md section 13 "Bayer sources"): BayerRG8 / GR8 /
GB8 / BG8 sources in device memory -> the slots, compared byte for byte through read_frame with tests/ingest_bayer_reference.py (the
bilinear demosaic of the WHOLE source in numpy int64, then ingest_reference's crop, mirror and shift of that image as BGR8), on a
160 x 80 RGB-D detector and a 48 x 32 colour-only one; then the match after a Bayer ingest, the rectified and the registered routes, the
producer stream and the refusals with their words."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ingest_bayer_reference as BR
import ingest_reference as IR
import ingest_yuv_reference as YR
import rectify_reference as QR
import rectify_scenes as S
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

SW, SH = 204, 98          # source size of the geometry sweep: even, and no multiple of 16
INVALID = 1
DETECTORS = [pytest.param(True, id="rgbd_160x80"), pytest.param(False, id="colour_48x32")]
PATTERNS = BR.PATTERNS
NAMES = {"rggb": "LM_PIX_BAYER_RGGB8", "grbg": "LM_PIX_BAYER_GRBG8", "gbrg": "LM_PIX_BAYER_GBRG8", "bggr": "LM_PIX_BAYER_BGGR8"}


class BayerSource:
    """One raw Bayer image in a DeviceBuffer that ends where the image ends, `offset` bytes behind the buffer's start, with rows `pad`
    bytes longer than their pixels: `arg` is what Detector.ingest_frame takes as `colour`, `host` the same bytes as the reference reads
    them (anything [h, w] uint8, or a fill(nbytes) that makes the buffer's bytes)."""

    def __init__(self, lm, pattern, w, h, fill, offset=0, pad=3):
        self.pattern, self.w, self.h = pattern, w, h
        rs = w + pad
        nbytes = offset + (h - 1) * rs + w
        if callable(fill):
            raw = fill(nbytes)
        else:
            raw = np.zeros(nbytes, np.uint8)
            np.lib.stride_tricks.as_strided(raw[offset:], (h, w), (rs, 1))[...] = fill
        assert raw.dtype == np.uint8 and raw.shape == (nbytes,)
        self.buf = lm.DeviceBuffer(nbytes)
        self.buf.upload(raw)
        self.arg = self.buf.view(np.uint8, (h, w), offset=offset, strides=(rs, 1))
        self.host = np.lib.stride_tricks.as_strided(raw[offset:], (h, w), (rs, 1), writeable=False)
        self._bgr = None

    def bgr(self):
        """The BGR image the rule yields from the whole source: computed once and shared."""
        if self._bgr is None:
            self._bgr = BR.demosaic(np.ascontiguousarray(self.host), self.pattern)
            self._bgr.setflags(write=False)
        return self._bgr

    def frame(self, **kw):
        return dict(colour=self.arg, layout="bayer_" + self.pattern, **kw)

    def close(self):
        self.buf.close()


def random_fill(rng):
    return lambda n: rng.integers(0, 256, n, dtype=np.uint8)


def depth_plane(lm, rng, w, h, f32):
    """A dense depth source and its expected u16 image."""
    v = rng.uniform(300.0, 4000.0, (h, w)).astype(np.float32) if f32 else rng.integers(0, 65536, (h, w), dtype=np.uint16)
    buf = lm.DeviceBuffer(v.nbytes)
    buf.upload(v)
    return buf, buf.view(v.dtype.type, (h, w)), v


def check_slot(d, slot, exp_bgr, exp_depth, what):
    bgr, depth = d.read_frame(slot)
    assert np.array_equal(bgr, exp_bgr), "%s: colour differs at %d bytes" % (what, int((bgr != exp_bgr).sum()))
    if exp_depth is not None:
        assert np.array_equal(depth, exp_depth), "%s: depth differs at %d pixels" % (what, int((depth != exp_depth).sum()))


def tiles(full, win):
    """Window origins that cover [0, full) with windows of `win`."""
    return sorted({min(o, full - win) for o in range(0, full, win)})


@pytest.fixture(scope="module")
def sweep_sources(lm):
    """204 x 98 sources of all four patterns at base offsets 0 .. 3, rows 3 bytes longer than their pixels; dense NV12, BGR8 and GRAY8
    sources for the mixed call; dense depth sources of both formats."""
    rng = np.random.default_rng(61)
    src = {(p, off): BayerSource(lm, p, SW, SH, random_fill(rng), offset=off) for p in PATTERNS for off in range(4)}
    other = {}
    for name, shape in (("nv12", (SH * 3 // 2, SW)), ("bgr", (SH, SW, 3)), ("gray", (SH, SW))):
        host = rng.integers(0, 256, shape, dtype=np.uint8)
        buf = lm.DeviceBuffer(host.nbytes)
        buf.upload(host)
        other[name] = (buf, buf.view(np.uint8, shape), host)
    dep = {f32: depth_plane(lm, rng, SW, SH, f32) for f32 in (False, True)}
    yield src, other, dep
    for s in src.values():
        s.close()
    for b, _, _ in list(other.values()) + list(dep.values()):
        b.close()


@pytest.mark.parametrize("rgbd", DETECTORS)
def test_geometry_and_phase(lm, sweep_sources, rgbd):
    """All four patterns x base offset 0 .. 3 x crop_x {0, 1, 2, 3, max - 1, max} x crop_y {0, 1, max} x mirror, each case with a shift of
    (3, -2), (-5, 1) or none and one of the two depth formats, four frames of four different patterns per call.  Crops 0 and max put the
    window on each source edge (the reflection); every other window takes its neighbours from the source outside it.  Then a call that
    mixes Bayer, NV12, BGR8 and GRAY8, which all three kernels serve."""
    W, H = (160, 80) if rgbd else (48, 32)
    src, other, dep = sweep_sources
    d = lm.Detector(color_only=not rgbd, width=W, height=H, frame_slots=4)
    shifts = ((3, -2), (-5, 1), (0, 0))
    geometry = list(itertools.product(range(4), (0, 1, 2, 3, SW - W - 1, SW - W), (0, 1, SH - H), (False, True), PATTERNS))
    pick = np.random.default_rng(63).integers(0, (3, 2), (len(geometry), 2))        # shift and depth format: drawn per case
    cases = [(p, off, cx, cy, flip, shifts[k[0]], bool(k[1])) for (off, cx, cy, flip, p), k in zip(geometry, pick)]
    assert len(cases) % 4 == 0
    # the case most likely to be wrong is there for every pattern: odd crop_x, odd crop_y, mirrored, shifted
    assert all(any(c[0] == p and c[2] % 2 and c[3] % 2 and c[4] and c[5] != (0, 0) for c in cases) for p in PATTERNS)

    def expected(p, off, cx, cy, flip, shift, f32):
        eb = IR.colour(src[p, off].bgr(), W, H, crop=(cx, cy), flip_x=flip, shift=shift)
        return eb, (IR.depth(dep[f32][2], W, H, (cx, cy), 1.0, flip, shift) if rgbd else None)

    for i in range(0, len(cases), 4):
        group = cases[i:i + 4]
        assert len({c[0] for c in group}) == 4
        d.ingest_frames(0, [src[p, off].frame(depth=dep[f32][1] if rgbd else None, crop=(cx, cy), flip_x=flip, shift=shift)
                            for p, off, cx, cy, flip, shift, f32 in group])
        for s, c in enumerate(group):
            check_slot(d, s, *expected(*c), what="%s offset %d crop (%d, %d) flip %s shift %s f32 %s" % c)
    # Bayer, NV12, BGR8 and GRAY8 in one call: k_ingest_bayer, k_ingest_yuv, k_ingest, k_ingest_yuv
    nv_host = other["nv12"][2]
    refs = (src["grbg", 1].bgr(), YR.yuv_to_bgr((nv_host[:SH], nv_host[SH:]), "nv12", ("bt709", "limited")), other["bgr"][2], YR.yuv_to_bgr(other["gray"][2], "gray"))
    for cx, cy, flip, shift in ((1, 1, True, (3, -2)), (SW - W, SH - H, False, (-5, 1)), (3, 0, True, (0, 0))):
        kw = dict(crop=(cx, cy), flip_x=flip, shift=shift, depth=dep[True][1] if rgbd else None)
        d.ingest_frames(0, [src["grbg", 1].frame(**kw), dict(colour=other["nv12"][1], layout="nv12", matrix="bt709", **kw), dict(colour=other["bgr"][1], **kw),
                            dict(colour=other["gray"][1], layout="gray", **kw)])
        ed = IR.depth(dep[True][2], W, H, (cx, cy), 1.0, flip, shift) if rgbd else None
        for s, eb in enumerate(refs):
            check_slot(d, s, IR.colour(eb, W, H, crop=(cx, cy), flip_x=flip, shift=shift), ed, "mixed call, slot %d, crop (%d, %d)" % (s, cx, cy))
    d.close()


@pytest.mark.parametrize("rgbd", DETECTORS)
def test_source_of_exactly_the_windows_size(lm, rgbd):
    """Dense (row_stride == W), in a buffer that ends with the image: all four edges reflect at once, and nothing lies beyond them."""
    W, H = (160, 80) if rgbd else (48, 32)
    rng = np.random.default_rng(65)
    d = lm.Detector(color_only=not rgbd, width=W, height=H, frame_slots=4)
    dbuf, dview, dhost = depth_plane(lm, rng, W, H, False) if rgbd else (None, None, None)
    for off in (0, 1):
        src = [BayerSource(lm, p, W, H, random_fill(rng), offset=off, pad=0) for p in PATTERNS]
        for flip, shift in ((False, (0, 0)), (True, (0, 0)), (True, (3, -2))):
            d.ingest_frames(0, [s.frame(depth=dview, flip_x=flip, shift=shift) for s in src])
            for k, s in enumerate(src):
                check_slot(d, k, IR.colour(s.bgr(), W, H, flip_x=flip, shift=shift), IR.depth(dhost, W, H, (0, 0), 1.0, flip, shift) if rgbd else None,
                           "%s offset %d flip %s shift %s" % (s.pattern, off, flip, shift))
        for s in src:
            s.close()
    d.close()
    if dbuf:
        dbuf.close()


VW, VH = 160, 80


def value_frames():
    """Two 160 x 80 frames: random bytes, and bytes drawn from {0, 1, 254, 255} with a block of each constant planted."""
    rng = np.random.default_rng(67)
    a = rng.integers(0, 256, (VH, VW), dtype=np.uint8)
    b = np.array([0, 1, 254, 255], np.uint8)[rng.integers(0, 4, (VH, VW))]
    b[10:15, 20:25] = 0
    b[40:45, 100:105] = 255
    b[0:3, 0:3] = 255           # ... and in a corner, where the neighbourhood is the reflection's
    b[VH - 3:, VW - 3:] = 0
    return a, b


def test_value_frames_reach_what_they_should():
    """(No GPU work: the frames themselves.)  Every residue of the p and d sums mod 4 and of the h and v sums mod 2, and the all-0 and the
    all-255 neighbourhoods -- every site is a site of every kind under one of the four patterns."""
    for k, raw in enumerate(value_frames()):
        Sp = np.pad(raw.astype(np.int64), 1, mode="reflect")
        hs, vs = Sp[1:-1, :-2] + Sp[1:-1, 2:], Sp[:-2, 1:-1] + Sp[2:, 1:-1]
        ds = Sp[:-2, :-2] + Sp[:-2, 2:] + Sp[2:, :-2] + Sp[2:, 2:]
        assert set(np.unique(hs % 2)) == {0, 1} and set(np.unique(vs % 2)) == {0, 1}
        assert set(np.unique((hs + vs) % 4)) == {0, 1, 2, 3} and set(np.unique(ds % 4)) == {0, 1, 2, 3}
        if k == 1:
            total = hs + vs + ds + raw
            assert (total == 0).any() and (total == 9 * 255).any()
            assert total[0, 0] == 9 * 255 and total[-1, -1] == 0
            assert hs.max() == 510 and ds.max() == 1020 and (hs == 509).any() and (ds == 1019).any()


@pytest.mark.parametrize("rgbd", DETECTORS)
def test_values(lm, rgbd):
    """The value frames, dense and 16-byte aligned (the fast path), under all four patterns: the RGB-D detector takes each whole, the
    48 x 32 one in windows that tile it."""
    W, H = (160, 80) if rgbd else (48, 32)
    d = lm.Detector(color_only=not rgbd, width=W, height=H, frame_slots=4)
    rng = np.random.default_rng(69)
    dbuf, dview, dhost = depth_plane(lm, rng, VW, VH, False) if rgbd else (None, None, None)
    windows = list(itertools.product(tiles(VW, W), tiles(VH, H)))
    assert any(cx % 16 == 0 for cx, _ in windows)
    for k, raw in enumerate(value_frames()):
        src = [BayerSource(lm, p, VW, VH, raw, pad=0) for p in PATTERNS]
        assert all(s.arg.__cuda_array_interface__["data"][0] % 16 == 0 for s in src)
        for cx, cy in windows:
            d.ingest_frames(0, [s.frame(depth=dview, crop=(cx, cy)) for s in src])
            for n, s in enumerate(src):
                check_slot(d, n, IR.colour(s.bgr(), W, H, crop=(cx, cy)), IR.depth(dhost, W, H, (cx, cy)) if rgbd else None,
                           "value frame %d %s window (%d, %d)" % (k, s.pattern, cx, cy))
        for s in src:
            s.close()
    d.close()
    if dbuf:
        dbuf.close()


class Rig:
    """The 320 x 240 rig of test_gpu_ingest.py with a Bayer camera: a synthetic scene seen through an RGGB mosaic, a 40-template bank cut
    from what the reference rule makes of it, 4 slots."""
    W, H, THR = 320, 240, 75.0

    def __init__(self, lm, orc, synth):
        W, H = self.W, self.H
        self.lm = lm
        self.d = d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
        scene, self.depth = synth.make_frame(W, H, seed=500)
        self.raw = BayerSource(lm, "rggb", W, H, BR.mosaic(scene, "rggb"), pad=0)
        self.bgr = self.raw.bgr().copy()
        o = orc.Detector(color_only=False)
        o.prepare(self.bgr, self.depth)
        q = {(l, m): o.stage(0, l, m).reshape(H >> l, W >> l) for l in range(2) for m in range(2)}
        descs, feats, _ = synth.make_bank(40, 2, 2, seed=99, size_range=(48, 120), quantized=q, crop_fraction=0.3, frame_size=(W, H),
                                          T0=d.get_T(0))
        d.add_class("c", descs, feats)
        self.db = lm.DeviceBuffer(self.depth.nbytes)
        self.db.upload(self.depth)
        self.frame = self.raw.frame(depth=self.db.view(np.uint16, self.depth.shape))

    def close(self):
        self.d.close()
        self.raw.close()
        self.db.close()


@pytest.fixture(scope="module")
def rig(lm, orc, synth):
    r = Rig(lm, orc, synth)
    yield r
    r.close()


def test_match_after_bayer_ingest(rig):
    """match_slot and match_batch after a Bayer ingest give the lists they give after upload_frame of the reference-demosaiced BGR frame."""
    d, THR = rig.d, rig.THR
    for s in range(4):
        d.upload_frame(s, rig.bgr, rig.depth)
    up_slot = d.match_slot(1, THR, 0)
    up_out, up_cnt = d.match_batch(4, THR, 0)
    assert len(up_slot) > 0
    d.ingest_frames(0, [rig.frame] * 4)
    check_slot(d, 2, rig.bgr, rig.depth, "Bayer rig frame")
    in_slot = d.match_slot(1, THR, 0)
    in_out, in_cnt = d.match_batch(4, THR, 0)
    assert_matches_equal(in_slot, up_slot)
    for s in range(4):
        assert_matches_equal(in_out[s, :in_cnt[s]], up_out[s, :up_cnt[s]])


def to_cam(lm, c):
    return lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])


def test_rectified_route(lm):
    """lm_stage_rectify of a 20 x 8 Bayer source into 19 x 7 and 20 x 8 ideal geometries through a caller's map with entries on all four
    borders, in the corners, far outside and not finite; then one lm_ingest_frames_rectified call of four patterns into the 160 x 80
    detector through a lens that leaves the source in the corners.  Expected: the reference's rectification of the reference's demosaic."""
    W, H = S.W, S.H
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    rng = np.random.default_rng(71)
    small = {p: BayerSource(lm, p, 20, 8, random_fill(rng), offset=k, pad=k % 2 * 3) for k, p in enumerate(PATTERNS)}
    tiny_cam = S.source_cam(w=20, h=8)
    for iw, ih in ((19, 7), (20, 8)):
        table = S.smooth_table(iw, ih, sw=20, sh=8)
        d.set_rectification(to_cam(lm, tiny_cam), to_cam(lm, S.ideal_cam(iw, ih)), map=table)
        qmap = QR.quant_table(table, tiny_cam)
        assert (qmap == -64).any() and (qmap[:, :, 0] > 32 * 20).any() and (qmap[:, :, 0] == 32 * 19).any() and (qmap[:, :, 1] == 32 * 7).any()
        for p, s in small.items():
            got = d.stage_rectify(s.arg, None, layout="bayer_" + p)
            assert got[1] is None and np.array_equal(got[0], QR.rectify_colour(s.bgr(), qmap)), "%s into %d x %d" % (p, iw, ih)
    # through the slots
    qmap = QR.build_map(S.source_cam(), S.wide_ideal())
    d.set_rectification(to_cam(lm, S.source_cam()), to_cam(lm, S.wide_ideal()))
    big = [BayerSource(lm, p, S.SW, S.SH, random_fill(rng), offset=(k + 1) % 4, pad=k) for k, p in enumerate(PATTERNS)]
    dhost = S.depth_u16()
    dbuf = lm.DeviceBuffer(dhost.nbytes)
    dbuf.upload(dhost)
    dview = dbuf.view(np.uint16, dhost.shape)
    Rd = QR.rectify_depth(dhost, qmap, 1.0)
    geometry = [((1, 3), True, (3, -2)), ((47, 39), False, (-5, 4)), ((48, 40), True, (-1, -7)), ((0, 0), False, (0, 0))]
    d.ingest_frames(0, [s.frame(depth=dview, crop=crop, flip_x=flip, shift=shift, rectified=True) for s, (crop, flip, shift) in zip(big, geometry)])
    for k, (s, (crop, flip, shift)) in enumerate(zip(big, geometry)):
        eb = QR.slot_colour(QR.rectify_colour(s.bgr(), qmap), W, H, crop, flip, shift)
        assert eb.any() and (k != 3 or (eb == 0).all(axis=2).sum() > 100)           # (the window at (0, 0) sees beyond the source)
        check_slot(d, k, eb, QR.slot_depth(Rd, W, H, crop, flip, shift), "rectified %s crop %s flip %s shift %s" % (s.pattern, crop, flip, shift))
    d.close()
    dbuf.close()
    for s in list(small.values()) + big:
        s.close()


def test_registered_route(lm):
    """lm_ingest_frames_registered with a Bayer colour image: the colour plane is the plain Bayer ingest's, the depth plane the one the same
    raw depth gives beside a BGR8 colour image."""
    import register_scenes as RS
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    d.set_registration(to_cam(lm, RS.depth_cam_a(RS.DIST)), to_cam(lm, RS.colour_cam(RS.DIST)), RS.ROT, RS.TRANS, splat=(1, 1))
    rng = np.random.default_rng(73)
    src = BayerSource(lm, "gbrg", RS.CW, RS.CH, random_fill(rng), offset=1)
    ref = np.ascontiguousarray(src.bgr())
    bbuf = lm.DeviceBuffer(ref.nbytes)
    bbuf.upload(ref)
    scene = np.ascontiguousarray(RS.scene_a())
    rbuf = lm.DeviceBuffer(scene.nbytes)
    rbuf.upload(scene)
    raw = rbuf.view(scene.dtype.type, scene.shape)
    kw = dict(depth=raw, crop=(23, 7), flip_x=True, shift=(2, -1), register_depth=True)
    d.ingest_frames(0, [dict(colour=bbuf.view(np.uint8, ref.shape), **kw)])
    d.ingest_frames(1, [src.frame(**kw), src.frame(**kw)])
    plain = d.read_frame(0)
    assert (plain[1] != 0).sum() > 5000
    for s in (1, 2):
        check_slot(d, s, IR.colour(ref, W, H, crop=(23, 7), flip_x=True, shift=(2, -1)), plain[1], "registered, slot %d" % s)
    assert np.array_equal(plain[0], d.read_frame(1)[0])
    d.close()
    for b in (src, bbuf, rbuf):
        b.close()


def test_producer_stream_with_bayer(lm):
    """The producer-stream path once with a Bayer source: filled by an asynchronous copy on a stream S, ingested at once with stream=S,
    released to S and overwritten on S -- the slot holds the demosaic of the FIRST data.  (As in test_gpu_ingest.py: this exercises the
    path, it cannot prove the ordering.)"""
    from hip_runtime import Runtime
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    rng = np.random.default_rng(75)
    nb = W * H
    pb = lm.PinnedBuffer(2 * nb)
    host = [pb.view(np.uint8, (H, W), offset=k * nb) for k in range(2)]
    for a in host:
        a[...] = rng.integers(0, 256, a.shape, dtype=np.uint8)
    first = host[0].copy()
    src = lm.DeviceBuffer(nb)
    dbuf, dview, dhost = depth_plane(lm, rng, W, H, False)
    rt = Runtime()
    St = rt.stream_create()
    try:
        rt.memcpy_h2d_async(src.ptr.value, pb.ptr.value, nb, St)
        d.ingest_frame(1, src.view(np.uint8, (H, W)), dview, layout="bayer_bggr", stream=St)
        d.ingest_release(1, 1, St)
        rt.memcpy_h2d_async(src.ptr.value, pb.ptr.value + nb, nb, St)
        check_slot(d, 1, BR.demosaic(first, "bggr"), dhost, "first data")
        rt.stream_synchronize(St)
        assert np.array_equal(src.download(np.uint8, (H, W)), host[1])
        d.upload_wait(-1)
    finally:
        rt.stream_synchronize(St)
        rt.stream_destroy(St)
    d.close()
    src.close()
    dbuf.close()
    pb.close()


def test_refusals(lm):
    """Every refusal the Bayer formats add or share, with its words, before anything is enqueued: the slot holds what it held."""
    import register_scenes as RS
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    lib, h = d.lib, d.h
    rng = np.random.default_rng(77)
    src = BayerSource(lm, "rggb", SW, SH, random_fill(rng), offset=3)
    dbuf, dview, dhost = depth_plane(lm, rng, SW, SH, False)
    good_c = lm.image_desc(src.arg, layout="bayer_rggb", crop=(3, 1))
    good_d = lm.image_desc(dview, depth=True, crop=(3, 1))

    def call(edit_c=None, edit_d=None, first=3, fn=None):
        ca, da = (lm.ImageDesc * 1)(), (lm.ImageDesc * 1)()
        for arr, one, edit in ((ca, good_c, edit_c), (da, good_d, edit_d)):
            C.memmove(C.byref(arr[0]), C.byref(one), C.sizeof(lm.ImageDesc))
            for name, value in (edit or {}).items():
                setattr(arr[0], name, value)
        rc = (fn or lib.lm_ingest_frames)(h, first, 1, ca, da, None, None)
        return rc, (lib.lm_last_error().decode() if rc else "")

    who = "colour image of frame 0: "
    keep = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 3000, (H, W)).astype(np.uint16))
    d.upload_frame(3, *keep)
    assert call(first=2) == (0, "")
    check_slot(d, 2, IR.colour(src.bgr(), W, H, crop=(3, 1)), IR.depth(dhost, W, H, (3, 1)), "the good descriptors")
    for p in PATTERNS:
        fmt, name = getattr(lm, "PIX_BAYER_%s8" % p.upper()), NAMES[p]
        assert call({"format": fmt}, first=2) == (0, "")
        # a colour format in `depth`
        assert call(edit_d={"format": fmt}) == (INVALID, "depth image of frame 0: %s is a colour format" % name)
        # half a tile at the source's edge
        even = who + "width and height of a %s source must be even" % name
        assert call({"format": fmt, "width": SW + 1}) == (INVALID, even)
        assert call({"format": fmt, "height": SH + 1}) == (INVALID, even)
        assert call({"format": fmt, "width": SW - 1, "height": SH - 1}) == (INVALID, even)
        # a YUV flag on a Bayer format names nothing
        for flags in (lm.PIX_YUV_BT709, lm.PIX_YUV_FULL, lm.PIX_YUV_BT709 | lm.PIX_YUV_FULL):
            assert call({"format": fmt | flags}) == (INVALID, who + "unknown pixel format %d" % (fmt | flags))
        # rows shorter than the window's, and shorter than the source's
        short = who + "row_stride smaller than a window row"
        for rs in (W - 1, 0, -SW, SW - 1):
            assert call({"format": fmt, "row_stride": rs}) == (INVALID, short)
        assert call({"format": fmt, "row_stride": SW, "height": SH - 2}, first=2) == (0, "")      # (still inside the buffer: two rows fewer)
    for bad in (13, 14, 15, 20, 13 | lm.PIX_YUV_BT709):
        assert call({"format": bad}) == (INVALID, who + "unknown pixel format %d" % bad)
    # the unchanged window, null-pointer and slot refusals
    roi = "0 <= roi.x && roi.x + roi.width <= m.cols && 0 <= roi.y && roi.y + roi.height <= m.rows failed: window 160 x 80 at "
    assert call({"crop_x": SW - W + 1}) == (INVALID, who + roi + "(%d, 1) in a 204 x 98 source" % (SW - W + 1))
    assert call({"crop_y": -1}) == (INVALID, who + roi + "(3, -1) in a 204 x 98 source")
    assert call({"data": None}) == (INVALID, who + "null data pointer")
    assert call(first=4) == (INVALID, "slot out of range")
    # as raw depth
    d.set_registration(to_cam(lm, RS.depth_cam_a(RS.DIST)), to_cam(lm, RS.colour_cam(RS.DIST)), RS.ROT, RS.TRANS)
    for p in PATTERNS:
        assert call(edit_d={"format": getattr(lm, "PIX_BAYER_%s8" % p.upper())}, fn=lib.lm_ingest_frames_registered) == \
            (INVALID, "raw depth image of frame 0: %s is a colour format" % NAMES[p])
    # the rectified route: a source row
    d.set_rectification(to_cam(lm, S.source_cam(w=SW, h=SH)), to_cam(lm, S.ideal_cam(SW, SH)))
    rect = lambda *a: lib.lm_ingest_frames_rectified(*a[:6], 0, a[6])
    assert call({"row_stride": SW - 1}, fn=rect) == (INVALID, "rectification: " + who + "row_stride smaller than a source row")
    assert call({"height": SH + 1}, fn=rect) == (INVALID, "rectification: " + who + "a 204 x 99 image is not the source camera (204 x 98)")
    # nothing was enqueued by any refusal: slot 3 holds what it held
    d.upload_wait(-1)
    check_slot(d, 3, keep[0], keep[1], "the slot of the refused calls")
    d.close()
    src.close()
    dbuf.close()
