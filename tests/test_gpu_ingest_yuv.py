"""The grey and YUV source formats of lm_ingest_frames on the GPU (ABI 0.12): GRAY8, NV12, NV21, YUY2 and UYVY
sources in device memory -> the slots, compared byte for byte through read_frame with tests/ingest_yuv_reference.py (the integer rule
in numpy int64 over the whole source, then ingest_reference's crop, mirror and shift of that image as BGR8), on a 160 x 80 RGB-D
detector and a 48 x 32 colour-only one; then the match after an NV12 ingest, the refusals with their words and the producer stream."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ingest_reference as IR
import ingest_yuv_reference as YR
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

SW, SH = 204, 98          # source size of the geometry sweep: even, as 4:2:0 wants, and no multiple of 16
INVALID = 1
DETECTORS = [pytest.param(True, id="rgbd_160x80"), pytest.param(False, id="colour_48x32")]
FORMATS = ("gray", "nv12", "nv21", "yuy2", "uyvy")


class YuvSource:
    """One grey / YUV source image in a DeviceBuffer that ends where the image ends, `offset` bytes behind the buffer's start, with rows
    `pad` bytes longer than their pixels (NV12 / NV21: the chroma plane 5 bytes further behind the Y plane than its rows need): `arg` is
    what Detector.ingest_frame takes as `colour`, `host` the same bytes as ingest_yuv_reference reads them."""

    def __init__(self, lm, fmt, w, h, fill, offset=0, pad=3):
        self.fmt, self.w, self.h = fmt, w, h
        row_bytes = w * (2 if fmt in ("yuy2", "uyvy") else 1)
        rs = row_bytes + pad
        nv = fmt in ("nv12", "nv21")
        ps = h * rs + (5 if pad else 0)
        nbytes = offset + (ps + (h // 2 - 1) * rs + row_bytes if nv else (h - 1) * rs + row_bytes)
        raw = fill(nbytes)
        assert raw.dtype == np.uint8 and raw.shape == (nbytes,)
        self.buf = lm.DeviceBuffer(nbytes)
        self.buf.upload(raw)
        strided = np.lib.stride_tricks.as_strided
        if nv:
            self.arg = (self.buf.view(np.uint8, (h, w), offset=offset, strides=(rs, 1)),
                        self.buf.view(np.uint8, (h // 2, w), offset=offset + ps, strides=(rs, 1)))
            self.host = (strided(raw[offset:], (h, w), (rs, 1), writeable=False), strided(raw[offset + ps:], (h // 2, w), (rs, 1), writeable=False))
        elif fmt == "gray":
            self.arg = self.buf.view(np.uint8, (h, w), offset=offset, strides=(rs, 1))
            self.host = strided(raw[offset:], (h, w), (rs, 1), writeable=False)
        else:
            self.arg = self.buf.view(np.uint8, (h, w, 2), offset=offset, strides=(rs, 2, 1))
            self.host = strided(raw[offset:], (h, w, 2), (rs, 2, 1), writeable=False)
        self._bgr = {}

    def bgr(self, flags):
        """The BGR image the rule yields from the whole source: computed once per (matrix, range) and shared."""
        key = ("bt601", "limited") if self.fmt == "gray" else tuple(flags)
        if key not in self._bgr:
            self._bgr[key] = YR.yuv_to_bgr(self.host, self.fmt, key)
            self._bgr[key].setflags(write=False)
        return self._bgr[key]

    def frame(self, flags=("bt601", "limited"), **kw):
        return dict(colour=self.arg, layout=self.fmt, matrix=flags[0], range=flags[1], **kw)

    def close(self):
        self.buf.close()


def random_fill(rng):
    return lambda n: rng.integers(0, 256, n, dtype=np.uint8)


def packed_fill(planes):
    """The dense bytes of packed planes (one array, or NV12's (y, uv))."""
    def fill(n):
        raw = np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in (planes if isinstance(planes, tuple) else (planes,))])
        assert raw.nbytes == n
        return raw
    return fill


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


# U and V of the value frames: the edges of the ranges, the neutral point and its neighbours, and every 8th value
CHROMA = sorted({0, 1, 15, 16, 17, 127, 128, 129, 239, 240, 241, 254, 255} | set(range(0, 256, 8)))
VW, VH = 160, 80


def value_planes(pattern, pairs_w, pairs_h):
    """U, V [pairs_h, pairs_w]: every (U, V) of CHROMA x CHROMA at least once, each chroma sample its own; Y [VH, VW] by `pattern`: a ramp
    through 0 .. 255, the ramp downwards, the range edges, or random -- so that every Y meets small and large chroma of both signs."""
    n = pairs_w * pairs_h
    combos = np.array(list(itertools.product(CHROMA, CHROMA)), np.uint8)
    assert len(combos) <= n
    idx = np.arange(n) % len(combos)
    U, V = combos[idx, 0].reshape(pairs_h, pairs_w), combos[idx, 1].reshape(pairs_h, pairs_w)
    ramp = (np.arange(VW * VH) * 37 % 256).astype(np.uint8).reshape(VH, VW)          # 37 is odd: every residue, neighbours far apart
    if pattern == 0:
        Y = ramp
    elif pattern == 1:
        Y = (255 - ramp[::-1, ::-1]).astype(np.uint8)
    elif pattern == 2:
        Y = np.array([0, 15, 16, 17, 234, 235, 236, 254, 255, 128], np.uint8)[np.arange(VW * VH) * 7 % 10].reshape(VH, VW)
    else:
        Y = np.random.default_rng(21).integers(0, 256, (VH, VW), dtype=np.uint8)
    return Y, U, V


@pytest.fixture(scope="module")
def value_sources(lm):
    """Four 160 x 80 value frames per format (dense, 16-byte aligned: the fast path), shared by both detectors."""
    src = {}
    for fmt in ("nv12", "nv21", "yuy2"):
        for pattern in range(4):
            if fmt == "yuy2":
                Y, U, V = value_planes(pattern, VW // 2, VH)
                packed = YR.pack_422(Y, U, V, fmt)
            else:
                Y, U, V = value_planes(pattern, VW // 2, VH // 2)
                packed = YR.pack_nv(Y, U, V, fmt)
            src[fmt, pattern] = YuvSource(lm, fmt, VW, VH, packed_fill(packed), pad=0)
            assert set(np.unique(Y)) == set(range(256)) or pattern == 2
    yield src
    for s in src.values():
        s.close()


def test_value_frames_reach_what_they_should(value_sources):
    """(No GPU work: the frames themselves.)  Every Y, every (U, V) of the set, both saturation sides of every channel and negative sums in
    front of the shift, under every matrix and range."""
    for fmt in ("nv12", "yuy2"):
        Y, U, V = (np.concatenate([YR.planes(value_sources[fmt, p].host, fmt)[k].reshape(-1) for p in range(4)]).astype(np.int64) for k in range(3))
        assert set(np.unique(Y)) == set(range(256))
        assert {(u, v) for u, v in zip(U.tolist(), V.tolist())} == set(itertools.product(CHROMA, CHROMA))
        for flags in YR.FLAGS:
            Y0, CY, CVR, CVG, CUG, CUB = YR.COEF[flags]
            y = np.maximum(0, Y - Y0) * CY + (1 << 19)
            for s in (y + CVR * (V - 128), y + CVG * (V - 128) + CUG * (U - 128), y + CUB * (U - 128)):
                assert (s < 0).any() and ((s >> 20) > 255).any() and (((s >> 20) > 0) & ((s >> 20) < 255)).any()


@pytest.mark.parametrize("rgbd", DETECTORS)
@pytest.mark.parametrize("fmt", ["nv12", "nv21", "yuy2"])
def test_values(lm, value_sources, rgbd, fmt):
    """The value frames under the four matrix / range combinations: the RGB-D detector takes each whole, the 48 x 32 one in windows that
    tile it."""
    W, H = (160, 80) if rgbd else (48, 32)
    d = lm.Detector(color_only=not rgbd, width=W, height=H, frame_slots=4)
    rng = np.random.default_rng(31)
    dbuf, dview, dhost = depth_plane(lm, rng, VW, VH, False) if rgbd else (None, None, None)
    windows = list(itertools.product(tiles(VW, W), tiles(VH, H)))
    for flags in YR.FLAGS:
        for cx, cy in windows:
            d.ingest_frames(0, [value_sources[fmt, p].frame(flags, depth=dview, crop=(cx, cy)) for p in range(4)])
            for p in range(4):
                check_slot(d, p, IR.colour(value_sources[fmt, p].bgr(flags), W, H, crop=(cx, cy)), IR.depth(dhost, W, H, (cx, cy)) if rgbd else None,
                           "%s %s %s pattern %d window (%d, %d)" % ((fmt,) + flags + (p, cx, cy)))
    d.close()
    if dbuf:
        dbuf.close()


@pytest.fixture(scope="module")
def sweep_sources(lm):
    """204 x 98 sources of all five formats at base offsets 0 .. 3, rows 3 bytes longer than their pixels, the chroma plane at an odd
    distance; a BGR8 source for the mixed calls; dense depth sources of both formats."""
    rng = np.random.default_rng(41)
    src = {(fmt, off): YuvSource(lm, fmt, SW, SH, random_fill(rng), offset=off) for fmt in FORMATS for off in range(4)}
    bgr = rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    bbuf = lm.DeviceBuffer(bgr.nbytes)
    bbuf.upload(bgr)
    dep = {f32: depth_plane(lm, rng, SW, SH, f32) for f32 in (False, True)}
    yield src, (bbuf.view(np.uint8, bgr.shape), bgr), dep
    for s in src.values():
        s.close()
    bbuf.close()
    for b, _, _ in dep.values():
        b.close()


@pytest.mark.parametrize("rgbd", DETECTORS)
def test_geometry_and_chroma_phase(lm, sweep_sources, rgbd):
    """All five formats x base offset 0 .. 3 x crop_x {0, 1, 2, 3, max - 1, max} x crop_y {0, 1, max} x mirror, each case with a shift of (3, -2), (-5, 1)
    or none, one of the two depth formats and one of the four matrices, four frames of different formats per call; then calls that mix NV12, BGR8, UYVY and
    GRAY8, which both kernels serve."""
    W, H = (160, 80) if rgbd else (48, 32)
    src, (bgr_view, bgr_host), dep = sweep_sources
    d = lm.Detector(color_only=not rgbd, width=W, height=H, frame_slots=4)
    shifts = ((3, -2), (-5, 1), (0, 0))
    matrices = YR.FLAGS
    geometry = list(itertools.product(range(4), (0, 1, 2, 3, SW - W - 1, SW - W), (0, 1, SH - H), (False, True), FORMATS))
    pick = np.random.default_rng(43).integers(0, (3, 2, 4), (len(geometry), 3))        # shift, depth format and matrix: drawn per case
    cases = [(fmt, off, cx, cy, flip, shifts[k[0]], bool(k[1]), matrices[k[2]]) for (off, cx, cy, flip, fmt), k in zip(geometry, pick)]
    assert len(cases) % 4 == 0
    # the case most likely to be wrong is there for every format that has chroma: odd crop_x, odd crop_y, mirrored, shifted
    assert all(any(c[0] == fmt and c[2] % 2 and c[3] % 2 and c[4] and c[5] != (0, 0) for c in cases) for fmt in FORMATS[1:])

    def expected(fmt, off, cx, cy, flip, shift, f32, flags):
        eb = IR.colour(src[fmt, off].bgr(flags), W, H, crop=(cx, cy), flip_x=flip, shift=shift)
        return eb, (IR.depth(dep[f32][2], W, H, (cx, cy), 1.0, flip, shift) if rgbd else None)

    for i in range(0, len(cases), 4):
        group = cases[i:i + 4]
        assert len({c[0] for c in group}) == 4
        d.ingest_frames(0, [src[fmt, off].frame(flags, depth=dep[f32][1] if rgbd else None, crop=(cx, cy), flip_x=flip, shift=shift)
                            for fmt, off, cx, cy, flip, shift, f32, flags in group])
        for s, c in enumerate(group):
            check_slot(d, s, *expected(*c), what="%s offset %d crop (%d, %d) flip %s shift %s f32 %s %s" % c)
    # NV12, BGR8, UYVY and GRAY8 in one call
    for cx, cy, flip, shift in ((1, 1, True, (3, -2)), (SW - W, SH - H, False, (-5, 1)), (3, 0, True, (0, 0))):
        kw = dict(crop=(cx, cy), flip_x=flip, shift=shift, depth=dep[True][1] if rgbd else None)
        d.ingest_frames(0, [src["nv12", 1].frame(("bt709", "limited"), **kw), dict(colour=bgr_view, **kw), src["uyvy", 3].frame(("bt601", "full"), **kw),
                            src["gray", 2].frame(**kw)])
        ed = IR.depth(dep[True][2], W, H, (cx, cy), 1.0, flip, shift) if rgbd else None
        for s, eb in enumerate((src["nv12", 1].bgr(("bt709", "limited")), bgr_host, src["uyvy", 3].bgr(("bt601", "full")), src["gray", 2].bgr(None))):
            check_slot(d, s, IR.colour(eb, W, H, crop=(cx, cy), flip_x=flip, shift=shift), ed, "mixed call, slot %d, crop (%d, %d)" % (s, cx, cy))
    d.close()


def bgr_to_nv12(bgr):
    """A camera's side of the link, good enough to carry a scene: BT.601 limited range in float, chroma averaged over 2 x 2."""
    b, g, r = (bgr[:, :, k].astype(np.float64) for k in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    H, W = y.shape
    sub = lambda c: c.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
    return YR.pack_nv(q(y), q(sub(u)), q(sub(v)), "nv12")


class Rig:
    """The 320 x 240 rig of test_gpu_ingest.py with an NV12 producer: a frame that went through NV12, a 40-template bank cut from what
    the reference rule makes of it, 4 slots."""
    W, H, THR = 320, 240, 75.0

    def __init__(self, lm, orc, synth):
        W, H = self.W, self.H
        self.lm = lm
        self.d = d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
        scene, self.depth = synth.make_frame(W, H, seed=500)
        self.nv12 = YuvSource(lm, "nv12", W, H, packed_fill(bgr_to_nv12(scene)), pad=0)
        self.bgr = self.nv12.bgr(("bt601", "limited")).copy()
        o = orc.Detector(color_only=False)
        o.prepare(self.bgr, self.depth)
        q = {(l, m): o.stage(0, l, m).reshape(H >> l, W >> l) for l in range(2) for m in range(2)}
        descs, feats, _ = synth.make_bank(40, 2, 2, seed=99, size_range=(48, 120), quantized=q, crop_fraction=0.3, frame_size=(W, H),
                                          T0=d.get_T(0))
        d.add_class("c", descs, feats)
        self.db = lm.DeviceBuffer(self.depth.nbytes)
        self.db.upload(self.depth)
        self.frame = self.nv12.frame(depth=self.db.view(np.uint16, self.depth.shape))

    def close(self):
        self.d.close()
        self.nv12.close()
        self.db.close()


@pytest.fixture(scope="module")
def rig(lm, orc, synth):
    r = Rig(lm, orc, synth)
    yield r
    r.close()


def test_match_after_nv12_ingest(rig):
    """match_slot and match_batch after an NV12 ingest give the lists they give after upload_frame of the reference-converted BGR frame."""
    d, THR = rig.d, rig.THR
    for s in range(4):
        d.upload_frame(s, rig.bgr, rig.depth)
    up_slot = d.match_slot(1, THR, 0)
    up_out, up_cnt = d.match_batch(4, THR, 0)
    assert len(up_slot) > 0
    d.ingest_frames(0, [rig.frame] * 4)
    check_slot(d, 2, rig.bgr, rig.depth, "NV12 rig frame")
    in_slot = d.match_slot(1, THR, 0)
    in_out, in_cnt = d.match_batch(4, THR, 0)
    assert_matches_equal(in_slot, up_slot)
    for s in range(4):
        assert_matches_equal(in_out[s, :in_cnt[s]], up_out[s, :up_cnt[s]])


def test_refusals(rig):
    """Every refusal the new formats add, with its words, before anything is enqueued; the old words for formats that name nothing."""
    lm, d, W, H = rig.lm, rig.d, rig.W, rig.H
    lib, h = d.lib, d.h
    good_c = lm.image_desc(rig.frame["colour"], layout="nv12")
    good_d = lm.image_desc(rig.frame["depth"], depth=True)

    def call(edit_c=None, edit_d=None, first=3):
        ca, da = (lm.ImageDesc * 1)(), (lm.ImageDesc * 1)()
        for arr, src, edit in ((ca, good_c, edit_c), (da, good_d, edit_d)):
            C.memmove(C.byref(arr[0]), C.byref(src), C.sizeof(lm.ImageDesc))
            for name, value in (edit or {}).items():
                setattr(arr[0], name, value)
        rc = lib.lm_ingest_frames(h, first, 1, ca, da, None, None)
        return rc, (lib.lm_last_error().decode() if rc else "")

    who = "colour image of frame 0: "
    d.upload_wait(-1)
    d.upload_frame(3, rig.bgr, rig.depth)
    before = d.read_frame(3)
    assert call(first=2) == (0, "")
    for flags in (0, lm.PIX_YUV_BT709, lm.PIX_YUV_FULL, lm.PIX_YUV_BT709 | lm.PIX_YUV_FULL):
        for fmt in (lm.PIX_NV12, lm.PIX_NV21):
            assert call({"format": fmt | flags}, first=2) == (0, "")
    # GRAY8 reads the Y plane alone
    assert call({"format": lm.PIX_GRAY8}, first=2) == (0, "")
    # formats that name nothing: the old words, N as given
    for bad in (99, -1, 13, lm.PIX_GRAY8 | lm.PIX_YUV_BT709, lm.PIX_BGR8 | lm.PIX_YUV_FULL, lm.PIX_DEPTH_U16 | lm.PIX_YUV_BT709, lm.PIX_NV12 | 0x400,
                lm.PIX_NV12 | 0x80, 13 | lm.PIX_YUV_BT709, 0x300, lm.PIX_NV12 - (1 << 31)):
        assert call({"format": bad}) == (INVALID, who + "unknown pixel format %d" % bad)
    assert call(edit_d={"format": -1}) == (INVALID, "depth image of frame 0: unknown pixel format -1")
    assert call(edit_d={"format": lm.PIX_DEPTH_U16 | lm.PIX_YUV_FULL}) == (INVALID, "depth image of frame 0: unknown pixel format %d" % (6 | 0x200))
    # a colour format in `depth`
    for name in ("GRAY8", "NV12", "NV21", "YUY2", "UYVY"):
        assert call(edit_d={"format": getattr(lm, "PIX_" + name)}) == (INVALID, "depth image of frame 0: LM_PIX_%s is a colour format" % name)
    assert call(edit_d={"format": lm.PIX_NV12 | lm.PIX_YUV_BT709}) == (INVALID, "depth image of frame 0: LM_PIX_NV12 is a colour format")
    # half a chroma pair at the source's edge
    for name in ("NV12", "NV21"):
        even = who + "width and height of a LM_PIX_%s source must be even" % name
        assert call({"format": getattr(lm, "PIX_" + name), "width": W + 1}) == (INVALID, even)
        assert call({"format": getattr(lm, "PIX_" + name), "height": H + 1}) == (INVALID, even)
        assert call({"format": getattr(lm, "PIX_" + name) | lm.PIX_YUV_FULL, "width": W + 3, "height": H + 1, "crop_x": 1}) == (INVALID, even)
    for name in ("YUY2", "UYVY"):
        assert call({"format": getattr(lm, "PIX_" + name), "width": W + 1, "row_stride": 2 * W + 2}) == \
            (INVALID, who + "width of a LM_PIX_%s source must be even" % name)
    # the chroma plane
    for ps in (0, -1, -W * H):
        assert call({"plane_stride": ps}) == (INVALID, who + "plane_stride must be positive")
        assert call({"format": lm.PIX_NV21, "plane_stride": ps}) == (INVALID, who + "plane_stride must be positive")
    # rows shorter than the window's
    short = who + "row_stride smaller than a window row"
    for fmt, least in ((lm.PIX_GRAY8, W), (lm.PIX_NV12, W), (lm.PIX_NV21 | lm.PIX_YUV_BT709, W), (lm.PIX_YUY2, 2 * W), (lm.PIX_UYVY, 2 * W)):
        assert call({"format": fmt, "row_stride": least - 1}) == (INVALID, short)
        assert call({"format": fmt, "row_stride": 0}) == (INVALID, short)
        assert call({"format": fmt, "row_stride": -least}) == (INVALID, short)
    # nothing was enqueued by any refusal: slot 3 holds what it held
    after = d.read_frame(3)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_producer_stream_with_nv12(lm):
    """The producer-stream path once with NV12: the source is filled by an asynchronous copy on a stream S, ingested at once with
    stream=S, released to S and overwritten on S -- the slot holds the conversion of the FIRST data.  (As in test_gpu_ingest.py: this
    exercises the path, it cannot prove the ordering.)"""
    from hip_runtime import Runtime
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    rng = np.random.default_rng(51)
    nb = W * H * 3 // 2
    pb = lm.PinnedBuffer(2 * nb)
    host = [pb.view(np.uint8, (H * 3 // 2, W), offset=k * nb) for k in range(2)]
    for a in host:
        a[...] = rng.integers(0, 256, a.shape, dtype=np.uint8)
    first = host[0].copy()
    src = lm.DeviceBuffer(nb)
    dbuf, dview, dhost = depth_plane(lm, rng, W, H, False)
    rt = Runtime()
    S = rt.stream_create()
    try:
        rt.memcpy_h2d_async(src.ptr.value, pb.ptr.value, nb, S)
        d.ingest_frame(1, src.view(np.uint8, (H * 3 // 2, W)), dview, layout="nv12", matrix="bt709", stream=S)
        d.ingest_release(1, 1, S)
        rt.memcpy_h2d_async(src.ptr.value, pb.ptr.value + nb, nb, S)
        check_slot(d, 1, YR.yuv_to_bgr((first[:H], first[H:]), "nv12", ("bt709", "limited")), dhost, "first data")
        rt.stream_synchronize(S)
        assert np.array_equal(src.download(np.uint8, (H * 3 // 2, W)), host[1])
        d.upload_wait(-1)
    finally:
        rt.stream_synchronize(S)
        rt.stream_destroy(S)
    d.close()
    src.close()
    dbuf.close()
    pb.close()
