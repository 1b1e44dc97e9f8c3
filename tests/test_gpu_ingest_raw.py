"""The high-bit raw source formats and the raw pipeline of lm_ingest_frames on the GPU (ABI 0.13 additive, DESIGN.md section 13 "High-bit
raw sources and the raw pipeline"): Bayer and mono sources of 10 .. 16 bits in u16 containers and PFNC-packed, and 8-bit Bayer under a
pipeline, in device memory -> the slots, compared byte for byte through read_frame with tests/ingest_raw_reference.py (the rule of
include/linemod_hip.h on the WHOLE source in numpy int64, then the window, mirror and shift of that image), on a 160 x 80 RGB-D detector
and a 48 x 32 colour-only one; then the setter between calls, the match after a raw ingest, the rectified and the registered routes, the
producer stream and the refusals with their words."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ingest_bayer_reference as BR
import ingest_raw_reference as RR
import ingest_reference as IR
import ingest_yuv_reference as YR
import rectify_reference as QR
import rectify_scenes as S
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

SW, SH = 204, 98          # source size of the geometry sweep: even, and no multiple of 16
INVALID = 1
DETECTORS = [pytest.param(True, id="rgbd_160x80"), pytest.param(False, id="colour_48x32")]
ALL = RR.PATTERNS + (RR.MONO,)
U16_12, P10, P12 = (12, False), (10, True), (12, True)
TILES = {"rggb": "BAYER_RGGB", "grbg": "BAYER_GRBG", "gbrg": "BAYER_GBRG", "bggr": "BAYER_BGGR", "mono": "MONO"}


def fmt_name(pattern, storage):
    return "LM_PIX_%s%d%s" % (TILES[pattern], storage[0], "P" if storage[1] else "")


def pin_pipe():
    return dict(black=64, gain=np.array([2048, 1024, 1536]), ccm=np.full((3, 3), -256) + 1792 * np.eye(3, dtype=np.int64),
                tone=((7 * np.arange(4096) + 3) & 255).astype(np.uint8))


def hard_pipe(bits):
    """Black above some samples, one gain that saturates, matrix entries that drive sums below 0 and above 65535, a random non-monotone
    table.  black scales with the sample range so that every depth has samples on both sides of it."""
    return dict(black=(1 << bits) // 5, gain=np.array([30000, 1100, 700]), ccm=np.array([[1900, -700, -300], [-5000, 2500, -400], [3000, 4000, 6000]]),
                tone=np.random.default_rng(5).integers(0, 256, 4096).astype(np.uint8))


def apply(d, pipe):
    """The pipeline's Q10 integers through the float interface, exactly (n / 1024 is a binary fraction)."""
    if pipe is None:
        d.set_raw_processing(None)
        return
    d.set_raw_processing(black=int(pipe["black"]), gains=np.asarray(pipe["gain"]) / 1024.0, ccm=np.asarray(pipe["ccm"]) / 1024.0, tone=pipe["tone"])
    got = d.raw_processing()
    assert got["black"] == pipe["black"] and np.array_equal(got["gain"], pipe["gain"]) and np.array_equal(got["ccm"], pipe["ccm"]) and np.array_equal(got["tone"], pipe["tone"])


class RawSource:
    """One raw image in a DeviceBuffer that ends where the image ends, `offset` bytes behind the buffer's start, with rows `pad` bytes
    longer than their samples.  storage = (bits, packed); bits 8: one byte per sample, an 8-bit Bayer format.  `words`: [h, w] integers --
    container words (bits above N may be set: they clamp), or samples below 2^bits.  `arg` and frame() are what Detector.ingest_frame
    takes, samples() what the rule reads."""

    def __init__(self, lm, pattern, storage, w, h, words, offset=0, pad=0):
        self.pattern, self.storage, self.w, self.h = pattern, storage, w, h
        bits, packed = storage
        words = np.asarray(words).astype(np.int64)
        assert words.shape == (h, w)
        if bits == 8:
            rows, self._samples = words.astype(np.uint8), words
        elif packed:
            rows, self._samples = RR.pack(words, bits), words
        else:
            assert offset % 2 == 0 and pad % 2 == 0
            rows, self._samples = RR.container(words).view(np.uint8).reshape(h, 2 * w), RR.uncontainer(words, bits)
        rb = rows.shape[1]
        rs = rb + pad
        nbytes = offset + (h - 1) * rs + rb
        raw = np.random.default_rng(w * h + offset).integers(0, 256, nbytes, dtype=np.uint8)      # (padding and lead-in: anything)
        np.lib.stride_tricks.as_strided(raw[offset:], (h, rb), (rs, 1))[...] = rows
        self.buf = lm.DeviceBuffer(nbytes)
        self.buf.upload(raw)
        if bits == 8 or packed:
            self.arg = self.buf.view(np.uint8, (h, rb), offset=offset, strides=(rs, 1))
        else:
            self.arg = self.buf.view(np.uint16, (h, w), offset=offset, strides=(rs, 2))
        self._bgr = {}

    def samples(self):
        return self._samples

    def bgr(self, pipe=None, key="identity"):
        """The BGR image the rule yields from the whole source under `pipe` (None: the identity): computed once per key and shared."""
        if key not in self._bgr:
            self._bgr[key] = RR.process(self._samples, self.storage[0], self.pattern, pipe)
            self._bgr[key].setflags(write=False)
        return self._bgr[key]

    def frame(self, **kw):
        bits, packed = self.storage
        if bits == 8:
            return dict(colour=self.arg, layout="bayer_" + self.pattern, **kw)
        layout = "mono" if self.pattern == RR.MONO else "bayer_" + self.pattern
        return dict(colour=self.arg, layout=layout, bits=bits, packed=packed, width=self.w if packed else None, **kw)

    def close(self):
        self.buf.close()


def random_words(rng, storage, w, h, stray=False):
    """Random samples; stray: container words with bits above N set in half of them."""
    bits = storage[0]
    s = rng.integers(0, 1 << bits, (h, w))
    if stray and not storage[1] and bits < 16:
        s = s | (rng.integers(0, 1 << (16 - bits), (h, w)) << bits) * (rng.random((h, w)) < 0.5)
    return s


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
def depth_sources(lm):
    rng = np.random.default_rng(81)
    dep = {f32: depth_plane(lm, rng, SW, SH, f32) for f32 in (False, True)}
    yield dep
    for b, _, _ in dep.values():
        b.close()


# (storage, the full crop set?): u16-12, 10p and 12p in full, u16-10 / 14 / 16 on a reduced crop set
SWEEPS = [pytest.param(U16_12, True, id="u16_12"), pytest.param(P10, True, id="10p"), pytest.param(P12, True, id="12p"),
          pytest.param((10, False), False, id="u16_10_reduced"), pytest.param((14, False), False, id="u16_14_reduced"), pytest.param((16, False), False, id="u16_16_reduced")]


@pytest.mark.parametrize("storage,full", SWEEPS)
@pytest.mark.parametrize("rgbd", DETECTORS)
def test_geometry_and_phase(lm, depth_sources, rgbd, storage, full):
    """Four patterns and mono in one call x base offset (packed 0 .. 3, containers 0 and 2; rows 3 or 2 bytes longer than their samples) x
    crop_x {0, 1, 2, 3, max - 1, max} x crop_y {0, 1, max} x mirror, each case with a shift of (3, -2), (-5, 1) or none and one of the two
    depth formats, under the pin's pipeline.  crop_x 0 .. 3 reaches all four bit phases of 10p and both of 12p; crops 0 and max put the
    window on each source edge (the reflection); every other window takes its neighbours from the source outside it."""
    W, H = (160, 80) if rgbd else (48, 32)
    dep = depth_sources
    bits, packed = storage
    rng = np.random.default_rng(83 + bits + packed)
    offsets = (range(4) if packed else (0, 2)) if full else (2,)
    src = {(p, off): RawSource(lm, p, storage, SW, SH, random_words(rng, storage, SW, SH, stray=True), offset=off, pad=3 if packed else 2) for p in ALL for off in offsets}
    d = lm.Detector(color_only=not rgbd, width=W, height=H, frame_slots=5)
    pipe = pin_pipe()
    apply(d, pipe)
    shifts = ((3, -2), (-5, 1), (0, 0))
    crops_x, crops_y = ((0, 1, 2, 3, SW - W - 1, SW - W), (0, 1, SH - H)) if full else ((1, SW - W), (1, SH - H))
    geometry = list(itertools.product(offsets, crops_x, crops_y, (False, True)))
    pick = np.random.default_rng(85).integers(0, (3, 2), (len(geometry), 2))        # shift and depth format: drawn per case
    if not full:
        pick = np.array([(i % 3, i % 2) for i in range(len(geometry))])             # (eight cases: by turns)
    cases = [(off, cx, cy, flip, shifts[k[0]], bool(k[1])) for (off, cx, cy, flip), k in zip(geometry, pick)]
    # the case most likely to be wrong is there: odd crop_x, odd crop_y, mirrored, shifted
    assert any(c[1] % 2 and c[2] % 2 and c[3] and c[4] != (0, 0) for c in cases)
    for off, cx, cy, flip, shift, f32 in cases:
        d.ingest_frames(0, [src[p, off].frame(depth=dep[f32][1] if rgbd else None, crop=(cx, cy), flip_x=flip, shift=shift) for p in ALL])
        ed = IR.depth(dep[f32][2], W, H, (cx, cy), 1.0, flip, shift) if rgbd else None
        for s, p in enumerate(ALL):
            check_slot(d, s, RR.slot(src[p, off].bgr(pipe, "pin"), W, H, (cx, cy), flip, shift), ed,
                       "%s %s offset %d crop (%d, %d) flip %s shift %s f32 %s" % (p, storage, off, cx, cy, flip, shift, f32))
    d.close()
    for s in src.values():
        s.close()


@pytest.mark.parametrize("rgbd", DETECTORS)
def test_source_of_exactly_the_windows_size(lm, rgbd):
    """Dense (row_stride == the row's bytes), in a buffer that ends with the image: all four edges reflect at once, and nothing lies
    beyond them.  Every storage; the patterns take turns."""
    W, H = (160, 80) if rgbd else (48, 32)
    rng = np.random.default_rng(87)
    d = lm.Detector(color_only=not rgbd, width=W, height=H, frame_slots=6)
    pipe = pin_pipe()
    apply(d, pipe)
    dbuf, dview, dhost = depth_plane(lm, rng, W, H, False) if rgbd else (None, None, None)
    storages = [(10, False), (12, False), (14, False), (16, False), P10, P12]
    for k, off in enumerate((0, 2, 1)):
        src = [RawSource(lm, ALL[(k + n) % 5], st, W, H, random_words(rng, st, W, H), offset=off if st[1] else off & 2) for n, st in enumerate(storages)]
        for flip, shift in ((False, (0, 0)), (True, (3, -2))):
            d.ingest_frames(0, [s.frame(depth=dview, flip_x=flip, shift=shift) for s in src])
            for n, s in enumerate(src):
                check_slot(d, n, RR.slot(s.bgr(pipe, "pin"), W, H, (0, 0), flip, shift), IR.depth(dhost, W, H, (0, 0), 1.0, flip, shift) if rgbd else None,
                           "%s %s offset %d flip %s shift %s" % (s.pattern, s.storage, off, flip, shift))
        for s in src:
            s.close()
    d.close()
    if dbuf:
        dbuf.close()


VW, VH = 160, 80
VALUE_STORAGES = [(10, False), (12, False), (14, False), (16, False), P10, P12]


def value_frames(storage):
    """Three 160 x 80 frames of a storage: random N-bit samples; samples drawn from {0, 1, 2^N - 2, 2^N - 1} with a block of each extreme
    planted (in a corner too, where the neighbourhood is the reflection's); and, for a container, random words with bits above N set."""
    bits = storage[0]
    rng = np.random.default_rng(89 + bits)
    top = (1 << bits) - 1
    a = rng.integers(0, top + 1, (VH, VW))
    b = np.array([0, 1, top - 1, top])[rng.integers(0, 4, (VH, VW))]
    b[10:15, 20:25] = 0
    b[40:45, 100:105] = top
    b[0:3, 0:3] = top
    b[VH - 3:, VW - 3:] = 0
    frames = [a, b]
    if not storage[1] and bits < 16:
        c = rng.integers(0, 65536, (VH, VW))
        c[5:9, 5:9] = top + 1           # (the first word that clamps)
        c[20:24, 30:34] = 65535
        frames.append(c)
    return frames


@pytest.mark.parametrize("storage", VALUE_STORAGES)
def test_value_frames_reach_what_they_should(storage):
    """(No GPU work: the frames themselves under the hard pipeline.)  Every clamp of the rule is reached on both sides: samples below and
    above black, a gain product that saturates and one that does not, matrix sums below 0, inside and above 65535; and a container's
    stray bits clamp."""
    bits = storage[0]
    pipe = hard_pipe(bits)
    frames = value_frames(storage)
    for k, words in enumerate(frames):
        s = RR.uncontainer(words, bits) if not storage[1] else words
        if k == 2:
            assert (words > (1 << bits) - 1).mean() > 0.5 and (s == (1 << bits) - 1).mean() > 0.5
        assert (s < pipe["black"]).any() and (s > pipe["black"]).any()
        sp = np.maximum(s - pipe["black"], 0)
        for pattern in ("rggb", "mono"):
            R, G, B = RR.demosaic_channels(sp, pattern)
            x = [np.minimum(((v << (16 - bits)) * g + 512) >> 10, 65535) for v, g in zip((R, G, B), pipe["gain"])]
            assert (((R << (16 - bits)) * pipe["gain"][0] + 512) >> 10 > 65535).any() and (x[0] < 65535).any() and (x[1] < 65535).all()
            sums = [(pipe["ccm"][i] * np.stack(x, -1)).sum(-1) + 512 >> 10 for i in range(3)]
            assert any((t < 0).any() for t in sums) and any((t > 65535).any() for t in sums)
            assert k == 2 or all(((t >= 0) & (t <= 65535)).any() for t in sums)         # (the stray-bit frame is mostly saturated: its point is the clamp in front)
    if bits < 16:
        Sp = np.pad(frames[1], 1, mode="reflect")
        total = Sp[1:-1, :-2] + Sp[1:-1, 2:] + Sp[:-2, 1:-1] + Sp[2:, 1:-1] + Sp[:-2, :-2] + Sp[:-2, 2:] + Sp[2:, :-2] + Sp[2:, 2:] + frames[1]
        assert total[0, 0] == 9 * ((1 << bits) - 1) and total[-1, -1] == 0


@pytest.mark.parametrize("storage", VALUE_STORAGES)
def test_values(lm, storage):
    """The value frames under the identity (nothing set), the pin's pipeline and the hard one, as RGGB, BGGR and mono in one call, on the
    RGB-D detector, which takes each whole; the 48 x 32 one takes the 12-bit container's frames in windows that tile them."""
    bits = storage[0]
    rng = np.random.default_rng(91)
    pipes = (("identity", None), ("pin", pin_pipe()), ("hard", hard_pipe(bits)))
    sources = [[RawSource(lm, p, storage, VW, VH, words) for p in ("rggb", "bggr", "mono")] for words in value_frames(storage)]
    d = lm.Detector(color_only=False, width=VW, height=VH, frame_slots=4)
    dbuf, dview, dhost = depth_plane(lm, rng, VW, VH, False)
    for key, pipe in pipes:
        apply(d, pipe)
        for k, src in enumerate(sources):
            d.ingest_frames(0, [s.frame(depth=dview) for s in src])
            for n, s in enumerate(src):
                check_slot(d, n, s.bgr(pipe, key), dhost, "value frame %d %s %s pipeline %s" % (k, s.pattern, storage, key))
                if key == "identity" and s.pattern == "mono":
                    assert np.array_equal(s.bgr(pipe, key)[..., 0], s.samples() >> (bits - 8))
    d.close()
    if storage == U16_12:
        W, H = 48, 32
        d = lm.Detector(color_only=True, width=W, height=H, frame_slots=4)
        apply(d, pipes[2][1])
        for k, src in enumerate(sources):
            for cx, cy in itertools.product(tiles(VW, W), tiles(VH, H)):
                d.ingest_frames(0, [s.frame(crop=(cx, cy)) for s in src])
                for n, s in enumerate(src):
                    check_slot(d, n, RR.slot(s.bgr(pipes[2][1], "hard"), W, H, (cx, cy)), None, "value frame %d %s window (%d, %d)" % (k, s.pattern, cx, cy))
        d.close()
    dbuf.close()
    for src in sources:
        for s in src:
            s.close()


@pytest.mark.parametrize("rgbd", DETECTORS)
def test_bayer8_and_the_setter_between_calls(lm, rgbd):
    """8-bit Bayer with nothing set (the unprocessed kernel), then under the identity, then under the hard pipeline: the first two are
    equal, the third is the reference's.  A call that mixes a 12-bit raw frame, an 8-bit Bayer frame, NV12 and BGR8 before and after a
    pipeline is set: set_raw_processing changes the calls behind it only, GRAY8 and the other formats never."""
    W, H = (160, 80) if rgbd else (48, 32)
    rng = np.random.default_rng(93)
    d = lm.Detector(color_only=not rgbd, width=W, height=H, frame_slots=5)
    dbuf, dview, dhost = depth_plane(lm, rng, SW, SH, True) if rgbd else (None, None, None)
    raw8 = rng.integers(0, 256, (SH, SW))
    raw8[30:40, 50:70] = 255
    b8 = {p: RawSource(lm, p, (8, False), SW, SH, raw8, offset=k, pad=3) for k, p in enumerate(RR.PATTERNS)}
    r12 = RawSource(lm, "gbrg", P12, SW, SH, random_words(rng, P12, SW, SH), offset=1, pad=1)
    other = {}
    for name, shape in (("nv12", (SH * 3 // 2, SW)), ("bgr", (SH, SW, 3)), ("gray", (SH, SW))):
        host = rng.integers(0, 256, shape, dtype=np.uint8)
        buf = lm.DeviceBuffer(host.nbytes)
        buf.upload(host)
        other[name] = (buf, buf.view(np.uint8, shape), host)
    nv = other["nv12"][2]
    geo = dict(crop=(3, 1), flip_x=True, shift=(3, -2))
    kw = dict(depth=dview, **geo)
    ed = IR.depth(dhost, W, H, (3, 1), 1.0, True, (3, -2)) if rgbd else None
    window = lambda img: RR.slot(img, W, H, **geo)
    hard = hard_pipe(8)
    for key, pipe in (("unset", None), ("identity", RR.identity()), ("hard", hard), ("unset again", None)):
        apply(d, pipe)
        d.ingest_frames(0, [b8[p].frame(**kw) for p in RR.PATTERNS])
        for s, p in enumerate(RR.PATTERNS):
            want = b8[p].bgr(hard, "hard") if key == "hard" else BR.demosaic(raw8.astype(np.uint8), p)
            if key != "hard":
                assert np.array_equal(want, b8[p].bgr())            # (the identity pipeline's bytes ARE the unprocessed demosaic's)
            check_slot(d, s, window(want), ed, "8-bit %s, pipeline %s" % (p, key))
        # raw 12p, 8-bit Bayer, NV12, BGR8 and GRAY8 in one call: k_ingest_raw, k_ingest_bayer (k_ingest_raw once a pipeline is set),
        # k_ingest_yuv, k_ingest, k_ingest_yuv
        d.ingest_frames(0, [r12.frame(**kw), b8["grbg"].frame(**kw), dict(colour=other["nv12"][1], layout="nv12", matrix="bt709", **kw),
                            dict(colour=other["bgr"][1], **kw), dict(colour=other["gray"][1], layout="gray", **kw)])
        refs = (r12.bgr(hard, "hard") if key == "hard" else r12.bgr(), b8["grbg"].bgr(hard, "hard") if key == "hard" else b8["grbg"].bgr(),
                YR.yuv_to_bgr((nv[:SH], nv[SH:]), "nv12", ("bt709", "limited")), other["bgr"][2], YR.yuv_to_bgr(other["gray"][2], "gray"))
        for s, ref in enumerate(refs):
            check_slot(d, s, window(ref), ed, "mixed call, slot %d, pipeline %s" % (s, key))
    assert not np.array_equal(r12.bgr(hard, "hard"), r12.bgr()) and not np.array_equal(b8["grbg"].bgr(hard, "hard"), b8["grbg"].bgr())
    d.close()
    for s in list(b8.values()) + [r12]:
        s.close()
    for b, _, _ in other.values():
        b.close()
    if dbuf:
        dbuf.close()


class Rig:
    """The 320 x 240 rig of test_gpu_ingest_bayer.py with a 12-bit camera: a synthetic scene seen through an RGGB mosaic at 12 bits
    (packed), white-balanced and tone-mapped by a pipeline, a 40-template bank cut from what the reference rule makes of it, 4 slots."""
    W, H, THR = 320, 240, 75.0

    def __init__(self, lm, orc, synth):
        W, H = self.W, self.H
        self.lm = lm
        self.d = d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
        scene, self.depth = synth.make_frame(W, H, seed=500)
        rng = np.random.default_rng(95)
        mosaic12 = (BR.mosaic(scene, "rggb").astype(np.int64) << 4 | rng.integers(0, 16, (H, W))) * 3 // 4 + 200
        self.pipe = dict(black=200, gain=np.array([1400, 1365, 1380]), ccm=np.array([[1100, -50, -26], [-30, 1090, -36], [-10, -60, 1094]]),
                         tone=lm.tone_curve(1.1))
        apply(d, self.pipe)
        self.raw = RawSource(lm, "rggb", P12, W, H, mosaic12, offset=1, pad=2)
        self.bgr = self.raw.bgr(self.pipe, "rig").copy()
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


def test_match_after_raw_ingest(rig):
    """match_slot and match_batch after a raw ingest give the lists they give after upload_frame of the reference frame; and while a lane
    has a match in flight the setter is refused and the setting stays."""
    d, THR, lm = rig.d, rig.THR, rig.lm
    for s in range(4):
        d.upload_frame(s, rig.bgr, rig.depth)
    up_slot = d.match_slot(1, THR, 0)
    up_out, up_cnt = d.match_batch(4, THR, 0)
    assert len(up_slot) > 0
    d.ingest_frames(0, [rig.frame] * 4)
    check_slot(d, 2, rig.bgr, rig.depth, "raw rig frame")
    in_slot = d.match_slot(1, THR, 0)
    in_out, in_cnt = d.match_batch(4, THR, 0)
    assert_matches_equal(in_slot, up_slot)
    for s in range(4):
        assert_matches_equal(in_out[s, :in_cnt[s]], up_out[s, :up_cnt[s]])
    d.match_begin(0, 0, 4, THR, 0)
    try:
        with pytest.raises(lm.LinemodError) as e:
            d.set_raw_processing(black=1)
        assert e.value.code == INVALID and d.lib.lm_last_error() == b"raw processing: a lane has a match in flight: call lm_match_end first"
        with pytest.raises(lm.LinemodError):
            d.set_raw_processing(None)
    finally:
        d.match_end(0, n_slots=4)
    got = d.raw_processing()
    assert got["black"] == 200 and np.array_equal(got["ccm"], rig.pipe["ccm"]) and np.array_equal(got["tone"], rig.pipe["tone"])


def to_cam(lm, c):
    return lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])


def test_rectified_route(lm):
    """lm_stage_rectify of a 20 x 8 RGGB12 and a 20 x 8 MONO10p source (and, under the pipeline, an 8-bit GRBG one) into 19 x 7 and 20 x 8
    ideal geometries through a caller's map with entries on all four borders, in the corners, far outside and not finite; then one
    lm_ingest_frames_rectified call of four storages into the 160 x 80 detector through a lens that leaves the source in the corners.
    Expected: the reference's rectification of the reference's processed image -- a tap is the processed pixel, 0 outside the source."""
    W, H = S.W, S.H
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    rng = np.random.default_rng(97)
    pipe = pin_pipe()
    apply(d, pipe)
    small = [RawSource(lm, "rggb", U16_12, 20, 8, random_words(rng, U16_12, 20, 8, stray=True), offset=2, pad=2),
             RawSource(lm, "mono", P10, 20, 8, random_words(rng, P10, 20, 8), offset=3, pad=1),
             RawSource(lm, "grbg", (8, False), 20, 8, rng.integers(0, 256, (8, 20)), offset=1, pad=3)]
    tiny_cam = S.source_cam(w=20, h=8)
    for iw, ih in ((19, 7), (20, 8)):
        table = S.smooth_table(iw, ih, sw=20, sh=8)
        d.set_rectification(to_cam(lm, tiny_cam), to_cam(lm, S.ideal_cam(iw, ih)), map=table)
        qmap = QR.quant_table(table, tiny_cam)
        assert (qmap == -64).any() and (qmap[:, :, 0] > 32 * 20).any() and (qmap[:, :, 0] == 32 * 19).any() and (qmap[:, :, 1] == 32 * 7).any()
        for s in small:
            f = s.frame()
            got = d.stage_rectify(f.pop("colour"), None, **f)
            assert got[1] is None and np.array_equal(got[0], QR.rectify_colour(s.bgr(pipe, "pin"), qmap)), "%s %s into %d x %d" % (s.pattern, s.storage, iw, ih)
    # through the slots
    qmap = QR.build_map(S.source_cam(), S.wide_ideal())
    d.set_rectification(to_cam(lm, S.source_cam()), to_cam(lm, S.wide_ideal()))
    big = [RawSource(lm, p, st, S.SW, S.SH, random_words(rng, st, S.SW, S.SH), offset=off, pad=pad)
           for p, st, off, pad in (("bggr", U16_12, 2, 0), ("gbrg", P10, 1, 3), ("mono", P12, 3, 0), ("rggb", (16, False), 0, 2))]
    dhost = S.depth_u16()
    dbuf = lm.DeviceBuffer(dhost.nbytes)
    dbuf.upload(dhost)
    dview = dbuf.view(np.uint16, dhost.shape)
    Rd = QR.rectify_depth(dhost, qmap, 1.0)
    geometry = [((1, 3), True, (3, -2)), ((47, 39), False, (-5, 4)), ((48, 40), True, (-1, -7)), ((0, 0), False, (0, 0))]
    d.ingest_frames(0, [s.frame(depth=dview, crop=crop, flip_x=flip, shift=shift, rectified=True) for s, (crop, flip, shift) in zip(big, geometry)])
    for k, (s, (crop, flip, shift)) in enumerate(zip(big, geometry)):
        eb = QR.slot_colour(QR.rectify_colour(s.bgr(pipe, "pin"), qmap), W, H, crop, flip, shift)
        assert eb.any() and (k != 3 or (eb == 0).all(axis=2).sum() > 100)           # (the window at (0, 0) sees beyond the source)
        check_slot(d, k, eb, QR.slot_depth(Rd, W, H, crop, flip, shift), "rectified %s %s crop %s flip %s shift %s" % (s.pattern, s.storage, crop, flip, shift))
    d.close()
    dbuf.close()
    for s in small + big:
        s.close()


def test_registered_route(lm):
    """lm_ingest_frames_registered with raw colour images: the colour plane is the plain raw ingest's, the depth plane the one the same
    raw depth gives beside a BGR8 colour image."""
    import register_scenes as RS
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    d.set_registration(to_cam(lm, RS.depth_cam_a(RS.DIST)), to_cam(lm, RS.colour_cam(RS.DIST)), RS.ROT, RS.TRANS, splat=(1, 1))
    pipe = pin_pipe()
    apply(d, pipe)
    rng = np.random.default_rng(99)
    a = RawSource(lm, "gbrg", P10, RS.CW, RS.CH, random_words(rng, P10, RS.CW, RS.CH), offset=1, pad=1)
    b = RawSource(lm, "mono", (14, False), RS.CW, RS.CH, random_words(rng, (14, False), RS.CW, RS.CH, stray=True), offset=2)
    ref = np.ascontiguousarray(a.bgr(pipe, "pin"))
    bbuf = lm.DeviceBuffer(ref.nbytes)
    bbuf.upload(ref)
    scene = np.ascontiguousarray(RS.scene_a())
    rbuf = lm.DeviceBuffer(scene.nbytes)
    rbuf.upload(scene)
    raw = rbuf.view(scene.dtype.type, scene.shape)
    geo = dict(crop=(23, 7), flip_x=True, shift=(2, -1))
    kw = dict(depth=raw, register_depth=True, **geo)
    d.ingest_frames(0, [dict(colour=bbuf.view(np.uint8, ref.shape), **kw)])
    d.ingest_frames(1, [a.frame(**kw), b.frame(**kw)])
    plain = d.read_frame(0)
    assert (plain[1] != 0).sum() > 5000
    check_slot(d, 1, RR.slot(ref, W, H, **geo), plain[1], "registered, 10p")
    check_slot(d, 2, RR.slot(b.bgr(pipe, "pin"), W, H, **geo), plain[1], "registered, mono 14")
    assert np.array_equal(plain[0], d.read_frame(1)[0])
    d.close()
    for x in (a, b, bbuf, rbuf):
        x.close()


def test_producer_stream_with_raw(lm):
    """The producer-stream path once with a raw source: filled by an asynchronous copy on a stream S, ingested at once with stream=S,
    released to S and overwritten on S -- the slot holds the processed FIRST data.  (As in test_gpu_ingest.py: this exercises the path,
    it cannot prove the ordering.)"""
    from hip_runtime import Runtime
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    pipe = pin_pipe()
    apply(d, pipe)
    rng = np.random.default_rng(101)
    rb = W * 12 // 8
    nb = rb * H
    pb = lm.PinnedBuffer(2 * nb)
    host = [pb.view(np.uint8, (H, rb), offset=k * nb) for k in range(2)]
    for a in host:
        a[...] = rng.integers(0, 256, a.shape, dtype=np.uint8)
    first = host[0].copy()
    src = lm.DeviceBuffer(nb)
    dbuf, dview, dhost = depth_plane(lm, rng, W, H, False)
    rt = Runtime()
    St = rt.stream_create()
    try:
        rt.memcpy_h2d_async(src.ptr.value, pb.ptr.value, nb, St)
        d.ingest_frame(1, src.view(np.uint8, (H, rb)), dview, layout="bayer_bggr", bits=12, packed=True, width=W, stream=St)
        d.ingest_release(1, 1, St)
        rt.memcpy_h2d_async(src.ptr.value, pb.ptr.value + nb, nb, St)
        check_slot(d, 1, RR.process(RR.unpack(first, 12, W), 12, "bggr", pipe), dhost, "first data")
        rt.stream_synchronize(St)
        assert np.array_equal(src.download(np.uint8, (H, rb)), host[1])
        d.upload_wait(-1)
    finally:
        rt.stream_synchronize(St)
        rt.stream_destroy(St)
    d.close()
    src.close()
    dbuf.close()
    pb.close()


def test_refusals(lm):
    """Every refusal the raw formats add or share, with its words, before anything is enqueued: the slot holds what it held."""
    import register_scenes as RS
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    lib, h = d.lib, d.h
    rng = np.random.default_rng(103)
    pipe = pin_pipe()
    apply(d, pipe)
    srcs = {st: RawSource(lm, "rggb", st, SW, SH, random_words(rng, st, SW, SH), offset=2, pad=2) for st in (U16_12, P10, P12)}
    dbuf, dview, dhost = depth_plane(lm, rng, SW, SH, False)
    good_d = lm.image_desc(dview, depth=True, crop=(3, 1))
    who = "colour image of frame 0: "
    keep = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 3000, (H, W)).astype(np.uint16))
    d.upload_frame(3, *keep)
    d.set_registration(to_cam(lm, RS.depth_cam_a(RS.DIST)), to_cam(lm, RS.colour_cam(RS.DIST)), RS.ROT, RS.TRANS)
    d.set_rectification(to_cam(lm, S.source_cam(w=SW, h=SH)), to_cam(lm, S.ideal_cam(SW, SH)))
    rect = lambda *a: lib.lm_ingest_frames_rectified(*a[:6], 0, a[6])
    for st, src in srcs.items():
        bits, packed = st
        f = src.frame(crop=(3, 1))
        good_c = lm.image_desc(f["colour"], layout=f["layout"], bits=bits, packed=packed, width=f["width"], crop=(3, 1))
        base = good_c.format & ~15
        row = (SW * (bits if packed else 16) + 7) // 8

        def call(edit_c=None, edit_d=None, first=3, fn=None):
            ca, da = (lm.ImageDesc * 1)(), (lm.ImageDesc * 1)()
            for arr, one, edit in ((ca, good_c, edit_c), (da, good_d, edit_d)):
                C.memmove(C.byref(arr[0]), C.byref(one), C.sizeof(lm.ImageDesc))
                for name, value in (edit or {}).items():
                    setattr(arr[0], name, value)
            rc = (fn or lib.lm_ingest_frames)(h, first, 1, ca, da, None, None)
            return rc, (lib.lm_last_error().decode() if rc else "")

        assert call(first=2) == (0, "")
        check_slot(d, 2, RR.slot(src.bgr(pipe, "pin"), W, H, (3, 1)), IR.depth(dhost, W, H, (3, 1)), "the good descriptors")
        for pat, p in enumerate(ALL):
            fmt, name = base | pat, fmt_name(p, st)
            assert getattr(lm, name[3:]) == fmt
            assert call({"format": fmt}, first=2) == (0, "")
            # a colour format in `depth`, and as raw depth
            assert call(edit_d={"format": fmt}) == (INVALID, "depth image of frame 0: %s is a colour format" % name)
            assert call(edit_d={"format": fmt}, fn=lib.lm_ingest_frames_registered) == (INVALID, "raw depth image of frame 0: %s is a colour format" % name)
            # half a tile at the source's edge; mono may have any size
            even = (0, "") if p == "mono" else (INVALID, who + "width and height of a %s source must be even" % name)
            assert call({"format": fmt, "width": SW - 1}, first=2) == even
            assert call({"format": fmt, "height": SH - 1}, first=2) == even
            # a YUV flag or any other bit on a raw format names nothing
            for bit in (lm.PIX_YUV_BT709, lm.PIX_YUV_FULL, 0x400, 0x800, 0x2000, 0x10000):
                assert call({"format": fmt | bit}) == (INVALID, who + "unknown pixel format %d" % (fmt | bit))
            # rows shorter than the source's
            short = who + "row_stride smaller than a window row"
            for rs in (row - 2, 0, -row, (W * (bits if packed else 16) + 7) // 8):        # (the last: a window row fits, the source's does not)
                assert call({"format": fmt, "row_stride": rs}) == (INVALID, short)
            assert call({"format": fmt, "row_stride": row, "height": SH - 2}, first=2) == (0, "")      # (still inside the buffer: two rows fewer)
            # containers are u16 sources
            if not packed:
                u16 = who + "data and row_stride of a u16 source must be multiples of 2"
                assert call({"format": fmt, "row_stride": row + 1}) == (INVALID, u16)
                assert call({"format": fmt, "data": good_c.data + 1}) == (INVALID, u16)
            else:
                assert call({"format": fmt, "row_stride": row + 1, "height": SH - 2}, first=2) == (0, "")
        for pat in (5, 8, 15):
            assert call({"format": base | pat}) == (INVALID, who + "unknown pixel format %d" % (base | pat))
        # the unchanged window, null-pointer and slot refusals
        roi = "0 <= roi.x && roi.x + roi.width <= m.cols && 0 <= roi.y && roi.y + roi.height <= m.rows failed: window 160 x 80 at "
        assert call({"crop_x": SW - W + 1}) == (INVALID, who + roi + "(%d, 1) in a 204 x 98 source" % (SW - W + 1))
        assert call({"crop_y": -1}) == (INVALID, who + roi + "(3, -1) in a 204 x 98 source")
        assert call({"data": None}) == (INVALID, who + "null data pointer")
        assert call(first=4) == (INVALID, "slot out of range")
        # the rectified route: a source row
        assert call({"row_stride": row - 2}, fn=rect) == (INVALID, "rectification: " + who + "row_stride smaller than a source row")
        assert call({"height": SH + 1}, fn=rect) == (INVALID, "rectification: " + who + "a 204 x 99 image is not the source camera (204 x 98)")
    for bad in (0x1060, 0x1064, 0x10F0, 0x1100, 13, 14, 15, 20, 99, -1, 0x300):
        assert call({"format": bad}) == (INVALID, who + "unknown pixel format %d" % bad)
    # the setter's refusals leave the setting, and nothing was enqueued by any refusal: slot 3 holds what it held
    for kw, words in ((dict(black=-1), "raw processing: black -1 lies outside 0 .. 65535"), (dict(gains=(64.0, 1, 1)), "raw processing: gain 65536 lies above 65535"),
                      (dict(ccm=np.eye(3) * 8.001), "raw processing: matrix entry 8193 lies outside -8192 .. 8192")):
        with pytest.raises(lm.LinemodError) as e:
            d.set_raw_processing(**kw)
        assert e.value.code == INVALID and lib.lm_last_error().decode() == words
    assert d.raw_processing()["black"] == 64
    d.upload_wait(-1)
    check_slot(d, 3, keep[0], keep[1], "the slot of the refused calls")
    d.close()
    for s in srcs.values():
        s.close()
    dbuf.close()
