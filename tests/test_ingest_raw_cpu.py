"""CPU tests of the high-bit raw ingest formats and the raw pipeline (ABI 0.13 additive, DESIGN.md section 13 "High-bit raw sources and the
raw pipeline"): the reference the GPU tests compare with (tests/ingest_raw_reference.py) against the header's hand pins, against a
per-pixel loop with explicit reflected indices and against properties of the rule; the constants, the version string, what the binding
makes of a __cuda_array_interface__, the setter's round trip and refusals (host state: no device), the refusal to ingest without a
device, and tests/cpp/ingest_raw_host.cpp: csrc/lm_ingest_raw.h -- the kernel's per-lane code --, the rectify taps and the descriptor
check on the host under ASan / UBSan."""
import os
import subprocess

import numpy as np
import pytest

import ingest_bayer_reference as BR
import ingest_raw_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
P = 0x7F0012345600
INVALID = 1
ALL = RR.PATTERNS + (RR.MONO,)
STORAGE = {(10, False): 0x00, (12, False): 0x10, (14, False): 0x20, (16, False): 0x30, (10, True): 0x40, (12, True): 0x50}


class Fake:
    """Something that claims to live in device memory: nothing but the interface, with a made-up pointer."""

    def __init__(self, shape, typestr, strides=None, ptr=P):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "strides": strides, "version": 2}


def fields(d):
    return (d.data, d.row_stride, d.plane_stride, d.width, d.height, d.format, d.crop_x, d.crop_y, d.scale)


def _has_gpu(lm):
    d = lm.Detector(color_only=True, width=64, height=64, T=[2, 8])
    try:
        d.stage_pyrdown(np.zeros((8, 8, 3), np.uint8))
        return True
    except lm.LinemodError:
        return False
    finally:
        d.close()


def pin_pipe():
    return dict(black=64, gain=np.array([2048, 1024, 1536]), ccm=np.full((3, 3), -256) + 1792 * np.eye(3, dtype=np.int64),
                tone=((7 * np.arange(4096) + 3) & 255).astype(np.uint8))


PIN_SOURCE = np.array([[100, 2000], [3000, 4095]])


def test_the_hand_pins():
    """include/linemod_hip.h: the 12-bit source under the pin's pipeline and under the identity, (B, G, R) in reading order."""
    px = lambda img: [tuple(p) for p in img.reshape(4, 3).tolist()]
    assert px(RR.process(PIN_SOURCE, 12, "rggb", pin_pipe())) == [(252, 111, 3), (252, 237, 3), (252, 241, 3), (252, 111, 3)]
    R, G, B = RR.demosaic_channels(np.maximum(PIN_SOURCE - 64, 0), "rggb")
    assert list(zip(R.ravel().tolist(), G.ravel().tolist(), B.ravel().tolist())) == [(36, 2436, 4031), (36, 1936, 4031), (36, 2936, 4031), (36, 2436, 4031)]
    assert px(RR.process(PIN_SOURCE, 12, "mono", pin_pipe())) == [(125, 157, 86), (107, 25, 252), (252, 111, 252), (252, 85, 252)]
    assert px(RR.process(PIN_SOURCE, 12, "rggb")) == [(255, 156, 6), (255, 125, 6), (255, 187, 6), (255, 156, 6)]
    assert px(RR.process(PIN_SOURCE, 12, "rggb", RR.identity())) == px(RR.process(PIN_SOURCE, 12, "rggb"))


def test_the_packing_pins():
    assert RR.pack(np.array([[1, 2, 3, 1023]]), 10).tolist() == [[1, 8, 48, 192, 255]]
    assert RR.pack(np.array([[0xABC, 0x123]]), 12).tolist() == [[0xBC, 0x3A, 0x12]]
    assert RR.unpack(np.array([[1, 8, 48, 192, 255]], np.uint8), 10, 4).tolist() == [[1, 2, 3, 1023]]
    assert RR.unpack(np.array([[0xBC, 0x3A, 0x12]], np.uint8), 12, 2).tolist() == [[0xABC, 0x123]]
    # a container: little-endian, the sample in the low bits; stray high bits clamp, they do not wrap
    assert RR.container(np.array([[0x3FF, 1]])).tobytes() == b"\xff\x03\x01\x00"
    assert RR.uncontainer(np.array([[0x3FF, 0x400, 0xFFFF, 7]], "<u2"), 10).tolist() == [[1023, 1023, 1023, 7]]
    assert RR.uncontainer(np.array([[0xFFFF, 0x4000]], "<u2"), 14).tolist() == [[16383, 16383]]
    assert RR.uncontainer(np.array([[0xFFFF]], "<u2"), 16).tolist() == [[65535]]


def test_packed_and_container_storage_agree():
    """pack / unpack are inverses at every width's tail phase, and both storages of the same samples give the same image."""
    rng = np.random.default_rng(3)
    for bits in (10, 12):
        for W in range(1, 18):
            s = rng.integers(0, 1 << bits, (3, W))
            s[0, -1] = (1 << bits) - 1
            rows = RR.pack(s, bits)
            assert rows.shape == (3, (W * bits + 7) // 8)
            assert np.array_equal(RR.unpack(rows, bits, W), s)
            assert np.array_equal(RR.uncontainer(RR.container(s), bits), s)
        s = rng.integers(0, 1 << bits, (6, 8))
        for pattern in ALL:
            a = RR.process(RR.unpack(RR.pack(s, bits), bits, 8), bits, pattern, pin_pipe())
            b = RR.process(RR.uncontainer(RR.container(s), bits), bits, pattern, pin_pipe())
            assert np.array_equal(a, b)


def loop_process(s, bits, pattern, pipe):
    """The rule once more, one pixel at a time in Python integers, with the reflected indices written out."""
    H, W = s.shape
    black, gain, ccm, tone = int(pipe["black"]), [int(v) for v in pipe["gain"]], np.asarray(pipe["ccm"]).reshape(9).tolist(), pipe["tone"]

    def S(x, y):
        x = 1 if x == -1 else W - 2 if x == W else x
        y = 1 if y == -1 else H - 2 if y == H else y
        assert 0 <= x < W and 0 <= y < H
        return max(int(s[y, x]) - black, 0)

    out = np.zeros((H, W, 3), np.uint8)
    for y in range(H):
        for x in range(W):
            c = S(x, y)
            if pattern == "mono":
                R = G = B = c
            else:
                i = RR.PATTERNS.index(pattern)
                h = (S(x - 1, y) + S(x + 1, y) + 1) >> 1
                v = (S(x, y - 1) + S(x, y + 1) + 1) >> 1
                p = (S(x - 1, y) + S(x + 1, y) + S(x, y - 1) + S(x, y + 1) + 2) >> 2
                d = (S(x - 1, y - 1) + S(x + 1, y - 1) + S(x - 1, y + 1) + S(x + 1, y + 1) + 2) >> 2
                site = ((x ^ (i & 1)) & 1, (y ^ (i >> 1)) & 1)
                R, G, B = {(0, 0): (c, p, d), (1, 1): (d, p, c), (1, 0): (h, c, v), (0, 1): (v, c, h)}[site]
            xs = [min(((v << (16 - bits)) * gain[k] + 512) >> 10, 65535) for k, v in enumerate((R, G, B))]
            ys = [min(max((ccm[3 * k] * xs[0] + ccm[3 * k + 1] * xs[1] + ccm[3 * k + 2] * xs[2] + 512) >> 10, 0), 65535) for k in range(3)]
            out[y, x] = (tone[ys[2] >> 4], tone[ys[1] >> 4], tone[ys[0] >> 4])
    return out


def test_reference_against_a_per_pixel_loop():
    """Every even size from 2 x 2 to 6 x 8 (rows x columns), all four patterns and mono, N = 8, 10, 12, 14, 16, under a pipeline that uses
    every step: at the tiny sizes both reflections land on one column or row."""
    rng = np.random.default_rng(7)
    n = 0
    for bits in (8, 10, 12, 14, 16):
        top = (1 << bits) - 1
        pipe = dict(black=top // 40, gain=rng.integers(600, 3000, 3), ccm=rng.integers(-700, 1900, (3, 3)), tone=rng.integers(0, 256, 4096).astype(np.uint8))
        for H in (2, 4, 6):
            for W in (2, 4, 6, 8):
                s = rng.integers(0, top + 1, (H, W))
                s[rng.random((H, W)) < 0.3] = rng.choice(np.array([0, 1, top - 1, top]))
                for pattern in ALL:
                    assert np.array_equal(RR.process(s, bits, pattern, pipe), loop_process(s, bits, pattern, pipe)), (bits, H, W, pattern)
                    n += 1
    assert n == 5 * 12 * 5


@pytest.mark.parametrize("pattern", RR.PATTERNS)
def test_identity_on_8_bits_is_the_bayer_demosaic(pattern):
    raw = np.random.default_rng(11).integers(0, 256, (10, 14), dtype=np.uint8)
    raw[2:5, 3:7] = 255
    raw[6:9, 8:12] = 0
    assert np.array_equal(RR.process(raw, 8, pattern, RR.identity()), BR.demosaic(raw, pattern))
    assert np.array_equal(RR.process(raw, 8, pattern), BR.demosaic(raw, pattern))


@pytest.mark.parametrize("pattern", RR.PATTERNS)
def test_a_constant_colour_survives_at_12_bits(pattern):
    """A constant 12-bit colour through the mosaic and the identity comes back as its top 8 bits; the identity yields v >> (N - 8)."""
    H, W = 10, 14
    bgr12 = np.empty((H, W, 3), np.int64)
    bgr12[...] = (277, 3211, 1490)
    rx, ry = RR.PATTERNS.index(pattern) & 1, RR.PATTERNS.index(pattern) >> 1
    y, x = np.mgrid[0:H, 0:W]
    dx, dy = (x ^ rx) & 1, (y ^ ry) & 1
    channel = np.where(dx != dy, 1, np.where(dy == 0, 2, 0))
    mosaic = np.take_along_axis(bgr12, channel[..., None], axis=2)[..., 0]
    out = RR.process(mosaic, 12, pattern)
    assert np.array_equal(out, np.broadcast_to(np.array([277 >> 4, 3211 >> 4, 1490 >> 4], np.uint8), (H, W, 3)))
    for bits in (10, 12, 14, 16):
        s = np.random.default_rng(bits).integers(0, 1 << bits, (5, 7))
        assert np.array_equal(RR.process(s, bits, "mono")[..., 1], s >> (bits - 8))


def test_the_arithmetic_bounds_at_their_extremes():
    """Step 4: gain 65535 on 65535 stays below 2^32 and saturates; step 5: nine entries of +8192 and of -8192 on 65535 stay within 32
    signed bits and clamp to 65535 and 0.  (pipeline_channels asserts the 32-bit bounds itself.)"""
    assert 65535 * 65535 + 512 < 2 ** 32 and 3 * 8192 * 65535 + 512 < 2 ** 31
    tone = ((np.arange(4096) * 5 + 1) & 255).astype(np.uint8)
    full = np.full((2, 2), 65535)
    for sign, y in ((1, 65535), (-1, 0)):
        pipe = dict(black=0, gain=np.full(3, 65535), ccm=np.full((3, 3), sign * 8192), tone=tone)
        out = RR.process(full, 16, "mono", pipe)
        assert (out == tone[y >> 4]).all()
        assert (RR.process(full, 16, "rggb", pipe) == tone[y >> 4]).all()
    # just below saturation: (x * gain + 512) >> 10 = 65534 is kept, 65535 and above clamp
    pipe = RR.identity()
    pipe["tone"] = tone
    one = np.array([[65535]])
    for gain, want in ((1023, (65535 * 1023 + 512) >> 10), (1024, 65535), (1025, 65535)):
        pipe["gain"] = np.full(3, gain)
        assert want <= 65535 and (RR.process(one, 16, "mono", pipe) == tone[want >> 4]).all()
    # rounding of a negative sum: >> is an arithmetic shift (floor), then the clamp to 0
    pipe = dict(black=0, gain=np.full(3, 1024), ccm=np.array([[-1, 0, 0], [1, 0, 0], [0, 0, 0]]), tone=tone)
    out = RR.process(np.array([[600 << 0]]), 16, "mono", pipe)
    assert out.reshape(3).tolist() == [tone[0], tone[((600 + 512) >> 10) >> 4], tone[0]]


def test_composition_rule():
    """Ingesting a raw image equals ingesting, as BGR8, the image the rule yields from the WHOLE source: the window's neighbours come from
    outside it, mirror and shift come last."""
    s = np.random.default_rng(13).integers(0, 4096, (12, 40))
    whole = RR.process(s, 12, "grbg", pin_pipe())
    got = RR.slot(whole, 16, 6, crop=(3, 1), flip_x=True, shift=(2, -1))
    assert np.array_equal(got[0:5, 2:16], whole[2:7, 3:19][:, ::-1][:, 0:14]) and not got[5].any() and not got[:, :2].any()
    cropped_first = RR.process(s[1:7, 3:19], 12, "grbg", pin_pipe())        # (wrong on purpose: the pattern's phase and the edges differ)
    assert not np.array_equal(RR.slot(cropped_first, 16, 6), RR.slot(whole, 16, 6, crop=(3, 1)))
    assert not RR.slot(whole, 16, 6, shift=(16, 0)).any() and not RR.slot(whole, 16, 6, shift=(0, -6)).any()


def test_constants_and_version(lm):
    assert lm.PIX_RAW == 0x1000
    names = {}
    for (bits, packed), st in STORAGE.items():
        for pat, tile in enumerate(("BAYER_RGGB", "BAYER_GRBG", "BAYER_GBRG", "BAYER_BGGR", "MONO")):
            names["PIX_%s%d%s" % (tile, bits, "P" if packed else "")] = 0x1000 | st | pat
    assert len(names) == 30
    for name, value in names.items():
        assert getattr(lm, name) == value, name
    assert (lm.PIX_BAYER_RGGB10, lm.PIX_MONO10, lm.PIX_BAYER_GRBG12, lm.PIX_BAYER_GBRG14, lm.PIX_BAYER_BGGR16, lm.PIX_BAYER_RGGB10P, lm.PIX_MONO12P) == \
        (0x1000, 0x1004, 0x1011, 0x1022, 0x1033, 0x1040, 0x1054)
    # none of them moved into the values the earlier formats pin as unknown
    every = {v for k, v in vars(lm).items() if k.startswith("PIX_") and isinstance(v, int)}
    assert not every & {13, 14, 15, 20, 99, -1, 0x300, lm.PIX_NV12 | 0x80, lm.PIX_NV12 | 0x400}
    v = lm.load_library().lm_version()
    assert v.startswith(b"linemod_hip 0.13 ") and b"0.13 additive: high-bit raw ingest formats and the raw pipeline" in v
    for earlier in (b"0.13 additive: raw Bayer ingest formats", b"0.13 = the 0.12 ABI plus the depth registration", b"lm_ingest_frames_rectified",
                    b"0.12 = the 0.11 ABI plus the YUV and grey ingest formats"):
        assert earlier in v
    assert "lm_set_raw_processing" in lm.EXPORTS and "lm_get_raw_processing" in lm.EXPORTS
    assert C_sizeof(lm) == 4 + 12 + 36 + 4096


def C_sizeof(lm):
    import ctypes
    return ctypes.sizeof(lm.RawProcessing)


LAYOUTS = ("bayer_rggb", "bayer_grbg", "bayer_gbrg", "bayer_bggr", "mono")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_raw_descriptors(lm, layout):
    pat = LAYOUTS.index(layout)
    for bits in (10, 12, 14, 16):
        fmt = 0x1000 | STORAGE[bits, False] | pat
        d = lm.image_desc(Fake((98, 204), "<u2"), layout=layout, bits=bits, crop=(3, 1))
        assert fields(d) == (P, 408, 0, 204, 98, fmt, 3, 1, 1.0)
        d = lm.image_desc(Fake((98, 204), "<u2", (412, 2), ptr=P + 2), layout=layout, bits=bits, matrix="bt709", range="full")
        assert fields(d) == (P + 2, 412, 0, 204, 98, fmt, 0, 0, 1.0)
        for obj, needle in ((Fake((98, 204), "|u1"), "'|u1'"), (Fake((98, 204), "<f4"), "'<f4'"), (Fake((98, 204, 1), "<u2"), "(98, 204, 1)"),
                            (Fake((98, 204), "<u2", (408, 4)), "(408, 4)"), (Fake((98, 204), "<u2", (-408, 2)), "(-408, 2)")):
            with pytest.raises(ValueError) as e:
                lm.image_desc(obj, layout=layout, bits=bits)
            assert needle in str(e.value) and layout in str(e.value), str(e.value)
        with pytest.raises(ValueError) as e:
            lm.image_desc(Fake((98, 204), "<u2"), layout=layout, bits=bits, width=204)
        assert "width" in str(e.value)
    for bits in (10, 12):
        fmt = 0x1000 | STORAGE[bits, True] | pat
        rb = (204 * bits + 7) // 8
        d = lm.image_desc(Fake((98, rb), "|u1"), layout=layout, bits=bits, packed=True, width=204, crop=(3, 1))
        assert fields(d) == (P, rb, 0, 204, 98, fmt, 3, 1, 1.0)
        d = lm.image_desc(Fake((98, rb + 1), "|u1", (rb + 4, 1), ptr=P + 3), layout=layout, bits=bits, packed=True, width=204)
        assert fields(d) == (P + 3, rb + 4, 0, 204, 98, fmt, 0, 0, 1.0)
        d = lm.image_desc(Fake((98, rb + 1), "|u1"), layout=layout, bits=bits, packed=True, width=203)       # (the binding leaves the even rule to the library)
        assert (d.width, d.row_stride) == (203, rb + 1)
        for kw, obj, needle in ((dict(width=204), Fake((98, rb), "<u2"), "'<u2'"), (dict(width=204), Fake((98, rb, 1), "|u1"), "(98, %d, 1)" % rb),
                                (dict(width=204), Fake((98, rb), "|u1", (rb, 2)), "(%d, 2)" % rb), (dict(width=204), Fake((98, rb), "|u1", (-rb, 1)), "(%d, 1)" % -rb),
                                (dict(), Fake((98, rb), "|u1"), "width None"), (dict(width=205), Fake((98, rb), "|u1"), "width 205"),
                                (dict(width=-2), Fake((98, rb), "|u1"), "width -2")):
            with pytest.raises(ValueError) as e:
                lm.image_desc(obj, layout=layout, bits=bits, packed=True, **kw)
            assert needle in str(e.value) and layout in str(e.value), str(e.value)
    # bits that name no storage
    for kw in (dict(bits=9), dict(bits=11), dict(bits=14, packed=True), dict(bits=16, packed=True), dict(bits=8, packed=True), dict(bits=0), dict(bits=32)):
        with pytest.raises(ValueError) as e:
            lm.image_desc(Fake((98, 204), "<u2"), layout=layout, width=204 if kw.get("packed") else None, **kw)
        assert "bits %d" % kw["bits"] in str(e.value), str(e.value)
    # (depth=True describes a depth image, whatever the colour keywords say)
    assert lm.image_desc(Fake((98, 204), "<u2"), depth=True, layout=layout, bits=12).format == lm.PIX_DEPTH_U16


def test_raw_keywords_on_other_layouts_and_bits_8(lm):
    # bits=8 behaves exactly as before: a <u2 object with a Bayer layout still raises, in the earlier words
    for layout in LAYOUTS[:4]:
        with pytest.raises(ValueError) as e:
            lm.image_desc(Fake((98, 204), "<u2"), layout=layout)
        assert "'<u2'" in str(e.value) and "uint8 [H, W] wanted" in str(e.value)
        d = lm.image_desc(Fake((98, 204), "|u1"), layout=layout, bits=8, packed=False, width=None)
        assert d.format == 16 + LAYOUTS.index(layout)
    with pytest.raises(ValueError) as e:
        lm.image_desc(Fake((98, 204), "|u1"), layout="mono")
    assert "bits 8" in str(e.value) and "gray" in str(e.value)
    for layout, obj in (("hwc", Fake((98, 204, 3), "|u1")), ("gray", Fake((98, 204), "|u1")), ("nv12", Fake((147, 204), "|u1")), ("chw", Fake((3, 98, 204), "|u1"))):
        for kw in (dict(bits=12), dict(bits=10, packed=True, width=204)):
            with pytest.raises(ValueError) as e:
                lm.image_desc(obj, layout=layout, **kw)
            assert "bits" in str(e.value) and layout in str(e.value)
        with pytest.raises(ValueError) as e:
            lm.image_desc(obj, layout=layout, width=204)
        assert "width" in str(e.value)
        assert lm.image_desc(obj, layout=layout).width == 204
    with pytest.raises(ValueError) as e:
        lm.image_desc(Fake((98, 204), "<u2"), layout="mono16", bits=16)
    assert "'mono16'" in str(e.value)


def hard_settings():
    rng = np.random.default_rng(17)
    return dict(black=37, gains=(3.5, 0.70019, 63.999), ccm=[[1.7, -0.45, -0.25], [-0.3, 1.6, -0.3], [-8.0, 8.0, 0.001]], tone=rng.integers(0, 256, 4096).astype(np.uint8))


def test_set_raw_processing_round_trip_and_refusals(lm):
    """Host state: the setter and the getter need no device.  Floats go to Q10 with numpy.rint; a refusal leaves the previous setting."""
    d = lm.Detector(color_only=True, width=48, height=32)
    ident = d.raw_processing()
    assert ident["black"] == 0 and ident["gain"].tolist() == [1024] * 3 and ident["ccm"].tolist() == (1024 * np.eye(3, dtype=int)).tolist()
    assert np.array_equal(ident["tone"], np.arange(4096) >> 4) and ident["tone"].dtype == np.uint8
    h = hard_settings()
    d.set_raw_processing(**h)
    got = d.raw_processing()
    assert got["black"] == 37 and got["gain"].tolist() == [3584, 717, 65535]
    assert got["ccm"].tolist() == np.rint(np.array(h["ccm"]) * 1024).astype(int).tolist() and got["ccm"][2].tolist() == [-8192, 8192, 1]
    assert np.array_equal(got["tone"], h["tone"])
    # rint: ties to even
    d.set_raw_processing(gains=(1.00048828125, 1.00146484375, 1.0), ccm=np.eye(3) * 0.99951171875)
    got = d.raw_processing()
    assert got["gain"].tolist() == [1024, 1026, 1024] and got["ccm"][0, 0] == 1024 and got["black"] == 0 and np.array_equal(got["tone"], np.arange(4096) >> 4)
    d.set_raw_processing(**h)
    lib = d.lib

    def refused(words, **edit):
        kw = dict(h)
        kw.update(edit)
        with pytest.raises(lm.LinemodError) as e:
            d.set_raw_processing(**kw)
        assert e.value.code == INVALID and str(e.value).endswith(": " + words), str(e.value)
        assert lib.lm_last_error().decode() == words
        now = d.raw_processing()
        assert now["black"] == 37 and now["gain"].tolist() == [3584, 717, 65535] and np.array_equal(now["tone"], h["tone"])

    refused("raw processing: black -1 lies outside 0 .. 65535", black=-1)
    refused("raw processing: black 65536 lies outside 0 .. 65535", black=65536)
    refused("raw processing: gain 65536 lies above 65535", gains=(1.0, 64.0, 1.0))
    refused("raw processing: gain 102400 lies above 65535", gains=(1.0, 1.0, 100.0))
    refused("raw processing: matrix entry 8193 lies outside -8192 .. 8192", ccm=[[1, 0, 0], [0, 8193 / 1024.0, 0], [0, 0, 1]])
    refused("raw processing: matrix entry -8193 lies outside -8192 .. 8192", ccm=[[1, 0, 0], [0, 1, 0], [-8193 / 1024.0, 0, 1]])
    refused("raw processing: black -1 lies outside 0 .. 65535", black=-1, gains=(100.0, 1.0, 1.0))      # (the first that fails wins)
    # the extremes themselves are taken
    d.set_raw_processing(black=65535, gains=(0.0, 63.9990234375, 1.0), ccm=[[8.0, -8.0, 0], [0, 1, 0], [0, 0, 1]])
    got = d.raw_processing()
    assert got["black"] == 65535 and got["gain"].tolist() == [0, 65535, 1024] and got["ccm"][0].tolist() == [8192, -8192, 0]
    # what the binding itself refuses
    for kw in (dict(gains=(1, 1)), dict(ccm=np.eye(4)), dict(tone=np.zeros(256, np.uint8)), dict(tone=np.full(4096, 256)), dict(tone=np.zeros(4096, np.float32)),
               dict(gains=(-1.0, 1, 1)), dict(gains=(float("nan"), 1, 1)), dict(ccm=np.full((3, 3), float("inf")))):
        with pytest.raises(ValueError):
            d.set_raw_processing(**kw)
    assert d.raw_processing()["black"] == 65535
    # NULL resets to the identity
    d.set_raw_processing(None)
    back = d.raw_processing()
    assert back["black"] == 0 and back["gain"].tolist() == [1024] * 3 and np.array_equal(back["tone"], ident["tone"]) and np.array_equal(back["ccm"], ident["ccm"])
    assert lib.lm_set_raw_processing(None, None) == INVALID and lib.lm_last_error() == b"null detector"
    assert lib.lm_get_raw_processing(d.h, None) == INVALID and lib.lm_last_error() == b"bad argument"
    d.close()


def test_tone_curve(lm):
    t = lm.tone_curve(2.2)
    assert t.dtype == np.uint8 and t.shape == (4096,) and t[0] == 0 and t[-1] == 255 and (np.diff(t.astype(int)) >= 0).all()
    assert t[2048] == int(np.rint(255 * (2048 / 4095) ** (1 / 2.2)))
    assert np.abs(lm.tone_curve(1.0).astype(int) - (np.arange(4096) >> 4)).max() <= 1
    for bad in (0, -1.0):
        with pytest.raises(ValueError):
            lm.tone_curve(bad)


def test_raw_ingest_fails_loudly_without_gpu(lm):
    if _has_gpu(lm):
        pytest.skip("a HIP device is present")
    d = lm.Detector(color_only=False, width=160, height=80)
    d.set_raw_processing(**hard_settings())
    dep = Fake((98, 204), "<u2")
    for kw, obj in ((dict(layout="bayer_rggb", bits=12), Fake((98, 204), "<u2")), (dict(layout="mono", bits=10, packed=True, width=204), Fake((98, 255), "|u1")),
                    (dict(layout="bayer_bggr"), Fake((98, 204), "|u1"))):
        with pytest.raises(lm.LinemodError) as e:
            d.ingest_frame(0, obj, dep, **kw)
        assert e.value.code == lm.LM_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
        with pytest.raises(lm.LinemodError) as e:
            d.ingest_frames(0, [dict(colour=obj, depth=dep, **kw)])
        assert e.value.code == lm.LM_ERR_NO_DEVICE
    d.close()


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_ingest_raw_host_program(tmp_path, flags):
    """The kernel's per-lane code, the rectify taps and the descriptor check on the host: every load aligned and inside `safe` or on a
    needed byte, every tap load inside the source, every pixel the rule's, every refusal its words."""
    exe = str(tmp_path / "ingest_raw_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "ingest_raw_host.cpp"), os.path.join(CSRC, "lm_ingest_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    # the lane cases alone: 11 (source, window) pairs x (3 packed / byte storages x 4 offsets + 4 containers x 2 offsets) x 2 paddings x 4
    # patterns x 2 mirrors x 3 shifts, at least one crop, one lane and 16 pixels each
    assert r.stdout.split()[4:6] == ["lane", "pixels,"] and int(r.stdout.split()[3]) >=11 * (3 * 4 + 4 * 2) * 2 * 4 * 2 * 3 * 16
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
