"""CPU tests of the raw Bayer ingest formats (ABI 0.13 additive, DESIGN.md section 13 "Bayer sources"): the reference the GPU tests compare
with (tests/ingest_bayer_reference.py) against the header's hand-computed table, against a per-pixel loop with explicit reflected
indices and against three properties of a bilinear demosaic; the constants, the version string, what the binding makes of a
__cuda_array_interface__, the refusal to run without a device, and tests/cpp/ingest_bayer_host.cpp: csrc/lm_ingest_bayer.h -- the
kernel's per-lane code --, the rectify taps and the descriptor check on the host under ASan / UBSan."""
import os
import subprocess

import numpy as np
import pytest

import ingest_bayer_reference as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
P = 0x7F0012345600


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


# include/linemod_hip.h: source [[1, 2], [3, 4]], the output pixels in reading order as (B, G, R)
TABLE = {"rggb": [(4, 3, 1), (4, 2, 1), (4, 3, 1), (4, 3, 1)], "grbg": [(3, 1, 2), (3, 3, 2), (3, 3, 2), (3, 4, 2)],
         "gbrg": [(2, 1, 3), (2, 3, 3), (2, 3, 3), (2, 4, 3)], "bggr": [(1, 3, 4), (1, 2, 4), (1, 3, 4), (1, 3, 4)]}


@pytest.mark.parametrize("pattern", BR.PATTERNS)
def test_the_pinned_2x2_table(pattern):
    out = BR.demosaic(np.array([[1, 2], [3, 4]], np.uint8), pattern)
    assert [tuple(px) for px in out.reshape(4, 3).tolist()] == TABLE[pattern]


def loop_demosaic(raw, pattern):
    """The rule once more, one pixel at a time, with the reflected indices written out."""
    H, W = raw.shape
    red_x, red_y = {"rggb": (0, 0), "grbg": (1, 0), "gbrg": (0, 1), "bggr": (1, 1)}[pattern]

    def S(x, y):
        x = 1 if x == -1 else W - 2 if x == W else x
        y = 1 if y == -1 else H - 2 if y == H else y
        assert 0 <= x < W and 0 <= y < H
        return int(raw[y, x])

    out = np.zeros((H, W, 3), np.uint8)
    for y in range(H):
        for x in range(W):
            c = S(x, y)
            h = (S(x - 1, y) + S(x + 1, y) + 1) >> 1
            v = (S(x, y - 1) + S(x, y + 1) + 1) >> 1
            p = (S(x - 1, y) + S(x + 1, y) + S(x, y - 1) + S(x, y + 1) + 2) >> 2
            d = (S(x - 1, y - 1) + S(x + 1, y - 1) + S(x - 1, y + 1) + S(x + 1, y + 1) + 2) >> 2
            site = ((x ^ red_x) & 1, (y ^ red_y) & 1)
            R, G, B = {(0, 0): (c, p, d), (1, 1): (d, p, c), (1, 0): (h, c, v), (0, 1): (v, c, h)}[site]
            out[y, x] = (B, G, R)
    return out


def test_reference_against_a_per_pixel_loop():
    """Every even size from 2 x 2 to 6 x 8 (rows x columns), all four patterns: at the tiny sizes both reflections land on one column or row."""
    rng = np.random.default_rng(7)
    n = 0
    for H in (2, 4, 6):
        for W in (2, 4, 6, 8):
            raw = rng.integers(0, 256, (H, W), dtype=np.uint8)
            raw[rng.random((H, W)) < 0.3] = rng.choice(np.array([0, 1, 254, 255], np.uint8))
            for pattern in BR.PATTERNS:
                assert np.array_equal(BR.demosaic(raw, pattern), loop_demosaic(raw, pattern)), (H, W, pattern)
                n += 1
    assert n == 48


@pytest.mark.parametrize("pattern", BR.PATTERNS)
def test_properties_of_the_rule(pattern):
    """A constant-colour scene comes back exactly; an integer affine ramp per channel comes back exactly except on the outermost ring (the
    reflection); the source samples survive."""
    H, W = 10, 14
    const = np.empty((H, W, 3), np.uint8)
    const[...] = (17, 200, 93)
    assert np.array_equal(BR.demosaic(BR.mosaic(const, pattern), pattern), const)
    y, x = np.mgrid[0:H, 0:W]
    ramp = np.stack([10 + 3 * x + 5 * y, 200 - 2 * x - 4 * y, 40 + 7 * x + y], axis=-1)
    assert ramp.min() >= 0 and ramp.max() <= 255
    ramp = ramp.astype(np.uint8)
    back = BR.demosaic(BR.mosaic(ramp, pattern), pattern)
    assert np.array_equal(back[1:-1, 1:-1], ramp[1:-1, 1:-1])
    assert not np.array_equal(back, ramp)           # (the ring is where the reflection shows)
    raw = np.random.default_rng(11).integers(0, 256, (H, W), dtype=np.uint8)
    assert np.array_equal(BR.mosaic(BR.demosaic(raw, pattern), pattern), raw)


def test_mosaic_keeps_the_named_tile():
    bgr = np.zeros((2, 2, 3), np.uint8)
    bgr[...] = (1, 2, 3)            # B, G, R
    tiles = {"rggb": [[3, 2], [2, 1]], "grbg": [[2, 3], [1, 2]], "gbrg": [[2, 1], [3, 2]], "bggr": [[1, 2], [2, 3]]}
    for pattern in BR.PATTERNS:
        assert BR.mosaic(bgr, pattern).tolist() == tiles[pattern]
        assert BR.red_site(pattern) == ({"rggb": 0, "grbg": 1, "gbrg": 2, "bggr": 3}[pattern] & 1, {"rggb": 0, "grbg": 1, "gbrg": 2, "bggr": 3}[pattern] >> 1)


def test_constants_and_version(lm):
    assert (lm.PIX_BAYER_RGGB8, lm.PIX_BAYER_GRBG8, lm.PIX_BAYER_GBRG8, lm.PIX_BAYER_BGGR8) == (16, 17, 18, 19)
    assert 13 not in {v for k, v in vars(lm).items() if k.startswith("PIX_")}        # 13 names nothing, as the existing refusal tests pin
    v = lm.load_library().lm_version()
    assert v.startswith(b"linemod_hip 0.13 ") and b"0.13 additive: raw Bayer ingest formats" in v
    for earlier in (b"0.13 = the 0.12 ABI plus the depth registration", b"lm_ingest_frames_rectified", b"0.12 = the 0.11 ABI plus the YUV and grey ingest formats"):
        assert earlier in v


@pytest.mark.parametrize("layout,fmt", [("bayer_rggb", 16), ("bayer_grbg", 17), ("bayer_gbrg", 18), ("bayer_bggr", 19)])
def test_bayer_descriptors(lm, layout, fmt):
    d = lm.image_desc(Fake((98, 204), "|u1"), layout=layout, crop=(3, 1))
    assert fields(d) == (P, 204, 0, 204, 98, fmt, 3, 1, 1.0)
    d = lm.image_desc(Fake((98, 204), "|u1", (207, 1), ptr=P + 3), layout=layout, matrix="bt709", range="full")       # (the YUV keywords play no part)
    assert fields(d) == (P + 3, 207, 0, 204, 98, fmt, 0, 0, 1.0)
    for obj, needle in ((Fake((98, 204, 1), "|u1"), "(98, 204, 1)"), (Fake((98, 204), "<u2"), "'<u2'"), (Fake((98, 204), "|u1", (408, 2)), "(408, 2)"),
                        (Fake((98, 204), "|u1", (-204, 1)), "(-204, 1)"), (Fake((3, 98, 204), "|u1"), "(3, 98, 204)")):
        with pytest.raises(ValueError) as e:
            lm.image_desc(obj, layout=layout)
        assert needle in str(e.value) and layout in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:
        lm.image_desc(Fake((98, 204), "|u1"), layout="bayer")
    assert "'bayer'" in str(e.value)
    with pytest.raises(ValueError) as e:
        lm.image_desc(Fake((98, 204), "|u1"), depth=True, layout=layout)
    assert "depth image" in str(e.value)


def test_bayer_ingest_fails_loudly_without_gpu(lm):
    if _has_gpu(lm):
        pytest.skip("a HIP device is present")
    d = lm.Detector(color_only=False, width=160, height=80)
    dep = Fake((98, 204), "<u2")
    for layout in ("bayer_rggb", "bayer_bggr"):
        with pytest.raises(lm.LinemodError) as e:
            d.ingest_frame(0, Fake((98, 204), "|u1"), dep, layout=layout)
        assert e.value.code == lm.LM_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
        with pytest.raises(lm.LinemodError) as e:
            d.ingest_frames(0, [dict(colour=Fake((98, 204), "|u1"), depth=dep, layout=layout)])
        assert e.value.code == lm.LM_ERR_NO_DEVICE
    d.close()


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_ingest_bayer_host_program(tmp_path, flags):
    """The kernel's per-lane code, the rectify taps and the descriptor check on the host: every load aligned and inside `safe` or on a
    needed byte, every tap load inside the source, every pixel the rule's, every refusal its words."""
    exe = str(tmp_path / "ingest_bayer_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "ingest_bayer_host.cpp"), os.path.join(CSRC, "lm_ingest_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    # the lane cases alone: 11 (source, window) pairs x 4 offsets x 2 paddings x 4 patterns x 2 mirrors x 3 shifts, at least one crop, one
    # lane and 16 pixels each
    assert int(r.stdout.split()[1]) >= 11 * 4 * 2 * 4 * 2 * 3 * 16
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
