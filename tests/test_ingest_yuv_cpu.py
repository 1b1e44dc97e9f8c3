"""CPU tests of the grey and YUV ingest formats (ABI 0.12): the integer conversion rule of the reference the GPU tests
compare with (tests/ingest_yuv_reference.py) against a float64 matrix conversion over all 2^24 (Y, U, V) triples, its packers and its
chroma replication, what the binding makes of a __cuda_array_interface__ for every new layout, the version string, the refusal to run
without a device, and tests/cpp/ingest_yuv_host.cpp: csrc/lm_ingest_yuv.h -- the kernel's per-lane code -- on the host under ASan / UBSan."""
import os
import subprocess

import numpy as np
import pytest

import ingest_yuv_reference as YR

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


# Kr, Kb of the two matrices
LUMA = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def float_conversion(Y, U, V, matrix, rng):
    """[..., 3] float64 B, G, R, unrounded, clamped to [0, 255]: the standard matrix with its exact coefficients.  Limited range: luma
    scaled by 255 / 219 from 16, chroma by 255 / 224; full range: neither.  Luma below the black level counts as black, as in the rule
    (and in OpenCV): max(0, Y - Y0) is part of the definition, not of the arithmetic under test."""
    kr, kb = LUMA[matrix]
    kg = 1.0 - kr - kb
    y0, sy, sc = (16.0, 255.0 / 219.0, 255.0 / 224.0) if rng == "limited" else (0.0, 1.0, 1.0)
    y = np.maximum(0.0, Y - y0) * sy
    u, v = (U - 128.0) * sc, (V - 128.0) * sc
    r = y + 2.0 * (1.0 - kr) * v
    b = y + 2.0 * (1.0 - kb) * u
    g = y - (2.0 * kr * (1.0 - kr) / kg) * v - (2.0 * kb * (1.0 - kb) / kg) * u
    return np.clip(np.stack([b, g, r], axis=-1), 0.0, 255.0)


@pytest.mark.parametrize("flags", YR.FLAGS, ids=["%s_%s" % f for f in YR.FLAGS])
def test_rule_against_float64_over_all_triples(flags):
    """Every channel of every one of the 2^24 triples lies within 1 of the float64 conversion; no intermediate of the rule leaves 32 signed
    bits and every product has operands of at most 24 signed bits (v_mad_i32_i24)."""
    Y0, CY, CVR, CVG, CUG, CUB = YR.COEF[flags]
    assert all(abs(c) < (1 << 23) for c in (CY, CVR, CVG, CUG, CUB))
    U, V = (a.astype(np.float64) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    worst = 0.0
    for Y in range(256):
        got = YR.convert(np.full(U.shape, Y), U, V, flags).astype(np.float64)
        worst = max(worst, float(np.abs(got - float_conversion(float(Y), U, V, *flags)).max()))
    print("largest distance from the float64 conversion, %s %s: %.4f" % (flags + (worst,)))
    assert worst <= 1.0
    y = max(0, 255 - Y0) * CY
    extremes = [y + (1 << 19) + a * v + b * u for v in (-128, 127) for u in (-128, 127) for a, b in ((CVR, 0), (CVG, CUG), (0, CUB))]
    extremes += [(1 << 19) + a * v + b * u for v in (-128, 127) for u in (-128, 127) for a, b in ((CVR, 0), (CVG, CUG), (0, CUB))]
    assert max(abs(e) for e in extremes) < (1 << 31)
    assert max(abs(e) for e in extremes) <= 574_000_000      # (5.74e8 is the largest over the four tables)


def test_the_tables_spelled_out():
    """OpenCV's ITUR_BT_601_* constants at shift 20 (1.164, 1.596, 0.813, 0.391, 2.018 times 2^20, rounded), as recalled -- not pinned
    against an OpenCV build --, and the three other rows as round(coefficient * 2^20) of the standard matrices."""
    assert YR.COEF["bt601", "limited"] == (16, 1220542, 1673527, -852492, -409993, 2116026)
    assert YR.COEF["bt601", "limited"][1:] == tuple(int(np.floor(c * (1 << 20) + 0.5)) for c in (1.164, 1.596, -0.813, -0.391, 2.018))
    assert YR.COEF["bt709", "limited"] == (16, 1220945, 1879825, -558796, -223607, 2215014)
    assert YR.COEF["bt601", "full"] == (0, 1048576, 1470104, -748826, -360853, 1858077)
    assert YR.COEF["bt709", "full"] == (0, 1048576, 1651297, -490864, -196424, 1945738)
    for (matrix, rng), row in YR.COEF.items():
        if (matrix, rng) == ("bt601", "limited"):
            continue
        kr, kb = LUMA[matrix]
        kg = 1.0 - kr - kb
        sy, sc = (255.0 / 219.0, 255.0 / 224.0) if rng == "limited" else (1.0, 1.0)
        exact = (sy, 2 * (1 - kr) * sc, -2 * kr * (1 - kr) / kg * sc, -2 * kb * (1 - kb) / kg * sc, 2 * (1 - kb) * sc)
        assert row[1:] == tuple(int(np.floor(c * (1 << 20) + 0.5)) for c in exact), (matrix, rng)
    # one pixel by hand: Y 16, U 128, V 0 -> R = sat8((2^19 - 1673527 * 128) >> 20) = 0, G = (2^19 + 852492 * 128) >> 20 = 104, B = 0
    assert YR.convert([16], [128], [0], ("bt601", "limited"))[0].tolist() == [0, 104, 0]


def test_packers_and_chroma_replication():
    """planes() undoes the packers and replicates: pixel (x, y) takes the sample of pair x >> 1 (4:2:0: and row y >> 1)."""
    rng = np.random.default_rng(3)
    H, W = 6, 8
    Y = rng.integers(0, 256, (H, W), dtype=np.uint8)
    for fmt in ("nv12", "nv21"):
        U, V = rng.integers(0, 256, (2, H // 2, W // 2), dtype=np.uint8)
        y, uv = YR.pack_nv(Y, U, V, fmt)
        assert uv.shape == (H // 2, W) and (uv[1, 2], uv[1, 3]) == ((U[1, 1], V[1, 1]) if fmt == "nv12" else (V[1, 1], U[1, 1]))
        py, pu, pv = YR.planes((y, uv), fmt)
        assert np.array_equal(py, Y)
        for yy in range(H):
            for xx in range(W):
                assert pu[yy, xx] == U[yy >> 1, xx >> 1] and pv[yy, xx] == V[yy >> 1, xx >> 1]
    for fmt in ("yuy2", "uyvy"):
        U, V = rng.integers(0, 256, (2, H, W // 2), dtype=np.uint8)
        m = YR.pack_422(Y, U, V, fmt)
        assert m.shape == (H, W, 2)
        quad = m.reshape(H, W * 2)[2, 4:8].tolist()
        assert quad == ([Y[2, 2], U[2, 1], Y[2, 3], V[2, 1]] if fmt == "yuy2" else [U[2, 1], Y[2, 2], V[2, 1], Y[2, 3]])
        py, pu, pv = YR.planes(m, fmt)
        assert np.array_equal(py, Y)
        for xx in range(W):
            assert np.array_equal(pu[:, xx], U[:, xx >> 1]) and np.array_equal(pv[:, xx], V[:, xx >> 1])
    g = rng.integers(0, 256, (H, W), dtype=np.uint8)
    assert np.array_equal(YR.yuv_to_bgr(g, "gray"), np.stack([g, g, g], axis=-1))
    # neutral chroma: a grey ramp, full range is the identity
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    out = YR.convert(ramp, np.full_like(ramp, 128), np.full_like(ramp, 128), ("bt709", "full"))
    assert np.array_equal(out, np.stack([ramp] * 3, axis=-1))


def test_constants_and_version(lm):
    assert (lm.PIX_GRAY8, lm.PIX_NV12, lm.PIX_NV21, lm.PIX_YUY2, lm.PIX_UYVY) == (8, 9, 10, 11, 12)
    assert (lm.PIX_YUV_BT709, lm.PIX_YUV_FULL) == (0x100, 0x200)
    v = lm.load_library().lm_version()
    assert b"0.12 = the 0.11 ABI plus the YUV and grey ingest formats" in v
    for earlier in (b"0.11", b"0.10", b"0.9", b"0.8", b"0.7", b"0.6", b"0.5", b"0.4", b"gfx950", b"lm_ingest_", b"lm_add_templates_slots"):
        assert earlier in v


def test_gray_descriptor(lm):
    d = lm.image_desc(Fake((98, 204), "|u1"), layout="gray", crop=(3, 1))
    assert fields(d) == (P, 204, 0, 204, 98, lm.PIX_GRAY8, 3, 1, 1.0)
    d = lm.image_desc(Fake((98, 204), "|u1", (207, 1), ptr=P + 3), layout="gray")
    assert fields(d) == (P + 3, 207, 0, 204, 98, lm.PIX_GRAY8, 0, 0, 1.0)
    for obj, needle in ((Fake((98, 204, 1), "|u1"), "(98, 204, 1)"), (Fake((98, 204), "<u2"), "'<u2'"), (Fake((98, 204), "|u1", (408, 2)), "(408, 2)")):
        with pytest.raises(ValueError) as e:
            lm.image_desc(obj, layout="gray")
        assert needle in str(e.value), str(e.value)


@pytest.mark.parametrize("layout,fmt", [("nv12", "PIX_NV12"), ("nv21", "PIX_NV21")])
def test_nv_descriptors(lm, layout, fmt):
    F = getattr(lm, fmt)
    # one object: the chroma rows behind the Y rows
    d = lm.image_desc(Fake((147, 204), "|u1"), layout=layout, crop=(5, 3))
    assert fields(d) == (P, 204, 98 * 204, 204, 98, F, 5, 3, 1.0)
    d = lm.image_desc(Fake((147, 204), "|u1", (207, 1), ptr=P + 1), layout=layout, matrix="bt709", range="full")
    assert fields(d) == (P + 1, 207, 98 * 207, 204, 98, F | 0x300, 0, 0, 1.0)
    assert lm.image_desc(Fake((147, 204), "|u1"), layout=layout, matrix="bt709").format == F | 0x100
    assert lm.image_desc(Fake((147, 204), "|u1"), layout=layout, range="full").format == F | 0x200
    # a pair: a decoder's two pointers and one pitch, the chroma plane as [H / 2, W / 2, 2] or as [H / 2, W]
    y = Fake((98, 204), "|u1", (256, 1))
    for uv in (Fake((49, 102, 2), "|u1", (256, 2, 1), ptr=P + 98 * 256 + 77), Fake((49, 204), "|u1", (256, 1), ptr=P + 98 * 256 + 77)):
        d = lm.image_desc((y, uv), layout=layout)
        assert fields(d) == (P, 256, 98 * 256 + 77, 204, 98, F, 0, 0, 1.0)
    bad = [((Fake((148, 204), "|u1"),), "(148, 204)"),                                                          # rows no multiple of 3
           ((Fake((147, 204, 1), "|u1"),), "(147, 204, 1)"),
           (((y, Fake((49, 102, 2), "|u1", (512, 2, 1), ptr=P + 98 * 256)),), "(512, 2, 1)"),                    # another row stride
           (((y, Fake((49, 102, 2), "|u1", (256, 2, 1), ptr=P - 49 * 256)),), hex(P - 49 * 256)),                # below the Y plane
           (((y, Fake((48, 102, 2), "|u1", (256, 2, 1), ptr=P + 98 * 256)),), "(48, 102, 2)"),                   # not H / 2 rows
           (((y, Fake((49, 102, 2), "<u2", None, ptr=P + 98 * 256)),), "'<u2'"),
           (((Fake((97, 204), "|u1", (256, 1)), Fake((48, 102, 2), "|u1", (256, 2, 1), ptr=P + 98 * 256)),), "(97, 204)"),   # odd height
           (((y, y, y),), "3 objects")]
    for args, needle in bad:
        with pytest.raises(ValueError) as e:
            lm.image_desc(*args, layout=layout)
        assert needle in str(e.value), str(e.value)
    for kw, needle in ((dict(matrix="bt2020"), "'bt2020'"), (dict(range="video"), "'video'")):
        with pytest.raises(ValueError) as e:
            lm.image_desc(Fake((147, 204), "|u1"), layout=layout, **kw)
        assert needle in str(e.value), str(e.value)


@pytest.mark.parametrize("layout,fmt", [("yuy2", "PIX_YUY2"), ("uyvy", "PIX_UYVY")])
def test_packed_422_descriptors(lm, layout, fmt):
    F = getattr(lm, fmt)
    d = lm.image_desc(Fake((98, 204, 2), "|u1"), layout=layout, crop=(1, 1))
    assert fields(d) == (P, 408, 0, 204, 98, F, 1, 1, 1.0)
    d = lm.image_desc(Fake((98, 204, 2), "|u1", (411, 2, 1), ptr=P + 2), layout=layout, matrix="bt709")
    assert fields(d) == (P + 2, 411, 0, 204, 98, F | 0x100, 0, 0, 1.0)
    for obj, needle in ((Fake((98, 204, 3), "|u1"), "(98, 204, 3)"), (Fake((98, 408), "|u1"), "(98, 408)"),
                        (Fake((98, 204, 2), "|u1", (816, 4, 1)), "(816, 4, 1)"), (Fake((98, 204, 2), "<u2"), "'<u2'")):
        with pytest.raises(ValueError) as e:
            lm.image_desc(obj, layout=layout)
        assert needle in str(e.value), str(e.value)


def test_the_existing_layouts_keep_their_descriptors(lm):
    d = lm.image_desc(Fake((97, 203, 3), "|u1"), order="rgb", crop=(3, 17), matrix="bt709", range="full")       # (the YUV keywords play no part)
    assert fields(d) == (P, 609, 0, 203, 97, lm.PIX_RGB8, 3, 17, 1.0)
    with pytest.raises(ValueError) as e:
        lm.image_desc(Fake((97, 203, 3), "|u1"), layout="i420")
    assert "'i420'" in str(e.value)


def test_yuv_ingest_fails_loudly_without_gpu(lm):
    if _has_gpu(lm):
        pytest.skip("a HIP device is present")
    d = lm.Detector(color_only=False, width=160, height=80)
    dep = Fake((98, 204), "<u2")
    for colour, kw in ((Fake((147, 204), "|u1"), dict(layout="nv12", matrix="bt709")), (Fake((98, 204, 2), "|u1"), dict(layout="uyvy", range="full")),
                       (Fake((98, 204), "|u1"), dict(layout="gray"))):
        with pytest.raises(lm.LinemodError) as e:
            d.ingest_frame(0, colour, dep, **kw)
        assert e.value.code == lm.LM_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
        with pytest.raises(lm.LinemodError) as e:
            d.ingest_frames(0, [dict(colour=colour, depth=dep, **kw)])
        assert e.value.code == lm.LM_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        d.ingest_frame(0, Fake((147, 204), "|u1"), dep, layout="nv12", matrix="bt2020")
    d.close()


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_ingest_yuv_host_program(tmp_path, flags):
    """The kernel's per-lane code on the host: every load aligned and inside `safe` or on a needed byte, every pixel the rule's."""
    exe = str(tmp_path / "ingest_yuv_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "ingest_yuv_host.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    # 5 formats x (4 offsets x 6 x 4 crops x 2 x 5 + 5 x 3 x 2 x 3 aligned) frames x 12 lanes x 16 pixels are the least it checks
    assert int(r.stdout.split()[1]) >= 5 * (4 * 6 * 4 * 2 * 5 + 5 * 3 * 2 * 3) * 12 * 16
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
