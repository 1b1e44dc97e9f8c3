"""CPU tests of the lens rectification (ABI 0.13 additive): csrc/lm_rectify.h -- the map builder and the per-pixel
functions k_rectify calls -- as a stand-alone host program (tests/cpp/rectify_host.cpp, g++ -ffp-contract=off, plain and under ASan /
UBSan) against the independent numpy reference tests/rectify_reference.py; the map through the library; lm_set_rectification's refusals,
which need no device; struct sizes, the version string, the refusal to run without a device, and the facade's readSettings /
rectificationOf."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rectify_reference as QR
import rectify_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SETTINGS = os.path.join(ROOT, "tests", "golden", "reference_data", "linemod_settings.yml")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
F = np.float32
KIND = {"bgr": 0, "rgb": 0, "bgra": 1, "rgba": 1, "bgr_planar": 2, "rgb_planar": 2, "u16": 3, "f32": 4, "gray": 5, "nv12": 6, "nv21": 7, "yuy2": 8, "uyvy": 9}
MATRIX = {("bt601", "limited"): 0, ("bt709", "limited"): 1, ("bt601", "full"): 2, ("bt709", "full"): 3}


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def host_program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rectify_host") / "rectify_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + request.param +
                          ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "rectify_host.cpp")])
    return exe


def run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return int(r.stdout.split()[1])


def host_map(exe, tmp_path, source, ideal):
    fout = str(tmp_path / "map.bin")
    # the library holds the cameras as floats: the program gets the doubles those floats are
    nums = [repr(float(F(v))) for v in (source["fx"], source["fy"], source["cx"], source["cy"]) + tuple(source["dist"]) +
            (ideal["fx"], ideal["fy"], ideal["cx"], ideal["cy"])]
    n = run(exe, ["map", fout, source["width"], source["height"], ideal["width"], ideal["height"]] + nums)
    assert n == 2 * ideal["width"] * ideal["height"]
    return np.fromfile(fout, np.int32).reshape(ideal["height"], ideal["width"], 2)


def settings_camera(lm):
    k = lm.yaml_numbers(SETTINGS, "distortion parameters")
    assert len(k) == 5 and k[1] != 0
    return QR.cam(640, 480, 1044.87, 1045.69141, 320.0, 240.0, tuple(float(v) for v in k))


def map_cases(lm):
    """(name, source camera, ideal camera)"""
    plain = S.source_cam(S.ZERO)
    return [("identity", plain, QR.pinhole_of(plain)),
            ("rescale", plain, S.ideal_cam(176, 96)),
            ("settings", settings_camera(lm), QR.pinhole_of(settings_camera(lm))),
            ("barrel", S.source_cam((-0.3, 0.0, 0.01, -0.02, 0.0)), QR.cam(S.SW, S.SH, 30.0, 30.0, 103.5, 59.5)),
            ("pincushion", S.source_cam((0.3, 0.05, -0.02, 0.01, 0.01)), QR.cam(S.SW, S.SH, 60.0, 60.0, 103.5, 59.5)),
            ("overflow", S.source_cam((0.3, 1e38, 0.0, 0.0, 1e38)), QR.cam(S.SW, S.SH, 1e-38, 1e-38, 103.5, 59.5))]


def check_map_properties(name, m, source):
    w, h = source["width"], source["height"]
    if name == "identity":
        i, j = np.meshgrid(np.arange(w), np.arange(h))
        assert np.array_equal(m[:, :, 0], 32 * i) and np.array_equal(m[:, :, 1], 32 * j), "the identity map is not (32 i, 32 j)"
    if name in ("barrel", "pincushion"):
        # both clamps of both coordinates are hit: a sweep that never reaches them pins nothing
        assert (m[:, :, 0] == -64).any() and (m[:, :, 0] == 32 * w + 32).any() and (m[:, :, 1] == -64).any() and (m[:, :, 1] == 32 * h + 32).any()
        assert ((m[:, :, 0] > 0) & (m[:, :, 0] < 32 * w) & (m[:, :, 1] > 0) & (m[:, :, 1] < 32 * h)).sum() > 1000
    if name == "settings":
        i, j = np.meshgrid(np.arange(w), np.arange(h))
        shift = np.hypot(m[:, :, 0] / 32.0 - i, m[:, :, 1] / 32.0 - j)
        print("the reference's lens moves the corner pixel by %.2f pixels" % shift[0, 0])
        assert shift[0, 0] > 2.0 and shift[h // 2, w // 2] < 0.1


def test_build_map_equals_reference(lm, host_program, tmp_path):
    not_finite = False
    for name, source, ideal in map_cases(lm):
        ref = QR.build_map(source, ideal)
        got = host_map(host_program, tmp_path, source, ideal)
        assert np.array_equal(got, ref), "%s: %d entries differ" % (name, int((got != ref).sum()))
        check_map_properties(name, ref, source)
        if name == "overflow":
            sx, sy = QR.source_coordinates(source, ideal)
            not_finite = bool((~np.isfinite(sx)).any())
            assert (ref[:, :, 0][~np.isfinite(sx)] == -64).all()
    assert not_finite, "no case reached a coordinate that is not finite"


def test_map_through_the_library(lm):
    """lm_set_rectification builds the map on the host (no device) and lm_get_rectification_map returns it: equal to the reference on
    every camera pair, on a caller's table, and gone after clearing."""
    d = lm.Detector(color_only=False, width=S.W, height=S.H)
    for name, source, ideal in map_cases(lm):
        to = lambda c: lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])
        d.set_rectification(to(source), to(ideal))
        got = d.rectification_map()
        assert got.dtype == np.int32 and got.shape == (ideal["height"], ideal["width"], 2)
        assert np.array_equal(got, QR.build_map(source, ideal)), name
    source = S.source_cam()
    d.set_rectification(lm.camera(S.SW, S.SH, 130.0, 131.0, 103.5, 59.5, S.LENS))          # ideal=None: the source's pinhole
    assert np.array_equal(d.rectification_map(), QR.build_map(source, QR.pinhole_of(source)))
    table = S.smooth_table(67, 45)
    d.set_rectification(lm.camera(S.SW, S.SH, 130.0, 131.0, 103.5, 59.5, S.LENS), lm.camera(67, 45, 50.0, 50.0, 33.0, 22.0), map=table)
    ref = QR.quant_table(table, source)
    assert np.array_equal(d.rectification_map(), ref)
    assert (ref == -64).any() and (ref[:, :, 0] == 32 * S.SW + 32).any() and (ref[:, :, 1] == 32 * S.SH + 32).any()
    with pytest.raises(ValueError):
        d.set_rectification(lm.camera(S.SW, S.SH, 130.0, 131.0, 103.5, 59.5), lm.camera(67, 45, 50.0, 50.0, 33.0, 22.0), map=np.zeros((45, 66, 2), F))
    d.set_rectification(None)
    with pytest.raises(lm.LinemodError) as e:
        d.rectification_map()
    assert e.value.code == lm.LM_ERR_INVALID and str(e.value).endswith("rectification: no rectification set: lm_set_rectification first")
    d.close()


def test_caller_table_on_the_host_program(host_program, tmp_path):
    table = S.smooth_table(67, 45)
    fin, fout = str(tmp_path / "table.bin"), str(tmp_path / "tmap.bin")
    table.tofile(fin)
    assert run(host_program, ["table", fin, fout, S.SW, S.SH, 67, 45]) == 2 * 67 * 45
    assert np.array_equal(np.fromfile(fout, np.int32).reshape(45, 67, 2), QR.quant_table(table, S.source_cam()))


def test_quant_value_sweep(host_program, tmp_path):
    """NaN, infinities, huge values, exact ties (k / 64, k odd: rint goes to the even neighbour), and the clamp edges +- 1."""
    n = 19
    hi = 32 * n + 32
    ties = np.arange(-131, 1400, 2) / 64.0
    edges = np.array([-64, -65, -63, hi, hi + 1, hi - 1], np.float64) / 32.0
    near = np.concatenate([edges, edges + 1 / 64.0, edges - 1 / 64.0, edges + 1 / 128.0, edges - 1 / 128.0])
    s = np.concatenate([[np.nan, np.inf, -np.inf, 1e30, -1e30, 1e308, -1e308, 0.0, -0.0, 1e-300, 5e-324], ties, near,
                        np.random.default_rng(2).uniform(-4, n + 4, 2000)])
    fin, fout = str(tmp_path / "s.bin"), str(tmp_path / "q.bin")
    s.astype(np.float64).tofile(fin)
    assert run(host_program, ["quant", fin, fout, n]) == len(s)
    got, ref = np.fromfile(fout, np.int32), QR.quant(s, n)
    assert np.array_equal(got, ref), "quant differs at s = %r" % s[got != ref][:8]
    assert list(ref[:7]) == [-64, -64, -64, hi, -64, hi, -64]
    t = QR.quant(ties, n)
    inside = (t > -64) & (t < hi)
    assert inside.sum() > 500 and (t[inside] % 2 == 0).all(), "a tie did not go to the even neighbour"
    assert {-64, -63, hi - 1, hi} <= set(ref.tolist())


def tap_pairs(w, h, seed):
    """Map entries that put taps on all four borders, at the four corners, fully outside, and at ax / ay in {0, 1, 16, 31}."""
    fr = [0, 1, 16, 31]
    xs = [-64, -33, -32, -31, -16, -1, 0, 1, 16, 31, 32, 32 * (w - 2) + 31, 32 * (w - 1) - 1, 32 * (w - 1), 32 * (w - 1) + 1, 32 * (w - 1) + 16,
          32 * (w - 1) + 31, 32 * w, 32 * w + 1, 32 * w + 31, 32 * w + 32]
    ys = [-64, -33, -32, -31, -16, -1, 0, 1, 16, 31, 32, 32 * (h - 2) + 31, 32 * (h - 1) - 1, 32 * (h - 1), 32 * (h - 1) + 1, 32 * (h - 1) + 16,
          32 * (h - 1) + 31, 32 * h, 32 * h + 1, 32 * h + 31, 32 * h + 32]
    pairs = [(x, y) for x in xs for y in ys]
    pairs += [(32 * i + a, 32 * j + b) for i in range(-1, w + 1) for j in (-1, 0, h // 2, h - 1, h) for a in fr for b in fr]
    pairs += [(32 * i + a, 32 * j + b) for i in (-1, 0, w - 1, w) for j in range(-1, h + 1) for a in fr for b in fr]
    rng = np.random.default_rng(seed)
    rnd = np.stack([rng.integers(-64, 32 * w + 33, 3000), rng.integers(-64, 32 * h + 33, 3000)], axis=1)
    return np.concatenate([np.array(pairs, np.int32), rnd.astype(np.int32)])


def host_pixels(exe, tmp_path, kind, swap, matrix, w, h, data, rs, ps, offset, scale, pairs):
    fin, fout = str(tmp_path / "px_in.bin"), str(tmp_path / "px_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([kind, swap, matrix, w, h, rs, ps, offset, len(data), len(pairs)], np.int64).tobytes())
        f.write(np.array([scale], np.float64).tobytes())
        f.write(data.tobytes())
        f.write(np.ascontiguousarray(pairs, np.int32).tobytes())
    assert run(exe, ["pixels", fin, fout]) == len(pairs)
    return np.fromfile(fout, np.uint32)


@pytest.mark.parametrize("fmt", S.COLOUR_FORMATS)
def test_colour_pixel_rule_through_the_kernels_loads(host_program, tmp_path, fmt):
    """Every colour kind, 19 x 7 (20 x 8 where the format needs an even size), the source ending where its malloc block ends, data pointer
    and row stride at every byte alignment 0 .. 3: the blend of lm_rectify.h equals the reference, and ASan sees no read outside the block."""
    even = fmt in ("nv12", "nv21", "yuy2", "uyvy")
    w, h = (20, 8) if even else (19, 7)
    host = S.source(fmt, w, h, seed=3)
    bgr = QR.decode(host, fmt, S.flags(fmt))
    pairs = tap_pairs(w, h, seed=4)
    ref_img = QR.rectify_colour(bgr, pairs.reshape(1, -1, 2))[0].astype(np.uint32)
    ref = ref_img[:, 0] | ref_img[:, 1] << 8 | ref_img[:, 2] << 16
    assert len({int(v) for v in ref}) > 200          # (gray has 256 values)
    for offset in range(4):
        for pad in range(4):
            data, rs = S.lay_out(host, pad, planar=fmt.endswith("planar"))
            ps = h * rs if fmt in ("bgr_planar", "rgb_planar", "nv12", "nv21") else 0
            got = host_pixels(host_program, tmp_path, KIND[fmt], int(fmt.startswith("rgb")), MATRIX[S.flags(fmt)], w, h, data, rs, ps, offset, 1.0, pairs)
            bad = got != ref
            assert not bad.any(), "%s offset %d pad %d: %d pixels differ, first at entry %r" % (fmt, offset, pad, int(bad.sum()), pairs[bad][0])


@pytest.mark.parametrize("fmt", ["u16", "f32"])
def test_depth_pixel_rule_through_the_kernels_loads(host_program, tmp_path, fmt):
    w, h = 19, 7
    host = S.depth_u16(w, h) if fmt == "u16" else S.depth_f32(w, h)
    scale = 1.0 if fmt == "u16" else 1000.0
    pairs = tap_pairs(w, h, seed=5)
    ref = QR.rectify_depth(host, pairs.reshape(1, -1, 2), scale)[0].astype(np.uint32)
    assert (ref == 0).any() and len(set(ref.tolist())) > 50
    item = host.dtype.itemsize
    for pad in (0, item, 3 * item):
        data, rs = S.lay_out(host, pad)
        got = host_pixels(host_program, tmp_path, KIND[fmt], 0, 0, w, h, data, rs, 0, 0, scale, pairs)
        bad = got != ref
        assert not bad.any(), "%s pad %d: %d pixels differ, first at entry %r" % (fmt, pad, int(bad.sum()), pairs[bad][0])


def test_setter_refusals(lm):
    d = lm.Detector(color_only=False, width=S.W, height=S.H)
    good = dict(width=96, height=64, fx=60.0, fy=60.0, cx=47.5, cy=31.5)

    def refused(words, source=None, ideal=None):
        with pytest.raises(lm.LinemodError) as e:
            d.set_rectification(lm.camera(**dict(dict(good, dist=S.LENS), **(source or {}))), lm.camera(**dict(good, **(ideal or {}))))
        assert e.value.code == lm.LM_ERR_INVALID and str(e.value).endswith(words) and "rectification: " in str(e.value), str(e.value)

    d.set_rectification(lm.camera(**dict(good, dist=S.LENS)), lm.camera(**good))
    before = d.rectification_map()
    finite = "rectification: every camera number must be finite"
    for bad in (np.nan, np.inf, -np.inf):
        for key in ("fx", "fy", "cx", "cy"):
            refused(finite, source={key: bad})
            refused(finite, ideal={key: bad})
        for k in range(5):
            dist = [0.0] * 5
            dist[k] = bad
            refused(finite, source={"dist": dist})
            refused(finite, ideal={"dist": dist})
    for key in ("fx", "fy"):
        for bad in (0.0, -60.0):
            refused("rectification: fx and fy of both cameras must be positive", source={key: bad})
            refused("rectification: fx and fy of both cameras must be positive", ideal={key: bad})
    for key in ("width", "height"):
        for bad in (0, -1, 16385):
            refused("rectification: width and height of both cameras must lie in 1 .. 16384", source={key: bad})
            refused("rectification: width and height of both cameras must lie in 1 .. 16384", ideal={key: bad})
    for k in range(5):
        dist = [0.0] * 5
        dist[k] = 1e-6
        refused("rectification: the ideal camera's coefficients must be 0", ideal={"dist": dist})
    # a refusal leaves the rectification as it was
    assert np.array_equal(d.rectification_map(), before)
    # the caller's map may hold anything
    d.set_rectification(lm.camera(**dict(good, dist=S.LENS)), lm.camera(**good), map=np.full((64, 96, 2), np.nan, F))
    assert (d.rectification_map() == -64).all()
    d.close()


def test_version_and_struct_sizes(lm):
    v = lm.load_library().lm_version()
    assert v.startswith(b"linemod_hip 0.13 ") and b"lm_ingest_frames_rectified" in v and b"lm_set_rectification" in v
    assert C.sizeof(lm.Camera) == 44 and C.sizeof(lm.RectificationDesc) == 2 * 44 + 8 == 96
    assert (lm.RECTIFY_DEPTH_ALIGNED, lm.RECTIFY_DEPTH_REGISTERED) == (0, 1)


def _has_gpu(lm):
    d = lm.Detector(color_only=True, width=64, height=64, T=[2, 8])
    try:
        d.stage_pyrdown(np.zeros((8, 8, 3), np.uint8))
        return True
    except lm.LinemodError:
        return False
    finally:
        d.close()


class Fake:
    def __init__(self, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (0x7F0012345600, False), "strides": None, "version": 2}


def test_rectified_ingest_fails_loudly_without_gpu(lm):
    if _has_gpu(lm):
        pytest.skip("a HIP device is present")
    d = lm.Detector(color_only=False, width=S.W, height=S.H)
    d.set_rectification(lm.camera(S.SW, S.SH, 130.0, 131.0, 103.5, 59.5, S.LENS))
    for route in (dict(), dict(registered=True)):
        with pytest.raises(lm.LinemodError) as e:
            d.ingest_frame(0, Fake((S.SH, S.SW, 3), "|u1"), Fake((S.SH, S.SW), "<u2"), crop=S.CROP, rectified=True, **route)
        assert e.value.code == lm.LM_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(lm.LinemodError) as e:
        d.stage_rectify(Fake((S.SH, S.SW, 3), "|u1"))
    assert e.value.code == lm.LM_ERR_NO_DEVICE
    ca, da = (lm.ImageDesc * 1)(), (lm.ImageDesc * 1)()
    assert d.lib.lm_ingest_frames_rectified(d.h, 0, 1, ca, da, None, 7, None) == lm.LM_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        d.ingest_frames(0, [dict(colour=Fake((S.SH, S.SW, 3), "|u1"), depth=Fake((S.SH, S.SW), "<u2"), rectified=True),
                            dict(colour=Fake((S.SH, S.SW, 3), "|u1"), depth=Fake((S.SH, S.SW), "<u2"))])
    d.close()


def test_facade_reads_the_distortion(lm, tmp_path):
    """readSettings on the reference's settings file yields the five coefficients; rectificationOf hands them on as the source camera,
    with the pinhole as the ideal camera and no map.  A file without the key leaves zeros."""
    exe = str(tmp_path / "rectify_settings")
    libdir = os.path.dirname(lm.LIB_PATH)
    host = os.path.join(ROOT, "line-mod-pipeline_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "rectify_settings.cpp"),
                           os.path.join(host, "HighLevelLinemod.cpp"), os.path.join(host, "PostProcess.cpp"),
                           os.path.join(host, "TemplateGenerator.cpp"), "-L" + libdir, "-llinemod_hip", "-lpthread", "-Wl,-rpath," + libdir])
    k = lm.yaml_numbers(SETTINGS, "distortion parameters")
    out = subprocess.run([exe, SETTINGS], capture_output=True, text=True, timeout=120, check=True).stdout.split("\n")
    assert out[0] == "defaults 0 0 0 0 0"
    got = [float(F(v)) for v in out[1].split()[1:]]           # (%.9g brings a float back exactly)
    assert out[1].startswith("read ") and got == [float(F(v)) for v in k] and got[1] != 0.0
    src = [float(F(v)) for v in out[2].split()[1:]]
    assert out[2].startswith("source ") and src == [float(F(v)) for v in (1044.87, 1045.69141, 320, 240)] + got + [640.0, 480.0]
    assert out[3] == "ideal " + " ".join(out[2].split()[1:5]) + " 0 0 0 0 0 640 480" and out[4] == "map 0"
    bare = tmp_path / "bare.yml"
    bare.write_text("%YAML:1.0\n---\nvideo width: 640\nvideo height: 480\ncamera fx: 500.\n")
    out = subprocess.run([exe, str(bare)], capture_output=True, text=True, timeout=120, check=True).stdout.split("\n")
    assert out[1] == "read 0 0 0 0 0"
