"""CPU tests of the rectified and reduced ingest (ABI 0.13 additive): csrc/lm_rectify_reduce.h -- lm_rectify.h's
pixel of the ideal geometry under lm_reduce.h's box and depth rules, the composition k_rectify_reduce runs -- as a stand-alone host
program (tests/cpp/rectify_reduce_host.cpp, g++ -ffp-contract=off, plain and under ASan / UBSan) against the composition of the two
independent numpy references (tests/rectify_reduce_scenes.py); the two identities; the host-only refusals through
tests/cpp/rectify_reduce_check_host.cpp; the entry points without a device; the Python keyword's rules; the version string."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rectify_reduce_scenes as X
import rectify_reference as QR
import rectify_scenes as S
import reduce_reference as RR
import reduce_scenes as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
INVALID = 1
NO_RECTIFICATION = "rectification: no rectification set: lm_set_rectification first"
NO_REDUCTION = "reduction: no reduction set: lm_set_reduction first"
# a small reduced geometry keeps the host runs short: 23 x 13 reduced pixels and a tail, but never less than the source camera's size
# (wide_ideal's focal length is fixed: a smaller ideal geometry would lie inside the source altogether)
RW, RH = 23, 13


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def host_program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rectify_reduce_host") / "rectify_reduce_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + request.param +
                          ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "rectify_reduce_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rectify_reduce_check_host") / "rectify_reduce_check_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g"] + SAN +
                          ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "rectify_reduce_check_host.cpp"), os.path.join(CSRC, "lm_ingest_check.cpp")])
    return exe


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def host_image(exe, tmp_path, kind, swap, matrix, w, h, data, rs, ps, offset, qmap, r, mode=0, scale=1.0, pipe=None):
    """The whole reduced ideal image of the host program: uint32 [Ry, Rx]."""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    nx, dx, ny, dy = RR.ratio(r)
    mh, mw = qmap.shape[:2]
    with open(fin, "wb") as f:
        f.write(np.array([kind, swap, matrix, w, h, rs, ps, offset, len(data), nx, dx, ny, dy, mode, int(pipe is not None), mw, mh, 0], np.int64).tobytes())
        f.write(np.array([scale], np.float64).tobytes())
        if pipe is not None:
            f.write(np.concatenate([[pipe["black"]], pipe["gain"], np.asarray(pipe["ccm"]).reshape(9)]).astype(np.int32).tobytes())
            f.write(np.asarray(pipe["tone"], np.uint8).tobytes())
        f.write(np.ascontiguousarray(qmap, np.int32).tobytes())
        f.write(np.ascontiguousarray(data).tobytes())
    out = run(exe, ["image", fin, fout]).split()
    assert out[0] == "OK"
    rw, rh = int(out[1]), int(out[2])
    assert (rw, rh) == (RR.reduced_size(mw, nx, dx), RR.reduced_size(mh, ny, dy))
    return np.fromfile(fout, np.uint32).reshape(rh, rw)


def packed(bgr):
    b = bgr.astype(np.uint32)
    return b[:, :, 0] | b[:, :, 1] << 8 | b[:, :, 2] << 16


def sides(r):
    nx, dx, ny, dy = RR.ratio(r)
    return max(RS.source_size(RW, (nx, dx), 0), S.SW), max(RS.source_size(RH, (ny, dy), 0), S.SH)


def colour_source(fmt):
    return X.cached(("cpu source", fmt), lambda: RS.colour(fmt, S.SW, S.SH, seed=3))


def colour_run(host_program, tmp_path, fmt, qmap, r, offset, pad):
    host, _ = colour_source(fmt)
    data, rs = S.lay_out(host, pad, planar=fmt.endswith("planar"))
    ps = S.SH * rs if fmt in ("bgr_planar", "nv12") else 0
    return host_image(host_program, tmp_path, RS.KIND[fmt], int(fmt.startswith("rgb")), RS.MATRIX[RS.flags(fmt)], S.SW, S.SH, data, rs, ps, offset, qmap, r,
                      pipe=RS.PIPE if fmt.startswith("raw") else None)


def test_the_reference_tells_the_rules_apart():
    """What the route's design relies on in the reference, on the 208 x 120 barrel scene: a zero-coefficient lens returns the source byte for
    byte, and at 3/1 the direct rectification onto the reduced camera is not the composition."""
    _, bgr = colour_source("bgr")
    source, ideal, qmap = X.identity_map()
    assert np.array_equal(QR.rectify_colour(bgr, qmap), bgr)
    source, ideal, qmap = X.lens_map(201, 102)
    composed = X.reduced_colour(bgr, qmap, (3, 1))
    third = QR.cam(67, 34, ideal["fx"] / 3, ideal["fy"] / 3, (ideal["cx"] + 0.5) / 3 - 0.5, (ideal["cy"] + 0.5) / 3 - 0.5)
    direct = QR.rectify_colour(bgr, QR.build_map(source, third))
    assert direct.shape == composed.shape == (34, 67, 3)
    assert int((direct != composed).sum()) > composed.size // 2          # (noise sources: a test that compares whole buffers tells them apart)


@pytest.mark.parametrize("fmt", RS.FAMILIES)
def test_colour_rule_through_the_kernels_loads(host_program, tmp_path, fmt):
    """One format per family under the barrel lens, the source ending where its malloc block ends: at 9/4 with the data pointer and the
    row stride at every byte alignment 0 .. 3; every other ratio of the list at one alignment.  The wide ideal camera's corners map
    outside the source: taps inside and outside it meet in one footprint."""
    _, bgr = colour_source(fmt)
    for r in RS.RATIOS:
        iw, ih = sides(r)
        source, ideal, qmap = X.lens_map(iw, ih)
        ref = X.cached(("cpu Ac", fmt, iw, ih, RR.ratio(r)), lambda: packed(X.reduced_colour(bgr, qmap, r)))
        assert X.straddling(qmap, S.SW, S.SH, r, ref.shape[1], ref.shape[0], (0, 0)) >= 40
        for offset, pad in ([(o, p) for o in range(4) for p in range(4)] if RR.ratio(r) == (9, 4, 9, 4) else [(1, 3)]):
            got = colour_run(host_program, tmp_path, fmt, qmap, r, offset, pad)
            bad = got != ref
            assert not bad.any(), "%s ratio %r offset %d pad %d: %d pixels differ, first at %r" % (fmt, r, offset, pad, int(bad.sum()), np.argwhere(bad)[0])
    assert len({int(v) for v in ref.reshape(-1)}) > 200


@pytest.mark.parametrize("dfmt", ["u16", "f32"])
@pytest.mark.parametrize("rule", ["nearest", "min_valid"])
def test_depth_rules_through_the_kernels_loads(host_program, tmp_path, dfmt, rule):
    item = 2 if dfmt == "u16" else 4
    host, scale = RS.depth(dfmt, S.SW, S.SH)
    for r in RS.RATIOS:
        iw, ih = sides(r)
        _, _, qmap = X.lens_map(iw, ih)
        ref = X.reduced_depth(host, qmap, r, rule, scale).astype(np.uint32)
        assert (ref != 0).any() and (ref == 0).any()
        for pad in (0, item, 3 * item):
            data, rs = S.lay_out(host, pad)
            got = host_image(host_program, tmp_path, RS.KIND[dfmt], 0, 0, S.SW, S.SH, data, rs, 0, 0, qmap, r, mode=1 if rule == "nearest" else 2, scale=scale)
            assert np.array_equal(got, ref), "%s %s ratio %r pad %d" % (dfmt, rule, r, pad)


@pytest.mark.parametrize("fmt", RS.FAMILIES)
def test_the_two_identities(host_program, tmp_path, fmt):
    """Zero coefficients and ideal = the source's pinhole reproduce reduce_reference alone; ratio 1/1 reproduces rectify_reference
    alone."""
    _, bgr = colour_source(fmt)
    _, _, ident = X.identity_map()
    for r in ((9, 4), ((3, 1), (9, 4))):
        got = colour_run(host_program, tmp_path, fmt, ident, r, 2, 1)
        assert np.array_equal(got, packed(RR.reduce_colour(bgr, r))), "%s: the identity lens at %r is not the reduction alone" % (fmt, r)
    _, _, qmap = X.lens_map(S.SW, S.SH)
    got = colour_run(host_program, tmp_path, fmt, qmap, (1, 1), 3, 2)
    assert np.array_equal(got, packed(QR.rectify_colour(bgr, qmap))), "%s: 1/1 is not the rectification alone" % fmt
    if fmt == "bgr":
        for dfmt, rule in (("u16", "min_valid"), ("f32", "nearest")):
            host, scale = RS.depth(dfmt, S.SW, S.SH)
            data, rs = S.lay_out(host, 0)
            mode = 1 if rule == "nearest" else 2
            got = host_image(host_program, tmp_path, RS.KIND[dfmt], 0, 0, S.SW, S.SH, data, rs, 0, 0, ident, (9, 4), mode=mode, scale=scale)
            assert np.array_equal(got, RR.reduce_depth(host, (9, 4), rule, scale))
            got = host_image(host_program, tmp_path, RS.KIND[dfmt], 0, 0, S.SW, S.SH, data, rs, 0, 0, qmap, (1, 1), mode=mode, scale=scale)
            assert np.array_equal(got, QR.rectify_depth(host, qmap, scale))


def test_descriptor_refusals_host_only(check_program):
    """lmc::check_image against lmc::rectified_reduced: the source's size against the source camera, the window against the REDUCED IDEAL
    geometry (the ideal one for an image outside `apply`), the row stride against a source row, the shared refusals in their words."""
    def image(role, whole, apply, row_stride, w, h, fmt, cx, cy, ratio=(9, 4, 9, 4), ideal=(152, 78), data=0x10000):
        return run(check_program, ["image", role, whole, 64, 32, 208, 120] + list(ideal) + list(ratio) + [apply, data, row_stride, 0, w, h, fmt, cx, cy]).strip()

    # ideal 152 x 78 at 9/4: 67 x 34 reduced
    assert image("c", 0, 3, 624, 208, 120, 0, 3, 2) == "0|0 0 3 2 208 120"
    assert image("c", 0, 3, 832, 208, 120, 2, 3, 2) == "0|1 1 3 2 208 120"            # BGRA, data and stride multiples of 4: dword loads
    assert image("c", 0, 3, 832, 208, 120, 2, 3, 2, data=0x10001) == "0|1 0 3 2 208 120"
    for cx, cy in ((4, 0), (0, 3), (-1, 0), (0, -1), (1 << 30, 0)):
        assert image("c", 0, 3, 624, 208, 120, 0, cx, cy) == \
            "1|rectification: colour image of frame 0: window 64 x 32 at (%d, %d) lies outside the 67 x 34 reduced ideal geometry" % (cx, cy)
    assert image("d", 0, 3, 416, 208, 120, 6, 4, 0) == "1|rectification: depth image of frame 0: window 64 x 32 at (4, 0) lies outside the 67 x 34 reduced ideal geometry"
    # a mixed-axis ratio: 3/1 x 9/4 of 202 x 78 is 67 x 34
    assert image("c", 0, 3, 624, 208, 120, 0, 3, 2, ratio=(3, 1, 9, 4), ideal=(202, 78)) == "0|0 0 3 2 208 120"
    assert image("c", 0, 3, 624, 208, 120, 0, 4, 2, ratio=(3, 1, 9, 4), ideal=(202, 78)).endswith("lies outside the 67 x 34 reduced ideal geometry")
    # an image outside `apply`: the rectified route's window in the ideal geometry itself
    assert image("d", 0, 1, 416, 208, 120, 6, 88, 46) == "0|3 0 88 46 208 120"
    assert image("d", 0, 1, 416, 208, 120, 6, 89, 46) == "1|rectification: depth image of frame 0: window 64 x 32 at (89, 46) lies outside the 152 x 78 ideal geometry"
    assert image("c", 0, 2, 624, 208, 120, 0, 88, 47) == "1|rectification: colour image of frame 0: window 64 x 32 at (88, 47) lies outside the 152 x 78 ideal geometry"
    # the source is the source camera's
    assert image("c", 0, 3, 624, 207, 120, 0, 0, 0) == "1|rectification: colour image of frame 0: a 207 x 120 image is not the source camera (208 x 120)"
    assert image("d", 0, 3, 416, 208, 121, 6, 0, 0) == "1|rectification: depth image of frame 0: a 208 x 121 image is not the source camera (208 x 120)"
    assert image("c", 0, 3, 623, 208, 120, 0, 0, 0) == "1|rectification: colour image of frame 0: row_stride smaller than a source row"
    assert image("d", 0, 3, 414, 208, 120, 6, 0, 0) == "1|rectification: depth image of frame 0: row_stride smaller than a source row"
    assert image("c", 0, 3, 624, 208, 120, 6, 0, 0) == "1|colour image of frame 0: LM_PIX_DEPTH_U16 is a depth format"
    assert image("d", 0, 3, 624, 208, 120, 9, 0, 0) == "1|depth image of frame 0: LM_PIX_NV12 is a colour format"
    assert image("c", 0, 3, 624, 208, 120, 99, 0, 0) == "1|colour image of frame 0: unknown pixel format 99"
    assert image("c", 0, 3, 624, 208, 120, 0, 0, 0, data=0) == "1|colour image of frame 0: null data pointer"
    # the stage hook: no window, crop ignored
    assert image("c", 1, 3, 624, 208, 120, 0, 500, 500) == "0|0 0 0 0 208 120"


class Fake:
    def __init__(self, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (0x7F0012345600, False), "strides": None, "version": 2}


def to_camera(lm, c):
    return lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])


def _has_gpu(lm):
    d = lm.Detector(color_only=True, width=64, height=64, T=[2, 8])
    try:
        d.stage_pyrdown(np.zeros((8, 8, 3), np.uint8))
        return True
    except lm.LinemodError:
        return False
    finally:
        d.close()


def test_through_the_library_without_a_device(lm):
    """The two setters compose -- each keeps what the other set -- and the route refuses, with or without a device, while either is
    missing, in that route's own words; with both set and no device, the entry and the stage hook answer LM_ERR_NO_DEVICE."""
    d = lm.Detector(color_only=False, width=RS.W, height=RS.H)
    source, ideal, qmap = X.lens_map(372, 190)
    ca, da = (lm.ImageDesc * 1)(), (lm.ImageDesc * 1)()
    call = lambda route=lm.RECTIFY_DEPTH_ALIGNED: d.lib.lm_ingest_frames_rectified_reduced(d.h, 0, 1, ca, da, None, route, None)
    words = lambda: d.lib.lm_last_error().decode()
    assert call() == INVALID and words() == NO_RECTIFICATION
    d.set_reduction((9, 4), depth_rule="min_valid")
    assert call() == INVALID and words() == NO_RECTIFICATION
    with pytest.raises(lm.LinemodError) as e:
        d.stage_rectify_reduce(Fake((120, 208, 3), "|u1"))
    assert e.value.code == INVALID and str(e.value).endswith(NO_RECTIFICATION)
    d.set_reduction(None)
    d.set_rectification(to_camera(lm, source), to_camera(lm, ideal))
    assert call() == INVALID and words() == NO_REDUCTION
    with pytest.raises(lm.LinemodError) as e:
        d.stage_rectify_reduce(Fake((120, 208, 3), "|u1"))
    assert e.value.code == INVALID and str(e.value).endswith(NO_REDUCTION)
    d.set_reduction((9, 4), depth_rule="min_valid")
    # each setter left the other's state alone
    assert d.reduction() == dict(ratio=((9, 4), (9, 4)), colour=True, depth=True, depth_rule="min_valid")
    assert np.array_equal(d.rectification_map(), qmap)
    d.set_rectification(to_camera(lm, source), to_camera(lm, ideal))
    assert d.reduction()["ratio"] == ((9, 4), (9, 4))
    assert call(7) == INVALID and words() == "rectification: unknown depth_route 7"
    if not _has_gpu(lm):
        with pytest.raises(lm.LinemodError) as e:
            d.ingest_frame(0, Fake((120, 208, 3), "|u1"), Fake((120, 208), "<u2"), rectify_reduce=True)
        assert e.value.code == lm.LM_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
        with pytest.raises(lm.LinemodError) as e:
            d.stage_rectify_reduce(Fake((120, 208, 3), "|u1"))
        assert e.value.code == lm.LM_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    d.close()


def test_rectify_reduce_is_a_property_of_the_call(lm):
    """rectify_reduce=True is a keyword of its own: not together with rectified, reduced or register_depth, the same for every frame of
    a call, and registered=True is allowed with it; the refusals of the calls that existed keep their words."""
    d = lm.Detector(color_only=False, width=RS.W, height=RS.H)
    d.set_reduction((2, 1))
    f = dict(colour=Fake((120, 208, 3), "|u1"), depth=Fake((120, 208), "<u2"), rectify_reduce=True)
    for other in (dict(rectified=True), dict(reduced=True), dict(register_depth=True), dict(rectified=True, registered=True), dict(reduced=True, rectified=True)):
        with pytest.raises(ValueError) as e:
            d.ingest_frames(0, [dict(f, **other)])
        assert "rectify_reduce=True does not go together with rectified, reduced or register_depth" in str(e.value)
    with pytest.raises(ValueError) as e:
        d.ingest_frames(0, [f, dict(f, rectify_reduce=False)])
    assert "rectify_reduce differs between the frames of one call" in str(e.value)
    # registered=True passes the keyword rules: the library is asked, and refuses for want of a rectification
    with pytest.raises(lm.LinemodError) as e:
        d.ingest_frames(0, [dict(f, registered=True)])
    assert e.value.code == INVALID and str(e.value).endswith(NO_RECTIFICATION)
    # the earlier calls' words, unchanged
    g = dict(f, rectify_reduce=False)
    with pytest.raises(ValueError) as e:
        d.ingest_frames(0, [dict(g, registered=True)])
    assert "registered=True belongs to rectified=True (without rectification: register_depth=True)" in str(e.value)
    with pytest.raises(ValueError) as e:
        d.ingest_frames(0, [dict(g, reduced=True, rectified=True)])
    assert "reduced=True does not go together with rectified / register_depth" in str(e.value)
    with pytest.raises(ValueError) as e:
        d.ingest_frames(0, [dict(g, bogus=1)])
    assert "unknown keys ['bogus']" in str(e.value)
    d.close()


def test_version_and_exports(lm):
    v = lm.load_library().lm_version()
    assert v.startswith(b"linemod_hip 0.13 ") and b"lm_ingest_frames_rectified_reduced" in v and b"lm_stage_rectify_reduce" in v
    for earlier in (b"0.13 additive: the area-averaged reduction at ingest, lm_set_reduction and lm_ingest_frames_reduced", b"lm_ingest_frames_rectified;",
                    b"0.13 additive: high-bit raw ingest formats and the raw pipeline", b"0.12 = the 0.11 ABI plus the YUV and grey ingest formats"):
        assert earlier in v
    lib = lm.load_library()
    assert lib.lm_ingest_frames_rectified_reduced.argtypes is not None and len(lib.lm_ingest_frames_rectified_reduced.argtypes) == 8
    assert len(lib.lm_stage_rectify_reduce.argtypes) == 5
    assert lm.TUNE_RECTIFY_REDUCE_GRID == 20
    d = lm.Detector(color_only=True, width=64, height=32, T=[2, 8])
    d.set_tuning(lm.TUNE_RECTIFY_REDUCE_GRID, 1)
    d.set_tuning(lm.TUNE_RECTIFY_REDUCE_GRID, 0)
    with pytest.raises(lm.LinemodError):
        d.set_tuning(lm.TUNE_RECTIFY_REDUCE_GRID, 2)
    d.close()
