"""CPU tests of the area-averaged reduction (ABI 0.13 additive): csrc/lm_reduce.h -- spans, weights, the converted
source pixel k_reduce stages, the colour rule, both depth rules and the tile planner -- as a stand-alone host program
(tests/cpp/reduce_host.cpp, g++ -ffp-contract=off, plain and under ASan / UBSan) against the independent numpy reference
tests/reduce_reference.py; the header's pins; the host-only refusals through tests/cpp/reduce_check_host.cpp and through the library
(lm_set_reduction needs no device); lm_reduced_camera; struct size, version string and the Python properties."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reduce_reference as RR
import reduce_scenes as RS
import rectify_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
INVALID = 1


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def host_program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reduce_host") / "reduce_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + request.param +
                          ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "reduce_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reduce_check_host") / "reduce_check_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g"] + SAN +
                          ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "reduce_check_host.cpp"), os.path.join(CSRC, "lm_ingest_check.cpp")])
    return exe


def run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def host_image(exe, tmp_path, kind, swap, matrix, w, h, data, rs, ps, offset, r, mode=0, scale=1.0, pipe=None):
    """The whole reduced image of the host program: uint32 [Ry, Rx]."""
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    nx, dx, ny, dy = RR.ratio(r)
    with open(fin, "wb") as f:
        f.write(np.array([kind, swap, matrix, w, h, rs, ps, offset, len(data), nx, dx, ny, dy, mode, int(pipe is not None), 0], np.int64).tobytes())
        f.write(np.array([scale], np.float64).tobytes())
        if pipe is not None:
            f.write(np.concatenate([[pipe["black"]], pipe["gain"], np.asarray(pipe["ccm"]).reshape(9)]).astype(np.int32).tobytes())
            f.write(np.asarray(pipe["tone"], np.uint8).tobytes())
        f.write(np.ascontiguousarray(data).tobytes())
    out = run(exe, ["image", fin, fout]).split()
    assert out[0] == "OK"
    rw, rh = int(out[1]), int(out[2])
    assert (rw, rh) == (RR.reduced_size(w, nx, dx), RR.reduced_size(h, ny, dy))
    return np.fromfile(fout, np.uint32).reshape(rh, rw)


def packed(bgr):
    b = bgr.astype(np.uint32)
    return b[:, :, 0] | b[:, :, 1] << 8 | b[:, :, 2] << 16


def test_the_headers_pins():
    """The numbers written into include/linemod_hip.h, from the reference."""
    row = np.array([[10, 20, 30, 40, 50, 60, 70, 80, 90]], np.uint8)
    assert RR.weights(9, 9, 4).tolist() == [[4, 4, 1, 0, 0, 0, 0, 0, 0], [0, 0, 3, 4, 2, 0, 0, 0, 0], [0, 0, 0, 0, 2, 4, 3, 0, 0], [0, 0, 0, 0, 0, 0, 1, 4, 4]]
    assert RR.reduce_colour(row[:, :, None].repeat(3, 2), ((9, 4), (1, 1)))[0, :, 1].tolist() == [17, 39, 61, 83]
    img = np.array([[10, 20, 30, 40, 50, 60, 70], [80, 90, 100, 110, 120, 130, 140], [150, 160, 170, 180, 190, 200, 210], [220, 230, 240, 250, 255, 0, 5],
                    [15, 25, 35, 45, 55, 65, 75]], np.uint8)
    assert RR.weights(7, 7, 3).tolist() == [[3, 3, 1, 0, 0, 0, 0], [0, 0, 2, 3, 2, 0, 0], [0, 0, 0, 0, 1, 3, 3]]
    assert RR.weights(5, 5, 2).tolist() == [[2, 2, 1, 0, 0], [0, 0, 1, 2, 2]]
    assert RR.reduce_colour(img[:, :, None].repeat(3, 2), ((7, 3), (5, 2)))[:, :, 2].tolist() == [[73, 96, 119], [131, 153, 83]]
    dep = np.array([[0, 500, 0, 700, 800, 900, 1000, 1100, 1200], [300, 0, 0, 650, 0, 950, 0, 1150, 1250]], np.uint16)
    assert RR.reduce_depth(dep, ((9, 4), (2, 1)), "nearest").tolist() == [[0, 650, 950, 1150]]
    assert RR.reduce_depth(dep, ((9, 4), (2, 1)), "min_valid").tolist() == [[300, 650, 800, 1100]]
    # the checkerboard and the stripes of the GPU suite's discriminating test
    y, x = np.mgrid[0:8, 0:12]
    board = (255 * ((x + y) & 1)).astype(np.uint8)[:, :, None].repeat(3, 2)
    assert (RR.reduce_colour(board, (2, 1)) == 128).all()
    stripes = (255 * (x & 1)).astype(np.uint8)[:, :, None].repeat(3, 2)
    assert RR.reduce_colour(stripes, (3, 1))[0, :, 0].tolist() == [85, 170, 85, 170]


def test_pins_on_the_host_program(host_program, tmp_path):
    row = np.array([10, 20, 30, 40, 50, 60, 70, 80, 90], np.uint8)
    data = np.concatenate([row, row, row])          # (planar BGR: the three channels are the row)
    got = host_image(host_program, tmp_path, 2, 0, 0, 9, 1, data, 9, 9, 0, ((9, 4), (1, 1)))
    assert got.tolist() == [[17 * 0x010101, 39 * 0x010101, 61 * 0x010101, 83 * 0x010101]]
    dep = np.array([[0, 500, 0, 700, 800, 900, 1000, 1100, 1200], [300, 0, 0, 650, 0, 950, 0, 1150, 1250]], np.uint16)
    assert host_image(host_program, tmp_path, 3, 0, 0, 9, 2, dep.view(np.uint8).reshape(-1), 18, 0, 0, ((9, 4), (2, 1)), mode=1).tolist() == [[0, 650, 950, 1150]]
    assert host_image(host_program, tmp_path, 3, 0, 0, 9, 2, dep.view(np.uint8).reshape(-1), 18, 0, 0, ((9, 4), (2, 1)), mode=2).tolist() == [[300, 650, 800, 1100]]


AXES = [(2, 1), (3, 1), (9, 4), (8, 1), (16, 5), (1, 1), (7, 3), (5, 2), (17, 16), (127, 16), (31, 16), (16, 3), (15, 2)]


@pytest.mark.parametrize("num,den", AXES)
def test_spans_and_weights(host_program, num, den):
    """Every reduced pixel of sides with a tail (203), without one (R num / den = n exactly) and of one reduced pixel: the span is exactly
    the reference's non-zero weights, they sum to num, a span never has more than ceil(num / den) + 1 taps, and the pixels beside a span
    weigh nothing."""
    for n in (203, 18 * num, num, -(-num // den)):
        lines = run(host_program, ["axis", num, den, n]).strip().split("\n")
        W = RR.weights(n, num, den)
        assert lines[0] == "OK %d" % W.shape[0]
        assert len(lines) == 1 + W.shape[0]
        if n == 18 * num:
            assert W.shape[0] * num == n * den and W[-1, -1] == den           # no tail: the last source pixel is used whole
        for X, line in enumerate(lines[1:]):
            taps, beside = line.split(" | ")
            v = [int(t) for t in taps.split()]
            first, count, w = v[0], v[1], v[2:]
            nz = np.flatnonzero(W[X])
            assert (first, count) == (int(nz[0]), len(nz)) and w == W[X, nz].tolist(), (num, den, n, X)
            assert sum(w) == num and count <= -(-num // den) + 1 and max(w) <= den
            assert beside == "0 0"


def colour_case(host_program, tmp_path, fmt, w, h, r, offset, pad, cache={}):
    key = (fmt, w, h)
    if key not in cache:
        cache[key] = RS.colour(fmt, w, h, seed=3)
    host, bgr = cache[key]
    rkey = (fmt, w, h, RR.ratio(r))
    if rkey not in cache:
        cache[rkey] = packed(RR.reduce_colour(bgr, r))
    ref = cache[rkey]
    data, rs = S.lay_out(host, pad, planar=fmt.endswith("planar"))
    ps = h * rs if fmt in ("bgr_planar", "nv12") else 0
    got = host_image(host_program, tmp_path, RS.KIND[fmt], int(fmt.startswith("rgb")), RS.MATRIX[RS.flags(fmt)], w, h, data, rs, ps, offset, r,
                     pipe=RS.PIPE if fmt.startswith("raw") else None)
    bad = got != ref
    assert not bad.any(), "%s %d x %d ratio %r offset %d pad %d: %d pixels differ, first at %r" % (fmt, w, h, r, offset, pad, int(bad.sum()), np.argwhere(bad)[0])
    return ref


@pytest.mark.parametrize("fmt", RS.FAMILIES)
def test_colour_rule_through_the_kernels_loads(host_program, tmp_path, fmt):
    """One format per family, the source ending where its malloc block ends: at 9/4 a 203 (204) wide source -- a tail -- with the data
    pointer and the row stride at every byte alignment 0 .. 3; every other ratio of the list on a source whose sides the ratio divides
    and on one with a tail; 1/1 returns the decoded source itself."""
    wide = 204 if RS.even(fmt) else 203
    for offset in range(4):
        for pad in range(4):
            ref = colour_case(host_program, tmp_path, fmt, wide, 18, (9, 4), offset, pad)
    assert ref.shape == (8, 90) and len({int(v) for v in ref.reshape(-1)}) > 200
    for r in RS.RATIOS:
        nx, dx, ny, dy = RR.ratio(r)
        exact = (2 * nx * (2 if RS.even(fmt) else 1), 2 * ny * (2 if RS.even(fmt) else 1))           # R num / den = n on both axes
        tail = (exact[0] + (2 if RS.even(fmt) else 1), exact[1] + (2 if RS.even(fmt) else 1))
        for w, h in (exact, tail):
            ref = colour_case(host_program, tmp_path, fmt, w, h, r, 1, 3)
            if (nx, dx, ny, dy) == (1, 1, 1, 1):
                assert np.array_equal(ref, packed(RS.colour(fmt, w, h, seed=3)[1]))


@pytest.mark.parametrize("dfmt", ["u16", "f32"])
@pytest.mark.parametrize("rule", ["nearest", "min_valid"])
def test_depth_rules_through_the_kernels_loads(host_program, tmp_path, dfmt, rule):
    item = 2 if dfmt == "u16" else 4
    for r in RS.RATIOS:
        nx, dx, ny, dy = RR.ratio(r)
        for w, h in ((203, 11), (2 * nx, 2 * ny)):
            host, scale = RS.depth(dfmt, w, h)
            ref = RR.reduce_depth(host, r, rule, scale).astype(np.uint32)
            for pad in (0, item, 3 * item):
                data, rs = S.lay_out(host, pad)
                got = host_image(host_program, tmp_path, RS.KIND[dfmt], 0, 0, w, h, data, rs, 0, 0, r, mode=1 if rule == "nearest" else 2, scale=scale)
                assert np.array_equal(got, ref), "%s %s ratio %r %d x %d pad %d" % (dfmt, rule, r, w, h, pad)
    # the rules differ where it matters: a hole at the footprint's centre with valid pixels beside it
    host, scale = RS.depth("u16", 203, 11)
    a, b = RR.reduce_depth(host, (3, 1), "nearest"), RR.reduce_depth(host, (3, 1), "min_valid")
    assert ((a == 0) & (b != 0)).any() and (b[a != 0] <= a[a != 0]).all()


def test_tile_plan(host_program):
    """Every ratio the setter accepts: the tile's LDS footprint stays inside the budget (8 : 1 on both axes included), the tile is a power
    of two with at most 256 pixels, and no tile position needs a larger source patch than the plan reserves."""
    from math import gcd
    seen = set()
    for den in range(1, 17):
        for num in range(den, 8 * den + 1):
            if gcd(num, den) == 1:
                seen.add((num, den))
    assert (8, 1) in seen and (9, 4) in seen and (127, 16) in seen
    pairs = [((8, 1), (8, 1)), ((1, 1), (1, 1)), ((8, 1), (1, 1)), ((1, 1), (8, 1)), ((9, 4), (9, 4)), ((3, 1), (9, 4)), ((127, 16), (127, 16))]
    pairs += [(a, a) for a in sorted(seen)][::7]
    for (nx, dx), (ny, dy) in pairs:
        out = run(host_program, ["plan", nx, dx, ny, dy]).split()
        tw, th, sw, sh, lds, need_w, need_h = (int(v) for v in out[1:])
        assert out[0] == "OK" and lds == 4 * sw * sh + 8 * sh * tw and lds <= 24 * 1024
        assert tw & (tw - 1) == 0 and th & (th - 1) == 0 and 1 <= tw * th <= 256
        assert need_w <= sw and need_h <= sh, "a tile needs %d x %d source pixels, the plan reserves %d x %d" % (need_w, need_h, sw, sh)
    assert run(host_program, ["plan", 9, 4, 9, 4]).split()[1:3] == ["32", "8"]


def test_the_division_free_quotients(host_program):
    """The kernel divides by num_x num_y with a float reciprocal and a remainder check, and splits a tile's small offsets by den the same
    way: every accumulator value 0 .. 256 N of every N of the ratio list (and the largest, 128 x 128) against `/`, and every small_div
    argument below 65536 for every den."""
    for nx, ny in [(2, 2), (3, 3), (9, 9), (8, 8), (16, 16), (1, 1), (3, 9), (128, 128), (127, 113), (7, 5)]:
        assert run(host_program, ["finish", nx, ny]).split() == ["OK", str(256 * nx * ny + 1)]


def desc_call(exe, *v):
    return run(exe, ["desc"] + list(v)).strip()


def test_reduction_refusals_host_only(check_program):
    """lmc::check_reduction: every refusal with its words, and the fractions in lowest terms."""
    assert desc_call(check_program, 18, 8, 3, 1, 3, 1) == "0|9 4 3 1 3 1"
    assert desc_call(check_program, 16, 16, 128, 16, 1, 0) == "0|1 1 8 1 1 0"
    for den in (0, 17, -1):
        assert desc_call(check_program, 20, den, 2, 1, 3, 0) == "1|reduction: den_x %d lies outside 1 .. 16" % den
        assert desc_call(check_program, 2, 1, 20, den, 3, 0) == "1|reduction: den_y %d lies outside 1 .. 16" % den
    assert desc_call(check_program, 3, 4, 2, 1, 3, 0) == "1|reduction: num_x 3 is smaller than den_x 4: an enlargement is not served"
    assert desc_call(check_program, 2, 1, 0, 1, 3, 0) == "1|reduction: num_y 0 is smaller than den_y 1: an enlargement is not served"
    assert desc_call(check_program, 33, 4, 2, 1, 3, 0) == "1|reduction: num_x 33 is larger than 8 den_x 4"
    assert desc_call(check_program, 2, 1, 9, 1, 3, 0) == "1|reduction: num_y 9 is larger than 8 den_y 1"
    assert desc_call(check_program, 2, 1, 2, 1, 0, 0) == "1|reduction: apply 0 names no image"
    for apply in (4, 7, -1):
        assert desc_call(check_program, 2, 1, 2, 1, apply, 0) == "1|reduction: apply %d has unknown bits" % apply
    for rule in (2, -1):
        assert desc_call(check_program, 2, 1, 2, 1, 3, rule) == "1|reduction: unknown depth_rule %d" % rule


def test_descriptor_refusals_host_only(check_program):
    """lmc::check_image against lmc::reduced: the window against the REDUCED geometry of the image's own size, the row stride against a
    SOURCE row, the shared format refusals in their words, and what an image outside `apply` is checked against."""
    def image(role, whole, apply, row_stride, w, h, fmt, cx, cy, ratio=(9, 4, 9, 4), data=0x10000):
        return run(check_program, ["image", role, whole, 64, 32] + list(ratio) + [apply, data, row_stride, 0, w, h, fmt, cx, cy]).strip()

    # 151 x 77 at 9/4: 67 x 34 reduced
    assert image("c", 0, 3, 453, 151, 77, 0, 3, 2) == "0|0 0 3 2 151 77"
    assert image("c", 0, 3, 604, 151, 77, 2, 3, 2) == "0|1 1 3 2 151 77"           # BGRA, data and stride multiples of 4: dword loads
    assert image("c", 0, 3, 604, 151, 77, 2, 3, 2, data=0x10001) == "0|1 0 3 2 151 77"
    for cx, cy in ((4, 0), (0, 3), (-1, 0), (0, -1), (1 << 30, 0)):
        assert image("c", 0, 3, 453, 151, 77, 0, cx, cy) == \
            "1|reduction: colour image of frame 0: window 64 x 32 at (%d, %d) lies outside the 67 x 34 reduced geometry of a 151 x 77 source" % (cx, cy)
    assert image("d", 0, 3, 302, 151, 77, 6, 4, 0) == \
        "1|reduction: depth image of frame 0: window 64 x 32 at (4, 0) lies outside the 67 x 34 reduced geometry of a 151 x 77 source"
    assert image("c", 0, 3, 452, 151, 77, 0, 0, 0) == "1|reduction: colour image of frame 0: row_stride smaller than a source row"
    assert image("d", 0, 3, 300, 151, 77, 6, 0, 0) == "1|reduction: depth image of frame 0: row_stride smaller than a source row"
    assert image("c", 0, 3, 1 << 20, 32769, 77, 0, 0, 0) == \
        "1|reduction: colour image of frame 0: width and height of a reduced source must lie in 1 .. 32768 (32769 x 77)"
    assert image("c", 0, 3, 453, 151, 77, 6, 0, 0) == "1|colour image of frame 0: LM_PIX_DEPTH_U16 is a depth format"
    assert image("d", 0, 3, 453, 151, 77, 9, 0, 0) == "1|depth image of frame 0: LM_PIX_NV12 is a colour format"
    assert image("c", 0, 3, 453, 151, 77, 99, 0, 0) == "1|colour image of frame 0: unknown pixel format 99"
    assert image("c", 0, 3, 453, 151, 77, 0, 0, 0, data=0) == "1|colour image of frame 0: null data pointer"
    assert image("c", 0, 3, 151, 151, 77, 9, 0, 0) == "1|colour image of frame 0: width and height of a LM_PIX_NV12 source must be even"
    # the stage hook: no window, crop ignored
    assert image("c", 1, 3, 453, 151, 77, 0, 500, 500) == "0|0 0 0 0 151 77"
    # an image outside `apply`: the plain ingest's window in the source itself, a row stride that holds the window
    assert image("d", 0, 1, 128, 70, 40, 6, 6, 8) == "0|3 0 6 8 70 40"
    assert image("d", 0, 1, 128, 70, 40, 6, 7, 8).startswith("1|depth image of frame 0: 0 <= roi.x && roi.x + roi.width <= m.cols")
    assert image("d", 0, 1, 126, 70, 40, 6, 0, 0) == "1|depth image of frame 0: row_stride smaller than a window row"


def test_setter_and_getter_through_the_library(lm):
    """lm_set_reduction is host state: it works without a device, normalises the fractions, refuses in check_reduction's words and keeps
    the previous setting; the reduced route without a reduction is refused whether or not a device is there."""
    d = lm.Detector(color_only=False, width=RS.W, height=RS.H)
    assert d.reduction() is None
    d.set_reduction((18, 8), depth_rule="min_valid")
    assert d.reduction() == dict(ratio=((9, 4), (9, 4)), colour=True, depth=True, depth_rule="min_valid")
    d.set_reduction(((3, 1), (9, 4)), depth=False)
    want = dict(ratio=((3, 1), (9, 4)), colour=True, depth=False, depth_rule="nearest")
    assert d.reduction() == want
    for args, words in ((dict(ratio=(2, 0)), "reduction: den_x 0 lies outside 1 .. 16"), (dict(ratio=(34, 17)), "reduction: den_x 17 lies outside 1 .. 16"),
                        (dict(ratio=(3, 4)), "reduction: num_x 3 is smaller than den_x 4: an enlargement is not served"),
                        (dict(ratio=((2, 1), (17, 2))), "reduction: num_y 17 is larger than 8 den_y 2"),
                        (dict(ratio=(2, 1), colour=False, depth=False), "reduction: apply 0 names no image"),
                        (dict(ratio=(2, 1), depth_rule=5), "reduction: unknown depth_rule 5")):
        with pytest.raises(lm.LinemodError) as e:
            d.set_reduction(**args)
        assert e.value.code == INVALID and str(e.value).endswith(words), str(e.value)
        assert d.reduction() == want
    r = lm.reduction_desc((2, 1))
    r.apply = 8
    assert d.lib.lm_set_reduction(d.h, C.byref(r)) == INVALID and d.lib.lm_last_error().decode() == "reduction: apply 8 has unknown bits"
    with pytest.raises(ValueError):
        d.set_reduction((2, 1), depth_rule="median")
    d.set_reduction(None)
    assert d.reduction() is None
    ca, da = (lm.ImageDesc * 1)(), (lm.ImageDesc * 1)()
    assert d.lib.lm_ingest_frames_reduced(d.h, 0, 1, ca, da, None, None) == INVALID
    assert d.lib.lm_last_error().decode() == "reduction: no reduction set: lm_set_reduction first"
    with pytest.raises(lm.LinemodError) as e:
        d.stage_reduce(Fake((77, 151, 3), "|u1"))
    assert e.value.code == INVALID and str(e.value).endswith("reduction: no reduction set: lm_set_reduction first")
    d.close()


class Fake:
    def __init__(self, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (0x7F0012345600, False), "strides": None, "version": 2}


def test_reduced_is_a_property_of_the_call(lm):
    """reduced=True does not go together with rectified / register_depth, and every frame of a call has the same."""
    d = lm.Detector(color_only=False, width=RS.W, height=RS.H)
    d.set_reduction((2, 1))
    f = dict(colour=Fake((170, 330, 3), "|u1"), depth=Fake((170, 330), "<u2"), reduced=True)
    for other in (dict(rectified=True), dict(register_depth=True), dict(rectified=True, registered=True)):
        with pytest.raises(ValueError) as e:
            d.ingest_frames(0, [dict(f, **other)])
        assert "reduced=True does not go together with rectified / register_depth" in str(e.value)
    with pytest.raises(ValueError) as e:
        d.ingest_frames(0, [f, dict(f, reduced=False)])
    assert "reduced differs between the frames of one call" in str(e.value)
    d.close()


def _has_gpu(lm):
    d = lm.Detector(color_only=True, width=64, height=64, T=[2, 8])
    try:
        d.stage_pyrdown(np.zeros((8, 8, 3), np.uint8))
        return True
    except lm.LinemodError:
        return False
    finally:
        d.close()


def test_reduced_ingest_fails_loudly_without_gpu(lm):
    if _has_gpu(lm):
        pytest.skip("a HIP device is present")
    d = lm.Detector(color_only=False, width=RS.W, height=RS.H)
    d.set_reduction((2, 1))
    with pytest.raises(lm.LinemodError) as e:
        d.ingest_frame(0, Fake((170, 330, 3), "|u1"), Fake((170, 330), "<u2"), reduced=True)
    assert e.value.code == lm.LM_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(lm.LinemodError) as e:
        d.stage_reduce(Fake((170, 330, 3), "|u1"))
    assert e.value.code == lm.LM_ERR_NO_DEVICE
    d.close()


def test_reduced_camera(lm):
    """lm_reduced_camera against the formula in float64, rounded once; and geometrically: a 3-D point projected through the source camera
    and mapped into the slot (pixel centres: u' = (u + 0.5) den / num - 0.5 - crop) lands where the returned camera projects it."""
    src = lm.camera(1920, 1080, 1081.37, 1083.2, 959.5, 539.5, (0.05, -0.01, 0.001, 0.002, 0.0))
    F = np.float32
    for ratio, crop, size in (((9, 4), (106, 0), (640, 480)), (((3, 1), (9, 4)), (0, 0), (640, 480)), ((2, 1), (13, 7), (64, 32)), ((16, 5), (5, 3), (160, 80)),
                              ((1, 1), (0, 0), (1920, 1080))):
        out = lm.reduced_camera(src, ratio, crop, size)
        fx, fy, cx, cy = RR.reduced_camera((src.fx, src.fy, src.cx, src.cy), ratio, crop)
        assert (out.fx, out.fy, out.cx, out.cy) == (F(fx), F(fy), F(cx), F(cy)), ratio
        assert (out.width, out.height) == size and (out.k1, out.k2, out.p1, out.p2, out.k3) == (src.k1, src.k2, src.p1, src.p2, src.k3)
        nx, dx, ny, dy = RR.ratio(ratio)
        for P in ((0.1, -0.2, 1.0), (-350.0, 120.0, 900.0), (0.0, 0.0, 2.5)):
            x, y = P[0] / P[2], P[1] / P[2]             # (the distortion acts on (x, y) and is the same for both cameras)
            u, v = float(src.fx) * x + float(src.cx), float(src.fy) * y + float(src.cy)
            us, vs = (u + 0.5) * dx / nx - 0.5 - crop[0], (v + 0.5) * dy / ny - 0.5 - crop[1]
            assert abs(float(out.fx) * x + float(out.cx) - us) < 1e-3 and abs(float(out.fy) * y + float(out.cy) - vs) < 1e-3
    # the documented example: 1920 x 1080 at 9/4 is 853 x 480, the 640-wide window is centred at crop 106
    assert (1920 * 4 // 9, 1080 * 4 // 9) == (853, 480) and (853 - 640) // 2 == 106
    whole = lm.reduced_camera(src, (9, 4))
    assert (whole.width, whole.height) == (853, 480)
    with pytest.raises(lm.LinemodError) as e:
        lm.reduced_camera(src, (3, 4))
    assert str(e.value).endswith("reduction: num_x 3 is smaller than den_x 4: an enlargement is not served")


def test_version_and_struct_sizes(lm):
    v = lm.load_library().lm_version()
    assert v.startswith(b"linemod_hip 0.13 ") and b"lm_set_reduction" in v and b"lm_ingest_frames_reduced" in v
    for earlier in (b"0.13 additive: high-bit raw ingest formats and the raw pipeline", b"lm_ingest_frames_rectified", b"0.12 = the 0.11 ABI plus the YUV and grey ingest formats"):
        assert earlier in v
    assert C.sizeof(lm.ReductionDesc) == 24
    assert (lm.REDUCE_COLOUR, lm.REDUCE_DEPTH, lm.REDUCE_DEPTH_NEAREST, lm.REDUCE_DEPTH_MIN_VALID) == (1, 2, 0, 1)
