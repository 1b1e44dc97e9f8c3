"""CPU tests of the float colour sources (0.13 additive, DESIGN.md section 13 "Float sources"): the pins of include/linemod_hip.h recomputed
with the numpy reference (tests/ingest_float_reference.py), and csrc/lm_ingest_float.h -- to_u8, the half conversions, the export
conversions and the kernel's per-lane code -- run on the host by tests/cpp/ingest_float_host.cpp (g++, plain and under ASan / UBSan;
nothing is loaded into Python) and compared with that reference byte for byte; the descriptor check through csrc/lm_ingest_check.cpp
(tests/cpp/ingest_check_host.cpp); what the binding makes of a float __cuda_array_interface__."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ingest_float_reference as FR
import ingest_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
P = 0x7F0012345600
BASE = 0x7F0012340000
F32 = np.float32
NAMES = {0x2000 | el | lay: "LM_PIX_" + name % tag for el, tag in ((0, "F32"), (0x10, "F16"))
         for lay, name in ((0, "BGR_%s"), (1, "RGB_%s"), (2, "BGRA_%s"), (3, "RGBA_%s"), (4, "BGR_%s_PLANAR"), (5, "RGB_%s_PLANAR"), (8, "GRAY_%s"))}
UNKNOWN_NEIGHBOURS = (0x2006, 0x2007, 0x2009, 0x2016, 0x2020, 0x2100, 0x2200, 0x3000)


def bits(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


def f32_of(b):
    return np.array(b, np.uint32).view(F32)


class Fake:
    """Something that claims to live in device memory: nothing but the interface, with a made-up pointer."""

    def __init__(self, shape, typestr, strides=None, ptr=P):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "strides": strides, "version": 2}


def fields(d):
    return (d.data, d.row_stride, d.plane_stride, d.width, d.height, d.format, d.crop_x, d.crop_y, d.scale)


def build(tmp, name, flags, sources):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, "-o", exe] + sources)
    return exe


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def host_program(request, tmp_path_factory):
    return build(tmp_path_factory.mktemp("ingest_float_host"), "ingest_float_host", request.param,
                 [os.path.join(ROOT, "tests", "cpp", "ingest_float_host.cpp"), os.path.join(CSRC, "lm_ingest_check.cpp"), os.path.join(CSRC, "lm_export_check.cpp")])


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def check_program(request, tmp_path_factory):
    return build(tmp_path_factory.mktemp("ingest_check_host"), "ingest_check_host", request.param,
                 [os.path.join(ROOT, "tests", "cpp", "ingest_check_host.cpp"), os.path.join(CSRC, "lm_ingest_check.cpp")])


def run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return int(r.stdout.split()[1])


# ---- the reference against the header's pins (recomputed, not copied)
def test_reference_meets_the_header_pins():
    nan, inf = F32(np.nan), F32(np.inf)
    v = np.array([0.5, 1.5, 2.5, 254.5, np.nextafter(F32(254.5), inf), 255, -0.0, nan, inf, -inf], F32)
    assert FR.to_u8(v, 1.0).tolist() == [0, 2, 2, 254, 255, 255, 0, 0, 255, 0]
    v = np.array([0, 1, 0.5, 0.1, 0.25, 0.75, -0.2], F32)
    assert FR.to_u8(v, 255.0).tolist() == [0, 255, 128, 26, 64, 191, 0]
    assert FR.to_u8(f32_of([0x00400000]), 2.0 ** 127).tolist() == [1]
    h = FR.half_bits([0x3800, 0x3C00, 0x0001, 0x7C00, 0xFC00, 0x7E00, 0x8000, 0x2E66])
    assert FR.to_u8(h, 255.0).tolist() == [128, 255, 0, 255, 0, 0, 0, 25]
    assert FR.to_u8(FR.half_bits([1]), 2.0 ** 24).tolist() == [1]
    out = FR.to_u8(FR.half_bits(np.arange(65536)), 255.0).astype(np.int64)
    assert (int(out.sum()), int((out == 255).sum()), int((out == 0).sum()), len(np.unique(out))) == (4569216, 16389, 39940, 256)


def test_reference_meets_the_export_pins_and_round_trip():
    s = F32(1.0) / F32(255.0)
    assert bits(s) == 0x3b808081
    c = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    assert FR.from_u8(c, s, False).tolist() == [0x0, 0x3b808081, 0x3efeff00, 0x3f008081, 0x3f7eff00, 0x3f800000]
    assert FR.from_u8(c, s, True).tolist() == [0x0, 0x1c04, 0x37f8, 0x3804, 0x3bf8, 0x3c00]
    # byte * (1 / 255)f * 255 rounds back to the byte for all 256 values: exporting F32 at 1 / 255 and ingesting at 255 is the identity
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(FR.to_u8(FR.from_u8(every, s, False).view(F32), 255.0), every)


# ---- csrc/lm_ingest_float.h on the host, against the reference
def test_header_pins_through_the_product(host_program, tmp_path):
    """The same pins through lmf::to_u8 / half_to_float / from_u8_f32 / from_u8_f16 themselves, with the numbers written out."""
    def u8(values, scale):
        fin, fout = str(tmp_path / "pin_in.bin"), str(tmp_path / "pin_out.bin")
        np.asarray(values, F32).view(np.uint32).tofile(fin)
        run(host_program, ["u8", bits(scale), fin, fout])
        return np.fromfile(fout, np.uint8).tolist()
    inf = F32(np.inf)
    assert u8([0.5, 1.5, 2.5, 254.5, np.nextafter(F32(254.5), inf), 255, -0.0, np.nan, inf, -inf], 1.0) == [0, 2, 2, 254, 255, 255, 0, 0, 255, 0]
    assert u8([0, 1, 0.5, 0.1, 0.25, 0.75, -0.2], 255.0) == [0, 255, 128, 26, 64, 191, 0]
    assert u8(f32_of([0x00400000]), 2.0 ** 127) == [1]
    out = str(tmp_path / "pin_h8.bin")
    run(host_program, ["h8", bits(255.0), out])
    h = np.fromfile(out, np.uint8).astype(np.int64)
    assert h[[0x3800, 0x3C00, 0x0001, 0x7C00, 0xFC00, 0x7E00, 0x8000, 0x2E66]].tolist() == [128, 255, 0, 255, 0, 0, 0, 25]
    assert (int(h.sum()), int((h == 255).sum()), int((h == 0).sum()), len(np.unique(h))) == (4569216, 16389, 39940, 256)
    run(host_program, ["h8", bits(2.0 ** 24), out])
    assert np.fromfile(out, np.uint8)[1] == 1
    run(host_program, ["export", 0x3b808081, out])
    raw = np.fromfile(out, np.uint8)
    f32b, f16b = raw[:1024].view(np.uint32), raw[1024:].view(np.uint16)
    assert f32b[[0, 1, 127, 128, 254, 255]].tolist() == [0x0, 0x3b808081, 0x3efeff00, 0x3f008081, 0x3f7eff00, 0x3f800000]
    assert f16b[[0, 1, 127, 128, 254, 255]].tolist() == [0x0, 0x1c04, 0x37f8, 0x3804, 0x3bf8, 0x3c00]
    # the round trip of the export's F32 at 1 / 255 through to_u8 at 255, in the product's own arithmetic
    fin, fout = str(tmp_path / "rt_in.bin"), str(tmp_path / "rt_out.bin")
    f32b.tofile(fin)
    run(host_program, ["u8", bits(255.0), fin, fout])
    assert np.fromfile(fout, np.uint8).tolist() == list(range(256))


@pytest.mark.parametrize("scale", [1.0, 255.0, 2.0 ** 24])
def test_to_u8_over_all_halves(host_program, tmp_path, scale):
    out = str(tmp_path / "h8.bin")
    assert run(host_program, ["h8", bits(scale), out]) == 65536
    want = FR.to_u8(FR.half_bits(np.arange(65536)), scale)
    got = np.fromfile(out, np.uint8)
    assert np.array_equal(got, want), "%d halves differ" % int((got != want).sum())


def boundary_floats():
    """F32 bit patterns strided by 1 << 15 (both signs, subnormals, infinities and NaNs among them), and for every k in 0 .. 255 the three
    floats around k - 0.5 and around k + 0.5."""
    strided = np.arange(0, 1 << 32, 1 << 15, dtype=np.uint64).astype(np.uint32)
    ties = np.concatenate([np.arange(256, dtype=F32) - F32(0.5), np.arange(256, dtype=F32) + F32(0.5)])
    around = np.concatenate([np.nextafter(ties, F32(-np.inf)), ties, np.nextafter(ties, F32(np.inf))]).astype(F32)
    return np.concatenate([strided, around.view(np.uint32), np.array([0x00400000, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC00000], np.uint32)])


@pytest.mark.parametrize("scale", [1.0, 255.0, 2.0 ** 127, 1.0 / 3.0])
def test_to_u8_over_the_f32_boundary_set(host_program, tmp_path, scale):
    src = boundary_floats()
    if scale == 255.0:        # the ties of a 0 .. 1 source: the floats around (k +- 0.5) / 255 too
        t = ((np.arange(-1, 257, dtype=F32) + F32(0.5)) / F32(255.0)).astype(F32)
        src = np.concatenate([src] + [np.nextafter(t, F32(d)).view(np.uint32) for d in (-np.inf, np.inf)] + [t.view(np.uint32)])
    fin, fout = str(tmp_path / "u8_in.bin"), str(tmp_path / "u8_out.bin")
    src.tofile(fin)
    assert run(host_program, ["u8", bits(scale), fin, fout]) == len(src)
    want = FR.to_u8(src.view(F32), scale)
    got = np.fromfile(fout, np.uint8)
    assert np.array_equal(got, want), "%d values differ" % int((got != want).sum())
    assert {0, 255} <= set(np.unique(want).tolist())


@pytest.mark.parametrize("scale", [1.0, float(F32(1.0) / F32(255.0)), float(F32(1.0) / F32(127.5)), 300.0, 2.0 ** -20], ids=["1", "1/255", "1/127.5", "300", "2^-20"])
def test_export_conversions(host_program, tmp_path, scale):
    """Both conversions over the 256 bytes; 300 overflows binary16 to +inf from 219 on, 2^-20 lands in its subnormals."""
    out = str(tmp_path / "export.bin")
    assert run(host_program, ["export", bits(scale), out]) == 256
    raw = np.fromfile(out, np.uint8)
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(raw[:1024].view(np.uint32), FR.from_u8(every, scale, False))
    assert np.array_equal(raw[1024:].view(np.uint16), FR.from_u8(every, scale, True))


W, H, SW, SH = 32, 4, 38, 7          # the lane assembler's window and its sources: crop_x 0 .. 6, crop_y 0 .. 3


def test_lane_assembler(host_program, tmp_path):
    """Every layout and element at every 16-byte misalignment class of `data` (four for F32, eight for F16), sources that end where their
    allocation ends, row and plane strides that are no multiples of 16; odd crops, mirrored or not, shifted or not, one shift beyond the
    frame.  The program checks every load address; the frames are the reference's."""
    rng = np.random.default_rng(7)
    geometry = [((0, 0), False, (0, 0)), ((6, 3), True, (0, 0)), ((3, 1), False, (7, -3)), ((5, 2), True, (-5, 1)), ((1, 0), True, (17, 0)), ((2, 1), False, (-32, 0))]
    blob, want = [], []
    for fmt in FR.FORMATS:
        es = 2 if fmt & FR.PIX_FLOAT_F16 else 4
        for offset in range(0, 16, es):
            s = FR.Source(fmt, SW, SH, rng, offset=offset)
            assert s.row_stride % 16 and (s.plane_stride % 16 or not s.plane_stride)
            for k, (crop, flip, shift) in enumerate(geometry):
                scale = (1.0, 0.5, 255.0)[k % 3]
                blob.append(struct.pack("<14if", fmt, W, H, SW, SH, crop[0], crop[1], int(flip), shift[0], shift[1], offset, s.row_stride, s.plane_stride,
                                        len(s.raw), scale) + s.raw.tobytes())
                want.append(IR.colour(s.bgr(scale), W, H, crop=crop, flip_x=flip, shift=shift))
    # the fast path: everything 16-byte aligned (pad 0 would leave odd strides: 48 columns of 4-byte-multiple pixels are a multiple of 16)
    for fmt in FR.FORMATS:
        s = FR.Source(fmt, 48, SH, rng, offset=0, pad=0)
        for crop, flip, shift in (((0, 1), False, (0, 0)), ((16, 0), True, (0, -1)), ((0, 2), False, (16, 0))):
            if s.row_stride % 16 or s.plane_stride % 16:
                continue
            blob.append(struct.pack("<14if", fmt, W, H, 48, SH, crop[0], crop[1], int(flip), shift[0], shift[1], 0, s.row_stride, s.plane_stride, len(s.raw), 255.0)
                        + s.raw.tobytes())
            want.append(IR.colour(s.bgr(255.0), W, H, crop=crop, flip_x=flip, shift=shift))
    fin, fout = str(tmp_path / "frames_in.bin"), str(tmp_path / "frames_out.bin")
    with open(fin, "wb") as f:
        f.write(b"".join(blob))
    assert run(host_program, ["frames", fin, fout]) == len(want)
    assert len(want) >= (7 * 4 + 7 * 8) * 6 + 14
    got = np.fromfile(fout, np.uint8).reshape(len(want), H, W, 3)
    for i, w_ in enumerate(want):
        assert np.array_equal(got[i], w_), "case %d: %d bytes differ" % (i, int((got[i] != w_).sum()))
    # the drawn values meet what they should, somewhere in the kept windows
    every = np.concatenate([w_.reshape(-1) for w_ in want])
    assert {0, 1, 2, 127, 128, 254, 255} <= set(np.unique(every).tolist())


# ---- the descriptor check (csrc/lm_ingest_check.cpp), through the program of tests/test_ingest_check_cpu.py
def case(geom, role, im, whole=0, win=(320, 240), a=(0, 0), b=(0, 0), flip=0, shift=0, frame=0):
    return " ".join(str(v) for v in (geom, role, int(whole), win[0], win[1], a[0], a[1], b[0], b[1], flip, shift, frame, im["data"], im["row_stride"],
                                     im["plane_stride"], im["width"], im["height"], im["format"], im["crop_x"], im["crop_y"], repr(float(im["scale"]))))


def image(fmt, width=320, height=240, row_stride=None, plane_stride=None, crop=(0, 0), scale=255.0, data=BASE, **edit):
    es = 2 if fmt & 0x10 else 4
    lay = fmt & 15
    px = es * (3 if lay <= 1 else 4 if lay <= 3 else 1)
    im = dict(data=data, row_stride=width * px if row_stride is None else row_stride,
              plane_stride=(width * height * es if lay in (4, 5) else 0) if plane_stride is None else plane_stride, width=width, height=height, format=fmt,
              crop_x=crop[0], crop_y=crop[1], scale=scale)
    im.update(edit)
    return im


def answers(exe, tmp_path, lines):
    fin, fout = str(tmp_path / "cases.txt"), str(tmp_path / "answers.txt")
    with open(fin, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert run(exe, ["cases", fin, fout]) == len(lines)
    out = []
    for line in open(fout).read().split("\n")[:-1]:
        rc, rest = line.split("|", 1)
        out.append((1, rest) if rc == "1" else (0, [int(x) for x in rest.split()]))
    return out


def test_descriptor_fields(check_program, tmp_path):
    """All fourteen formats through the plain, the rectified and the whole-image geometry: kind = 128 + element * 4 + shape, swap_rb = the
    layout's bit 0, the plane stride kept where planes are, the scale carried."""
    lines, want = [], []
    for fmt in FR.FORMATS:
        lay, half = fmt & 15, (fmt >> 4) & 1
        shape = 0 if lay <= 1 else 1 if lay <= 3 else 2 if lay <= 5 else 3
        for geom, whole, kw in (("plain", 0, {}), ("rect", 0, dict(win=(160, 80), a=(320, 240), b=(176, 96))), ("rect", 1, dict(win=(160, 80), a=(320, 240), b=(176, 96)))):
            im = image(fmt, crop=(2, 4) if geom == "rect" else (0, 0), scale=0.5 + lay)
            lines.append(case(geom, "c", im, whole=whole, **kw))
            want.append([128 + half * 4 + shape, lay & 1 if lay != 8 else 0, im["row_stride"], im["plane_stride"], 0 if whole or geom == "plain" else 2,
                         0 if whole or geom == "plain" else 4, bits(0.5 + lay), 0, BASE])
    for line, w, (rc, g) in zip(lines, want, answers(check_program, tmp_path, lines)):
        assert rc == 0, (line, g)
        assert g[:2] + g[3:] == w, (line, g, w)
        assert g[2] == (1 if line.startswith("plain") else 0)       # (dense, aligned, crop 0: the fast path; the tiled routes: no dword rule)


def test_refusals_and_their_order(check_program, tmp_path):
    c, d = "colour image of frame 0: ", "depth image of frame 0: "
    BGR_F32, RGBA_F16, PLANAR_F32, PLANAR_F16, GRAY_F16 = 0x2000, 0x2013, 0x2004, 0x2015, 0x2018
    f32, f16 = "data and row_stride of a f32 source must be multiples of 4", "data and row_stride of a f16 source must be multiples of 2"
    scale = "scale must be finite and positive"
    dep = dict(data=BASE, row_stride=640, plane_stride=0, width=320, height=240, format=6, crop_x=0, crop_y=0, scale=1.0)
    exp = []
    for bad in UNKNOWN_NEIGHBOURS + (0x2000 | 0x1000, 0x200F, 0x201F, 0x2040, 0x2080, 0x2400, 0x2800, 0x12000, 0x2000 - (1 << 31)):
        exp.append((case("plain", "c", image(BGR_F32, format=bad)), c + "unknown pixel format %d" % bad))
        exp.append((case("plain", "d", dict(dep, format=bad)), d + "unknown pixel format %d" % bad))
    for fmt, name in NAMES.items():
        exp.append((case("plain", "d", dict(dep, format=fmt)), d + name + " is a colour format"))
        exp.append((case("raw", "d", dict(dep, format=fmt, width=96, height=64), win=(160, 80), a=(96, 64), b=(208, 120)), "raw depth image of frame 0: " + name + " is a colour format"))
    exp += [(case("plain", "c", image(BGR_F32, data=BASE + 2)), c + f32), (case("plain", "c", image(BGR_F32, row_stride=3842)), c + f32),
            (case("plain", "c", image(RGBA_F16, data=BASE + 1)), c + f16), (case("plain", "c", image(GRAY_F16, row_stride=641)), c + f16),
            (case("plain", "c", image(PLANAR_F32, plane_stride=320 * 240 * 4 + 2)), c + "plane_stride of a f32 source must be a multiple of 4"),
            (case("plain", "c", image(PLANAR_F16, plane_stride=320 * 240 * 2 + 1)), c + "plane_stride of a f16 source must be a multiple of 2"),
            (case("plain", "c", image(BGR_F32, row_stride=3839)), c + "row_stride smaller than a window row"),
            (case("plain", "c", image(GRAY_F16, row_stride=638)), c + "row_stride smaller than a window row"),
            (case("rect", "c", image(RGBA_F16, width=208, height=120, row_stride=208 * 8 - 2), win=(160, 80), a=(208, 120), b=(176, 96)),
             "rectification: " + c + "row_stride smaller than a source row")]
    exp += [(case("plain", "c", image(fmt, scale=bad)), c + scale) for fmt in (BGR_F32, RGBA_F16, PLANAR_F32, GRAY_F16) for bad in (0.0, -1.0, float("inf"), float("nan"))]
    # the earlier check wins: format < colour-or-depth < null < window < row stride < plane stride < alignment (data, row; then plane) < scale
    exp += [(case("plain", "d", dict(dep, format=0x2006, data=0)), d + "unknown pixel format %d" % 0x2006),
            (case("plain", "d", dict(dep, format=BGR_F32, data=0)), d + "LM_PIX_BGR_F32 is a colour format"),
            (case("plain", "c", image(BGR_F32, data=0, crop=(1, 0))), c + "null data pointer"),
            (case("plain", "c", image(PLANAR_F32, crop=(1, 0), row_stride=2)),
             c + "0 <= roi.x && roi.x + roi.width <= m.cols && 0 <= roi.y && roi.y + roi.height <= m.rows failed: window 320 x 240 at (1, 0) in a 320 x 240 source"),
            (case("plain", "c", image(PLANAR_F32, row_stride=1278, plane_stride=0)), c + "row_stride smaller than a window row"),
            (case("plain", "c", image(PLANAR_F32, plane_stride=-2, data=BASE + 2)), c + "plane_stride must be positive"),
            (case("plain", "c", image(PLANAR_F32, plane_stride=320 * 240 * 4 + 2, data=BASE + 2)), c + f32),
            (case("plain", "c", image(PLANAR_F16, plane_stride=320 * 240 * 2 + 1, scale=0.0)), c + "plane_stride of a f16 source must be a multiple of 2"),
            (case("plain", "c", image(RGBA_F16, data=BASE + 1, scale=float("nan"))), c + f16)]
    got = answers(check_program, tmp_path, [line for line, _ in exp])
    for (line, words), g in zip(exp, got):
        assert g == (1, words), (line, g)
    # 8-bit colour formats: the scale stays ignored; u16 depth too
    ok = [case("plain", "c", dict(image(BGR_F32, scale=0.0), format=0, row_stride=960)), case("plain", "c", image(BGR_F32, data=BASE + 4, row_stride=3844))]
    assert [rc for rc, _ in answers(check_program, tmp_path, ok)] == [0, 0]


# ---- the export's descriptor check (csrc/lm_export_check.cpp)
def export_answers(exe, tmp_path, lines):
    fin, fout = str(tmp_path / "export_in.txt"), str(tmp_path / "export_out.txt")
    with open(fin, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert run(exe, ["export_check", fin, fout]) == len(lines)
    return open(fout).read().split("\n")[:-1]


def dst(fmt, width=176, height=96, row_stride=None, plane_stride=None, window=(8, 4), scale=1.0 / 255, data=BASE):
    es = 2 if fmt & 0x10 else 4
    lay = fmt & 15
    px = es * (3 if lay <= 1 else 4 if lay <= 3 else 1)
    rs = width * px if row_stride is None else row_stride
    ps = (height * rs if lay in (4, 5) else 0) if plane_stride is None else plane_stride
    return "%d %d %d %d %d %d %d %d %d" % (data, rs, ps, width, height, fmt, window[0], window[1], bits(scale))


def test_export_destinations_and_refusals(host_program, tmp_path):
    """The twelve non-grey values are destinations (kind, channel order, element size, scale); the grey ones are source formats; the
    neighbours stay unknown; alignment and scale are refused in the ingest's sentences behind the export's prefix, after the plane stride;
    the overlap of two windows counts element bytes."""
    W, H = 160, 80
    d = "destination image of frame 3: "
    im = lambda *a, **k: "image %d %d 3 " % (W, H) + dst(*a, **k)
    lines, want = [], []
    for fmt in FR.FORMATS:
        lay, es = fmt & 15, 2 if fmt & 0x10 else 4
        lines.append(im(fmt))
        if lay == 8:
            want.append(d + "LM_PIX_GRAY_F%d is a source format: not served as a destination" % (8 * es))
        else:
            want.append("OK %d %d %d %d %d" % (lay // 2, lay & 1, es, bits(1.0 / 255), 96 * 176 * es if lay >= 4 else 0))
    for bad in UNKNOWN_NEIGHBOURS + (0x200F, 0x2040, 0x2400):
        lines.append(im(0x2000, window=(0, 0)).replace(" %d 0 0 " % 0x2000, " %d 0 0 " % bad))
        want.append(d + "unknown pixel format %d" % bad)
    f32, f16 = "data and row_stride of a f32 source must be multiples of 4", "data and row_stride of a f16 source must be multiples of 2"
    cases = [(im(0x2000, data=BASE + 2), f32), (im(0x2003, row_stride=176 * 16 + 2), f32), (im(0x2011, data=BASE + 1), f16), (im(0x2012, row_stride=176 * 8 + 1), f16),
             (im(0x2004, plane_stride=96 * 176 * 4 + 2), "plane_stride of a f32 source must be a multiple of 4"),
             (im(0x2015, plane_stride=96 * 176 * 2 + 1), "plane_stride of a f16 source must be a multiple of 2"),
             (im(0x2000, row_stride=176 * 12 - 4), "row_stride smaller than a surface row"), (im(0x2013, row_stride=176 * 8 - 2), "row_stride smaller than a surface row"),
             (im(0x2000, window=(17, 4)), "window 160 x 80 at (17, 4) lies outside the 176 x 96 surface"), (im(0x2000, data=0), "null data pointer"),
             # the earlier check wins
             (im(0x2004, plane_stride=0, data=BASE + 2), "plane_stride must be positive"), (im(0x2004, plane_stride=96 * 176 * 4 + 2, data=BASE + 2), f32),
             (im(0x2014, plane_stride=96 * 176 * 2 + 1, scale=0.0), "plane_stride of a f16 source must be a multiple of 2"),
             (im(0x2010, data=BASE + 1, scale=0.0), f16), (im(0x2000, row_stride=4, data=BASE + 2), "row_stride smaller than a surface row")]
    cases += [(im(fmt, scale=bad), "scale must be finite and positive") for fmt in (0x2000, 0x2015) for bad in (0.0, -1.0, float("inf"), float("nan"))]
    lines += [line for line, _ in cases]
    want += [d + words for _, words in cases]
    # the overlap counts element bytes: a second surface that starts right behind the first window's last element does not overlap it, one
    # that starts an element sooner does -- interleaved F32 (12 bytes per pixel) and planar F16 (the third plane's last element)
    size = ((H - 1) * 176 + W) * 12          # bytes from a window's first to behind its last
    lines += ["overlap %d %d " % (W, H) + dst(0x2000, window=(0, 0)) + " " + dst(0x2000, window=(0, 0), data=BASE + size),
              "overlap %d %d " % (W, H) + dst(0x2000, window=(0, 0)) + " " + dst(0x2000, window=(0, 0), data=BASE + size - 4),
              "overlap %d %d " % (W, H) + dst(0x2014, window=(0, 0)) + " " + dst(0x2014, window=(0, 0), data=BASE + 2 * 96 * 176 * 2 + ((H - 1) * 176 + W) * 2),
              "overlap %d %d " % (W, H) + dst(0x2014, window=(0, 0)) + " " + dst(0x2014, window=(0, 0), data=BASE + 2 * 96 * 176 * 2 + ((H - 1) * 176 + W) * 2 - 2)]
    over = "destination images of frames 0 and 1 overlap in memory"
    want += ["OK", over, "OK", over]
    got = export_answers(host_program, tmp_path, lines)
    for line, w_, g in zip(lines, want, got):
        assert g == w_, (line, g, w_)


# ---- the binding
def test_constants(lm):
    for fmt, name in NAMES.items():
        assert getattr(lm, name[3:]) == fmt
    assert (lm.PIX_FLOAT, lm.PIX_FLOAT_F16, lm.PIX_BGR_F32, lm.PIX_GRAY_F16) == (0x2000, 0x10, 0x2000, 0x2018)
    assert b"0.13" in lm.load_library().lm_version()
    assert set(lm.launch_counts()) == {"rgb", "yuv", "bayer", "raw", "float", "reduce_conv", "export", "export_float"}


@pytest.mark.parametrize("typestr,es,el", [("<f4", 4, 0), ("<f2", 2, 0x10)])
def test_image_desc_of_float_objects(lm, typestr, es, el):
    F = 0x2000 | el
    d = lm.image_desc(Fake((97, 203, 3), typestr), float_scale=255.0, crop=(3, 1))
    assert fields(d) == (P, 203 * 3 * es, 0, 203, 97, F | 0, 3, 1, 255.0)
    d = lm.image_desc(Fake((97, 203, 3), typestr, (203 * 3 * es + es, 3 * es, es), ptr=P + es), order="rgb", float_scale=1.0)
    assert fields(d) == (P + es, 203 * 3 * es + es, 0, 203, 97, F | 1, 0, 0, 1.0)
    d = lm.image_desc(Fake((97, 203, 4), typestr), float_scale=0.5)
    assert fields(d) == (P, 203 * 4 * es, 0, 203, 97, F | 2, 0, 0, 0.5)
    assert lm.image_desc(Fake((97, 203, 4), typestr), order="rgb", float_scale=1).format == F | 3
    d = lm.image_desc(Fake((3, 97, 203), typestr), layout="chw", order="rgb", float_scale=255)
    assert fields(d) == (P, 203 * es, 203 * 97 * es, 203, 97, F | 5, 0, 0, 255.0)
    d = lm.image_desc(Fake((3, 97, 203), typestr, (97 * 206 * es + es, 206 * es, es)), layout="chw", float_scale=255, crop=(43, 0))
    assert fields(d) == (P, 206 * es, 97 * 206 * es + es, 203, 97, F | 4, 43, 0, 255.0)
    d = lm.image_desc(Fake((97, 203), typestr, (204 * es, es)), layout="gray", float_scale=2.0 ** 24)
    assert fields(d) == (P, 204 * es, 0, 203, 97, F | 8, 0, 0, 2.0 ** 24)
    bad = [(Fake((97, 203, 3), typestr, (203 * 6 * es, 6 * es, es)), {}),                     # every second pixel
           (Fake((97, 203, 3), typestr, (203 * 6 * es, 3 * es, 2 * es)), {}),                 # every second channel
           (Fake((97, 203, 2), typestr), {}), (Fake((97, 203), typestr), {}),                 # two channels; a grey image as colour
           (Fake((4, 97, 203), typestr), dict(layout="chw")), (Fake((3, 97, 203), typestr, (97 * 203 * es, 203 * 2 * es, 2 * es)), dict(layout="chw")),
           (Fake((97, 203, 1), typestr), dict(layout="gray")), (Fake((97, 203), typestr, (406 * es, 2 * es)), dict(layout="gray")),
           (Fake((147, 204), typestr), dict(layout="nv12")), (Fake((98, 204, 2), typestr), dict(layout="yuy2")),
           (Fake((98, 204), typestr), dict(layout="bayer_rggb")), (Fake((98, 204), typestr), dict(layout="mono", bits=12)),
           (Fake((98, 204), typestr), dict(layout="gray", bits=12))]
    for obj, kw in bad:
        with pytest.raises(ValueError) as e:
            lm.image_desc(obj, float_scale=255.0, **kw)
        assert repr(typestr) in str(e.value), str(e.value)


def test_image_desc_default_call_and_depth_unchanged(lm):
    for typestr in ("<f4", "<f2"):
        for shape, kw in (((97, 203, 3), {}), ((3, 97, 203), dict(layout="chw")), ((97, 203), dict(layout="gray"))):
            with pytest.raises(ValueError) as e:
                lm.image_desc(Fake(shape, typestr), **kw)
            assert repr(typestr) in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:      # float16 depth stays refused, with or without a float_scale
        lm.image_desc(Fake((97, 203), "<f2"), depth=True)
    assert "'<f2'" in str(e.value)
    with pytest.raises(ValueError):
        lm.image_desc(Fake((97, 203), "<f2"), depth=True, float_scale=1.0)
    d = lm.image_desc(Fake((97, 203), "<f4"), depth=True, scale=1000.0, float_scale=3.0)
    assert fields(d) == (P, 812, 0, 203, 97, lm.PIX_DEPTH_F32, 0, 0, 1000.0)
    # uint8 objects: float_scale plays no part
    d = lm.image_desc(Fake((97, 203, 3), "|u1"), float_scale=255.0)
    assert fields(d) == (P, 609, 0, 203, 97, lm.PIX_BGR8, 0, 0, 1.0)
    # a DeviceView carries float16
    v = lm.DeviceView(0x1000, np.float16, (3, 4, 6))
    assert v.__cuda_array_interface__["typestr"] == "<f2"
    assert lm.image_desc(v, layout="chw", float_scale=255.0).format == lm.PIX_BGR_F16_PLANAR
