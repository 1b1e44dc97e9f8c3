"""CPU tests of lm_export_frames' host side.  A stand-alone program (tests/cpp/export_host.cpp, g++, plain and under
ASan / UBSan) drives the rule's shared functions (csrc/lm_draw.h: the code k_export runs), the descriptor and primitive checks
(csrc/lm_export_check.cpp) and the tile planner (lmh::plan_export); its dumps are compared with tests/export_reference.py (numpy, written
from the header's rule) and with the numbers the header pins.  Then the Python side: the forward YUV integers against the float
matrices, the three primitive builders against hand-computed lists, the struct size and the ABI addition."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import export_reference as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SOURCES = [os.path.join(ROOT, "tests", "cpp", "export_host.cpp"), os.path.join(CSRC, "lm_export_check.cpp"), os.path.join(CSRC, "lm_host.cpp")]
RING, SEGMENT, BOX = 0, 1, 2
BGR8, RGB8, BGRA8, RGBA8, BGR8_PLANAR, RGB8_PLANAR, DEPTH_U16, DEPTH_F32, GRAY8, NV12, NV21, YUY2, UYVY = range(13)
BT709, FULL = 0x100, 0x200
BASE = 0x7F0012340000       # an address that is never written


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def host_program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("export_host") / "export_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + request.param + ["-I", CSRC, "-o", exe] + SOURCES + ["-lz"])
    return exe


def run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().split("\n")[-1].startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def prim(kind, x0, y0, x1, y1, t, frame=0):
    return dict(kind=kind, frame=frame, x0=x0, y0=y0, x1=x1, y1=y1, thickness=t)


def program_coverage(exe, tmp_path, w, h, prims):
    fin, fout = str(tmp_path / "prims.txt"), str(tmp_path / "cover.bin")
    with open(fin, "w") as f:
        for p in prims:
            f.write("%d %d %d %d %d %d\n" % (p["kind"], p["x0"], p["y0"], p["x1"], p["y1"], p["thickness"]))
    run(exe, ["cover", w, h, fin, fout])
    return np.fromfile(fout, np.uint8).reshape(len(prims), h, w).astype(bool)


def test_pins(host_program):
    """The numbers the header writes out: ring and segment pixel counts, the NV12 triples, the blend at the opacities' edges."""
    got = {}
    for line in run(host_program, ["pins"]).split("\n"):
        v = line.split()
        if v:
            got.setdefault(v[0], []).append([int(x) for x in v[1:]])
    assert [c for _, c in got["ring"]] == [1, 8, 12, 16, 32, 28]
    assert got["segment"] == [[1, 10], [2, 22]]
    assert got["zero"] == [[1, 1], [2, 5], [3, 9]]
    assert [v[1:] for v in got["white"]] == [[235, 128, 128], [235, 128, 128], [255, 128, 128], [255, 128, 128]]
    assert [v[1:] for v in got["red"]] == [[81, 90, 240], [63, 102, 240], [76, 85, 255], [54, 99, 255]]
    assert len(got["blend"]) == 6 * 4 * 4
    for a, c, p, v in got["blend"]:
        assert v == int(np.floor((c * (255 - a) + p * a) / 255.0 + 0.5)), (a, c, p, v)
        if a == 255:
            assert v == p
        if a == 0:
            assert v == c
    assert got["blendall"] == [[0]]
    # blend_pixel: the three channels of B | G << 8 | R << 16 under b | g << 8 | r << 16 | a << 24, each by the same rule
    px, col = 0x00102030, 0x80FF8000
    want = sum(int(ER.blend(np.array([(px >> s) & 255]), (col >> s) & 255, col >> 24)[0]) << s for s in (0, 8, 16))
    assert got["pixel"] == [[want]]


def crafted_prims(w, h):
    """Every kind, crossing every frame edge, wholly outside, of zero length, and the coordinate extremes with the largest thickness"""
    out = [prim(RING, 10, 10, r, 0, t) for r in (0, 1, 2, 3, 4, 5, 9) for t in (1, 2, 3, 7)]
    out += [prim(RING, cx, cy, 6, 0, 2) for cx, cy in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (-3, 15), (w + 2, 15), (20, -4), (20, h + 3))]
    out += [prim(RING, -100, -100, 20, 0, 3), prim(RING, w + 100, 10, 20, 0, 64), prim(RING, 24, 16, 8191, 0, 64), prim(RING, 24, 16, 30, 0, 64),
            prim(RING, -8192, -8192, 8191, 0, 64), prim(RING, 8191, 8191, 8191, 0, 1)]
    ends = [(2, 2, 10, 5), (10, 5, 2, 2), (5, 25, 40, 3), (40, 3, 5, 25), (3, 3, 3, 28), (3, 28, 3, 3), (4, 9, 44, 9), (44, 9, 4, 9),
            (-20, 10, 70, 20), (10, -20, 30, 60), (-5, -5, 60, 40), (60, -8, -7, 39), (7, 9, 7, 9), (-50, -50, -10, -3), (100, 5, 60, 5),
            (-8191, -8191, 8191, 8191), (8191, -8191, -8191, 8191), (-8192, 16, 8191, 17), (24, -8192, 23, 8191), (-8192, -8192, -8192, -8192)]
    out += [prim(SEGMENT, *e, t) for e in ends for t in (1, 2, 3, 64)]
    boxes = [(5, 5, 30, 20), (0, 0, w - 1, h - 1), (-10, -10, w + 10, h + 10), (-5, 8, 12, 40), (20, 20, 20, 20), (10, 10, 11, 30), (40, -3, 60, 12),
             (-8192, -8192, 8191, 8191), (60, 60, 70, 70)]
    out += [prim(BOX, *b, t) for b in boxes for t in (1, 2, 5, 64)]
    return out


def test_coverage_every_kind(host_program, tmp_path):
    """48 x 32: lm_draw.h's coverage equals the reference's on Python's unbounded integers, for the crafted list and a random one"""
    w, h = 48, 32
    rng = np.random.default_rng(5)
    prims = crafted_prims(w, h)
    for _ in range(200):
        kind = int(rng.integers(0, 3))
        x0, y0, x1, y1 = (int(v) for v in rng.integers(-30, 80, 4))
        if kind == RING:
            x1, y1 = int(rng.integers(0, 40)), 0
        if kind == BOX:
            x0, x1, y0, y1 = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        prims.append(prim(kind, x0, y0, x1, y1, int(rng.choice([1, 2, 3, 4, 9, 64]))))
    got = program_coverage(host_program, tmp_path, w, h, prims)
    some, none = 0, 0
    for p, g in zip(prims, got):
        want = ER.coverage(p, w, h, exact=True)
        assert np.array_equal(g, want), (p, int((g != want).sum()))
        some += bool(want.any())
        none += not want.any()
    assert some > 100 and none > 10         # (both kinds of primitive are in the list: drawn, and wholly outside)


def test_segment_products_at_the_64_bit_extreme(host_program, tmp_path):
    """Coordinates at +-8191 / -8192 with t = 64 and pixels in the corners of the largest frame: s, L2, cross, 4 cross^2 and t^2 L2 as the
    program computed them equal Python's integers, and the largest of them needs more than 32 bits"""
    ends = [(-8191, -8191, 8191, 8191), (8191, -8191, -8191, 8191), (-8192, -8192, 8191, 8191), (-8192, 8191, 8191, -8192), (8191, 8191, -8192, -8192),
            (-8192, 0, 8191, 1)]
    pixels = [(0, 0), (8191, 0), (0, 8191), (8191, 8191), (47, 31), (4096, 4095)]
    lines = [e + (64,) + p for e in ends for p in pixels]
    fin, fout = str(tmp_path / "p.txt"), str(tmp_path / "o.txt")
    open(fin, "w").write("".join(" ".join(str(v) for v in ln) + "\n" for ln in lines))
    run(host_program, ["products", fin, fout])
    got = [[int(v) for v in ln.split()] for ln in open(fout).read().split("\n")[:-1]]
    assert len(got) == len(lines)
    top = 0
    for (x0, y0, x1, y1, t, x, y), g in zip(lines, got):
        dx, dy, wx, wy = x1 - x0, y1 - y0, x - x0, y - y0
        s, L2, cross = wx * dx + wy * dy, dx * dx + dy * dy, wx * dy - wy * dx
        if s <= 0:
            cov = 4 * (wx * wx + wy * wy) <= t * t
        elif s >= L2:
            cov = 4 * ((x - x1) ** 2 + (y - y1) ** 2) <= t * t
        else:
            cov = 4 * cross * cross <= t * t * L2
        assert g == [s, L2, cross, 4 * cross * cross, t * t * L2, int(cov)], ((x0, y0, x1, y1, x, y), g)
        assert abs(s) < 2 ** 31 and L2 < 2 ** 31 and abs(cross) < 2 ** 31 and 4 * cross * cross < 2 ** 63
        top = max(top, 4 * cross * cross)
    assert top > 2 ** 57         # (4 * 16383^4, reached: far beyond 32 bits)


def test_thin_segments_are_8_connected(host_program, tmp_path):
    w, h = 48, 32
    rng = np.random.default_rng(6)
    prims = [prim(SEGMENT, *(int(v) for v in (rng.integers(0, w), rng.integers(0, h), rng.integers(0, w), rng.integers(0, h))), 1) for _ in range(100)]
    for p, c in zip(prims, program_coverage(host_program, tmp_path, w, h, prims)):
        assert c[p["y0"], p["x0"]] and c[p["y1"], p["x1"]]
        seen = np.zeros_like(c)
        todo = [(p["y0"], p["x0"])]
        seen[todo[0]] = True
        while todo:
            y, x = todo.pop()
            for yy in range(max(y - 1, 0), min(y + 2, h)):
                for xx in range(max(x - 1, 0), min(x + 2, w)):
                    if c[yy, xx] and not seen[yy, xx]:
                        seen[yy, xx] = True
                        todo.append((yy, xx))
        assert np.array_equal(seen, c), p


def random_prims(rng, w, h, frames, n):
    out = []
    for _ in range(n):
        kind = int(rng.integers(0, 3))
        x0, x1 = (int(v) for v in rng.integers(-w // 2, w + w // 2, 2))
        y0, y1 = (int(v) for v in rng.integers(-h // 2, h + h // 2, 2))
        if kind == RING:
            x1, y1 = int(rng.integers(0, max(w, h) // 2)), 0
        if kind == BOX:
            x0, x1, y0, y1 = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
        out.append(prim(kind, x0, y0, x1, y1, int(rng.choice([1, 2, 3, 5, 64])), frame=int(rng.integers(0, frames))))
    return out


def program_plan(exe, tmp_path, w, h, undo, prims, max_entries=1 << 22):
    fin, fout = str(tmp_path / "plan_in.txt"), str(tmp_path / "plan_out.txt")
    with open(fin, "w") as f:
        for flip, sx, sy in undo:
            f.write("%d %d %d\n" % (flip, sx, sy))
        for p in prims:
            f.write("%d %d %d %d %d %d %d\n" % (p["kind"], p["frame"], p["x0"], p["y0"], p["x1"], p["y1"], p["thickness"]))
    run(exe, ["plan", w, h, len(undo), max_entries, fin, fout])
    head, off, idx, boxes = open(fout).read().split("\n")[:4]
    head = head.split()
    return dict(ok=head[0] == "ok", tiles_x=int(head[1]), tiles_y=int(head[2]), entries=int(head[3]), tw=int(head[4]), th=int(head[5]),
                off=[int(v) for v in off.split()], idx=[int(v) for v in idx.split()], boxes=np.array([int(v) for v in boxes.split()]).reshape(-1, 4))


@pytest.mark.parametrize("size", [(16, 16), (48, 32), (160, 80)], ids=lambda s: "%dx%d" % s)
def test_planner_is_conservative(host_program, tmp_path, size):
    """Brute force: for every primitive and every pixel of the frame it covers, the tile of the EXPORTED image that shows the pixel lists
    the primitive (and the record's box, which a lane rejects by, contains the pixel); every tile's list ascends; the offsets are a CSR
    table over [frame][tile]."""
    w, h = size
    rng = np.random.default_rng(w)
    undo = [(0, 0, 0), (1, 0, 0), (0, 7, -3), (1, -5, 4), (0, w, 0)]
    prims = random_prims(rng, w, h, len(undo), 120)
    plan = program_plan(host_program, tmp_path, w, h, undo, prims)
    assert plan["ok"] and plan["tiles_x"] == -(-w // plan["tw"]) and plan["tiles_y"] == -(-h // plan["th"])
    tiles = plan["tiles_x"] * plan["tiles_y"]
    off, idx = plan["off"], plan["idx"]
    assert len(off) == len(undo) * tiles + 1 and off[0] == 0 and off[-1] == len(idx) == plan["entries"]
    assert all(a <= b for a, b in zip(off, off[1:]))
    lists = [idx[off[t]:off[t + 1]] for t in range(len(off) - 1)]
    for f in range(len(undo)):
        for t in range(tiles):
            ln = lists[f * tiles + t]
            assert all(a < b for a, b in zip(ln, ln[1:])) and all(prims[k]["frame"] == f for k in ln)
    listed = 0
    for k, p in enumerate(prims):
        flip, sx, sy = undo[p["frame"]]
        ys, xs = np.nonzero(ER.coverage(p, w, h))
        bx0, by0, bx1, by1 = plan["boxes"][k]
        assert ((xs >= bx0) & (xs <= bx1) & (ys >= by0) & (ys <= by1)).all()
        # the exported pixel (u, v) that shows frame pixel (x, y): x = (flip ? w - 1 - u : u) + sx, y = v + sy
        u = (w - 1 - (xs - sx)) if flip else xs - sx
        v = ys - sy
        shown = (u >= 0) & (u < w) & (v >= 0) & (v < h)
        for tu, tv in set(zip((u[shown] // plan["tw"]).tolist(), (v[shown] // plan["th"]).tolist())):
            assert k in lists[p["frame"] * tiles + tv * plan["tiles_x"] + tu], (p, tu, tv)
            listed += 1
    assert listed > 50


def test_planner_overflow_bound(host_program, tmp_path):
    """A call above the bound plans nothing and says what it needs; at the bound it plans"""
    w, h = 160, 80
    prims = [prim(BOX, 0, 0, w - 1, h - 1, 1) for _ in range(10)]          # 3 x 3 tiles each: 90 entries
    assert program_plan(host_program, tmp_path, w, h, [(0, 0, 0)], prims, max_entries=90)["ok"]
    over = program_plan(host_program, tmp_path, w, h, [(0, 0, 0)], prims, max_entries=89)
    assert not over["ok"] and over["entries"] == 90 and over["off"] == [] and over["idx"] == []
    # the shipped bound holds at least 2^20 entries
    src = open(os.path.join(CSRC, "lm_host.h")).read()
    assert "EXPORT_MAX_ENTRIES = (size_t)1 << 22" in src


def image(fmt, width, height, row_stride, plane_stride=0, window=(0, 0), data=BASE):
    return "%d %d %d %d %d %d %d %d" % (data, row_stride, plane_stride, width, height, fmt, window[0], window[1])


def refusals(exe, tmp_path, lines):
    fin, fout = str(tmp_path / "refuse_in.txt"), str(tmp_path / "refuse_out.txt")
    open(fin, "w").write("\n".join(lines) + "\n")
    run(exe, ["refuse", fin, fout])
    out = open(fout).read().split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def test_refusals(host_program, tmp_path):
    """Every refusal the checks make, by its words; the host program holds no detector, so nothing can have been claimed"""
    W, H = 160, 80
    d = "destination image of frame 3: "
    im = lambda *a, **k: "image %d %d 3 " % (W, H) + image(*a, **k)
    exp = [("counts 1 2 0 0", "export: bad argument: a null dst or n_slots <= 0"),
           ("counts 0 0 0 0", "export: bad argument: a null dst or n_slots <= 0"),
           ("counts 0 -1 1 0", "export: bad argument: a null dst or n_slots <= 0"),
           ("counts 0 1 1 5", "export: bad argument: null prims with n_prims > 0"),
           ("counts 0 1 0 65537", "export: 65537 primitives exceed 65536"),
           ("counts 0 1 0 65536", "OK"), ("counts 0 1 1 0", "OK"),
           ("frame 8208 16", "export: a 8208 x 16 frame is wider or higher than 8192"),
           ("frame 16 8193", "export: a 16 x 8193 frame is wider or higher than 8192"),
           ("frame 24 16", "export: lm_export_frames needs a frame width that is a multiple of 16"),
           ("frame 8192 8192", "OK"), ("frame 16 16", "OK")]
    for bad in (99, -1, 13, BGR8 | BT709, BGRA8 | FULL, RGB8_PLANAR | BT709, NV12 | 0x400, GRAY8 | FULL, DEPTH_U16 | BT709, 16 | BT709, 0x1060):
        exp.append((im(bad, W, H, 4 * W, 1), d + "unknown pixel format %d" % bad))
    exp += [(im(DEPTH_U16, W, H, 4 * W), d + "LM_PIX_DEPTH_U16 is a depth format: depth export is not served"),
            (im(DEPTH_F32, W, H, 4 * W), d + "LM_PIX_DEPTH_F32 is a depth format: depth export is not served")]
    for fmt, name in ((GRAY8, "LM_PIX_GRAY8"), (NV21, "LM_PIX_NV21"), (NV21 | BT709, "LM_PIX_NV21"), (YUY2, "LM_PIX_YUY2"), (UYVY | FULL, "LM_PIX_UYVY"),
                      (16, "LM_PIX_BAYER_RGGB8"), (19, "LM_PIX_BAYER_BGGR8"), (0x1000, "a raw format"), (0x1054, "a raw format")):
        exp.append((im(fmt, W, H, 4 * W, 1), d + name + " is a source format: not served as a destination"))
    exp += [(im(BGR8, W, H, 3 * W, data=0), d + "null data pointer"),
            (im(BGR8, W + 8, H + 4, 3 * W + 24, window=(9, 0)), d + "window 160 x 80 at (9, 0) lies outside the 168 x 84 surface"),
            (im(BGR8, W + 8, H + 4, 3 * W + 24, window=(0, 5)), d + "window 160 x 80 at (0, 5) lies outside the 168 x 84 surface"),
            (im(BGR8, W + 8, H + 4, 3 * W + 24, window=(-1, 0)), d + "window 160 x 80 at (-1, 0) lies outside the 168 x 84 surface"),
            (im(BGRA8, W - 1, H, 4 * W), d + "window 160 x 80 at (0, 0) lies outside the 159 x 80 surface"),
            (im(BGR8, W + 8, H, 3 * (W + 8) - 1), d + "row_stride smaller than a surface row"),
            (im(RGBA8, W, H, 4 * W - 1), d + "row_stride smaller than a surface row"),
            (im(BGR8_PLANAR, W, H, W - 1, W * H), d + "row_stride smaller than a surface row"),
            (im(NV12, W, H, W - 1, W * H), d + "row_stride smaller than a surface row"),
            (im(BGR8, W, H, 0), d + "row_stride smaller than a surface row"),
            (im(BGR8_PLANAR, W, H, W, 0), d + "plane_stride must be positive"),
            (im(NV12 | BT709, W, H, W, -5), d + "plane_stride must be positive")]
    odd = d + "crop_x, crop_y, width and height of a LM_PIX_NV12 destination, and the frame's height, must be even"
    exp += [(im(NV12, W + 3, H + 2, W + 3, 99999, window=(2, 2)), odd), (im(NV12, W + 4, H + 3, W + 4, 99999), odd),
            (im(NV12, W + 4, H + 4, W + 4, 99999, window=(1, 2)), odd), (im(NV12 | FULL, W + 4, H + 4, W + 4, 99999, window=(2, 3)), odd),
            ("image 16 15 3 " + image(NV12, 16, 16, 16, 999), odd)]
    # what is accepted, and what it becomes: kind, swap_rb, matrix, strides, window
    exp += [(im(BGR8, W + 8, H + 4, 3 * W + 25, window=(8, 4), data=BASE + 3), "OK 0 0 0 %d 0 8 4" % (3 * W + 25)),
            (im(RGB8, W, H, 3 * W), "OK 0 1 0 %d 0 0 0" % (3 * W)), (im(BGRA8, W, H, 4 * W), "OK 1 0 0 %d 0 0 0" % (4 * W)),
            (im(RGBA8, W, H, 4 * W + 1), "OK 1 1 0 %d 0 0 0" % (4 * W + 1)), (im(BGR8_PLANAR, W, H, W, 7), "OK 2 0 0 %d 7 0 0" % W),
            (im(RGB8_PLANAR, W, H, W + 3, W * H), "OK 2 1 0 %d %d 0 0" % (W + 3, W * H))]
    for flags in (0, BT709, FULL, BT709 | FULL):
        exp.append((im(NV12 | flags, W + 4, H + 2, W + 5, 20000, window=(4, 2), data=BASE + 1), "OK 3 0 %d %d 20000 4 2" % (flags >> 8, W + 5)))
    # primitives
    p = "primitive 7: "
    pr = lambda kind, frame, x0, y0, x1, y1, t, n=3: "prim %d 7 %d %d %d %d %d %d %d" % (n, kind, frame, x0, y0, x1, y1, t)
    exp += [(pr(3, 0, 1, 1, 2, 2, 1), p + "unknown kind 3"), (pr(-1, 0, 1, 1, 2, 2, 1), p + "unknown kind -1"),
            (pr(RING, 3, 1, 1, 2, 0, 1), p + "frame 3 lies outside 0 .. 2"), (pr(BOX, -1, 1, 1, 2, 2, 1), p + "frame -1 lies outside 0 .. 2"),
            (pr(SEGMENT, 0, 8192, 1, 2, 2, 1), p + "coordinate 8192 lies outside -8192 .. 8191"),
            (pr(SEGMENT, 0, 1, -8193, 2, 2, 1), p + "coordinate -8193 lies outside -8192 .. 8191"),
            (pr(BOX, 0, 1, 1, 9000, 2, 1), p + "coordinate 9000 lies outside -8192 .. 8191"),
            (pr(BOX, 0, 1, 1, 2, -9000, 1), p + "coordinate -9000 lies outside -8192 .. 8191"),
            (pr(RING, 0, 1, 8192, 2, 0, 1), p + "coordinate 8192 lies outside -8192 .. 8191"),
            (pr(RING, 0, 1, 1, 2, 0, 0), p + "thickness 0 lies outside 1 .. 64"), (pr(BOX, 0, 1, 1, 2, 2, 65), p + "thickness 65 lies outside 1 .. 64"),
            (pr(RING, 0, 1, 1, 2, 1, 1), p + "a ring needs y1 == 0 and a radius in 0 .. 8191"),
            (pr(RING, 0, 1, 1, -1, 0, 1), p + "a ring needs y1 == 0 and a radius in 0 .. 8191"),
            (pr(RING, 0, 1, 1, 8192, 0, 1), p + "a ring needs y1 == 0 and a radius in 0 .. 8191"),
            (pr(BOX, 0, 5, 1, 4, 2, 1), p + "inverted box"), (pr(BOX, 0, 1, 3, 4, 2, 1), p + "inverted box"),
            (pr(RING, 2, -8192, 8191, 8191, 0, 64), "OK"), (pr(SEGMENT, 0, -8192, 8191, 8191, -8192, 64), "OK"), (pr(BOX, 1, 4, 4, 4, 4, 1), "OK")]
    # two destinations of one call that overlap in memory: by first and last byte per plane
    ov = lambda *images: "overlap %d %d %d " % (W, H, len(images)) + " ".join(images)
    bgr = lambda data, window=(0, 0), sw=W, sh=H: image(BGR8, sw, sh, 3 * sw, window=window, data=data)
    n = 3 * W * H
    exp += [(ov(bgr(BASE), bgr(BASE + n)), "OK"), (ov(bgr(BASE), bgr(BASE + n - 1)), "destination images of frames 0 and 1 overlap in memory"),
            (ov(bgr(BASE), bgr(BASE + 2 * n), bgr(BASE + n), bgr(BASE + 2 * n + 5)), "destination images of frames 1 and 3 overlap in memory"),
            (ov(bgr(BASE), bgr(BASE)), "destination images of frames 0 and 1 overlap in memory"),
            # one surface, windows stacked: disjoint; side by side: refused conservatively
            (ov(bgr(BASE, (0, 0), W, 2 * H), bgr(BASE, (0, H), W, 2 * H)), "OK"),
            (ov(bgr(BASE, (0, 0), 2 * W, H), bgr(BASE, (W, 0), 2 * W, H)), "destination images of frames 0 and 1 overlap in memory"),
            # a chroma plane that runs into another image's luma plane
            (ov(image(NV12, W, H, W, W * H, data=BASE), image(NV12, W, H, W, W * H, data=BASE + W * H * 3 // 2)), "OK"),
            (ov(image(NV12, W, H, W, W * H, data=BASE), image(NV12, W, H, W, W * H, data=BASE + W * H * 3 // 2 - 1)),
             "destination images of frames 0 and 1 overlap in memory"),
            (ov(image(BGR8_PLANAR, W, H, W, W * H, data=BASE), image(RGBA8, W, H, 4 * W, data=BASE + 2 * W * H + W * H - 1)),
             "destination images of frames 0 and 1 overlap in memory"),
            # a bad descriptor inside the list is named first
            (ov(bgr(BASE), image(GRAY8, W, H, W, data=BASE + n)), "destination image of frame 1: LM_PIX_GRAY8 is a source format: not served as a destination")]
    got = refusals(host_program, tmp_path, [line for line, _ in exp])
    for (line, want), g in zip(exp, got):
        assert g == want, (line, g)


def test_forward_yuv_against_the_float_matrices(host_program, tmp_path):
    """The integer luma of a pixel, and the integer chroma of a 2 x 2 block's sums, lie within 1 of the float64 value of the standard
    matrix (the block's mean for chroma): the coefficient rounding moves a value by less than 0.01 (at most 3 * 255 * 0.5 / 65536), the
    rest is the final rounding."""
    rng = np.random.default_rng(9)
    n = 5000
    rgb = rng.integers(0, 256, (n, 4, 3))
    rgb[:64] = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)] * 8)[:, None, :]
    lines, fl = [], []
    for row, (matrix, range_) in enumerate((("bt601", "limited"), ("bt709", "limited"), ("bt601", "full"), ("bt709", "full"))):
        for k in range(n):
            R, G, B = rgb[k, 0]
            lines.append("%d %d %d %d" % (row, R, G, B))                     # -> luma of the first pixel
            s = rgb[k].sum(axis=0)
            lines.append("%d %d %d %d" % (row, s[0], s[1], s[2]))            # -> chroma of the block
        y, _, _ = ER.yuv_float(rgb[:, 0, :].astype(np.float64), matrix, range_)
        _, u, v = ER.yuv_float(rgb.mean(axis=1), matrix, range_)
        fl.append((y, u, v))
    fin, fout = str(tmp_path / "yuv_in.txt"), str(tmp_path / "yuv_out.txt")
    open(fin, "w").write("\n".join(lines) + "\n")
    run(host_program, ["yuv", fin, fout])
    got = np.array([[int(v) for v in ln.split()] for ln in open(fout).read().split("\n")[:-1]]).reshape(4, n, 2, 3)
    for row in range(4):
        y, u, v = fl[row]
        for name, integer, real in (("Y", got[row, :, 0, 0], y), ("U", got[row, :, 1, 1], u), ("V", got[row, :, 1, 2], v)):
            diff = np.abs(integer - np.clip(real, 0.0, 255.0))
            assert diff.max() <= 1.0, (row, name, float(diff.max()))
            assert np.abs(integer - np.clip(np.floor(real + 0.5), 0, 255)).max() <= 1, (row, name)
    # the reference's own integers say the same
    for row, key in enumerate((("bt601", "limited"), ("bt709", "limited"), ("bt601", "full"), ("bt709", "full"))):
        img = rgb[:, :, ::-1].astype(np.uint8).reshape(n, 2, 2, 3).transpose(1, 0, 2, 3).reshape(2, 2 * n, 3)       # block k = columns 2k, 2k + 1
        Y, UV = ER.nv12(img, *key)
        assert np.array_equal(Y[0, 0::2], got[row, :, 0, 0])
        assert np.array_equal(UV[0, 0::2], got[row, :, 1, 1]) and np.array_equal(UV[0, 1::2], got[row, :, 1, 2])


def test_draw_prim_struct(lm):
    assert lm.DRAW_PRIM_DTYPE.itemsize == 32
    assert [lm.DRAW_PRIM_DTYPE.fields[k][1] for k in ("kind", "frame", "x0", "y0", "x1", "y1", "thickness", "b", "g", "r", "a")] == [0, 4, 8, 12, 16, 20, 24, 28, 29, 30, 31]
    assert (lm.DRAW_RING, lm.DRAW_SEGMENT, lm.DRAW_BOX) == (0, 1, 2)
    src = open(os.path.join(ROOT, "include", "linemod_hip.h")).read()
    assert "enum { LM_DRAW_RING = 0, LM_DRAW_SEGMENT = 1, LM_DRAW_BOX = 2 };" in src


def rows(p):
    return [tuple(int(v) for v in r) for r in p.tolist()]


def test_draw_box_and_axes(lm):
    assert rows(lm.draw_box((5, 7, 10, 4), (1, 2, 3), 2, frame=4)) == [(2, 4, 5, 7, 14, 10, 2, 1, 2, 3, 255)]
    assert rows(lm.draw_box((0, 0, 1, 1), (9, 8, 7, 6))) == [(2, 0, 0, 0, 0, 0, 1, 9, 8, 7, 6)]
    # the identity pose 1000 in front of a 640 x 480 camera, fx = fy = 500: origin (320, 240); x tip 75 * 500 / 1000 = 37.5 -> 357.5 -> 358
    # (half to even), y tip (320, 277.5 -> 278); z tip at Z = 1075: the principal point again
    I = np.eye(3)
    got = rows(lm.draw_axes(I, (0, 0, 1000), 500, 500, 640, 480, frame=2))
    assert got == [(1, 2, 320, 240, 358, 240, 2, 0, 0, 255, 255), (1, 2, 320, 240, 320, 278, 2, 0, 255, 0, 255), (1, 2, 320, 240, 320, 240, 2, 255, 0, 0, 255)]
    # half to even the other way: 25 * 500 / 1000 = 12.5 -> 332.5 -> 332
    assert rows(lm.draw_axes(I, (0, 0, 1000), 500, 500, 640, 480, length=25.0))[0][4:6] == (332, 240)
    # a rotation about z by 90 degrees: x points down the image, y to the left
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    got = rows(lm.draw_axes(Rz, (100, -50, 500), 400, 300, 160, 80, length=50.0))
    assert got == [(1, 0, 160, 10, 160, 40, 2, 0, 0, 255, 255), (1, 0, 160, 10, 120, 10, 2, 0, 255, 0, 255), (1, 0, 160, 10, 153, 13, 2, 255, 0, 0, 255)]
    # an endpoint behind the camera or beyond the coordinate bound leaves its axis out; the origin takes all three with it
    assert [r[7:10] for r in rows(lm.draw_axes(I, (0, 0, 50), 500, 500, 640, 480, length=-75.0))] == [(0, 0, 255), (0, 255, 0)]
    assert [r[7:10] for r in rows(lm.draw_axes(I, (0, 0, 1), 500, 500, 640, 480, length=75.0))] == [(255, 0, 0)]
    assert len(lm.draw_axes(I, (0, 0, -10), 500, 500, 640, 480)) == 0 and len(lm.draw_axes(I, (1e6, 0, 10), 500, 500, 640, 480)) == 0
    assert lm.draw_axes(I, (0, 0, -10), 500, 500, 640, 480).dtype == lm.DRAW_PRIM_DTYPE


def test_draw_response(lm):
    """One ring per level-0 feature of the match's template, at the feature plus the match's position: blue for the colour modality, green
    for depth; the radius is T(0) // 2 unless T is given.  Level-1 features are not drawn."""
    d = lm.Detector(color_only=False)
    descs = np.zeros(4, lm.DESC_DTYPE)          # one template: (level 0, colour), (level 0, depth), (level 1, colour), (level 1, depth)
    descs["pyramid_level"] = [0, 0, 1, 1]
    descs["width"], descs["height"] = [40, 40, 20, 20], [30, 30, 15, 15]
    descs["num_features"] = [3, 2, 1, 1]
    feats = np.zeros(7, lm.FEATURE_DTYPE)
    feats["x"], feats["y"] = [1, 10, 39, 5, 6, 2, 3], [2, 20, 29, 7, 8, 4, 5]
    feats["label"] = [0, 1, 2, 3, 4, 5, 6]
    assert d.add_class("obj", descs, feats) == 0
    m = np.zeros(1, lm.MATCH_DTYPE)[0]
    m["x"], m["y"], m["template_id"], m["class_idx"] = 100, 50, 0, 0
    got = rows(lm.draw_response(d, m, 3))
    blue, green = (255, 0, 0, 255), (0, 255, 0, 255)
    r = d.get_T(0) // 2
    assert d.get_T(0) == 5 and r == 2
    assert got == [(0, 3, 101, 52, r, 0, 1) + blue, (0, 3, 110, 70, r, 0, 1) + blue, (0, 3, 139, 79, r, 0, 1) + blue,
                   (0, 3, 105, 57, r, 0, 1) + green, (0, 3, 106, 58, r, 0, 1) + green]
    assert [g[4] for g in rows(lm.draw_response(d, m, 0, T=9))] == [4] * 5
    d.close()


def test_export_frames_needs_a_device_or_a_frame(lm):
    """The ABI addition: without a device the call fails loudly (no CPU fallback); with one, a slot without a frame is refused"""
    lib = lm.load_library()
    assert "lm_export_frames" in lm.EXPORTS and lib.lm_export_frames.argtypes is not None
    d = lm.Detector(color_only=True, width=48, height=32, T=[2, 8])
    target = lm.DeviceView(BASE, np.uint8, (32, 48, 3))
    with pytest.raises(lm.LinemodError) as e:
        d.export_frame(0, target)
    if e.value.code == lm.LM_ERR_NO_DEVICE:
        assert "no CPU fallback" in str(e.value)
    else:
        assert e.value.code == lm.LM_ERR_INVALID and "no frame uploaded to slot" in str(e.value)
    # the binding's own refusals need no library call
    with pytest.raises(ValueError):
        d.export_frames(0, [dict(target=target, layout="yuy2")])
    with pytest.raises(ValueError):
        d.export_frames(0, [target], undo=[None, None])
    with pytest.raises(ValueError):
        d.export_frames(0, [target], prims=np.zeros(2, np.int32))
    d.close()
