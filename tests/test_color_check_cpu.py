"""The colour check without a GPU: the references of tests/color_check_reference.py against each other (the table rule of the 8-bit HSV
against the real-valued one on all 2^24 colours; every generated hull's fill is one run per row), and the host colour check
(host/PostProcess.cpp: bgr2hsv_inrange, convex_hull, hull_counts) against them through tests/cpp/color_check_dump.cpp, built with g++
as it is and under ASan / UBSan."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import color_check_reference as R  # noqa: E402

HOST = os.path.join(ROOT, "line-mod-pipeline_amd", "host")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
BUILDS = [pytest.param(["-O2"], id="plain"), pytest.param(["-O1", "-g"] + SAN, id="asan_ubsan")]


def all_colours():
    """All 2^24 BGR triples, [2^24, 3] uint8, index = b + 256 g + 65536 r."""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=1).astype(np.uint8)


def build_dump(tmp_path, flags):
    """tests/cpp/color_check_dump.cpp + PostProcess.cpp alone: the functions it calls need nothing of the GPU library, and the sections
    of the rest of PostProcess.cpp (which does) are dropped by the linker."""
    exe = str(tmp_path / "color_check_dump")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "color_check_dump.cpp"), os.path.join(HOST, "PostProcess.cpp")])
    return exe


def run_dump(exe, cases, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, cases], capture_output=True, timeout=900, env=env)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err[-4000:]
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]
    return r.stdout.decode() if text else r.stdout


def test_division_tables_have_no_rounding_tie():
    """Neither (255 << 12) / i nor (180 << 12) / (6 i) lies half-way between two integers for i = 1 .. 255, so rounding half up and half
    to even (lrint's default) give the same tables: the rounding mode is not part of the rule."""
    assert R.division_table_ties() == []
    up, even = R.division_tables(R._round_half_up), R.division_tables(R._round_half_even)
    assert np.array_equal(up[0], even[0]) and np.array_equal(up[1], even[1])
    assert up[0][255] == 4096 and up[0][1] == 255 << 12 and up[1][1] == (180 << 12) // 6


def test_table_hsv_is_the_integer_next_to_the_real_hsv():
    """All 2^24 colours: V equal, |S - S_real| < 1, circular |H - H_real| < 1 (the table rule gives an integer next to the real value; the
    bound is that statement, not a tuned figure), H in 0 .. 179, so the rule's final clamp to 255 never acts.
    Measured: max |S - S_real| = 0.5215, max circular |H - H_real| = 0.6400."""
    ds = dh = 0.0
    hmin, hmax = 255, 0
    for r in range(0, 256, 16):                                   # 2^20 colours at a time
        i = np.arange(r << 16, (r + 16) << 16, dtype=np.uint32)
        c = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=1).astype(np.uint8)
        h, s, v = R.hsv8_table(c)
        hr, sr, vr = R.hsv_real(c)
        assert np.array_equal(v, vr.astype(np.int64))
        assert hr.min() >= 0.0 and hr.max() < 180.0
        d = np.abs(h - hr)
        dh = max(dh, float(np.minimum(d, 180.0 - d).max()))
        ds = max(ds, float(np.abs(s - sr).max()))
        hmin, hmax = min(hmin, int(h.min())), max(hmax, int(h.max()))
        assert s.min() >= 0 and s.max() <= 255
    print("max |S - S_real| = %.4f, max circular |H - H_real| = %.4f, H in %d .. %d" % (ds, dh, hmin, hmax))
    assert ds < 1.0 and dh < 1.0
    assert hmin == 0 and hmax == 179


def test_sector_priority_does_not_change_any_hue():
    """Which of two equal maxima names the sector (R before G before B in the rule) changes no H of any of the 2^24 colours: on a sector
    border both formulas give the same multiple of diff, or multiples that differ by 6 diff = 180 exactly.  So a kernel that asks the
    channels in another order is not wrong, and no test can tell the orders apart."""
    for r in range(0, 256, 32):
        i = np.arange(r << 16, (r + 32) << 16, dtype=np.uint32)
        c = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=1).astype(np.uint8)
        h = R.hsv8_table(c)[0]
        for order in ("grb", "bgr", "brg", "gbr", "rbg"):
            assert np.array_equal(R.hsv8_table(c, order)[0], h), order


def test_round_bound_is_half_to_even_and_unbounded():
    assert [R.round_bound(x) for x in (10.5, 11.5, -0.5, 0.5, 1.5, 99.49, 99.51, -1.5)] == [10, 12, 0, 0, 2, 99, 100, -2]
    assert R.round_bound(1e12) == 10 ** 12 and R.round_bound(-1e12) == -10 ** 12
    one = np.array([7])
    assert R.inrange_mask(one, one, one, [0, 0, 0], [1e12, 1e12, 1e12]).all()
    assert R.inrange_mask(one, one, one, [-1e12, -1e12, -1e12], [7, 7, 7]).all()
    assert not R.inrange_mask(one, one, one, [1e12, 0, 0], [1e12, 255, 255]).any()
    assert not R.inrange_mask(one, one, one, [8, 0, 0], [6, 255, 255]).any()


def host_masks(exe, tmp_path, name, col, ranges):
    """bgr2hsv_inrange of the colours col[n, 3] for every range, as [len(ranges), n / 8] packed bits (least significant bit first)."""
    assert len(col) % 8 == 0
    cases = str(tmp_path / name)
    with open(cases, "wb") as f:
        f.write(struct.pack("<iqi", 1, len(col), len(ranges)))
        f.write(np.array([list(lo) + list(hi) for lo, hi in ranges], "<f8").tobytes())
        f.write(col.tobytes())
    out = np.frombuffer(run_dump(exe, cases, text=False), np.uint8)
    assert out.size == len(col) // 8 * len(ranges)
    return out.reshape(len(ranges), len(col) // 8)


def check_masks(got, col, ranges):
    h, s, v = (c.astype(np.uint8) for c in R.hsv8_table(col))
    for k, (lo, hi) in enumerate(ranges):
        exp = np.packbits(R.inrange_mask(h, s, v, lo, hi), bitorder="little")
        if not np.array_equal(got[k], exp):
            bad = np.flatnonzero(np.unpackbits(got[k] ^ exp, bitorder="little"))
            raise AssertionError("range %r .. %r: %d colours differ, first BGR %r (reference HSV %d %d %d)" %
                                 (lo, hi, bad.size, col[bad[0]].tolist(), h[bad[0]], s[bad[0]], v[bad[0]]))


@pytest.mark.parametrize("flags", BUILDS)
def test_host_hsv_inrange_on_every_colour(tmp_path, flags):
    """bgr2hsv_inrange on all 2^24 colours, every combined range: the mask equals inrange_mask of the table rule's HSV.  The ranges with
    bounds far outside 8 bits (1e12, 2^31, 2^32) are the ones a plain (int) of the rounded bound got wrong (fixed with this test).
    Then single-value ranges, since equal masks for every value mean equal values: every H on all 2^24 colours (sanitised build: every
    12th), every S and every V on the colours of R.sv_pair_colours() -- S is a function of (V, diff) alone and every pair is there."""
    exe = build_dump(tmp_path, flags)
    col = all_colours()
    ranges = R.combined_ranges() + [([t, 0, 0], [t, 255, 255]) for t in range(0, 181, 1 if flags == ["-O2"] else 12)]
    check_masks(host_masks(exe, tmp_path, "all.bin", col, ranges), col, ranges)
    col = R.sv_pair_colours()
    ranges = [([0, t, 0], [255, t, 255]) for t in range(256)] + [([0, 0, t], [255, 255, t]) for t in range(256)]
    check_masks(host_masks(exe, tmp_path, "pairs.bin", col, ranges), col, ranges)


def hull_cases(seed):
    rng = np.random.default_rng(seed)
    fam = R.hull_families(rng)
    fam.append(("convex126", R.circle_lattice_points(126)))
    fam.append(("convex63", R.circle_lattice_points(63)))
    return fam


def test_every_generated_hull_fills_one_run_per_row():
    """The property k_hull_counts relies on when it counts R - L + 1 per row: outline plus interior of a convex hull is one run of pixels
    in every row.  Checked on the reference's pixel sets, which know nothing of rows."""
    n = ties = 0
    for seed in range(12):
        fam = hull_cases(seed)
        hulls = [R.convex_hull(p) for _, p in fam]
        ties += R.count_tie_edges(hulls)
        for (name, pts), hull in zip(fam, hulls):
            x0, y0, img = R.hull_pixels(hull)
            assert R.rows_are_runs(img), (name, pts)
            assert img.any(axis=1).all() and img.any(axis=0).all(), (name, pts)          # convex: no empty row or column in the box
            n += 1
    print("%d hulls, %d edges with a tie" % (n, ties))
    assert n >= 4000 and ties >= 200


@pytest.mark.parametrize("flags", BUILDS)
def test_host_hull_and_fill_against_the_reference(tmp_path, flags):
    """convex_hull + hull_counts of host/PostProcess.cpp on the hull families at every placement: the same vertex cycle in the same
    direction as the reference's hull, and the reference's counts.  This is also where the line's tie rule is established: the family
    holds edges with exact ties walked in both directions (asserted: at least 200)."""
    exe = build_dump(tmp_path, flags)
    W, H = 320, 240
    rng = np.random.default_rng(77)
    mask = np.repeat(np.repeat(rng.random((H // 8, W // 8)) < 0.5, 8, axis=0), 8, axis=1)
    mask ^= rng.random((H, W)) < 0.05
    seeds = (0, 1, 2) if flags == ["-O2"] else (0,)
    cases, expect = [], []
    ties = 0
    for seed in seeds:
        fam = hull_cases(seed)
        for name, pts in fam:
            hull = R.convex_hull(pts)
            ties += R.count_tie_edges([hull])
            px = R.hull_pixels(hull)
            bw, bh = max(p[0] for p in pts), max(p[1] for p in pts)
            for off in R.placements(rng, bw, bh, W, H):
                cases.append((pts, off))
                expect.append((name, hull, R.counts_of_pixels(px, off, mask, W, H)))
    assert ties >= 200, ties
    path = str(tmp_path / "hulls.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", 2, W, H))
        f.write(mask.astype(np.uint8).tobytes())
        f.write(struct.pack("<i", len(cases)))
        for pts, off in cases:
            f.write(struct.pack("<iii", len(pts), off[0], off[1]))
            f.write(np.array(pts, "<i4").tobytes())
    lines = run_dump(exe, path, text=True).splitlines()
    assert len(lines) == len(cases)
    for line, (pts, off), (name, hull, (in_hull, in_both)) in zip(lines, cases, expect):
        w = [int(t) for t in line.split()]
        got = [(w[3 + 2 * i], w[4 + 2 * i]) for i in range(w[0])]
        assert len(got) == len(hull) and got[0] in hull, (name, pts, got, hull)
        k = hull.index(got[0])
        assert got == hull[k:] + hull[:k], (name, pts, got, hull)              # same cycle, same direction
        assert (w[1], w[2]) == (in_hull, in_both), (name, pts, off, w[1:3], (in_hull, in_both))
    print("%d cases, %d edges with a tie" % (len(cases), ties))
