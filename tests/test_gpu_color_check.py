"""The GPU colour check (k_hsv_mask, k_hull_counts, build_hull_table, reached through lm_color_check_counts, lm_color_check_counts_slots and
lm_color_mask_prepare) against tests/color_check_reference.py: an 8-bit HSV rule with exact tables, exact bound rounding, scipy's hull
and a pixel-by-pixel polygon fill.  Nothing is compared GPU against GPU, and nothing with host/PostProcess.cpp (that one is compared
with the same references in tests/test_color_check_cpu.py).

A mask is read back through the public path: a template whose only feature is (0, 0) has a one-point hull, so for a match at (x, y) the
check returns in_hull = 1 and in_both = the mask bit of pixel (x, y)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_check_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

MID_LO, MID_HI = [0, 40, 40], [100, 255, 255]            # the hull tests' range: about half of random colours


def bank_of(lm, point_sets, modalities, levels=2):
    """descs / features of one class: template t has the points of point_sets[t] as level-0 features (with two modalities the first half
    as colour, the second as depth features) and the halved coordinates on the level above."""
    descs, feats = [], []
    for pts in point_sets:
        n0 = (len(pts) + 1) // 2 if modalities == 2 else len(pts)
        parts = [pts[:n0], pts[n0:]][:modalities]
        for l in range(levels):
            for part in parts:
                f = np.zeros(len(part), lm.FEATURE_DTYPE)
                f["x"] = [p[0] >> l for p in part]; f["y"] = [p[1] >> l for p in part]
                f["label"] = np.arange(len(part)) % 8
                feats.append(f)
                descs.append(((max(p[0] for p in pts) + 1) >> l, (max(p[1] for p in pts) + 1) >> l, l, len(part)))
    return np.array(descs, lm.DESC_DTYPE), np.concatenate(feats)


def matches_of(lm, triples):
    m = np.zeros(len(triples), lm.MATCH_DTYPE)
    if len(triples):
        a = np.array(triples, np.int64)
        m["template_id"], m["x"], m["y"] = a[:, 0], a[:, 1], a[:, 2]
    m["similarity"] = 90.0
    return m


def every_pixel(lm, w, h, template_id=0):
    m = np.zeros(w * h, lm.MATCH_DTYPE)
    m["x"] = np.tile(np.arange(w), h); m["y"] = np.repeat(np.arange(h), w)
    m["template_id"] = template_id
    return m


def read_mask(d, slot, lo, hi, pixels, w, h):
    """The colour mask of the slot's frame for one range, through the one-point template at every pixel."""
    a, b = d.color_check_counts(slot, lo, hi, pixels)
    assert (a == 1).all()
    assert ((b == 0) | (b == 1)).all()
    return b.reshape(h, w).astype(bool)


def ref_mask(bgr, lo, hi):
    return R.inrange_mask(*R.hsv8_table(bgr), lo, hi)


def block_image(rng, w, h):
    """Random 8 x 8 blocks of uniform colour, one pixel in ten replaced by an independent random colour."""
    b = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8)
    img = np.kron(b, np.ones((8, 8, 1), np.uint8))[:h, :w]
    noise = rng.random((h, w)) < 0.1
    img[noise] = rng.integers(0, 256, (int(noise.sum()), 3), dtype=np.uint8)
    return np.ascontiguousarray(img)


def mixed_colours(rng, n):
    """n colours: uniform ones, dark ones (every channel below a small random maximum), greys and two-channel ties, every pure extreme."""
    u = rng.integers(0, 256, (n, 3))
    top = rng.integers(0, 64, (n, 1))
    dark = rng.integers(0, 64, (n, 3)) % (top + 1)
    tie = u.copy(); k = rng.integers(0, 3, n); tie[np.arange(n), k] = tie[np.arange(n), (k + 1) % 3]
    grey = np.repeat(rng.integers(0, 256, (n, 1)), 3, axis=1)
    kind = rng.integers(0, 8, n)
    c = np.where((kind < 4)[:, None], u, np.where((kind < 6)[:, None], dark, np.where((kind < 7)[:, None], tie, grey)))
    ext = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)])
    c[:len(ext)] = ext
    return c.astype(np.uint8)


def hull_point_sets(seed, with_126):
    rng = np.random.default_rng(seed)
    fam = R.hull_families(rng)
    sets = [[(0, 0)]] + [pts for _, pts in fam]                  # template 0: the one-point template at (0, 0)
    sets.append(R.circle_lattice_points(126 if with_126 else 63))
    return sets


def hull_queries(rng, sets, w, h, placements=None):
    """(triples (template, x, y), reference pixel sets per template, number of hull edges with a tie in the line)."""
    hulls = [R.convex_hull(p) for p in sets]
    px = [R.hull_pixels(hl) for hl in hulls]
    triples = []
    for t, pts in enumerate(sets):
        bw, bh = max(p[0] for p in pts), max(p[1] for p in pts)
        for off in (placements or R.placements)(rng, bw, bh, w, h):
            triples.append((t, off[0], off[1]))
    return triples, px, R.count_tie_edges(hulls)


def expected_counts(triples, px, mask, w, h):
    e = np.array([R.counts_of_pixels(px[t], (x, y), mask, w, h) for t, x, y in triples], np.int64).reshape(-1, 2)
    return e[:, 0], e[:, 1]


def assert_counts(got, exp, triples, what):
    for k in (0, 1):
        bad = np.flatnonzero(np.asarray(got[k]) != exp[k])
        assert bad.size == 0, "%s: %s differs for %d of %d matches, first (template, x, y) = %r: got %d, expected %d" % (
            what, ("in_hull", "in_both")[k], bad.size, len(triples), triples[bad[0]], got[k][bad[0]], exp[k][bad[0]])


# ---- every colour through k_hsv_mask -------------------------------------------------------------------------------------------------
def test_every_colour_has_the_reference_hsv(lm):
    """All 2^24 BGR triples, three times: ordered by the reference's H, by its S and by its V, laid out over 640 x 480 frames.  A frame
    then holds a narrow band [a, b] of that channel, and the mask of `channel in [0, t]` (the other two unbounded) is read for every t
    from a - 1 to b.  Equal masks for all t mean the kernel's value of that channel equals the reference's for every pixel of the
    frame -- so H, S and V of every colour are compared, not only their verdict for one range."""
    W, H = 640, 480
    P = W * H
    i = np.arange(1 << 24, dtype=np.uint32)
    col = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=1).astype(np.uint8)
    hsv = [c.astype(np.uint8) for c in R.hsv8_table(col)]
    assert hsv[0].max() == 179
    d = lm.Detector(color_only=True, width=W, height=H, frame_slots=2)
    d.add_class("point", *bank_of(lm, [[(0, 0)]], 1))
    pixels = every_pixel(lm, W, H)
    queries = 0
    for ch in range(3):
        order = np.argsort(hsv[ch], kind="stable")
        order = np.concatenate([order, np.repeat(order[-1:], -len(order) % P)])
        for f in range(len(order) // P):
            idx = order[f * P:(f + 1) * P]
            d.upload_frame(0, col[idx].reshape(H, W, 3))
            val = [c[idx] for c in hsv]
            a, b = int(val[ch][0]), int(val[ch][-1])
            for t in range(a - 1, b + 1):
                lo, hi = [0, 0, 0], [255, 255, 255]
                hi[ch] = t
                got = read_mask(d, 0, lo, hi, pixels, W, H).ravel()
                exp = R.inrange_mask(val[0], val[1], val[2], lo, hi)
                if not np.array_equal(got, exp):
                    k = int(np.flatnonzero(got != exp)[0])
                    raise AssertionError("%s <= %d: %d colours differ, first BGR %r (reference HSV %d %d %d)" % (
                        "HSV"[ch], t, int((got != exp).sum()), col[idx[k]].tolist(), val[0][k], val[1][k], val[2][k]))
                queries += 1
    print("%d mask read-backs of %d pixels" % (queries, P))
    d.close()


@pytest.mark.parametrize("size", [(640, 480), (80, 480)], ids=["640x480", "80x480"])
def test_combined_ranges_on_mixed_colours(lm, size):
    """The combined ranges (the shipped model's, bounds at 0 / 179 / 180 / 255, fractional bounds, lower > upper, bounds of -1, 256, +-1e12
    and beyond 32 bits) on one frame of mixed colours, every pixel read back; at 80 columns a mask row is two and a half words.
    A bound beyond 32 bits is where (int) of the rounded bound kept its low bits and emptied the mask (clamped with this test)."""
    W, H = size
    rng = np.random.default_rng(5)
    bgr = mixed_colours(rng, W * H).reshape(H, W, 3)
    d = lm.Detector(color_only=True, width=W, height=H, frame_slots=2)
    d.add_class("point", *bank_of(lm, [[(0, 0)]], 1))
    d.upload_frame(1, bgr)
    pixels = every_pixel(lm, W, H)
    hsv = R.hsv8_table(bgr)
    kinds = set()
    for lo, hi in R.combined_ranges():
        exp = R.inrange_mask(*hsv, lo, hi)
        got = read_mask(d, 1, lo, hi, pixels, W, H)
        assert np.array_equal(got, exp), (lo, hi, int((got != exp).sum()), int(exp.sum()))
        kinds.add("empty" if not exp.any() else "full" if exp.all() else "mixed")
    assert kinds == {"empty", "full", "mixed"}
    d.close()


# ---- mask geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(80, 480), (640, 480)], ids=["80x480", "640x480"])
def test_mask_words_and_row_spans(lm, size):
    """A random image (every pixel an independent colour), per-pixel read-back of its mask -- the last word of every row, pixels 31 / 32 /
    63 / 64 among them -- and horizontal hull rows (segments and three-row boxes) that lie inside one mask word, start at bit 0, end at
    bit 31, cover exactly one word, and span three words and more, clipped at both borders, against the exact fill."""
    W, H = size
    rng = np.random.default_rng(11)
    bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = ref_mask(bgr, MID_LO, MID_HI)
    assert 0.25 < mask.mean() < 0.75
    spans = [1, 2, 24, 30, 31, 32, 33, 62, 63, 64, 65, 70, 95, 96, 97, 128]
    sets = [[(0, 0)]] + [[(0, 0), (s, 0)] for s in spans] + [[(0, 0), (s, 0), (s, 2), (0, 2), (s // 2, 1)] for s in spans]
    d = lm.Detector(color_only=True, width=W, height=H, frame_slots=2)
    d.add_class("rows", *bank_of(lm, sets, 1))
    d.upload_frame(0, bgr)
    got = read_mask(d, 0, MID_LO, MID_HI, every_pixel(lm, W, H), W, H)
    assert np.array_equal(got, mask), int((got != mask).sum())
    for x in (31, 32, 63, 64, W - 1, (W - 1) // 32 * 32):
        assert np.array_equal(got[:, x], mask[:, x])
    px = [R.hull_pixels(R.convex_hull(p)) for p in sets]
    triples = []
    for t in range(1, len(sets)):
        s = sets[t][1][0]
        for x in sorted({0, 1, 30, 31, 32, 33, 34, 63, 64, 65, 31 - s, 32 - s, 63 - s, 64 - s, W - 1 - s, W - s, W - 2 - s, W - 1, -1, -s, -s - 1, W}):
            triples.append((t, x, int(rng.integers(0, H - 3))))
    cases = {"one_word": 0, "bit0": 0, "bit31": 0, "whole_word": 0, "three_words": 0}
    for t, x, _ in triples:
        L, Rr = max(x, 0), min(x + sets[t][1][0], W - 1)
        if L > Rr:
            continue
        cases["one_word"] += L >> 5 == Rr >> 5
        cases["bit0"] += L & 31 == 0
        cases["bit31"] += Rr & 31 == 31
        cases["whole_word"] += L & 31 == 0 and Rr == L + 31
        cases["three_words"] += (Rr >> 5) - (L >> 5) >= 2
    assert all(v >= 8 for v in cases.values()), cases
    got = d.color_check_counts(0, MID_LO, MID_HI, matches_of(lm, triples))
    assert_counts(got, expected_counts(triples, px, mask, W, H), triples, "row spans")
    d.close()


# ---- general hulls through build_hull_table and k_hull_counts -------------------------------------------------------------------------
@pytest.mark.parametrize("color_only", [False, True], ids=["rgbd_126", "colour_63"])
def test_hull_families_at_every_placement(lm, color_only):
    """Templates whose level-0 features are the point sets of R.hull_families (random polygons with duplicates, slivers, flat and thin
    boxes, collinear sets, points, edges with exact ties in the line) plus lattice points in convex position -- 126 of them, 63 colour
    and 63 depth features of one RGB-D template, or 63 in a colour-only detector -- so the product builds every hull itself.  Each is
    placed well inside, across each border and corner, wholly outside on each side and 10^6 pixels away; in_hull and in_both of the
    one-slot call, of the four-slot call over four images in shuffled order, of the call after lm_color_mask_prepare and of
    lm_color_check_begin_slots / _end are each compared with the exact fill, never with each other."""
    W, H = 640, 480
    rng = np.random.default_rng(21 + color_only)
    sets, triples, px, ties = [], [], [], 0
    for seed in ((3, 4, 5, 6, 7, 8) if not color_only else (9, 10, 11)):
        s = hull_point_sets(seed, with_126=not color_only)
        tr, p, n = hull_queries(rng, s, W, H)
        triples += [(t + len(sets), x, y) for t, x, y in tr]
        sets += s; px += p; ties += n
    print("%d templates, %d matches, %d hull edges with a tie in the line" % (len(sets), len(triples), ties))
    assert ties >= 200, ties
    assert max(len(R.convex_hull(p)) for p in sets) == (63 if color_only else 126)
    d = lm.Detector(color_only=color_only, width=W, height=H, frame_slots=4)
    d.add_class("hulls", *bank_of(lm, sets, 1 if color_only else 2))
    images = [block_image(rng, W, H) for _ in range(4)]
    masks = [ref_mask(b, MID_LO, MID_HI) for b in images]
    depth = np.full((H, W), 800, np.uint16)
    for k in range(4):
        print("slot %d: %.3f of the pixels in range" % (k, masks[k].mean()))
        assert 0.25 < masks[k].mean() < 0.75
        d.upload_frame(k, images[k], None if color_only else depth)
    m = matches_of(lm, triples)
    exp = [expected_counts(triples, px, masks[k], W, H) for k in range(4)]
    assert exp[0][0].max() > 3000 and (exp[0][0] == 0).sum() >= 8 * len(sets)
    inside = exp[0][0] > 0
    assert (exp[0][1][inside] < exp[0][0][inside]).mean() > 0.5 and (exp[0][1][inside] > 0).mean() > 0.5       # in_both is informative
    assert_counts(d.color_check_counts(0, MID_LO, MID_HI, m), exp[0], triples, "one slot")
    # four slots, shuffled
    perm = rng.permutation(len(triples))
    slot_of = rng.integers(0, 4, len(triples)).astype(np.int32)
    tr4 = [triples[i] for i in perm]
    e4 = (np.array([exp[slot_of[j]][0][i] for j, i in enumerate(perm)]), np.array([exp[slot_of[j]][1][i] for j, i in enumerate(perm)]))
    assert_counts(d.color_check_counts_slots(slot_of, MID_LO, MID_HI, m[perm]), e4, tr4, "four slots")
    # prepared masks: another range first (so the masks in the slots are not this range's), then prepare + check
    other = d.color_check_counts_slots(slot_of, [0, 0, 0], [255, 255, 255], m[perm])
    assert np.array_equal(other[0], other[1])
    d.color_mask_prepare(1, 0, 4, MID_LO, MID_HI)
    assert_counts(d.color_check_counts_slots(slot_of, MID_LO, MID_HI, m[perm]), e4, tr4, "prepared, four slots")
    d.color_mask_prepare(2, 0, 4, MID_LO, MID_HI)
    assert_counts(d.color_check_counts(3, MID_LO, MID_HI, m), exp[3], triples, "prepared, one slot")
    # the two halves, lm_color_check_begin_slots / _end, with an upload to a slot the list does not name in between
    import ctypes as C
    mm, sl = np.ascontiguousarray(m[perm]), np.ascontiguousarray(slot_of)
    sl[sl == 3] = 2
    e3 = (np.array([exp[sl[j]][0][i] for j, i in enumerate(perm)]), np.array([exp[sl[j]][1][i] for j, i in enumerate(perm)]))
    lo, hi = (C.c_double * 3)(*MID_LO), (C.c_double * 3)(*MID_HI)
    d._check(d.lib.lm_color_check_begin_slots(d.h, sl.ctypes.data_as(C.c_void_p), lo, hi, mm.ctypes.data_as(C.c_void_p), len(mm)))
    d.upload_frame(3, images[0], None if color_only else depth)
    a, b = np.zeros(len(mm), np.int64), np.zeros(len(mm), np.int64)
    d._check(d.lib.lm_color_check_end(d.h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
    assert_counts((a, b), e3, tr4, "begin / end, three slots")
    assert_counts(d.color_check_counts(3, MID_LO, MID_HI, m), exp[0], triples, "slot 3 after its new upload")
    d.close()


# ---- tall frames -----------------------------------------------------------------------------------------------------------------------
def tall_placements(h):
    def f(rng, bw, bh, w, _h):
        cx = (w - bw) // 2 if bw < w else -(bw - w) // 2
        return [(cx, 0), (cx, -(bh // 2) - 1), (cx, h // 2), (cx, 1920), (cx, 1921), (cx, h - 1 - bh), (cx, h - 1 - bh // 2), (cx, h - 1),
                (cx, h - bh), (cx, h), (cx, -bh - 1), (0, 1919 - bh // 2), (w - 1 - bw // 2, h - 1 - bh // 2), (-(bw // 2) - 1, h - 2)]
    return f


def test_frames_taller_than_1920_rows(lm):
    """80 x 1936, the smallest frame a colour-only detector accepts above 1920 rows: k_hull_counts then needs more than 64 KB of dynamic
    LDS and the launcher raises the kernel's limit.  The hull families at the top, in the rows from 1920 on, touching and crossing the
    last row; then a 480-row detector in the same process (the raised limit must do no harm); then the tall one once more."""
    W, H = 80, 1936
    rng = np.random.default_rng(31)
    sets = hull_point_sets(6, with_126=False)
    sets = [p for p in sets if max(q[1] for q in p) < 400]
    d = lm.Detector(color_only=True, width=W, height=H, frame_slots=2)
    d.add_class("hulls", *bank_of(lm, sets, 1))
    bgr = block_image(rng, W, H)
    mask = ref_mask(bgr, MID_LO, MID_HI)
    assert 0.25 < mask.mean() < 0.75
    d.upload_frame(0, bgr)
    got = read_mask(d, 0, MID_LO, MID_HI, every_pixel(lm, W, H), W, H)
    assert np.array_equal(got, mask)
    triples, px, _ = hull_queries(rng, sets, W, H, tall_placements(H))
    exp = expected_counts(triples, px, mask, W, H)
    assert (exp[0] > 0).mean() > 0.7
    m = matches_of(lm, triples)
    assert_counts(d.color_check_counts(0, MID_LO, MID_HI, m), exp, triples, "1936 rows")
    # a 480-row detector afterwards
    W2, H2 = 640, 480
    d2 = lm.Detector(color_only=True, width=W2, height=H2, frame_slots=2)
    d2.add_class("hulls", *bank_of(lm, sets, 1))
    bgr2 = block_image(rng, W2, H2)
    mask2 = ref_mask(bgr2, MID_LO, MID_HI)
    d2.upload_frame(0, bgr2)
    tr2, px2, _ = hull_queries(rng, sets, W2, H2)
    assert_counts(d2.color_check_counts(0, MID_LO, MID_HI, matches_of(lm, tr2)), expected_counts(tr2, px2, mask2, W2, H2), tr2, "480 rows after 1936")
    assert_counts(d.color_check_counts(0, MID_LO, MID_HI, m), exp, triples, "1936 rows again")
    d2.close()
    d.close()


def test_frames_taller_than_4992_rows_are_refused(lm):
    """80 x 5008 (a frame of 0.4 megapixels: no more memory than 640 x 626): four waves' rows no longer fit a workgroup's LDS, the check
    returns LM_ERR_INVALID with its documented message, and the detector goes on working: uploads, a match, an empty check."""
    W, H = 80, 5008
    rng = np.random.default_rng(41)
    d = lm.Detector(color_only=True, width=W, height=H, frame_slots=2)
    d.add_class("two", *bank_of(lm, [[(int(x), int(y)) for x, y in rng.integers(0, 60, (40, 2))], [(0, 0), (9, 4), (2, 7)]], 1))
    bgr = block_image(rng, W, H)
    d.upload_frame(0, bgr)
    m = matches_of(lm, [(1, 10, 10), (0, 5, 5000)])
    for _ in range(2):
        with pytest.raises(lm.LinemodError) as e:
            d.color_check_counts(0, MID_LO, MID_HI, m)
        assert e.value.code == lm.LM_ERR_INVALID
        assert "frame too tall for the GPU colour check (more than 4992 rows): use the host colour check" in str(e.value)
    a, b = d.color_check_counts(0, MID_LO, MID_HI, m[:0])
    assert len(a) == 0 and len(b) == 0
    d.upload_frame(1, bgr[::-1].copy())
    out = d.match_slot(1, 90.0, class_idx=0)
    assert out.dtype == lm.MATCH_DTYPE
    with pytest.raises(lm.LinemodError):
        d.color_check_counts_slots(np.array([1, 0], np.int32), MID_LO, MID_HI, m)
    d.upload_frame(0, bgr)
    d.close()
