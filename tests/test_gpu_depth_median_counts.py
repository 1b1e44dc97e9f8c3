"""k_dmedian's counting median with cumulative counters (lm_median_counts.h, lm_dev_depth.h): the quantised depth image of resident
frames -- lm_debug_read, what 0, level 0, modality 1 -- against oracle.depth_quantize of the same depth image, byte for byte, at
the smallest shapes at which the form can go wrong: widths of 2, 3, 5 and 9 lanes (a lane is 8 pixels of a row), heights below, at
and above one band of rows and no multiples of the bands (4 rows per lane for few frames, 16 for batches).

Both instantiations run: one slot takes the few-frame kernels, phase_max_slots + 1 slots (at least 16: plan_depth_quantize's own
rule) the batch kernels.  lm_create refuses frames whose rows x cols is no multiple of 16 (upstream's assertion in
computeResponseMaps), so 24 x 11 and 40 x 21 cannot be detectors: they run through lm_stage_depth_quantize, the same launcher on a
loose image, with LM_TUNE_DMEDIAN_VARIANT choosing the instantiation; 24 x 10 and 40 x 22 stand in for them as detectors.  The
16-slot detectors are those whose width is no multiple of 16 (16 x 8 takes the stage hook there): the batch calls of the colour
modality's strip kernels have only ever run on heights that are multiples of their strips, and this file is about the depth
modality.

Before anything runs on the GPU, `cases` asserts from the oracle alone that the inputs reach what the word arithmetic can get
wrong: every output label; for every rank k a window whose count of ranks <= k is exactly 12 and one where it is exactly 13 (the two
sides of the median's compare); a counter of the first three rows' sum at 15 and one of the last two rows' at 10 (the largest
values the carry-free average takes); windows clipped at every border and corner.  test_cases_cover_the_arithmetic is that
assertion on its own, without a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = [0, 1, 2, 4, 8, 16, 32, 64, 128]                                    # ranks 0..8
DETECTOR_SHAPES = [(16, 8), (24, 10), (24, 16), (40, 22), (72, 38)]          # (w, h): rows x cols a multiple of 16, even (T = 2)
STAGE_SHAPES = [(16, 8), (24, 11), (40, 21)]                                 # the hook takes any height
N_IMAGES = 16                                                                # per shape: one per slot of the smallest batch


def make_depth(w, h, seed):
    """Small tilted planes (one of eight slope directions per patch) in front of a far background (label 0), some patches far:
    a 5 x 5 window sees one to four patches, so the counts around the median take every value."""
    rng = np.random.default_rng(seed)
    depth = np.full((h, w), 2500, np.float64)                  # beyond the distance threshold
    ys, xs = np.mgrid[0:h, 0:w]
    ph, pw = int(rng.integers(5, 9)), int(rng.integers(5, 9))
    for py in range(0, h, ph):
        for px in range(0, w, pw):
            if rng.random() < 0.12:
                continue
            ang = (int(rng.integers(0, 8)) + 0.5) * np.pi / 4 + rng.normal(0, 0.05)
            slope = rng.uniform(1.0, 2.5)
            sl = (slice(py, min(py + ph, h)), slice(px, min(px + pw, w)))
            depth[sl] = 900 + slope * np.cos(ang) * (xs[sl] - px) + slope * np.sin(ang) * (ys[sl] - py)
    return depth.round().astype(np.uint16)


def raw_labels(depth, lut, dist_thr=2000, diff_thr=50):
    """The labels before the median: numpy restatement of the oracle's loop (the same integer sums, the same float32 operations in
    the same order).  The oracle has no hook for them; `cases` checks that oracle.median5 of these is oracle.depth_quantize."""
    h, w = depth.shape
    raw = np.zeros((h, w), np.uint8)
    if h < 12 or w < 12:
        return raw
    d = depth.astype(np.int64)
    ys, xs = np.mgrid[5:h - 6, 5:w - 6]
    c = d[ys, xs]
    A0, A1, A3, b0, b1 = (np.zeros_like(c) for _ in range(5))
    for jj in (-1, 0, 1):
        for ii in (-1, 0, 1):
            if ii == 0 and jj == 0:
                continue
            i, j = 5 * ii, 5 * jj
            delta = d[ys + j, xs + i] - c
            f = (np.abs(delta) < diff_thr).astype(np.int64)
            A0 += f * i * i; A1 += f * i * j; A3 += f * j * j; b0 += f * i * delta; b1 += f * j * delta
    det = A0 * A3 - A1 * A1
    ddx = A3 * b0 - A1 * b1
    ddy = -A1 * b0 + A0 * b1
    nx = (1150 * ddx).astype(np.float32); ny = (1150 * ddy).astype(np.float32); nz = (-det * c).astype(np.float32)
    ln = np.sqrt(nx * nx + ny * ny + nz * nz)
    ok = (ln > 0) & (c < dist_thr)
    inv = np.float32(1.0) / np.where(ln > 0, ln, np.float32(1.0))
    nx = nx * inv; ny = ny * inv; nz = nz * inv
    v1 = (nx * np.float32(10) + np.float32(10)).astype(np.int32)
    v2 = (ny * np.float32(10) + np.float32(10)).astype(np.int32)
    v3 = (nz * np.float32(20) + np.float32(20)).astype(np.int32)
    flat = v3 * 400 + v2 * 20 + v1
    inside = ok & (flat >= 0) & (flat < 8000)
    raw[5:h - 6, 5:w - 6] = np.where(inside, lut[np.clip(flat, 0, 7999)], 0)
    return raw


def window_counts(raw):
    """For every pixel's 5 x 5 window (BORDER_REPLICATE) and every rank k < 8: how many of its pixels have a rank <= k -- in the whole
    window, in its first three rows (A) and in its last two (B).  Arrays [8][h][w]."""
    h, w = raw.shape
    rank = np.where(raw == 0, 0, np.log2(np.maximum(raw, 1)).astype(np.int64) + 1)
    pad = np.pad(rank, 2, mode="edge")
    le = np.stack([(pad <= k).astype(np.int64) for k in range(8)])
    rows = sum(le[:, :, i:i + w] for i in range(5))                           # horizontal 5-sums of every padded row
    A = sum(rows[:, j:j + h] for j in range(3))
    B = sum(rows[:, j:j + h] for j in range(3, 5))
    return A + B, A, B


@pytest.fixture(scope="module")
def cases(orc):
    """{(w, h): [(depth, expected quantised image)] * N_IMAGES}, computed once; asserts the coverage the module docstring lists."""
    lut = orc.normal_lut()
    out = {}
    seen_labels, exact12, exact13, a15, b10 = set(), set(), set(), False, False
    for w, h in sorted(set(DETECTOR_SHAPES + STAGE_SHAPES)):
        # windows clipped at each border and at the corners exist, and the rows of a lane's first and last band are clipped ones
        assert w % 8 == 0 and w >= 5 and h >= 5
        out[(w, h)] = []
        for k in range(N_IMAGES):
            depth = make_depth(w, h, 1000 * w + 10 * h + k)
            exp = orc.depth_quantize(depth)
            raw = raw_labels(depth, lut)
            assert np.array_equal(orc.median5(raw), exp), (w, h, k)
            total, A, B = window_counts(raw)
            seen_labels |= set(np.unique(exp).tolist())
            exact12 |= {r for r in range(8) if (total[r] == 12).any()}
            exact13 |= {r for r in range(8) if (total[r] == 13).any()}
            # (not the all-zero window, whose counters are all full: windows that hold other ranks too)
            a15 |= bool(((A == 15) & (total < 25)).any())
            b10 |= bool(((B == 10) & (total < 25)).any())
            out[(w, h)].append((depth, exp))
    assert seen_labels == set(LABELS), sorted(seen_labels)
    assert exact12 == set(range(8)) and exact13 == set(range(8)), (sorted(exact12), sorted(exact13))
    assert a15 and b10
    return out


def test_cases_cover_the_arithmetic(cases):
    assert set(cases) == set(DETECTOR_SHAPES + STAGE_SHAPES)


def batch_slots():
    """The fewest slots that take the batch kernels: more than phase_max_slots (lm_detector_impl.h, enqueue_preprocess) and at least
    the 16 the planner's plan_depth_quantize (lm_host.cpp) asks for."""
    src = open(os.path.join(ROOT, "line-mod-pipeline_amd", "csrc", "lm_detector_impl.h")).read()
    m = re.search(r"int\s+phase_max_slots\s*=\s*(\d+)\s*;", src)
    assert m, "phase_max_slots not found in lm_detector_impl.h"
    return max(int(m.group(1)) + 1, 16)


# (batch calls of widths that are multiples of 16 run the colour modality's strip kernels: see the module docstring; test_stage_hook runs the
# batch median on 16 x 8)
RESIDENT = [(s, b) for s in DETECTOR_SHAPES for b in (False, True) if not (b and s[0] % 16 == 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,batch", RESIDENT, ids=["%dx%d-%s" % (s[0], s[1], "batch" if b else "one_slot") for s, b in RESIDENT])
def test_resident_frames(lm, cases, shape, batch):
    w, h = shape
    n = batch_slots() if batch else 1
    assert n <= N_IMAGES
    d = lm.Detector(color_only=False, width=w, height=h, T=[2], frame_slots=n)
    try:
        rng = np.random.default_rng(w * h)
        bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for k in range(n):
            d.upload_frame(k, bgr, cases[shape][k][0])
        if batch:
            _, cnt = d.match_batch(n, 80.0)                   # (an empty bank: the call is its pre-processing)
            assert not cnt.any()
        else:
            d.prepare_slot(0)
        for k in range(n):
            got = d.debug_read(k, 0, 0, 1).reshape(h, w)
            assert np.array_equal(got, cases[shape][k][1]), (shape, n, k, np.argwhere(got != cases[shape][k][1])[:4].tolist())
    finally:
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [1, 2], ids=["rows4", "rows16"])      # LM_TUNE_DMEDIAN_VARIANT: the few-frame / the batch instantiation
@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_stage_hook(lm, cases, shape, variant):
    d = lm.Detector(color_only=False)     # (the hooks take loose images of any size)
    try:
        d.set_tuning(lm.TUNE_DMEDIAN_VARIANT, variant)
        for k, (depth, exp) in enumerate(cases[shape]):
            got = d.stage_depth_quantize(depth)
            assert np.array_equal(got, exp), (shape, variant, k, np.argwhere(got != exp)[:4].tolist())
    finally:
        d.set_tuning(lm.TUNE_DMEDIAN_VARIANT, 0)
        d.close()


@pytest.mark.gpu
def test_code_table_through_the_tail(lm, orc):
    """k_dnormal's rank-code table (ensure_luts) has no read hook; what shows it is the label image: planes of all eight slope
    directions and a far patch give all nine labels through both kernels, and a substituted one-hot table that permutes the labels
    permutes the output."""
    d = lm.Detector(color_only=False)     # (the hooks take loose images of any size)
    try:
        ys, xs = np.mgrid[0:40, 0:72]
        depth = np.full((40, 72), 2500, np.uint16)
        for o in range(8):
            ang = (o + 0.5) * np.pi / 4
            sl = (slice(20 * (o // 4), 20 * (o // 4) + 20), slice(16 * (o % 4), 16 * (o % 4) + 16))
            depth[sl] = (900 + 1.8 * np.cos(ang) * (xs[sl] - xs[sl].min()) + 1.8 * np.sin(ang) * (ys[sl] - ys[sl].min())).round().astype(np.uint16)
        exp = orc.depth_quantize(depth)
        assert set(np.unique(exp).tolist()) == set(LABELS)
        assert np.array_equal(d.stage_depth_quantize(depth), exp)
        lut = orc.normal_lut()
        perm = np.zeros(256, np.uint8)
        for r in range(8):
            perm[1 << r] = 1 << ((3 * r + 5) % 8)
        d.set_normal_lut(perm[lut])
        exp2 = orc.depth_quantize(depth, lut=perm[lut])
        assert not np.array_equal(exp2, exp)
        assert np.array_equal(d.stage_depth_quantize(depth), exp2)
    finally:
        d.close()
