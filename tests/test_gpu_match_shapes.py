"""Whole matches at awkward frame shapes, and k_refine's edge rules.

Every other whole-match test runs at a shape whose level-0 pitch W = width / T is a multiple of 4, so that plan_match (lm_host.cpp) picks
k_refine<., true> and the general form of rf_patch -- per-lane aligned base and byte shift -- is never launched.  Here:

  1. lists at shapes with W % 4 = 1, 2, 3 (two and three levels), widths that are no multiple of 8, T = 3, 6, 7, a scanned level without
     nibble memories, and a nibble-capable scanned level under a non-W4 level 0 with every scan form forced -- quantised images, scan
     candidates and lists through one frame, a batch of 8 (k_refine_plan) and a batch of 16 (the batch pre-processing kernels);
  2. the refinement's clamp below zero at sizes where max_x, max_y are no multiples of T: x / T truncates toward zero as in C, and a
     flooring division gives ANOTHER list (shown on the CPU by the numpy reference with its division replaced);
  3. thresholds that equal an attainable score: `sim < threshold` keeps equality, one float further drops it.

Expected lists: tests/match_shapes.py -- the oracle and the numpy restatement tests/masked_reference.py, which must agree first; computed
once per scene and shared.  All comparisons at tolerance 0."""
import numpy as np
import pytest

import match_shapes as ms
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

THRESHOLDS = (60.0, 80.0)
REFINE_WAVES = 1024      # blocks_per_slot * 4 of the plan table (MatchPlan::blocks_per_slot = 256): a list longer than this takes the pair route

_scenes = {}


def _scene(orc, synth, name):
    """The table scene of `name`, made once per module (frames, quantised pyramids, bank, lists as they are first asked for)."""
    if name not in _scenes:
        _scenes[name] = ms.table_scene(orc, synth, ms.BY_NAME[name])
    return _scenes[name]


def _upload_alternating(d, s, n):
    for k in range(n):
        d.upload_frame(k, s.bgr(k % 2), s.depth(k % 2))


def _check_batch(d, s, n, thr):
    _upload_alternating(d, s, n)
    out, cnt = d.match_batch(n, thr, cap_per_frame=4096)
    for k in range(n):
        assert_matches_equal(out[k, :cnt[k]], s.expected(k % 2, thr))


def _check_stages(d, s, slot=0):
    """Slot `slot` holds frame A, prepared: its quantised images are the oracle's, level by level and modality by modality."""
    c = s.case
    for l in range(c.L):
        w, h = c.level_size(l)
        for m in range(c.M):
            assert np.array_equal(d.debug_read(slot, 0, l, m).reshape(h, w), s.quant[0][(l, m)]), ("quantised image", c.name, l, m)


# ---- 1. lists at awkward shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in ms.CASES])
def test_lists_at_awkward_shapes(lm, orc, synth, name):
    """pitch W per level / what the row reaches / k_refine instantiations by plan_match's rule (level L-2 .. 0) / oracle = numpy list
    lengths at thresholds 60, 80 of frame A (frame B, A rolled by (7, 13), gives 16 or more everywhere):
      rgbd-212x160-T4.2     53, 53        W % 4 = 1, byte scan since nibble_supported() is false   <true,false>                  26 / 21
      rgbd-216x160-T4.4     54, 27        W % 4 = 2                                                <true,false>                  44 / 21
      color-220x160-T4.2    55, 55        W % 4 = 3                                                <true,false>                  36 / 20
      rgbd-210x160-T5.5     42, 21        the reference's T0 = 5, width % 4 = 2                    <true,false>                  40 / 25
      color-210x160-T2.5    105, 21       odd pitch at T0 = 2                                      <true,false>                  93 / 32
      rgbd-424x320-T4.4.2   106, 53, 53   both general forms in one call                           <false,false> <true,false>    41 / 17
      color-424x320-T2.2.2  212, 106, 53  W4 last level behind a non-W4 middle level               <false,false> <true,true>     98 / 60
      rgbd-240x168-T3.6     80, 20        T outside {2, 4, 5, 8}; W4 (the control)                 <true,true>                  151 / 34
      color-224x224-T7.7    32, 16        T = 7                                                    <true,true>                   87 / 26
      rgbd-240x320-T8.5     30, 24        nibble-capable scanned level under a non-W4 level 0      <true,false>                  50 / 24
      color-240x320-T8.5    30, 24        the same, one modality                                   <true,false>                  66 / 34"""
    case = ms.BY_NAME[name]
    ms.check_properties(case)
    s = _scene(orc, synth, name)
    for f in (0, 1):
        for thr in THRESHOLDS:
            assert len(s.expected(f, thr)) >= 10, (name, f, thr)
    d = s.detector(lm, slots=16)
    # pre-processing and scan alone, so that a list mismatch below says which stage broke
    d.upload_frame(0, s.bgr(0), s.depth(0))
    d.prepare_slot(0)
    _check_stages(d, s)
    for thr in THRESHOLDS:
        assert np.array_equal(d.stage_scan(0, thr), s.scan_expected(0, thr)), ("scan candidates", name, thr)
    for thr in THRESHOLDS:
        for f in (0, 1):                                          # one frame: an entry per wave
            assert_matches_equal(d.match(s.bgr(f), s.depth(f), thr), s.expected(f, thr))
        _check_batch(d, s, 8, thr)                                # k_refine_plan: pairs and odd tails over the XCD lists
        _check_batch(d, s, 16, thr)                               # the batch pre-processing kernels
    d.close()


def test_pair_route_on_one_frame(lm, orc, synth):
    """Without a plan a wave takes list entries in pairs only when the frame's list is longer than the launch has waves.  Threshold 20 on
    the W % 4 = 1 scene leaves 2423 scan candidates (odd: the last entry goes alone) and 183 matches."""
    name = "rgbd-212x160-T4.2"
    case = ms.BY_NAME[name]
    assert case.pitch(0) % 4 != 0
    s = _scene(orc, synth, name)
    thr = 20.0
    exp_c = s.scan_expected(0, thr)
    assert len(exp_c) > REFINE_WAVES
    exp = s.expected(0, thr)
    assert len(exp) >= 10
    d = s.detector(lm, slots=2)
    d.upload_frame(0, s.bgr(0), s.depth(0))
    d.prepare_slot(0)
    cands = d.stage_scan(0, thr)
    assert len(cands) > REFINE_WAVES
    assert np.array_equal(cands, exp_c)
    assert_matches_equal(d.match(s.bgr(0), s.depth(0), thr, cap=1 << 16), exp)
    assert d.last_counts(0)[0] == len(exp_c)
    d.close()


# what lm_get_scan_form_stats' "lanes per frame of the last scan launch" says after a launch of the forced form
_FORM_RAN = {1: lambda st: st == 0,                 # k_scan4 (the nibble scan)
             2: lambda st: 0 < st < 1000,           # k_scan1: 1 .. 64 lanes per frame
             3: lambda st: st >= 1000}              # k_scanl: 1000 + workgroups per frame


@pytest.mark.parametrize("form", [1, 2, 3])
@pytest.mark.parametrize("name", ["rgbd-240x320-T8.5", "color-240x320-T8.5"])
def test_forced_scan_forms_feed_the_general_refine(lm, orc, synth, name, form):
    """k_scan4, k_scan1 and k_scanl (LM_TUNE_SCAN_FORM 1, 2, 3) on the 120 x 160 scanned level (24 columns, nibble-capable; its planes,
    19200 bits per orientation, fit k_scanl's LDS image) in front of k_refine<true,false>.  The library declines none of the three at
    this shape: each launch is asserted to have been of the forced form."""
    case = ms.BY_NAME[name]
    ms.check_properties(case)
    s = _scene(orc, synth, name)
    d = s.detector(lm, slots=8)
    d.set_tuning(lm.TUNE_SCAN_FORM, form)
    d.upload_frame(0, s.bgr(0), s.depth(0))
    d.prepare_slot(0)
    _check_stages(d, s)
    for thr in THRESHOLDS:
        assert np.array_equal(d.stage_scan(0, thr), s.scan_expected(0, thr)), ("scan candidates", name, form, thr)
        assert _FORM_RAN[form](d.get_scan_form_stats()[3]), (name, form, d.get_scan_form_stats())
    for thr in THRESHOLDS:
        before = d.get_scan_form_stats()
        assert_matches_equal(d.match(s.bgr(0), s.depth(0), thr), s.expected(0, thr))
        _check_batch(d, s, 8, thr)
        after = d.get_scan_form_stats()
        assert after[1] - before[1] >= 2 and _FORM_RAN[form](after[3]), (name, form, before, after)
        assert (after[0] - before[0] == after[1] - before[1]) if form >= 2 else (after[0] == before[0]), (name, form, before, after)
    d.close()


# ---- 2. the clamp below zero -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tmpl_size,max_xy,n_matches", [
    ("rgbd-212x160-T4.2", (190, 138), (-10, -10), 10),
    ("rgbd-210x160-T5.5", (178, 126), (-8, -6), 12),
    ("rgbd-424x320-T4.4.2", (402, 298), (-10, -10), 12),
])
def test_refine_clamp_below_zero_truncates(lm, orc, synth, name, tmpl_size, max_xy, n_matches):
    """max_x = w - tw - 8 T and max_y are negative and no multiples of T0, so every candidate refines at (max_x, max_y) with features
    shifted out of the frame (the zero-block reads), and bx = max_x / T - 8 differs between C's truncating division and a flooring one
    (a reciprocal multiply that is right for x >= 0 only).  Oracle = numpy (truncating): 10, 12, 12 matches at threshold 0; the numpy
    reference with floor division gives a different list in all three cases.  The GPU equals the truncating one."""
    case = ms.BY_NAME[name]
    w, h = case.size
    T0 = case.T[0]
    assert (w - tmpl_size[0] - 8 * T0, h - tmpl_size[1] - 8 * T0) == max_xy
    assert all(v < 0 and v % T0 != 0 for v in max_xy)
    s = ms.clamp_scene(orc, synth, case, tmpl_size)
    exp = s.expected(0, 0.0)                                     # oracle == numpy with C's division
    assert len(exp) == n_matches
    floored = s.numpy_list(0, 0.0, div=ms.floor_div)
    assert floored.tobytes() != exp.tobytes()                    # the case tells the two divisions apart
    d = s.detector(lm, slots=8)
    d.upload_frame(0, s.bgr(0), s.depth(0))
    d.prepare_slot(0)
    assert np.array_equal(d.stage_scan(0, 0.0), s.scan_expected(0, 0.0))
    assert_matches_equal(d.match(s.bgr(0), s.depth(0), 0.0), exp)
    for k in range(8):
        d.upload_frame(k, s.bgr(0), s.depth(0))
    out, cnt = d.match_batch(8, 0.0)
    for k in range(8):
        assert_matches_equal(out[k, :cnt[k]], exp)
    d.close()


# ---- 3. threshold equal to a score -------------------------------------------------------------------------------------------------
_equal = {}


def _kept_scores(s):
    """Similarities s of the list at threshold 50 (frame A) for which the list at threshold s still holds an entry with similarity == s
    (the others lose theirs to the scan's raw threshold, whose float expression rounds the other way), each with the next float above."""
    if "kept" not in _equal:
        base = s.expected(0, 50.0)
        kept = []
        for v in sorted(set(float(x) for x in base["similarity"])):
            # (chosen with the oracle alone -- 35 distinct values; the kept ones are then confirmed by both references in expected())
            if np.any(s.oracle_list(0, v)["similarity"] == np.float32(v)):
                kept.append((v, float(np.nextafter(np.float32(v), np.float32(200)))))
        _equal["kept"] = kept
    return _equal["kept"]


@pytest.mark.parametrize("n_frames", [1, 8])
def test_threshold_equal_to_a_score(lm, orc, synth, n_frames):
    """`sim < threshold` drops, equality keeps -- in the scan's raw threshold, in k_refine's pruning test `reach < threshold` and in the final
    filter.  On the CPU six scores of the 210 x 160 [5, 5] RGB-D scene survive at their own value (52.604168, 54.6875 with two entries,
    55.729168, 56.770832, 76.5625, 77.604164); the list at the next float above lacks them.  One frame and a batch of 8 (frames A, B)."""
    name = "rgbd-210x160-T5.5"
    s = _scene(orc, synth, name)
    kept = _kept_scores(s)
    assert len(kept) >= 3, kept
    for v, up in kept:
        assert np.float32(up) > np.float32(v)
        at, above = s.expected(0, v), s.expected(0, up)
        assert np.any(at["similarity"] == np.float32(v)) and not np.any(above["similarity"] == np.float32(v))
        assert at.tobytes() != above.tobytes()                   # the two thresholds are told apart
    d = s.detector(lm, slots=8)
    if n_frames == 1:
        d.upload_frame(1, s.bgr(0), s.depth(0))
        d.prepare_slot(1)
    for v, up in kept:
        for thr in (v, up):
            if n_frames == 1:
                assert np.array_equal(d.stage_scan(1, thr), s.scan_expected(0, thr)), ("scan candidates", thr)
                assert_matches_equal(d.match(s.bgr(0), s.depth(0), thr), s.expected(0, thr))
            else:
                _check_batch(d, s, 8, thr)
    d.close()
