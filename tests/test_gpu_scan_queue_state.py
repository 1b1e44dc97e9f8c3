"""The survivor queue's state across scan launches (k_scan1, LM_TUNE_SCAN_FORM 2): a lane's queue has two sets of counters, a launch counts
into one and its k_scan1_exact zeroes the other; scan variant 256 (the waves sum their survivors themselves) re-arms both and runs no
k_scan1_exact, and the lane still moves on to the other set.  Two sequences the rest of the suite does not cross, against the oracle:
variant 256 followed by normal launches, and class lists of several ranges (several scan launches of one call on one lane's queue) on
two lanes at once."""
import numpy as np
import pytest

from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

W, H, T, SLOTS, THR = 128, 96, [2, 8], 16, 80.0


@pytest.fixture(scope="module")
def scene(lm, orc, synth):
    d = lm.Detector(lm.default_config(color_only=True, width=W, height=H, T=T, frame_slots=SLOTS))
    o = orc.Detector(color_only=True, T=T)
    frames = [synth.make_frame(W, H, seed=4100 + k, n_shapes=12)[0] for k in range(2)]
    o.prepare(frames[0], None)
    q = {(l, 0): o.stage(0, l, 0).reshape(H >> l, W >> l) for l in range(2)}
    for c in range(3):
        descs, feats, _ = synth.make_bank(14, 1, 2, seed=4200 + c, quantized=q, crop_fraction=0.5, frame_size=(W, H), T0=T[0], num_features=24,
                                          size_range=(16, 32))
        d.add_class("c%d" % c, descs, feats); o.add_class("c%d" % c, descs, feats)
    exp = {(k, c): o.match(frames[k], None, THR, class_idx=c, threads=4, cap=1 << 18) for k in range(2) for c in (-1, 0, 1, 2)}
    assert sum(len(exp[0, c]) for c in (0, 1, 2)) > 0
    d.set_tuning(lm.TUNE_SCAN_FORM, 2)
    for k in range(SLOTS):
        d.upload_frame(k, frames[k % 2], None)
    yield d, orc, exp
    d.close()


def _check_all(d, exp):
    before = d.get_scan_form_stats()
    got, cnt = d.match_batch(SLOTS, THR, cap_per_frame=1 << 14)
    after = d.get_scan_form_stats()
    assert after[0] - before[0] == after[1] - before[1] >= 1 and after[3] > 0        # k_scan1 took every scan launch
    for k in range(SLOTS):
        assert_matches_equal(got[k, :cnt[k]], exp[k % 2, -1])


def test_variant_256_then_normal_launches(scene):
    """Variant 256 flips the lane's counter set without a k_scan1_exact behind it; the next two normal launches each count into a zeroed set."""
    d, _, exp = scene
    d.set_scan_variant(256)
    _check_all(d, exp)
    d.set_scan_variant(0)
    _check_all(d, exp)
    _check_all(d, exp)


def test_two_ranges_per_lane_on_two_lanes(scene):
    """Classes {0, 2} are two item ranges: two scan launches of one call, one after the other on the lane's queue; lane 1 runs another list
    on its own queue meanwhile."""
    d, orc, exp = scene
    half = SLOTS // 2
    want = {(k, "02"): orc.merge([exp[k, 0], exp[k, 2]]) for k in range(2)}
    for lists in (([0, 2], [1]), ([1], [0, 2]), ([0, 2], [0, 2])):
        for lane in (0, 1):
            d.match_begin_classes(lane, lane * half, half, THR, lists[lane])
        for lane in (0, 1):
            got, cnt = d.match_end(lane, cap_per_frame=1 << 14, n_slots=half)
            for k in range(half):
                e = exp[k % 2, 1] if lists[lane] == [1] else want[k % 2, "02"]
                assert_matches_equal(got[k, :cnt[k]], e)
