"""Every plane of every slot of every pre-processing route, bit for bit.

The single-stage hooks (tests/test_gpu_stages.py) run one image through one launch; the whole-route diffs run 640 x 480 and larger frames
of smooth content and look at three slots.  Here each row of tests/preprocess_routes.py is one call -- the few-frame phases, the batch
phases of colour-only and RGB-D detectors, the separate launches, shapes outside the fused routes, a slot range that starts at 3 -- at the
smallest shape that still has a partial strip, a tall image, a row wider than a wave, a batch that is a multiple of nothing; every slot
holds its own frame (noise, extremes, blocks, a scene, a rectangle on two borders, pixels at the weak threshold's edge, channel ties;
depth noise, steps at the gate, zero-length normals, the full u16 range).  What the rows claim -- route, kernels, geometry, contents -- is
proved on the CPU by tests/test_preprocess_routes_cpu.py.

For EVERY slot of the call, every level and modality: the quantised image (lm_debug_read 0) and the linear memories (2) equal the
oracle's, and the match list equals orc.Detector's.  Oracle planes are computed once per (shape, T, config, content) and shared."""
import numpy as np
import pytest

import preprocess_routes as pr
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

_refs = {}
_users = {}
for _c in pr.CASES:
    _users[_c.reference_key()] = _users.get(_c.reference_key(), 0) + 1


def _reference(orc, synth, case):
    key = case.reference_key()
    if key not in _refs:
        _refs[key] = pr.Reference(orc, synth, case)
    return _refs[key]


def _set_knobs(lm, d, knobs):
    for k, v in knobs.items():
        d.set_tuning(getattr(lm, "TUNE_" + k), v)


def _check_slot(d, case, ref, slot, when=""):
    _, _, planes, _ = ref.slot(slot)
    for key in pr.plane_keys(case):
        what, l, m = key
        got = d.debug_read(slot, what, l, m)
        if not np.array_equal(got, planes[key]):
            raise AssertionError("%s%s: slot %d (colour '%s'%s), %s of level %d, modality %d: %s" % (
                case.name, when, slot, pr.colour_kind(slot), ", depth '%s'" % pr.depth_kind(case, slot) if case.M == 2 else "",
                "quantised image" if what == 0 else "linear memories", l, m, pr.first_difference(case, key, got, planes[key])))


def _check_lists(case, ref, out, cnt, first):
    for k in range(case.n_slots):
        try:
            assert_matches_equal(out[k, :cnt[k]], ref.slot(first + k)[3])
        except AssertionError as e:
            raise AssertionError("%s: match list of slot %d (colour '%s'): %s" % (case.name, first + k, pr.colour_kind(first + k), e))


@pytest.mark.parametrize("name", [c.name for c in pr.CASES])
def test_route_planes(lm, orc, synth, name):
    case = pr.BY_NAME[name]
    ref = _reference(orc, synth, case)
    ref.prefetch(range(case.first_slot, case.first_slot + case.n_slots))
    w, h = case.size
    c = case.config
    d = lm.Detector(lm.default_config(color_only=(case.M == 1), width=w, height=h, T=case.T, frame_slots=case.total_slots, flags=c["flags"],
                                      weak_threshold=c["weak_threshold"], distance_threshold=c["distance_threshold"],
                                      difference_threshold=c["difference_threshold"]))
    try:
        lut = pr.normal_lut(orc, case.lut)
        if lut is not None:
            d.set_normal_lut(lut)
        d.add_class("c", ref.descs, ref.feats)
        first, n = case.first_slot, case.n_slots
        cap = 8192 if n <= 24 else 2048
        outside = [s for s in range(case.total_slots) if not first <= s < first + n] if first else []
        if outside:
            # the slots around the range are prepared by calls of their own (default knobs) and must read back unchanged afterwards
            for s in outside:
                d.upload_frame(s, *ref.slot(s)[:2])
            for lo, cnt_ in ((0, first), (first + n, case.total_slots - first - n)):
                d.match_batch_classes(lo, cnt_, case.threshold, [-1], cap_per_frame=cap)
            for s in outside:
                _check_slot(d, case, ref, s, " (before the call)")
        _set_knobs(lm, d, case.knobs)
        for s in range(first, first + n):
            d.upload_frame(s, *ref.slot(s)[:2])
        if first == 0:
            out, cnt = d.match_batch(n, case.threshold, cap_per_frame=cap)
        else:
            d.match_begin(1, first, n, case.threshold)
            out, cnt = d.match_end(1, cap_per_frame=cap, n_slots=n)
        for s in range(first, first + n):           # every slot of the call
            _check_slot(d, case, ref, s)
        _check_lists(case, ref, out, cnt, first)
        for s in outside:
            _check_slot(d, case, ref, s, " (outside the call's range, after it)")
    finally:
        _set_knobs(lm, d, pr.KNOB_DEFAULTS)
        d.close()
        _users[case.reference_key()] -= 1
        if _users[case.reference_key()] <= 0:       # the last row of a reference: its frames and planes are not kept for the rest of the session
            _refs.pop(case.reference_key(), None)
