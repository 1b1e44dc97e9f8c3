"""The feature selection on the GPU (csrc/lm_k_select.hip): lm_stage_select on the crafted lists of
tests/select_fixtures.py against the numpy restatement of select_color / select_depth (tests/select_reference.py, which
tests/test_select_cpu.py holds to csrc/lm_extract.cpp).  Every comparison is for equality: the same features in the same order, or
"fewer than want" for the same lists.  The references are computed once per module."""
import numpy as np
import pytest

import select_fixtures as SF
import select_reference as SR

pytestmark = pytest.mark.gpu

COLOUR, DEPTH = SF.colour_cases(), SF.depth_cases()
_REF = {}


def reference(key, l):
    if key not in _REF:
        _REF[key] = SR.select(l["modality"], l["xy"], l["labels"], l["scores"], l["want"], l["area"])
    return _REF[key]


@pytest.fixture(scope="module")
def det(lm):
    d = lm.Detector(color_only=True, width=64, height=64, T=[2, 8])
    yield d
    d.close()


def run(d, lists):
    m = lists[0]["modality"]
    return d.stage_select(m, [(l["xy"], l["labels"], l["scores"]) for l in lists], [l["want"] for l in lists],
                          None if m == 0 else [l["area"] for l in lists])


def rows(f):
    return None if f is None else np.stack([f["x"], f["y"], f["label"]], 1).astype(np.int32)


def assert_same(got, exp, name):
    assert (got is None) == (exp is None), name
    if exp is not None:
        assert got.shape == exp.shape and np.array_equal(got, exp), "%s: first difference at feature %d" % (
            name, int(np.flatnonzero((got != exp).any(1))[0]) if got.shape == exp.shape else -1)


@pytest.mark.parametrize("name", list(COLOUR))
def test_colour_list(det, name):
    l = COLOUR[name]
    got = rows(run(det, [l])[0])
    assert_same(got, reference(("c", name), l), name)
    if name.startswith("too_few"):
        assert got is None


@pytest.mark.parametrize("name", list(DEPTH))
def test_depth_list(det, name):
    l = DEPTH[name]
    got = rows(run(det, [l])[0])
    assert_same(got, reference(("d", name), l), name)
    if name.startswith("too_few"):
        assert got is None


def test_too_few_writes_no_features(lm, det):
    """n == want - 1 and n == 0: n_out = -1 and the caller's feature rows stay as they were."""
    import ctypes as C
    lists = [COLOUR["too_few_want_minus_1"], COLOUR["n_eq_want_31"], COLOUR["too_few_empty"]]
    offs = np.cumsum([0] + [len(l["labels"]) for l in lists]).astype(np.int32)
    xy = np.concatenate([l["xy"] for l in lists]); lab = np.concatenate([l["labels"] for l in lists]); sc = np.concatenate([l["scores"] for l in lists])
    want = np.array([l["want"] for l in lists], np.int32)
    feats = np.full((3, 63, 3), -77, np.int32)
    nout = np.full(3, 5, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert det.lib.lm_stage_select(det.h, 0, 3, p(offs), p(xy), p(lab), p(sc), p(want), None, p(feats), p(nout)) == lm.LM_OK
    assert nout.tolist() == [-1, 31, -1]
    assert np.all(feats[0] == -77) and np.all(feats[2] == -77) and np.all(feats[1, 31:] == -77)
    assert np.array_equal(feats[1, :31], reference(("c", "n_eq_want_31"), lists[1]))


@pytest.mark.parametrize("modality,count", [(0, 96), (1, 24)])
def test_batch_equals_one_list_per_call(det, modality, count):
    lists = SF.batch_lists(modality, count, 77 + modality)
    together = [rows(f) for f in run(det, lists)]
    assert any(t is None for t in together) and any(t is not None for t in together)
    for k, l in enumerate(lists):
        alone = rows(run(det, [l])[0])
        assert_same(together[k], alone, "list %d of the batch against the list alone" % k)
        assert_same(together[k], reference((modality, k), l), "list %d of the batch against the reference" % k)


def test_results_repeat(det):
    l = COLOUR["len_70001_ties"]
    a, b = rows(run(det, [l])[0]), rows(run(det, [l])[0])
    assert np.array_equal(a, b)


def test_hook_refuses_bad_lists(lm, det):
    l = COLOUR["n_eq_want_31"]
    one = [(l["xy"], l["labels"], l["scores"])]
    for bad in (lambda: det.stage_select(2, one, [31]),
                lambda: det.stage_select(0, one, [0]),
                lambda: det.stage_select(0, one, [64]),
                lambda: det.stage_select(1, one, [31]),                                   # depth without areas
                lambda: det.stage_select(0, [(l["xy"], l["labels"] + 8, l["scores"])], [31]),
                lambda: det.stage_select(0, [(l["xy"], l["labels"], -l["scores"])], [31])):
        with pytest.raises(lm.LinemodError) as e:
            bad()
        assert e.value.code == lm.LM_ERR_INVALID
