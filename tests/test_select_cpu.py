"""CPU side of the feature selection on the GPU.  tests/select_reference.py restates select_color / select_depth
in numpy; tests/cpp/select_dump.cpp links csrc/lm_extract.cpp and prints what the project's own host code selects from the same crafted
lists (tests/select_fixtures.py): the two must be equal, feature for feature, which pins the reference the GPU tests use without a
GPU.  The ABI: the version string names 0.11, the binding declares the new entry points, and they fail with LM_ERR_NO_DEVICE here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import select_fixtures as SF
import select_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")


def bits(v):
    return int(np.float32(v).view(np.uint32))


def host_select(exe, lists):
    """What lm_extract.cpp selects from each list: FEATURE rows or None."""
    lines = []
    for l in lists:
        lines.append("%d %d %d %d" % (l["modality"], len(l["labels"]), l["want"], bits(l["area"] or 0.0)))
        sb = l["scores"].view(np.uint32)
        lines += ["%d %d %d %d" % (x, y, lab, s) for (x, y), lab, s in zip(l["xy"].tolist(), l["labels"].tolist(), sb.tolist())]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    tok = iter(r.stdout.split())
    out = []
    for _ in lists:
        n = int(next(tok))
        out.append(None if n < 0 else np.array([[int(next(tok)) for _ in range(3)] for _ in range(n)], np.int32).reshape(n, 3))
    return out


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("select") / "select_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "select_dump.cpp"), os.path.join(CSRC, "lm_extract.cpp")])
    return exe


def reference(l):
    return SR.select(l["modality"], l["xy"], l["labels"], l["scores"], l["want"], l["area"])


def assert_same(got, exp, name):
    assert (got is None) == (exp is None), name
    if exp is not None:
        assert got.shape == exp.shape and np.array_equal(got, exp), name


@pytest.mark.parametrize("which", ["colour", "depth"])
def test_numpy_reference_equals_host_selection(dump_exe, which):
    cases = SF.colour_cases() if which == "colour" else SF.depth_cases()
    host = host_select(dump_exe, list(cases.values()))
    for (name, l), h in zip(cases.items(), host):
        assert_same(reference(l), h, name)
        if h is not None:
            assert len(h) == l["want"]
    assert sum(h is None for h in host) == 2        # the two too-few lists, nothing else


@pytest.mark.parametrize("modality", [0, 1])
def test_numpy_reference_equals_host_selection_on_the_batch(dump_exe, modality):
    lists = SF.batch_lists(modality, 96 if modality == 0 else 24, 77 + modality)
    host = host_select(dump_exe, lists)
    for k, (l, h) in enumerate(zip(lists, host)):
        assert_same(reference(l), h, "list %d" % k)
    assert any(h is None for h in host) and any(h is not None for h in host)


def test_crafted_lists_hold_what_they_are_for():
    """The properties the lists are built for: ties in the sort, ties that exist only after the division, walks that relax."""
    c, d = SF.colour_cases(), SF.depth_cases()
    assert len(np.unique(c["stable_all_equal"]["scores"])) == 1
    assert len(np.unique(c["len_70001_ties"]["scores"])) == 16 and len(c["len_70001_ties"]["labels"]) == 70001
    assert SR.initial_distance(0, 1600, 63) == 26 and SR.initial_distance(0, 64, 63) == 2
    l = d["division_ties"]
    cnt = np.bincount(l["labels"], minlength=8)
    q = (l["scores"] / cnt[l["labels"]].astype(np.float32)).astype(np.float32)
    assert set(np.unique(q[np.isin(l["labels"], [0, 1])])) == {np.float32(0.5)} and set(np.unique(q[np.isin(l["labels"], [2, 3, 4])])) == {np.float32(1.0)}
    assert len(np.unique(l["scores"][np.isin(l["labels"], [0, 1])])) == 2
    assert SR.initial_distance(1, 21, 16, 36.0) == 3.0
    f = SR.initial_distance(1, 21, 20, 50.0)
    assert f != np.floor(f)
    for l in list(c.values()) + list(d.values()):       # row-major order, distinct positions
        key = l["xy"][:, 1].astype(np.int64) * 4096 + l["xy"][:, 0]
        assert np.all(np.diff(key) > 0)


def test_version_and_binding(lm):
    lib = lm.load_library()
    v = lib.lm_version()
    assert b"0.11" in v and b"lm_add_templates_slots" in v and b"0.10" in v
    for n in ("lm_add_templates_slots", "lm_stage_select"):
        assert n in lm.EXPORTS and getattr(lib, n).argtypes is not None
    assert C.sizeof(lm.ObjectMask) == 32 and lm.ObjectMask.on_device.offset == 16 and lm.ObjectMask.rule.offset == 24


def _has_gpu(lm):
    d = lm.Detector(color_only=True, width=64, height=64, T=[2, 8])
    try:
        d.stage_pyrdown(np.zeros((8, 8, 3), np.uint8))
        return True
    except lm.LinemodError:
        return False
    finally:
        d.close()


def test_entry_points_fail_loudly_without_gpu(lm):
    if _has_gpu(lm):
        pytest.skip("a HIP device is present")
    d = lm.Detector(color_only=True, width=64, height=64, T=[2, 8])
    l = SF.colour_cases()["n_eq_want_eq_1"]
    for call in (lambda: d.add_templates_slots("x", 0, [None]),
                 lambda: d.stage_select(0, [(l["xy"], l["labels"], l["scores"])], [1])):
        with pytest.raises(lm.LinemodError) as e:
            call()
        assert e.value.code == lm.LM_ERR_NO_DEVICE
    # argument errors that need no device come first
    with pytest.raises(lm.LinemodError) as e:
        d.add_templates_slots("x", 0, [])
    assert e.value.code == lm.LM_ERR_INVALID
    d.close()
