"""The best-pose check of the ICP branch without a GPU (tests/icp_verify_reference.py): the two-pass erosion against
the clipped 5x5 window the kernel computes, the selection rule's quirks on crafted lists of means -- in the numpy restatement and in the
facade's HighLevelLinemodIcp::selectBestMatch -- and the binding's declarations."""
import os
import subprocess

import numpy as np
import pytest

import icp_verify_reference as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 3), (64, 16), (65, 17), (70, 37)]      # (w, h)

# (name, means, accepted, best index)
SELECTION = [
    ("a first pose with mean 0 is kept and accepted", [0.0], True, 0),
    ("nothing undercuts a best of 0", [0.0, 5.0, 3.0], True, 0),
    ("a later mean of 0 is skipped", [20.0, 0.0, 10.0], True, 2),
    ("a later mean of 0 alone changes nothing", [20.0, 0.0], True, 0),
    ("34.9 undercuts a truncated best of 35", [35.7, 34.9], True, 1),
    ("35.2 does not undercut a truncated best of 35", [35.7, 35.2], True, 0),
    ("35.7 truncates to 35 and is accepted", [35.7], True, 0),
    ("36.0 is rejected", [36.0], False, 0),
    ("the comparison is with the truncated best: 10.5 after 10.9 is not below 10", [10.9, 10.5], True, 0),
    ("a rejected first pose is replaced by a good later one", [100.0, 50.0, 20.0, 30.0], True, 2),
    ("all poor", [100.0, 60.0], False, 1),
    ("an empty list is rejected", [], False, 0),
]


def _masks(w, h, rng):
    out = [np.ones((h, w), bool), np.zeros((h, w), bool)]
    for p in (0.02, 0.1, 0.3):
        out.append(rng.random((h, w)) >= p)
    # holes on every border and in every corner
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)):
        m = np.ones((h, w), bool)
        m[y, x] = False
        out.append(m)
    # set pixels touching every border in an otherwise unset image
    m = np.zeros((h, w), bool)
    m[:3, :] = m[-3:, :] = True
    m[:, :3] = m[:, -3:] = True
    out.append(m)
    return out


@pytest.mark.parametrize("w,h", SIZES)
def test_two_erosions_equal_the_clipped_5x5_window(w, h):
    rng = np.random.default_rng(1000 * w + h)
    for m in _masks(w, h, rng):
        two = V.erode3(V.erode3(m))
        assert np.array_equal(two, V.window5(m))
        if m.all():
            assert two.all()                                     # the border does not erode: a full frame stays full
            assert not V.erode3_border_erodes(m).all()               # ... which a zero border would not


def test_verify_counts_by_hand():
    render = np.full((9, 9), 1000, np.uint16)
    scene = np.full((9, 9), 1010, np.uint16)
    assert V.verify(render, scene) == (81, 810, 10.0)
    scene[4, 4] = 600                                            # not above 600: a 5x5 hole
    assert V.verify(render, scene) == (81 - 25, 10 * (81 - 25), 10.0)
    render[:] = 1                                                # not rendered
    assert V.verify(render, scene) == (0, 0, 0.0)


@pytest.mark.parametrize("name,means,accepted,best", SELECTION, ids=[s[0] for s in SELECTION])
def test_selection_rule_reference(name, means, accepted, best):
    ok, idx = V.select_best(means)
    assert ok == accepted
    if accepted:
        assert idx == best


def test_selection_rule_of_the_facade_equals_the_reference(lm, tmp_path):
    """HighLevelLinemodIcp::selectBestMatch, the loop estimateBestMatch and estimateBestMatchGpu share, on the crafted lists and on
    random ones."""
    exe = str(tmp_path / "icp_select")
    libdir = os.path.dirname(lm.LIB_PATH)
    host = os.path.join(ROOT, "line-mod-pipeline_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "icp_select.cpp"),
                           os.path.join(host, "HighLevelLinemod.cpp"), os.path.join(host, "PostProcess.cpp"),
                           os.path.join(host, "TemplateGenerator.cpp"), "-L" + libdir, "-llinemod_hip", "-lpthread",
                           "-Wl,-rpath," + libdir])
    rng = np.random.default_rng(5)
    lists = [s[1] for s in SELECTION]
    for _ in range(40):
        n = int(rng.integers(1, 7))
        vals = np.round(rng.uniform(30, 40, n), 1)
        vals[rng.random(n) < 0.2] = 0.0
        lists.append([float(v) for v in vals])
    args = [",".join(repr(v) for v in l) if l else "-" for l in lists]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lists)
    for l, line in zip(lists, out):
        ok, idx = V.select_best(l)
        got_ok, got_idx = (int(v) for v in line.split())
        assert bool(got_ok) == ok, (l, line)
        assert got_idx == (idx if ok else 65535), (l, line)      # a rejected group leaves the caller's index alone


def test_binding_declares_verify_entry_points(lm):
    lib = lm.load_library()
    for name in ("lm_stage_icp_verify_host", "lm_icp_verify", "lm_stage_icp_verify_counts"):
        assert name in lm.EXPORTS
        assert hasattr(lib, name)
    assert b"0.8" in lib.lm_version() and b"lm_icp_verify" in lib.lm_version()
    import ctypes as C
    assert C.sizeof(lm.IcpVerifyQuery) == 72
    assert lm.ICP_VERIFY_RESULT_DTYPE.itemsize == 24
    assert hasattr(lm.Detector, "icp_verify") and hasattr(lm.Detector, "icp_verify_counts")
