"""The route table of tests/preprocess_routes.py, proved on the CPU with the planner and the oracle alone: every row's route, kernels and
geometry are what plan_preprocess (lm_host.cpp) plans for the row's call; the rows together launch every name of lmh::pre_kernel_name but
a justified list of exceptions; the two CPU references of the planes agree on every content kind at every shape; the contents have what
they claim.  tests/test_gpu_preprocess_routes.py then asks the GPU for the same planes.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import preprocess_routes as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """({row name: (route, [(kernel, param, grid)])}, every kernel name) from tests/cpp/preprocess_route_dump.cpp, built with g++."""
    exe = str(tmp_path_factory.mktemp("route_dump") / "preprocess_route_dump")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "preprocess_route_dump.cpp"), os.path.join(CSRC, "lm_host.cpp"), "-lz"])
    names = subprocess.run([exe, "--kernels"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    rows = "".join(c.plan_line() + "\n" for c in pr.CASES)
    out = subprocess.run([exe], input=rows, capture_output=True, text=True, timeout=60, check=True).stdout
    got = {}
    for ln in out.splitlines():
        name, route, steps = ln.split("|", 2)
        got[name] = (route, pr.parse_plan(steps))
    assert set(got) == set(pr.BY_NAME)
    return got, names


_refs = {}


def _reference(orc, synth, case):
    key = case.reference_key()
    if key not in _refs:
        _refs[key] = pr.Reference(orc, synth, case)
    return _refs[key]


def _distinct_references():
    seen = {}
    for c in pr.CASES:
        seen.setdefault(c.reference_key(), c)
    return list(seen.values())


def test_every_row_plans_what_it_claims(plans):
    got, _ = plans
    bad = []
    for c in pr.CASES:
        try:
            pr.check_claims(c, *got[c.name])
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)
    # the claims the table exists for are made by some row
    claimed = {f for c in pr.CASES for f in c.flags}
    for f in ("partial_strip0", "partial_strip1", "half_strip1", "tall", "one_band1", "grad_row_gt62", "blur_row_gt62", "n_not_mult4", "n_odd", "one_frame",
              "first_slot_nonzero", "lm_pitch80", "row_bytes1_not32", "w_8_not_16", "w_not_8", "three_levels", "interleave", "no_interleave", "lut_bytes",
              "weak_off_integer", "depth_full_range", "per_pixel_taps", "double_products", "slots_gt256"):
        assert f in claimed, f
    assert {c.route for c in pr.CASES} == {"phases", "batch_phases", "separate"}


def test_rows_cover_every_kernel_of_the_planner(plans):
    """The union of the rows' launches is the whole pre_kernel_name list but the exceptions; an exception is run by no row, says why, and
    names a test of the suite that diffs the planes of resident slots."""
    got, names = plans
    assert len(names) == len(set(names)) and len(names) >= 57
    ran = {k for _, steps in got.values() for k, _, _ in steps}
    assert ran <= set(names)
    assert set(pr.EXCEPTIONS) <= set(names)
    assert not (ran & set(pr.EXCEPTIONS)), sorted(ran & set(pr.EXCEPTIONS))
    missing = set(names) - ran - set(pr.EXCEPTIONS)
    assert not missing, "no row runs %s" % sorted(missing)
    for k, (why, test_file) in pr.EXCEPTIONS.items():
        assert len(why) > 40, k
        path = os.path.join(ROOT, test_file)
        assert os.path.exists(path), (k, test_file)
        text = open(path).read()
        assert "pytest.mark.gpu" in text and "debug_read(" in text, "%s: %s does not diff planes" % (k, test_file)
    # which rows run a kernel, for every kernel (the table's index)
    by_kernel = pr.rows_by_kernel()
    assert set(by_kernel) == set(names) - set(pr.EXCEPTIONS) and all(by_kernel.values())


@pytest.mark.parametrize("name", [c.name for c in _distinct_references()])
def test_references_agree(orc, synth, name):
    """orc.Detector's planes (prepare + stage 0 / 2) equal the planes composed from the oracle's single stages -- color_quantize of the
    pyrDown chain, depth_quantize and its [::2, ::2] pyramid, linearize(response_maps(spread)) -- for one frame of every content kind."""
    case = pr.BY_NAME[name]
    ref = _reference(orc, synth, case)
    kinds_c, kinds_d = set(), set()
    for s in range(max(len(pr.COLOUR_KINDS), len(pr.depth_kinds(case)) if case.M == 2 else 0)):
        bgr, depth, planes, _ = ref.slot(s)
        assert bgr.shape == (case.size[1], case.size[0], 3) and (depth is None) == (case.M == 1)
        kinds_c.add(pr.colour_kind(s))
        kinds_d.add(pr.depth_kind(case, s))
        comp = pr.composed_planes(orc, case, bgr, depth)
        assert set(comp) == set(planes) == set(pr.plane_keys(case))
        for key in pr.plane_keys(case):
            assert np.array_equal(planes[key], comp[key]), (name, s, key, pr.first_difference(case, key, planes[key], comp[key]))
    assert kinds_c == set(pr.COLOUR_KINDS) and (case.M == 1 or kinds_d == set(pr.depth_kinds(case)))


def test_edge_values():
    assert pr.edge_values(10.0) == [98, 100, 104]       # 101 = 10^2 + 1^2 needs dx, dy of different parity
    assert pr.edge_values(3.5) == [10, 16]              # nothing at 12.25; 13 = 3^2 + 2^2 cannot occur
    assert pr.edge_values(1.0) == [0, 2]                # 1 = 1^2 + 0^2 cannot occur


@pytest.mark.parametrize("name", [c.name for c in _distinct_references()])
def test_contents_have_what_they_claim(orc, synth, name):
    """Counted on the oracle's output, for the first frame of each kind: the threshold-edge frame has 50 interior pixels at each value of
    edge_values(weak_threshold), the tie frame 200 pixels with two channels sharing the largest magnitude^2 (50 of them between
    channels of different gradients), the extremes frame only 0 and 255, the rectangle touches two borders; the depth kinds reach what they are for; no two slots of a call hold the same frame."""
    case = pr.BY_NAME[name]
    ref = _reference(orc, synth, case)
    t = case.config["weak_threshold"]
    w, h = case.size
    by_kind = {pr.colour_kind(s): ref.slot(s)[0] for s in range(len(pr.COLOUR_KINDS))}
    counts = pr.edge_counts(orc, by_kind["edge"], t)
    assert len(counts) == (3 if float(t * t) == int(t * t) else 2) and min(counts) >= pr.EDGE_MIN, (name, pr.edge_values(t), counts)
    # the edge decides: pixels at and below the threshold are off, the ones just above can be on
    q, mag = orc.color_quantize(by_kind["edge"], t, want_magnitude=True)
    assert not q[mag <= t * t].any() and q[mag == pr.edge_values(t)[-1]].any()
    # ... so the frame tells the rule from its neighbours: `>=` instead of `>` (a threshold just below), a threshold rounded down or up
    # to an integer before it is squared -- each gives another quantised image
    vals = pr.edge_values(t)
    for other in ([float(np.sqrt(vals[1] - 0.5))] if len(vals) == 3 else [float(int(t)), float(int(t) + 1)]):
        assert not np.array_equal(orc.color_quantize(by_kind["edge"], other), q), (name, t, other)
    ties, different = pr.tie_counts(orc, by_kind["tie"], t)
    assert ties >= pr.TIE_MIN and different >= pr.TIE_DIFFERENT_MIN, (name, ties, different)
    # ... and the tie frame tells the B, G, R cascade from its reverse: with the channels swapped (R, G, B) another channel wins the ties
    assert not np.array_equal(orc.color_quantize(np.ascontiguousarray(by_kind["tie"][..., ::-1]), t), orc.color_quantize(by_kind["tie"], t))
    assert set(np.unique(by_kind["extremes"])) == {0, 255}
    rect = by_kind["rect"]
    assert len(np.unique(rect.reshape(-1, 3), axis=0)) == 2 and (rect[0, w - 1] != rect[h - 1, 0]).any() and (rect[0, w - 2] == rect[0, w - 1]).all() and (rect[1, w - 1] == rect[0, w - 1]).all()
    assert (np.abs(by_kind["blocks"][:8, :8].astype(int) - by_kind["blocks"][0, 0].astype(int)) <= 6).all()
    if case.M == 2:
        d = {pr.depth_kind(case, s): ref.slot(s)[1] for s in range(len(pr.depth_kinds(case)))}
        diff = case.config["difference_threshold"]
        assert d["noise"].max() >= 2000 and d["noise"].min() < 100      # beyond the default distance threshold, deltas far beyond the gate
        assert set(np.unique(d["steps"])) == {600, 600 + diff - 1, 600 + 2 * (diff - 1)}
        assert (d["lattice"] == 0).any() and (d["lattice"] == 700).any() and (d["lattice"] == 300).any()
        if "full" in d:
            assert d["full"].max() > 60000 and d["full"].min() < 5000 and d["near"].min() >= 30000 - diff
    n = min(max(c.first_slot + c.n_slots for c in pr.CASES if c.reference_key() == case.reference_key()), 24)
    frames = [ref.slot(s)[0].tobytes() + (ref.slot(s)[1].tobytes() if case.M == 2 else b"") for s in range(n)]
    assert len(set(frames)) == n
