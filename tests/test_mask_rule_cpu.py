"""CPU tests of the mask rules: the numpy reference (tests/mask_rule_reference.py) against scipy and against the definition, the crafted
inputs of the GPU test (each keeps the reference mask non-trivial, except `full` and `empty`), and the binding's view of the new ABI."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mask_rule_reference as mrr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nontrivial(mask):
    return bool((mask == 0).any() and (mask == 255).any() and np.isin(mask, (0, 255)).all())


# ---- the reference's dilation -----------------------------------------------------------------------
@pytest.mark.parametrize("r", [0, 1, 2, 7, 16])
def test_dilation_equals_scipy_maximum_filter(r):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(r)
    for shape in ((40, 50), (33, 7), (1, 64), (64, 1), (80, 160)):
        for density in (0.02, 0.5):
            seed = rng.random(shape) < density
            exp = ndi.maximum_filter(seed.astype(np.uint8), size=2 * r + 1, mode="constant", cval=0).astype(bool)
            assert np.array_equal(mrr.dilate(seed, r), exp), (r, shape, density)


@pytest.mark.parametrize("r", [0, 1, 2, 7, 16])
def test_dilation_equals_the_definition(r):
    rng = np.random.default_rng(100 + r)
    for shape in ((24, 31), (40, 9)):
        seed = rng.random(shape) < 0.05
        assert np.array_equal(mrr.dilate(seed, r), mrr.dilate_windows(seed, r)), (r, shape)


def test_dilation_clips_at_all_four_corners():
    h, w, r = 30, 40, 3
    for (y, x), (ys, xs) in {(0, 0): (slice(0, 4), slice(0, 4)), (0, w - 1): (slice(0, 4), slice(w - 4, w)),
                             (h - 1, 0): (slice(h - 4, h), slice(0, 4)), (h - 1, w - 1): (slice(h - 4, h), slice(w - 4, w))}.items():
        seed = np.zeros((h, w), bool)
        seed[y, x] = True
        exp = np.zeros((h, w), bool)
        exp[ys, xs] = True                               # the (2r + 1)^2 square cut to the image: (r + 1)^2 pixels, nothing wraps round
        got = mrr.dilate(seed, r)
        assert np.array_equal(got, exp) and got.sum() == (r + 1) ** 2


def test_grow_zero_is_the_identity():
    rng = np.random.default_rng(5)
    seed = rng.random((50, 70)) < 0.4
    assert np.array_equal(mrr.dilate(seed, 0), seed)
    depth = mrr.depth_from_seed(seed)
    assert np.array_equal(mrr.mask_of(dict(depth_range=(mrr.ZMIN, mrr.ZMAX), grow=0), None, depth), seed.astype(np.uint8) * 255)


# ---- the GPU test's inputs are non-trivial ------------------------------------------------------------
@pytest.mark.parametrize("w,h", mrr.SIZES + [(100, 80)])
def test_crafted_seeds_keep_the_mask_nontrivial(w, h):
    for r in mrr.GROWS:
        seeds = mrr.crafted_seeds(w, h, r)
        assert [n for n, _ in seeds] == ["corner00", "corner0w", "cornerh0", "cornerhw", "x63", "x64", "xw1", "y0", "yh1", "pair%d" % (2 * r + 1),
                                         "pair%d" % (2 * r + 2), "full", "empty", "rand10", "rand90"]
        for name, seed in seeds:
            depth = mrr.depth_from_seed(seed)
            assert np.array_equal(mrr.depth_gate(depth, mrr.ZMIN, mrr.ZMAX, False), seed), name
            m = mrr.mask_of(dict(depth_range=(mrr.ZMIN, mrr.ZMAX), grow=r), None, depth)
            if name == "full":
                assert (m == 255).all()
            elif name == "empty":
                assert (m == 0).all()
            else:
                assert _nontrivial(m), (w, h, r, name)
            if name.startswith("pair"):
                gap = int(name[4:])
                x0 = min(64 - r - 1, w - 1 - gap)
                assert seed[h // 2, x0] and seed[h // 2, x0 + gap] and seed[10, 5] and seed[10 + gap, 5]
                merged = gap == 2 * r + 1                # 2r + 1 apart: the two squares touch; 2r + 2: one pixel stays open
                assert mrr.gap_is_merged(m[h // 2], x0, x0 + gap) == merged
                assert mrr.gap_is_merged(m[:, 5], 10, 10 + gap) == merged


def test_depth_edge_cases_are_nontrivial_and_hit_every_edge():
    depth, rules = mrr.depth_edge_cases()
    for v in (mrr.ZMIN - 1, mrr.ZMIN, mrr.ZMAX, mrr.ZMAX + 1, 0, 65535):
        assert (depth == v).any()
    for rule in rules:
        assert _nontrivial(mrr.mask_of(rule, None, depth)), rule
    off, on = mrr.mask_of(rules[0], None, depth), mrr.mask_of(rules[1], None, depth)
    assert np.array_equal(on != off, depth == 0)          # keep_invalid changes the pixels without a measurement, and only those
    assert (off[depth == mrr.ZMIN] == 255).all() and (off[depth == mrr.ZMAX] == 255).all()
    assert (off[depth == mrr.ZMIN - 1] == 0).all() and (off[depth == mrr.ZMAX + 1] == 0).all() and (off[depth == 65535] == 0).all()


def test_hsv_edge_frame_holds_every_edge_of_the_gate():
    bgr = mrr.hsv_edge_frame()
    cov = mrr.hsv_edge_coverage(bgr)
    assert all(n > 0 for n in cov.values()), cov
    assert _nontrivial(mrr.mask_of(dict(hsv_range=(mrr.HSV_LOWER, mrr.HSV_UPPER)), bgr, None))


@pytest.mark.parametrize("w,h", [(80, 80), (400, 240)])
def test_rect_cases_are_nontrivial_and_do_not_leak(w, h):
    for name, seed, rule in mrr.rect_cases(w, h):
        m = mrr.mask_of(rule, None, mrr.depth_from_seed(seed))
        assert _nontrivial(m), name
        x, y, rw, rh = rule["rect"]
        outside = np.ones((h, w), bool)
        outside[y:y + rh, x:x + rw] = False
        assert (m[outside] == 0).all(), name
        if name in ("one", "corner"):
            assert m.sum() == 255 and m[y, x] == 255
        if name == "leak":
            assert not seed[y:y + rh, x:x + rw].any() and 0 < (m == 255).sum() < rw * rh


# ---- the binding --------------------------------------------------------------------------------------
def test_binding_declares_the_mask_rule_entry_points(lm):
    lib = lm.load_library()
    for name in ("lm_set_mask_rule", "lm_get_mask_rule", "lm_stage_mask_rule"):
        assert name in lm.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert b"0.9" in lib.lm_version()
    r = lm.make_mask_rule(3, depth_range=(600, 800), keep_invalid=True, hsv_range=((1, 2, 3), (4, 5, 6)), grow=8, rect=(1, 2, 30, 40))
    assert (r.modalities, r.use_depth, r.keep_invalid, r.zmin, r.zmax, r.use_hsv, r.grow) == (3, 1, 1, 600, 800, 1, 8)
    assert list(r.lower) == [1, 2, 3] and list(r.upper) == [4, 5, 6] and (r.x, r.y, r.width, r.height) == (1, 2, 30, 40)
    d = lm.Detector(color_only=False, frame_slots=2)
    assert d.mask_rule(0) is None and d.mask_rule(1) is None     # (host state: no device needed)
    with pytest.raises(lm.LinemodError):
        d.mask_rule(2)
    d.close()


def test_mask_rule_struct_has_the_headers_size_and_offsets(lm, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "a C compiler is needed to read the header's layout"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "linemod_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(lm_mask_rule), offsetof(lm_mask_rule, use_hsv), '
                   'offsetof(lm_mask_rule, lower), offsetof(lm_mask_rule, upper), offsetof(lm_mask_rule, grow), offsetof(lm_mask_rule, rect)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_hsv, o_lo, o_hi, o_grow, o_rect = (int(v) for v in subprocess.check_output([str(exe)]).split())
    M = lm.MaskRule
    assert C.sizeof(M) == size == 96
    assert (M.use_hsv.offset, M.lower.offset, M.upper.offset, M.grow.offset, M.x.offset) == (o_hsv, o_lo, o_hi, o_grow, o_rect)
