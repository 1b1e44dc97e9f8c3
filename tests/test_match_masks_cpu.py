"""CPU side of Detector::match's masks (lm_match_masked / lm_upload_match_mask): the independent reference the GPU tests compare
masked lists with (tests/masked_reference.py) reproduces the oracle on unmasked input, the mask pyramid rule the kernel relies on
holds for every size the GPU tests use, and the binding declares the new entry points."""
import inspect

import numpy as np
import pytest

import masked_reference as mr
from conftest import assert_matches_equal

# (width, height, pyramid levels) of the masked GPU tests (tests/test_gpu_match_masks.py)
MASK_SIZES = [(640, 480, 1), (640, 480, 2), (640, 480, 3), (1280, 960, 2)]


def _quant(o, bgr, depth, M, L):
    o.prepare(bgr, depth if M == 2 else None)
    return {(l, m): o.stage(0, l, m).reshape(bgr.shape[0] >> l, bgr.shape[1] >> l) for l in range(L) for m in range(M)}


@pytest.mark.parametrize("M", [2, 1])
def test_reference_helper_equals_oracle_unmasked(orc, synth, frame0, M):
    """The numpy restatement on the oracle's own quantised pyramid gives the oracle's lists record for record."""
    bgr, depth = frame0
    o = orc.Detector(color_only=(M == 1))
    T = [o.cfg.T[l] for l in range(o.cfg.pyramid_levels)]
    q = _quant(o, bgr, depth, M, len(T))
    classes = []
    for k, seed in enumerate((21, 22)):
        descs, feats, _ = synth.make_bank(12, M, 2, seed=seed, quantized=q, crop_fraction=0.4, T0=T[0])
        o.add_class("m%d" % k, descs, feats)
        classes.append((descs, feats))
    for thr, ci in ((80.0, -1), (65.0, 1)):
        exp = o.match(bgr, depth if M == 2 else None, thr, class_idx=ci)
        assert len(exp) > 0
        got = mr.match(orc, q, classes, T, thr, class_idx=ci)
        assert_matches_equal(got, exp)
    o.close()


@pytest.mark.parametrize("w,h,L", MASK_SIZES)
def test_mask_pyramid_is_the_even_samples(orc, w, h, L):
    """resize(mask, INTER_NEAREST) to half size, l times, is mask0[y << l][x << l] at these sizes (what k_match_mask reads)."""
    rng = np.random.default_rng(w + h + L)
    m0 = (rng.random((h, w)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
    pyr = mr.mask_pyramid(orc, m0, L)
    for l in range(L):
        assert pyr[l].shape == (h >> l, w >> l)
        assert np.array_equal(pyr[l], m0[::1 << l, ::1 << l][:h >> l, :w >> l]), l


def test_binding_declares_mask_entry_points(lm):
    lib = lm.load_library()
    for name in ("lm_match_masked", "lm_upload_match_mask"):
        assert name in lm.EXPORTS
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert "masks" in inspect.signature(lm.Detector.match).parameters
    assert inspect.signature(lm.Detector.match).parameters["masks"].default is None
    assert callable(getattr(lm.Detector, "upload_match_mask", None))
    assert b"0.4" in lib.lm_version()
