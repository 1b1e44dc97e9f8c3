"""CPU side of template-bank generation on the GPU: the new entry points fail with LM_ERR_* codes without a GPU
(no fallback), the binding declares them, and the separable L-infinity distance the GPU computes (a row pass, then a column pass) agrees
with the chessboard-distance rule of lm_extract.cpp (two raster sweeps, outside the image far away), restated here."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = (2 ** 31 - 1) >> 2


def chessboard_two_pass(nz):
    """lm_extract.cpp chessboard_distance: distance to the nearest zero pixel, two raster sweeps of the 8-neighbour chamfer."""
    h, w = nz.shape
    d = np.where(nz != 0, FAR, 0).astype(np.int64)
    get = lambda y, x: FAR if (x < 0 or y < 0 or x >= w or y >= h) else d[y, x]
    for y in range(h):
        for x in range(w):
            if d[y, x]:
                d[y, x] = min(d[y, x], min(get(y - 1, x - 1), get(y - 1, x), get(y - 1, x + 1), get(y, x - 1)) + 1)
    for y in range(h - 1, -1, -1):
        for x in range(w - 1, -1, -1):
            if d[y, x]:
                d[y, x] = min(d[y, x], min(get(y + 1, x + 1), get(y + 1, x), get(y + 1, x - 1), get(y, x + 1)) + 1)
    return d


def separable_linf(nz):
    """k_gen_rowdist + gen_coldist: per row the distance to the nearest zero of the row (none: far), then per column
    min over rows y' of max(|y - y'|, row distance at y')."""
    h, w = nz.shape
    INF = np.int64(1) << 40
    row = np.full((h, w), INF, np.int64)
    xs = np.arange(w)
    for y in range(h):
        zeros = np.flatnonzero(nz[y] == 0)
        if len(zeros):
            row[y] = np.abs(xs[:, None] - zeros[None, :]).min(1)
    ys = np.arange(h)
    d = np.maximum(np.abs(ys[:, None, None] - ys[None, :, None]), row[None, :, :]).min(1)
    return np.where(d >= INF, FAR, d)


@pytest.mark.parametrize("seed", range(6))
def test_separable_linf_equals_chessboard_rule(seed):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(1, 23)), int(rng.integers(1, 29))
    p = [0.5, 0.9, 0.97, 1.0, 0.75, 0.99][seed]
    nz = (rng.random((h, w)) < p).astype(np.uint8)
    if seed == 4:   # one big blob: large distances
        nz[:] = 0
        nz[1:h - 1, 2:w - 1] = 1
    assert np.array_equal(separable_linf(nz), chessboard_two_pass(nz))


def test_binding_declares_generation_entry_points(lm):
    lib = lm.load_library()
    for n in ("lm_set_render_mesh", "lm_add_templates_rendered", "lm_stage_render", "lm_stage_rotate"):
        assert n in lm.EXPORTS and getattr(lib, n).argtypes is not None
    v = lib.lm_version()
    assert b"0.6" in v and b"0.5" in v and b"0.4" in v


def test_entry_points_fail_with_codes_without_gpu(lm):
    """Argument errors come first (LM_ERR_INVALID); without a device every call that needs it fails with LM_ERR_NO_DEVICE."""
    lib = lm.load_library()
    cfg = lm.default_config(color_only=True)
    h = C.c_void_p()
    assert lib.lm_create(C.byref(cfg), C.byref(h)) == lm.LM_OK
    try:
        v = np.zeros((3, 3), np.float32); v[1, 0] = 1; v[2, 1] = 1
        f = np.array([0, 1, 2], np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.lm_set_render_mesh(h, 0, p(v), 0, p(f), 3) == lm.LM_ERR_INVALID
        assert lib.lm_set_render_mesh(h, 0, p(v), 3, p(f), 2) == lm.LM_ERR_INVALID
        rc = lib.lm_set_render_mesh(h, 0, p(v), 3, p(f), 3)
        gpu = rc == lm.LM_OK
        assert gpu or rc == lm.LM_ERR_NO_DEVICE
        vp = np.eye(4, dtype=np.float32).ravel()
        an = np.zeros(1, np.float32)
        ids = np.zeros(1, np.int32); bbs = np.zeros(4, np.int32); crops = np.zeros(16, np.uint16); offs = np.zeros(2, np.uint64)
        assert lib.lm_add_templates_rendered(h, b"c", 0, p(vp), 0, p(an), 1, p(ids), p(bbs), p(crops), 16, p(offs)) == lm.LM_ERR_INVALID
        assert lib.lm_add_templates_rendered(h, b"c", 1, p(vp), 1, p(an), 1, p(ids), p(bbs), p(crops), 16, p(offs)) == lm.LM_ERR_INVALID
        assert lib.lm_stage_render(h, 1, p(vp), 4, 4, p(np.zeros(16, np.uint8)), p(np.zeros(16, np.uint16))) == lm.LM_ERR_INVALID
        assert ids[0] == -1 and lib.lm_num_templates(h) == 0
        a8 = np.zeros((4, 4), np.uint8); a16 = np.zeros((4, 4), np.uint16)
        assert lib.lm_stage_rotate(h, p(a8), p(a16), 4, 4, 10.0, p(a8.copy()), p(a16.copy())) == (lm.LM_OK if gpu else lm.LM_ERR_NO_DEVICE)
    finally:
        lib.lm_destroy(h)
