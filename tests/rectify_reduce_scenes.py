"""The scenes and the reference of the rectify-and-reduce tests (tests/test_rectify_reduce_cpu.py, tests/test_gpu_rectify_reduce.py).

The reference is a composition and holds no arithmetic of its own: tests/rectify_reference.py makes the rectified images Rc / Rd of the
WHOLE ideal geometry, tests/reduce_reference.py reduces them, ingest_reference places the window.  The scenes are rectify_scenes' 208 x 120
source camera under its barrel lens and wide_ideal(iw, ih) -- an ideal camera that sees more than the lens delivers -- with the ideal
geometry sized just above slot * ratio, so that a tail of ideal pixels stays unused.  Everything is built once per key and left unchanged."""
import numpy as np

import rectify_reference as QR
import rectify_scenes as S
import reduce_reference as RR
import reduce_scenes as RS

# the three scenes whose straddling pixels were counted when the route was specified: (ideal size, ratio, slot, crop)
LENS_SCENES = [((208, 120), (2, 1), (RS.MW, RS.MH), (3, 2)), ((201, 102), (3, 1), (RS.MW, RS.MH), (2, 1)), ((372, 190), (9, 4), (RS.W, RS.H), (2, 2))]
_cache = {}


def ideal_sides(slot_w, slot_h, r):
    """The ideal geometry for a slot and a ratio: the listed scene where there is one; otherwise R = slot + 3 x slot + 2 with a tail, and
    no smaller than 208 x 120 (wide_ideal's focal length is fixed: a smaller geometry would lie inside the source altogether)."""
    for size, ratio, slot, _ in LENS_SCENES:
        if RR.ratio(ratio) == RR.ratio(r) and slot == (slot_w, slot_h):
            return size
    nx, dx, ny, dy = RR.ratio(r)
    return max(RS.source_size(slot_w, (nx, dx), 3), S.SW), max(RS.source_size(slot_h, (ny, dy), 2), S.SH)


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def lens_map(iw, ih, dist=S.LENS):
    """(source camera, ideal camera, the reference's map int32 [ih, iw, 2])."""
    def make():
        source, ideal = S.source_cam(dist), S.wide_ideal(iw, ih)
        return source, ideal, QR.build_map(source, ideal)
    return cached(("map", iw, ih, tuple(dist)), make)


def identity_map(w=S.SW, h=S.SH):
    """Zero coefficients and ideal = the source's pinhole: every entry is (32 i, 32 j)."""
    def make():
        source = S.source_cam(S.ZERO, w, h)
        return source, QR.pinhole_of(source), QR.build_map(source, QR.pinhole_of(source))
    return cached(("identity", w, h), make)


def reduced_colour(bgr, qmap, r):
    """Ac: reduce_reference's box over rectify_reference's Rc."""
    return RR.reduce_colour(QR.rectify_colour(bgr, qmap), r)


def reduced_depth(depth, qmap, r, rule, scale=1.0):
    """Ad: reduce_reference's depth rule over rectify_reference's Rd (uint16 already: no second conversion)."""
    return RR.reduce_depth(QR.rectify_depth(depth, qmap, scale), r, rule)


def straddling(qmap, src_w, src_h, r, slot_w, slot_h, crop):
    """How many pixels of the slot window at `crop` of the reduced ideal geometry have a footprint that holds an ideal pixel with taps
    inside AND taps outside the source: from the map alone."""
    ix, iy = qmap[:, :, 0].astype(np.int64) >> 5, qmap[:, :, 1].astype(np.int64) >> 5
    inside = lambda x, y: (x >= 0) & (x < src_w) & (y >= 0) & (y < src_h)
    n_in = sum(inside(ix + a, iy + b).astype(np.int64) for a in (0, 1) for b in (0, 1))
    nx, dx, ny, dy = RR.ratio(r)
    count = 0
    for Y in range(crop[1], crop[1] + slot_h):
        j0, j1 = Y * ny // dy, ((Y + 1) * ny - 1) // dy
        for X in range(crop[0], crop[0] + slot_w):
            i0, i1 = X * nx // dx, ((X + 1) * nx - 1) // dx
            foot = n_in[j0:j1 + 1, i0:i1 + 1]
            count += bool(((foot > 0) & (foot < 4)).any())
    return count
