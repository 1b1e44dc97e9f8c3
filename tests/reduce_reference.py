"""Numpy reference of the area-averaged reduction (include/linemod_hip.h, "Area-averaged reduction at ingest"),
written from the header's text and not from csrc/lm_reduce.h.

Colour: the dense weight matrices Wy [Ry, h] and Wx [Rx, w] are built from the interval definition -- reduced pixel X covers
[X num, (X + 1) num), source pixel i covers [i den, (i + 1) den), the weight is the length of the overlap -- with integer arithmetic,
and the image is (Wy @ img @ Wx.T + N // 2) // N per channel in int64, N = num_x num_y.  The source's BGR image is decoded by the
format's own reference over the WHOLE source (rectify_reference.decode, ingest_bayer_reference, ingest_raw_reference).  Depth: plain
loops over the reduced pixels.  The expected content of a slot is ingest_reference's crop, mirror and shift of the reduced image."""
from fractions import Fraction
from math import gcd

import numpy as np

import ingest_reference as IR


def ratio(r):
    """(num, den) or ((num_x, den_x), (num_y, den_y)) -> (num_x, den_x, num_y, den_y) in lowest terms."""
    rx, ry = (r, r) if isinstance(r[0], int) else r
    out = []
    for num, den in (rx, ry):
        g = gcd(num, den)
        out += [num // g, den // g]
    return tuple(out)


def reduced_size(n, num, den):
    return (n * den) // num


def weights(n, num, den):
    """W int64 [R, n]: W[X, i] = |[X num, (X + 1) num) & [i den, (i + 1) den)|."""
    R = reduced_size(n, num, den)
    W = np.zeros((R, n), np.int64)
    for X in range(R):
        for i in range(n):
            W[X, i] = max(0, min((X + 1) * num, (i + 1) * den) - max(X * num, i * den))
    assert (W.sum(axis=1) == num).all() and W.max(initial=0) <= den
    return W


def reduce_colour(bgr, r):
    """bgr [H, W, 3] uint8 (the whole source, decoded) -> [Ry, Rx, 3] uint8."""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    nx, dx, ny, dy = ratio(r)
    Wy, Wx = weights(bgr.shape[0], ny, dy), weights(bgr.shape[1], nx, dx)
    N = nx * ny
    out = np.zeros((Wy.shape[0], Wx.shape[0], 3), np.uint8)
    for c in range(3):
        acc = Wy @ bgr[:, :, c].astype(np.int64) @ Wx.T
        assert acc.max(initial=0) <= 255 * N
        out[:, :, c] = (acc + (N >> 1)) // N
    return out


def reduce_depth(depth, r, rule="nearest", scale=1.0):
    """depth [H, W] uint16 or float32 (times scale = millimetres) -> [Ry, Rx] uint16 by `rule`: "nearest" (the source pixel that holds
    the footprint's centre) or "min_valid" (the smallest non-zero value among the source pixels whose centre lies in the footprint)."""
    depth = np.asarray(depth)
    d16 = IR.to_u16(depth, scale) if depth.dtype == np.float32 else depth
    assert d16.dtype == np.uint16 and rule in ("nearest", "min_valid")
    nx, dx, ny, dy = ratio(r)
    H, W = d16.shape
    Ry, Rx = reduced_size(H, ny, dy), reduced_size(W, nx, dx)
    out = np.zeros((Ry, Rx), np.uint16)
    # per axis and reduced pixel, once: the source pixel that holds the centre (X + 1/2) num / den, and the source pixels whose own
    # centre i + 1/2 lies in [X num / den, (X + 1) num / den) -- exact fractions
    def axis(R, n, num, den):
        centre = [int(Fraction((2 * X + 1) * num, 2 * den)) for X in range(R)]
        near = lambda X: range(max(0, X * num // den - 2), min(n, (X + 1) * num // den + 3))          # (a generous window: the rest is far away)
        under = [[i for i in near(X) if Fraction(X * num, den) <= Fraction(2 * i + 1, 2) < Fraction((X + 1) * num, den)] for X in range(R)]
        return centre, under
    row_centre, rows_under = axis(Ry, H, ny, dy)
    col_centre, cols_under = axis(Rx, W, nx, dx)
    for Y in range(Ry):
        for X in range(Rx):
            if rule == "nearest":
                out[Y, X] = d16[row_centre[Y], col_centre[X]]
            else:
                vals = [int(d16[j, i]) for j in rows_under[Y] for i in cols_under[X] if d16[j, i] != 0]
                out[Y, X] = min(vals) if vals else 0
    return out


def slot_colour(Rc, W, H, crop=(0, 0), flip_x=False, shift=(0, 0)):
    return IR.colour(Rc, W, H, "bgr", "hwc", crop, flip_x, shift)


def slot_depth(Rd, W, H, crop=(0, 0), flip_x=False, shift=(0, 0)):
    return IR.depth(Rd, W, H, crop, 1.0, flip_x, shift)


def reduced_camera(cam, r, crop=(0, 0)):
    """(fx, fy, cx, cy) float64 of the slot's frame: fx' = fx den / num, cx' = (cx + 0.5) den / num - 0.5 - crop (pixel centres)."""
    nx, dx, ny, dy = ratio(r)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in cam)
    return (fx * dx / nx, fy * dy / ny, (cx + 0.5) * dx / nx - 0.5 - crop[0], (cy + 0.5) * dy / ny - 0.5 - crop[1])
