"""Numpy reference of lm_ingest_frames, per image, written from the definition (include/linemod_hip.h) and not
from the kernel.  Output pixel (x, y) of the W x H frame:

    xs = x - shift_x;  ys = y - shift_y
    xs, ys outside [0, W) x [0, H):  out = 0
    u  = W - 1 - xs if flip_x else xs
    p  = source pixel (crop_x + u, crop_y + ys)
    colour: out = (B, G, R) of p          depth: out = to_u16(p)

The sources are host arrays in the producer's layout: colour [h, w, 3 | 4] (hwc) or [3, h, w] (chw) uint8 in `order`, depth [h, w]
uint16 or float32."""
import numpy as np


def to_u16(v, scale):
    """t = v * scale as ONE float32 multiply; 0 for NaN, +-inf and t <= 0; 65535 for t >= 65535; else round to nearest, ties to even."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = v * np.float32(scale)
    assert t.dtype == np.float32
    out = np.zeros(t.shape, np.uint16)
    ordinary = np.isfinite(t) & (t > 0) & (t < np.float32(65535))
    out[ordinary] = np.rint(t[ordinary]).astype(np.uint16)
    out[np.isfinite(t) & (t >= np.float32(65535))] = 65535
    return out          # NaN, +inf, -inf, t <= 0 stay 0


def _place(window, W, H, flip_x, shift):
    """window: [H, W, ...] the cropped, converted image.  Mirror, then translate with zeros shifted in -- pixel by pixel index arithmetic."""
    sx, sy = int(shift[0]), int(shift[1])
    out = np.zeros_like(window)
    ys = np.arange(H) - sy
    xs = np.arange(W) - sx
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    u = np.where(flip_x, W - 1 - xs, xs)
    yy, xx = np.nonzero(oky[:, None] & okx[None, :])
    out[yy, xx] = window[ys[yy], u[xx]]
    return out


def colour(src, W, H, order="bgr", layout="hwc", crop=(0, 0), flip_x=False, shift=(0, 0)):
    src = np.asarray(src)
    assert src.dtype == np.uint8
    if layout == "chw":
        src = np.transpose(src, (1, 2, 0))
    cx, cy = crop
    assert 0 <= cx and cx + W <= src.shape[1] and 0 <= cy and cy + H <= src.shape[0]
    win = src[cy:cy + H, cx:cx + W, :3]
    if order == "rgb":
        win = win[:, :, ::-1]
    return _place(np.ascontiguousarray(win), W, H, flip_x, shift)


def depth(src, W, H, crop=(0, 0), scale=1.0, flip_x=False, shift=(0, 0)):
    src = np.asarray(src)
    cx, cy = crop
    assert 0 <= cx and cx + W <= src.shape[1] and 0 <= cy and cy + H <= src.shape[0]
    win = src[cy:cy + H, cx:cx + W]
    if src.dtype == np.float32:
        win = to_u16(win, scale)
    else:
        assert src.dtype == np.uint16
    return _place(np.ascontiguousarray(win), W, H, flip_x, shift)
