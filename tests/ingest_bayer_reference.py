"""The reference of the raw Bayer ingest formats (include/linemod_hip.h, DESIGN.md section 13 "Bayer sources"): the bilinear demosaic of
the WHOLE source in numpy int64, vectorised, and the mosaic that undoes it.  Patterns are the names "rggb", "grbg", "gbrg", "bggr": the
colours of the source's top-left 2 x 2 tile in reading order.  No GPU, no library."""
import numpy as np

PATTERNS = ("rggb", "grbg", "gbrg", "bggr")


def red_site(pattern):
    """(red_x, red_y): where the red sample lies inside the 2 x 2 tile; PIX_BAYER_* - 16 = red_x | red_y << 1."""
    i = PATTERNS.index(pattern)
    return i & 1, i >> 1


def demosaic(raw, pattern):
    """[H, W] uint8 (H, W even, >= 2) -> [H, W, 3] uint8 B, G, R.  Neighbours beyond an edge are reflected without repeating the edge
    (-1 -> 1, w -> w - 2: numpy's "reflect")."""
    raw = np.asarray(raw)
    assert raw.ndim == 2 and raw.dtype == np.uint8 and raw.shape[0] % 2 == 0 and raw.shape[1] % 2 == 0 and min(raw.shape) >= 2
    H, W = raw.shape
    S = np.pad(raw.astype(np.int64), 1, mode="reflect")
    c = S[1:-1, 1:-1]
    left, right, up, down = S[1:-1, :-2], S[1:-1, 2:], S[:-2, 1:-1], S[2:, 1:-1]
    h = (left + right + 1) >> 1
    v = (up + down + 1) >> 1
    p = (left + right + up + down + 2) >> 2
    d = (S[:-2, :-2] + S[:-2, 2:] + S[2:, :-2] + S[2:, 2:] + 2) >> 2
    rx, ry = red_site(pattern)
    y, x = np.mgrid[0:H, 0:W]
    dx, dy = (x ^ rx) & 1, (y ^ ry) & 1
    red, blue, g_red_row, g_blue_row = (dx == 0) & (dy == 0), (dx == 1) & (dy == 1), (dx == 1) & (dy == 0), (dx == 0) & (dy == 1)
    R = np.select([red, blue, g_red_row, g_blue_row], [c, d, h, v])
    G = np.select([red, blue, g_red_row, g_blue_row], [p, p, c, c])
    B = np.select([red, blue, g_red_row, g_blue_row], [d, c, v, h])
    return np.stack([B, G, R], axis=-1).astype(np.uint8)


def mosaic(bgr, pattern):
    """[H, W, 3] B, G, R -> [H, W] uint8: every site keeps the channel its filter passes."""
    bgr = np.asarray(bgr)
    H, W = bgr.shape[:2]
    rx, ry = red_site(pattern)
    y, x = np.mgrid[0:H, 0:W]
    dx, dy = (x ^ rx) & 1, (y ^ ry) & 1
    channel = np.where(dx != dy, 1, np.where(dy == 0, 2, 0))       # green; red in a red row's red column; blue
    return np.take_along_axis(bgr, channel[..., None], axis=2)[..., 0].astype(np.uint8)
