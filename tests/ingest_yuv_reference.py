"""Numpy reference of the grey and YUV source formats of lm_ingest_frames (include/linemod_hip.h), written from the
contract and not from the kernel: the conversion rule in int64, chroma replicated from the sample whose pair (4:2:0: 2 x 2 block)
covers the pixel, over the WHOLE source.  The expected content of a slot is ingest_reference's result for that converted image given
as BGR8 -- convert, crop, flip, shift.

Formats are the names "gray", "nv12", "nv21", "yuy2", "uyvy"; flags = (matrix, range) with matrix "bt601" / "bt709" and range "limited" /
"full"."""
import numpy as np

import ingest_reference as IR

# (matrix, range) -> Y0, CY, CVR, CVG, CUG, CUB
COEF = {
    ("bt601", "limited"): (16, 1220542, 1673527, -852492, -409993, 2116026),      # OpenCV's ITUR_BT_601_* constants at shift 20
    ("bt709", "limited"): (16, 1220945, 1879825, -558796, -223607, 2215014),
    ("bt601", "full"): (0, 1048576, 1470104, -748826, -360853, 1858077),
    ("bt709", "full"): (0, 1048576, 1651297, -490864, -196424, 1945738),
}
FLAGS = list(COEF)


def convert(Y, U, V, flags=("bt601", "limited")):
    """Arrays of samples (any equal shape) -> [..., 3] uint8 in B, G, R order.  int64 throughout; >> floors."""
    Y0, CY, CVR, CVG, CUG, CUB = COEF[tuple(flags)]
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    y = np.maximum(0, Y - Y0) * CY
    u, v = U - 128, V - 128
    r = (y + (1 << 19) + CVR * v) >> 20
    g = (y + (1 << 19) + CVG * v + CUG * u) >> 20
    b = (y + (1 << 19) + CUB * u) >> 20
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def planes(src, fmt):
    """The full-resolution Y, U, V planes ([H, W] each) of a source: fmt nv12 / nv21: src = (y [H, W], uv [H / 2, W] bytes), yuy2 / uyvy:
    src = [H, W, 2] bytes (equally [H, 2 W])."""
    if fmt in ("nv12", "nv21"):
        y, uv = (np.asarray(a) for a in src)
        H, W = y.shape
        assert H % 2 == 0 and W % 2 == 0 and uv.shape[0] == H // 2
        uv = uv.reshape(H // 2, W // 2, 2)
        first, second = uv[:, :, 0], uv[:, :, 1]
        u, v = (first, second) if fmt == "nv12" else (second, first)
        rows, cols = np.arange(H) >> 1, np.arange(W) >> 1
        return y, u[rows][:, cols], v[rows][:, cols]
    assert fmt in ("yuy2", "uyvy")
    src = np.asarray(src)
    H, W = src.shape[0], src.shape[1]
    assert W % 2 == 0
    m = src.reshape(H, W // 2, 4)
    if fmt == "yuy2":
        y0, u, y1, v = (m[:, :, k] for k in range(4))
    else:
        u, y0, v, y1 = (m[:, :, k] for k in range(4))
    cols = np.arange(W) >> 1
    y = np.where((np.arange(W) & 1)[None, :] == 0, y0[:, cols], y1[:, cols])
    return y, u[:, cols], v[:, cols]


def yuv_to_bgr(src, fmt, flags=("bt601", "limited")):
    """The [H, W, 3] BGR image the rule yields from the whole source (gray: src = [H, W], the flags play no part)."""
    if fmt == "gray":
        g = np.asarray(src)
        assert g.dtype == np.uint8 and g.ndim == 2
        return np.repeat(g[:, :, None], 3, axis=2)
    return convert(*planes(src, fmt), flags)


def expected(src, fmt, flags, W, H, crop=(0, 0), flip_x=False, shift=(0, 0)):
    return IR.colour(yuv_to_bgr(src, fmt, flags), W, H, "bgr", "hwc", crop, flip_x, shift)


# ---- packers: byte images from Y [H, W] and U, V [H / 2, W / 2] (4:2:0) or [H, W / 2] (4:2:2)
def pack_nv(Y, U, V, fmt):
    """-> (y [H, W], uv [H / 2, W]) uint8"""
    Y, U, V = (np.asarray(a, np.uint8) for a in (Y, U, V))
    H, W = Y.shape
    assert U.shape == V.shape == (H // 2, W // 2)
    uv = np.stack([U, V] if fmt == "nv12" else [V, U], axis=-1).reshape(H // 2, W)
    return Y.copy(), uv


def pack_422(Y, U, V, fmt):
    """-> [H, W, 2] uint8"""
    Y, U, V = (np.asarray(a, np.uint8) for a in (Y, U, V))
    H, W = Y.shape
    assert U.shape == V.shape == (H, W // 2)
    y0, y1 = Y[:, 0::2], Y[:, 1::2]
    m = np.stack([y0, U, y1, V] if fmt == "yuy2" else [U, y0, V, y1], axis=-1)
    return m.reshape(H, W, 2)
