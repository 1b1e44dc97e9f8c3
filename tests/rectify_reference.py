"""Numpy reference of the lens rectification (include/linemod_hip.h, "Lens rectification at ingest"), written from
the header's text and not from csrc/lm_rectify.h.

The map: float64, one ufunc per operation in the order the header writes them, from the cameras' numbers rounded to float32 first (the
library holds them as floats); np.rint (ties to even), clip, int32.  The pixel rule: integer arrays -- the four taps of the bilinear
blend read from the source's BGR image (decoded by the format's own rule over the WHOLE source: tests/ingest_reference.py and
tests/ingest_yuv_reference.py) inside a zero border, the nearest rule for depth.  The expected content of a slot is ingest_reference's
crop, mirror and shift of the rectified image."""
import numpy as np

import ingest_reference as IR
import ingest_yuv_reference as YR

F = np.float32
ZERO = (0.0,) * 5


def cam(width, height, fx, fy, cx, cy, dist=ZERO):
    return dict(width=int(width), height=int(height), fx=fx, fy=fy, cx=cx, cy=cy, dist=tuple(dist))


def pinhole_of(c):
    return cam(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"])


def quant(s, n):
    """-64 if s is not finite; otherwise rint(32 s) clamped into [-64, 32 n + 32]; int32."""
    s = np.asarray(s, np.float64)
    with np.errstate(all="ignore"):
        r = np.rint(np.multiply(32.0, s))
        r = np.clip(r, -64.0, 32.0 * n + 32.0)
    r = np.where(np.isfinite(s), r, -64.0)
    return r.astype(np.int32)


def _f(c):
    """The camera's nine numbers as the doubles their float32 values are."""
    return [np.float64(F(v)) for v in (c["fx"], c["fy"], c["cx"], c["cy"]) + tuple(c["dist"])]


def source_coordinates(source, ideal):
    """(sx, sy) float64 [h', w'] of every ideal pixel: the forward Brown model."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = _f(source)
    fxi, fyi, cxi, cyi = _f(ideal)[:4]
    i, j = np.meshgrid(np.arange(ideal["width"], dtype=np.float64), np.arange(ideal["height"], dtype=np.float64))
    mul, add, sub, div = np.multiply, np.add, np.subtract, np.divide
    with np.errstate(all="ignore"):
        x = div(sub(i, cxi), fxi)
        y = div(sub(j, cyi), fyi)
        r2 = add(mul(x, x), mul(y, y))
        rad = add(1.0, mul(r2, add(k1, mul(r2, add(k2, mul(r2, k3))))))
        xy = mul(x, y)
        xd = add(mul(x, rad), add(mul(mul(2.0, p1), xy), mul(p2, add(r2, mul(2.0, mul(x, x))))))
        yd = add(mul(y, rad), add(mul(p1, add(r2, mul(2.0, mul(y, y)))), mul(mul(2.0, p2), xy)))
        sx = add(mul(fx, xd), cx)
        sy = add(mul(fy, yd), cy)
    return sx, sy


def build_map(source, ideal):
    """int32 [h', w', 2] = (qx, qy)."""
    sx, sy = source_coordinates(source, ideal)
    return np.stack([quant(sx, source["width"]), quant(sy, source["height"])], axis=-1)


def quant_table(table, source):
    """A caller's float32 [h', w', 2] table of (sx, sy) -> the map."""
    t = np.asarray(table, F).astype(np.float64)
    return np.stack([quant(t[:, :, 0], source["width"]), quant(t[:, :, 1], source["height"])], axis=-1)


def rectify_colour(bgr, qmap):
    """bgr [H, W, 3] uint8 (the whole source, decoded), qmap int32 [h', w', 2] -> Rc [h', w', 3] uint8."""
    bgr = np.asarray(bgr)
    assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape[2] == 3
    H, W = bgr.shape[:2]
    qx, qy = qmap[:, :, 0].astype(np.int64), qmap[:, :, 1].astype(np.int64)
    assert qx.min() >= -64 and qx.max() <= 32 * W + 32 and qy.min() >= -64 and qy.max() <= 32 * H + 32
    ix, ax, iy, ay = qx >> 5, qx & 31, qy >> 5, qy & 31
    pad = np.zeros((H + 6, W + 6, 3), np.int64)             # BORDER_CONSTANT: a tap outside the source is (0, 0, 0)
    pad[3:3 + H, 3:3 + W] = bgr
    t00, t10, t01, t11 = pad[iy + 3, ix + 3], pad[iy + 3, ix + 4], pad[iy + 4, ix + 3], pad[iy + 4, ix + 4]
    w00, w10, w01, w11 = ((32 - ax) * (32 - ay))[..., None], (ax * (32 - ay))[..., None], ((32 - ax) * ay)[..., None], (ax * ay)[..., None]
    out = (w00 * t00 + w10 * t10 + w01 * t01 + w11 * t11 + 512) >> 10
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def rectify_depth(depth, qmap, scale=1.0):
    """depth [H, W] uint16 or float32 (times scale = millimetres), qmap -> Rd [h', w'] uint16: the nearest source pixel, 0 outside."""
    depth = np.asarray(depth)
    d16 = IR.to_u16(depth, scale) if depth.dtype == np.float32 else depth
    assert d16.dtype == np.uint16
    H, W = d16.shape
    x, y = (qmap[:, :, 0].astype(np.int64) + 16) >> 5, (qmap[:, :, 1].astype(np.int64) + 16) >> 5
    pad = np.zeros((H + 6, W + 6), np.uint16)
    pad[3:3 + H, 3:3 + W] = d16
    return pad[y + 3, x + 3]


def decode(host, fmt, flags=("bt601", "limited")):
    """The [H, W, 3] BGR image of a whole source in the layout rectify_scenes.source builds."""
    host = np.asarray(host)
    if fmt in ("bgr", "bgra"):
        return np.ascontiguousarray(host[:, :, :3])
    if fmt in ("rgb", "rgba"):
        return np.ascontiguousarray(host[:, :, 2::-1])
    if fmt in ("bgr_planar", "rgb_planar"):
        img = np.transpose(host, (1, 2, 0))
        return np.ascontiguousarray(img if fmt == "bgr_planar" else img[:, :, ::-1])
    if fmt in ("nv12", "nv21"):
        h = host.shape[0] // 3 * 2
        return YR.yuv_to_bgr((host[:h], host[h:]), fmt, flags)
    return YR.yuv_to_bgr(host, fmt, flags)          # gray, yuy2, uyvy


def slot_colour(Rc, W, H, crop=(0, 0), flip_x=False, shift=(0, 0)):
    return IR.colour(Rc, W, H, "bgr", "hwc", crop, flip_x, shift)


def slot_depth(Rd, W, H, crop=(0, 0), flip_x=False, shift=(0, 0)):
    return IR.depth(Rd, W, H, crop, 1.0, flip_x, shift)
