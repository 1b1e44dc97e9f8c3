"""Numpy reference of the float colour sources of lm_ingest_frames and the float destinations of lm_export_frames (include/linemod_hip.h,
DESIGN.md section 13 "Float sources"), written from the rule and not from the C++: a float32 multiply, np.rint, and numpy's own float16
for both directions of the half conversion.

    to_u8(v, scale):  t = float32(v) * float32(scale);  0 if t is NaN or t <= 0;  255 if t >= 255;  else rint(t) (ties to even)
    from_u8(c, scale): f = float32(c) * float32(scale);  F16: f.astype(float16) (one rounding, nearest even, overflow to +inf)

The sources are host arrays in the producer's layout: [h, w, 3 | 4] (hwc), [3, h, w] (chw) or [h, w] (gray), float32 or float16."""
import numpy as np

LAYOUTS = {0: ("hwc", 3, "bgr"), 1: ("hwc", 3, "rgb"), 2: ("hwc", 4, "bgr"), 3: ("hwc", 4, "rgb"), 4: ("chw", 3, "bgr"), 5: ("chw", 3, "rgb"),
           8: ("gray", 1, "bgr")}
PIX_FLOAT, PIX_FLOAT_F16 = 0x2000, 0x10
FORMATS = [PIX_FLOAT | el | lay for el in (0, PIX_FLOAT_F16) for lay in LAYOUTS]


def widen(v):
    """float16 or float32 array -> float32, exactly."""
    v = np.asarray(v)
    assert v.dtype in (np.float16, np.float32), v.dtype
    return v.astype(np.float32)


def half_bits(bits):
    """uint16 bit patterns -> float32 values, through numpy's float16."""
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def to_u8(v, scale):
    v = widen(v)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = v * np.float32(scale)
    assert t.dtype == np.float32
    out = np.zeros(t.shape, np.uint8)
    mid = (t > 0) & (t < np.float32(255))          # (comparisons with NaN are False)
    out[mid] = np.rint(t[mid]).astype(np.uint8)
    out[t >= np.float32(255)] = 255
    return out


def to_bgr(src, layout, order, scale):
    """The 8-bit BGR image [h, w, 3] the rule yields from the WHOLE source."""
    src = np.asarray(src)
    if layout == "gray":
        g = to_u8(src, scale)
        return np.stack([g, g, g], axis=-1)
    if layout == "chw":
        src = np.transpose(src, (1, 2, 0))
    px = to_u8(src[:, :, :3], scale)
    return np.ascontiguousarray(px[:, :, ::-1] if order == "rgb" else px)


def from_u8(c, scale, half):
    """Channel values -> the float32 bit patterns (uint32) or the float16 bit patterns (uint16) the export writes."""
    with np.errstate(over="ignore", under="ignore"):
        f = np.asarray(c, np.uint8).astype(np.float32) * np.float32(scale)
        assert f.dtype == np.float32
        return f.astype(np.float16).view(np.uint16) if half else f.view(np.uint32)


def draw_values(rng, n, dtype):
    """n source values for scale 1 (0 .. 255 floats): ties at k + 0.5, values next to them, negatives, values above 255, -0, NaN, +-inf and
    a subnormal, drawn so that every kind lands at every position of a 16-pixel lane sooner or later."""
    k = rng.integers(0, 256, n).astype(np.float32)
    kind = rng.integers(0, 12, n)
    v = rng.uniform(-20.0, 300.0, n).astype(np.float32)
    v = np.where(kind == 0, k + np.float32(0.5), v)
    v = np.where(kind == 1, np.nextafter(k + np.float32(0.5), np.float32(np.inf)), v)
    v = np.where(kind == 2, np.nextafter(k + np.float32(0.5), np.float32(-np.inf)), v)
    v = np.where(kind == 3, k, v)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 255.0, 254.5, 1e-40, -1e-3, 65504.0, 0.5], np.float32)
    v = np.where(kind >= 10, special[rng.integers(0, len(special), n)], v).astype(np.float32)
    with np.errstate(over="ignore"):
        return v.astype(dtype)


class Source:
    """One float colour source of `fmt` (PIX_FLOAT | element | layout) in a byte block that ENDS where the source ends: pixel (0, 0)
    `offset` bytes into it, rows `pad` elements longer than their pixels, planes `pad` elements further apart than their rows need.
    raw: the block (uint8); host: the same elements as a numpy array in the producer's layout ([h, w, 3 | 4], [3, h, w] or [h, w])."""

    def __init__(self, fmt, w, h, rng, offset=0, pad=1, values=None):
        self.fmt, self.w, self.h, self.offset = fmt, w, h, offset
        self.dtype = np.float16 if fmt & PIX_FLOAT_F16 else np.float32
        es = self.es = np.dtype(self.dtype).itemsize
        self.layout, self.nch, self.order = LAYOUTS[fmt & 15]
        assert fmt & ~0x1F == PIX_FLOAT and offset % es == 0
        inter = self.nch if self.layout != "chw" else 1
        row_bytes = w * inter * es
        self.row_stride = row_bytes + pad * es
        self.plane_stride = h * self.row_stride + pad * es if self.layout == "chw" else 0
        extent = 2 * self.plane_stride + (h - 1) * self.row_stride + row_bytes
        assert extent % es == 0
        # (offset is a multiple of es: the block's elements and the source's lie on one grid, the padding holds drawn values too)
        self.raw = np.frombuffer(draw_values(rng, (offset + extent) // es, self.dtype).tobytes(), np.uint8).copy()
        strided = np.lib.stride_tricks.as_strided
        el = self.raw[offset:].view(self.dtype)
        if self.layout == "gray":
            self.host = strided(el, (h, w), (self.row_stride, es))
        elif self.layout == "hwc":
            self.host = strided(el, (h, w, self.nch), (self.row_stride, es * self.nch, es))
        else:
            self.host = strided(el, (3, h, w), (self.plane_stride, self.row_stride, es))
        if values is not None:
            self.host[...] = values
        self._bgr = {}

    def strides(self):
        es = self.es
        return {"gray": (self.row_stride, es), "hwc": (self.row_stride, es * self.nch, es), "chw": (self.plane_stride, self.row_stride, es)}[self.layout]

    def bgr(self, scale):
        """The BGR image the rule yields from the whole source: computed once per scale and shared."""
        if scale not in self._bgr:
            self._bgr[scale] = to_bgr(self.host, self.layout, self.order, scale)
            self._bgr[scale].setflags(write=False)
        return self._bgr[scale]
