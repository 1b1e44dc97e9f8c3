"""lm_export_frames in numpy, written from the rule in include/linemod_hip.h and from nothing else: whole-image
integer arrays and one loop over the primitives.  coverage() also runs on Python's unbounded integers (exact=True), so the 64-bit
extremes of the segment test are checked against arithmetic that cannot overflow.

    annotate(F, prims, frame)        -> A: F with the primitives of `frame` composited in list order
    undo(A, flip_x, (sx, sy))        -> E: the ingest's mirror and shift undone
    pack(E, fmt) / nv12(E, row)      -> the destination window's bytes
    render(...)                      -> a whole destination surface, written into a copy of what was there
"""
import numpy as np

RING, SEGMENT, BOX = 0, 1, 2

# matrix / range -> Y0, (cyr, cyg, cyb), (cur, cug, cub), (cvr, cvg, cvb)
YUV_ROWS = {
    ("bt601", "limited"): (16, (16829, 33039, 6416), (-9714, -19071, 28784), (28784, -24103, -4681)),
    ("bt709", "limited"): (16, (11966, 40254, 4064), (-6596, -22189, 28784), (28784, -26145, -2639)),
    ("bt601", "full"): (0, (19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329)),
    ("bt709", "full"): (0, (13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005)),
}
# the float matrices the integer rows round: (Kr, Kb) and the range's scales
YUV_FLOAT = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def coverage(p, w, h, exact=False):
    """bool [h, w]: the pixels primitive p covers.  p: anything indexable by the lm_draw_prim field names."""
    dt = object if exact else np.int64
    y, x = np.mgrid[0:h, 0:w]
    x, y = x.astype(dt), y.astype(dt)
    kind, x0, y0, x1, y1, t = (int(p[k]) for k in ("kind", "x0", "y0", "x1", "y1", "thickness"))
    if kind == RING:
        r = x1
        q = 4 * ((x - x0) ** 2 + (y - y0) ** 2)
        c = q < (2 * r + t) ** 2
        if 2 * r >= t:
            c = c & (q >= (2 * r - t) ** 2)
        return c.astype(bool)
    if kind == SEGMENT:
        dx, dy = x1 - x0, y1 - y0
        L2 = dx * dx + dy * dy
        wx, wy = x - x0, y - y0
        s = wx * dx + wy * dy
        cap_a = 4 * (wx * wx + wy * wy) <= t * t
        cap_b = 4 * ((x - x1) ** 2 + (y - y1) ** 2) <= t * t
        cross = wx * dy - wy * dx
        inner = 4 * cross * cross <= t * t * L2
        first = (s <= 0) if L2 else np.ones((h, w), bool)
        return np.where(first.astype(bool), cap_a, np.where((s >= L2).astype(bool), cap_b, inner)).astype(bool)
    if kind == BOX:
        outer = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
        inner = (x >= x0 + t) & (x <= x1 - t) & (y >= y0 + t) & (y <= y1 - t)
        return (outer & ~inner).astype(bool)
    raise ValueError("kind %d" % kind)


def blend(c, p, a):
    t = c.astype(np.int64) * (255 - a) + int(p) * a + 128
    return ((t + (t >> 8)) >> 8).astype(np.uint8)


def annotate(F, prims, frame):
    A = F.copy()
    h, w = A.shape[:2]
    for p in prims:
        if int(p["frame"]) != frame:
            continue
        c = coverage(p, w, h)
        for ch, name in enumerate("bgr"):
            A[..., ch][c] = blend(A[..., ch][c], p[name], int(p["a"]))
    return A


def undo(A, flip_x=False, shift=(0, 0)):
    h, w = A.shape[:2]
    v, u = np.mgrid[0:h, 0:w]
    x = np.where(flip_x, w - 1 - u, u) + int(shift[0])
    y = v + int(shift[1])
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    E = np.zeros_like(A)
    E[inside] = A[y[inside], x[inside]]
    return E


def nv12(E, matrix="bt601", range_="limited"):
    """(Y [h, w], UV [h / 2, w]) uint8 of the BGR image E"""
    y0, cy, cu, cv = YUV_ROWS[matrix, range_]
    B, G, R = (E[..., k].astype(np.int64) for k in range(3))
    Y = np.clip((cy[0] * R + cy[1] * G + cy[2] * B + (y0 << 16) + 32768) >> 16, 0, 255).astype(np.uint8)
    h, w = Y.shape
    s = [c.reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3)) for c in (R, G, B)]
    U = np.clip((cu[0] * s[0] + cu[1] * s[1] + cu[2] * s[2] + (128 << 18) + (1 << 17)) >> 18, 0, 255).astype(np.uint8)
    V = np.clip((cv[0] * s[0] + cv[1] * s[1] + cv[2] * s[2] + (128 << 18) + (1 << 17)) >> 18, 0, 255).astype(np.uint8)
    return Y, np.stack([U, V], axis=-1).reshape(h // 2, w)


def yuv_float(rgb, matrix, range_):
    """float64 (Y, U, V) of float64 (R, G, B) triples [n, 3] in 0 .. 255, unrounded and unclamped: the standard matrices"""
    kr, kb = YUV_FLOAT[matrix]
    kg = 1.0 - kr - kb
    R, G, B = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    y = kr * R + kg * G + kb * B
    u = (B - y) / (2.0 * (1.0 - kb))
    v = (R - y) / (2.0 * (1.0 - kr))
    if range_ == "limited":
        return 16.0 + y * 219.0 / 255.0, 128.0 + u * 224.0 / 255.0, 128.0 + v * 224.0 / 255.0
    return y, 128.0 + u, 128.0 + v


class Surface:
    """A destination: `raw` bytes (guards included) that stand for device memory, and where the window's planes lie in them.
    layout hwc (px 3 | 4) / chw / nv12; offset = data's offset in raw; everything else as lm_image_desc."""

    def __init__(self, layout, order, px, width, height, window, row_stride, plane_stride, offset, nbytes, matrix="bt601", range_="limited"):
        self.layout, self.order, self.px, self.width, self.height = layout, order, px, width, height
        self.window, self.row_stride, self.plane_stride, self.offset, self.nbytes = window, row_stride, plane_stride, offset, nbytes
        self.matrix, self.range = matrix, range_

    def write(self, raw, E):
        """E into the window of `raw` (a uint8 array of nbytes); every other byte is left as it is"""
        h, w = E.shape[:2]
        cx, cy = self.window
        C = E[..., ::-1] if self.order == "rgb" else E
        rows = (np.arange(h) + cy)[:, None] * self.row_stride
        if self.layout == "hwc":
            cols = (np.arange(w) + cx)[None, :] * self.px
            for c in range(3):
                raw[self.offset + rows + cols + c] = C[..., c]
            if self.px == 4:
                raw[self.offset + rows + cols + 3] = 255
        elif self.layout == "chw":
            cols = (np.arange(w) + cx)[None, :]
            for c in range(3):
                raw[self.offset + c * self.plane_stride + rows + cols] = C[..., c]
        else:
            Y, UV = nv12(E, self.matrix, self.range)
            cols = (np.arange(w) + cx)[None, :]
            raw[self.offset + rows + cols] = Y
            crow = (np.arange(h // 2) + cy // 2)[:, None] * self.row_stride
            raw[self.offset + self.plane_stride + crow + cols] = UV
        return raw


def render(raw, surface, F, prims, frame, flip_x=False, shift=(0, 0)):
    """What an export of frame F leaves in the surface's memory"""
    return surface.write(raw.copy(), undo(annotate(F, prims, frame), flip_x, shift))
