"""The scenes of the rectification tests (tests/test_rectify_cpu.py, tests/test_gpu_rectify.py): cameras, lenses and seeded sources with
per-pixel noise in every source format, so that an error of one pixel or one weight shows.  Built once and left unchanged."""
import numpy as np

import rectify_reference as QR

W, H = 160, 80                      # the RGB-D detector
MW, MH = 64, 32                     # the colour-only detector
SW, SH = 208, 120                   # the source camera's geometry
CROP = (24, 20)
ZERO = QR.ZERO
LENS = (-0.25, 0.06, 0.004, -0.003, 0.01)           # k1 = -0.25: a barrel strong enough to leave the source in the corners

COLOUR_FORMATS = ["bgr", "rgb", "bgra", "rgba", "bgr_planar", "rgb_planar", "gray", "nv12", "nv21", "yuy2", "uyvy"]
# what image_desc wants for each, and one non-default matrix per YUV format
DESC = {
    "bgr": dict(order="bgr", layout="hwc"), "rgb": dict(order="rgb", layout="hwc"), "bgra": dict(order="bgr", layout="hwc"),
    "rgba": dict(order="rgb", layout="hwc"), "bgr_planar": dict(order="bgr", layout="chw"), "rgb_planar": dict(order="rgb", layout="chw"),
    "gray": dict(layout="gray"), "nv12": dict(layout="nv12", matrix="bt709", range="limited"), "nv21": dict(layout="nv21", matrix="bt601", range="full"),
    "yuy2": dict(layout="yuy2", matrix="bt709", range="full"), "uyvy": dict(layout="uyvy", matrix="bt709", range="limited"),
}


def flags(fmt):
    d = DESC[fmt]
    return (d.get("matrix", "bt601"), d.get("range", "limited"))


def source_cam(dist=LENS, w=SW, h=SH):
    return QR.cam(w, h, 130.0, 131.0, 103.5 * w / SW, 59.5 * h / SH, dist)


def ideal_cam(w=SW, h=SH):
    """The source's pinhole, or (another size) a pure rescale of it about the principal point."""
    return QR.cam(w, h, 130.0 * w / SW, 131.0 * h / SH, (103.5 + 0.5) * w / SW - 0.5, (59.5 + 0.5) * h / SH - 0.5)


def source(fmt, w=SW, h=SH, seed=1):
    """A whole source image of `fmt` as the host array image_desc's layout wants (uint8): [h, w, 3 | 4], [3, h, w], [h, w] (gray),
    [h * 3 / 2, w] (nv12 / nv21: the chroma rows behind the Y rows), [h, w, 2] (yuy2 / uyvy).  Every byte is noise."""
    rng = np.random.default_rng(1000 * seed + COLOUR_FORMATS.index(fmt))
    shape = {"bgr": (h, w, 3), "rgb": (h, w, 3), "bgra": (h, w, 4), "rgba": (h, w, 4), "bgr_planar": (3, h, w), "rgb_planar": (3, h, w),
             "gray": (h, w), "nv12": (h * 3 // 2, w), "nv21": (h * 3 // 2, w), "yuy2": (h, w, 2), "uyvy": (h, w, 2)}[fmt]
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    a.setflags(write=False)
    return a


def depth_u16(w=SW, h=SH, seed=5):
    rng = np.random.default_rng(seed)
    d = rng.integers(400, 3000, (h, w)).astype(np.uint16)
    d[rng.random((h, w)) < 0.02] = 0
    d.setflags(write=False)
    return d


def depth_f32(w=SW, h=SH, seed=6):
    """Metres (scale 1000) with NaN, infinities, negatives, ties and values beyond the u16 range strewn in."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.4, 3.0, (h, w)).astype(np.float32)
    special = np.array([0.0, np.nan, np.inf, -1.0, 1e9, -np.inf, 0.0005, 0.0015, 65.535, 70.0], np.float32)
    at = rng.random((h, w)) < 0.05
    d[at] = special[rng.integers(0, len(special), int(at.sum()))]
    d.setflags(write=False)
    return d


def smooth_table(w, h, sw=SW, sh=SH, seed=21):
    """A caller's map: a smooth warp of the source (a rotation by a few degrees plus a sinusoidal wobble) with special entries strewn in:
    NaN, infinities, far outside, exact ties (k / 64, k odd) and entries on the last row and column."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    a = np.deg2rad(4.0)
    x, y = i * (sw - 1) / max(w - 1, 1) - sw / 2, j * (sh - 1) / max(h - 1, 1) - sh / 2
    sx = np.cos(a) * x - np.sin(a) * y + sw / 2 + 1.5 * np.sin(j / 7.0)
    sy = np.sin(a) * x + np.cos(a) * y + sh / 2 + 1.5 * np.cos(i / 9.0)
    t = np.stack([sx, sy], axis=-1).astype(np.float32)
    special = [(np.nan, 10.0), (10.0, np.nan), (np.inf, 5.0), (5.0, -np.inf), (1e30, 1e30), (-1e30, 3.0), (-500.0, 20.0), (20.0, 5000.0),
               (33.0 / 64.0, 35.0 / 64.0), (1001.0 / 64.0, 2047.0 / 64.0), (sw - 1.0, sh - 1.0), (sw - 1.0, 7.25), (9.5, sh - 1.0),
               (sw - 0.5, sh - 0.5), (-0.5, -0.5), (-1.0, -1.0), (sw, sh), (sw + 1.0, 3.0), (-2.0, -2.0), (sw - 1.0 + 1.0 / 64.0, 0.0)]
    flat = t.reshape(-1, 2)
    where = rng.choice(len(flat), size=min(len(flat), 3 * len(special)), replace=False)
    for n, k in enumerate(where):
        flat[k] = special[n % len(special)]
    t.setflags(write=False)
    return t


def lay_out(host, pad, planar=False):
    """A source array -> (its bytes with every row `pad` bytes longer than its pixels, cut where the last row's pixels end; row_stride).
    The planes of a planar source ([3, h, w]) and the chroma rows of NV12 / NV21 are further rows of the same stride."""
    a = np.ascontiguousarray(host)
    rows2d = a.view(np.uint8).reshape(a.shape[0] * a.shape[1] if planar else a.shape[0], -1)
    n, rb = rows2d.shape
    rs = rb + pad
    buf = np.zeros(n * rs, np.uint8)
    buf.reshape(n, rs)[:, :rb] = rows2d
    return buf[:(n - 1) * rs + rb], rs


def wide_ideal(w=SW, h=SH):
    """An ideal camera that sees more than the lens delivers: part of its geometry maps outside the source."""
    return QR.cam(w, h, 90.0, 90.0, (w - 1) / 2.0, (h - 1) / 2.0)
