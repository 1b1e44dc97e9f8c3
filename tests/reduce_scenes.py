"""The scenes of the reduction tests (tests/test_reduce_cpu.py, tests/test_gpu_reduce.py): the ratio list, one seeded noise source per
colour format family -- interleaved, 4-byte, planar, 4:2:0, 4:2:2, an 8-bit Bayer mosaic and a packed 10-bit raw one under a raw
pipeline -- with the BGR image its format's own reference decodes from the WHOLE source, and the depth sources.  Built once per size and
left unchanged."""
import numpy as np

import ingest_bayer_reference as BR
import ingest_raw_reference as WR
import rectify_reference as QR
import rectify_scenes as S

W, H = S.W, S.H                     # the RGB-D detector, 160 x 80
MW, MH = S.MW, S.MH                 # the colour-only detector, 64 x 32

# num / den, or one per axis
RATIOS = [(2, 1), (3, 1), (9, 4), (8, 1), (16, 5), (1, 1), ((3, 1), (9, 4))]
FAMILIES = ["bgr", "rgba", "bgr_planar", "nv12", "yuy2", "bayer_grbg", "raw_rggb10p"]

# the raw pipeline of the raw family: a black level, unequal gains, a matrix with negative entries, a display curve
PIPE = dict(black=40, gain=np.array([1434, 1024, 1741], np.int64), ccm=np.array([[1331, -205, -102], [-154, 1280, -102], [-51, -307, 1382]], np.int64),
            tone=np.rint(255.0 * (np.arange(4096) / 4095.0) ** (1 / 2.2)).astype(np.uint8))
PIPE_FLOAT = dict(black=40, gains=PIPE["gain"] / 1024.0, ccm=PIPE["ccm"] / 1024.0, tone=PIPE["tone"])

KIND = {"bgr": 0, "rgba": 1, "bgr_planar": 2, "u16": 3, "f32": 4, "nv12": 6, "yuy2": 8, "bayer_grbg": 10 + 1, "raw_rggb10p": 14 + 4 * 8 + 0}
MATRIX = {("bt601", "limited"): 0, ("bt709", "limited"): 1, ("bt601", "full"): 2, ("bt709", "full"): 3}
# what image_desc wants for each family
DESC = dict(S.DESC, bayer_grbg=dict(layout="bayer_grbg"), raw_rggb10p=dict(layout="bayer_rggb", bits=10, packed=True))


def even(fmt):
    """The format needs an even width and height."""
    return fmt in ("nv12", "yuy2", "bayer_grbg", "raw_rggb10p")


def colour(fmt, w, h, seed=1):
    """(host array as image_desc's layout wants it, the decoded [h, w, 3] BGR image of the whole source)."""
    if fmt in S.COLOUR_FORMATS:
        host = S.source(fmt, w, h, seed)
        return host, QR.decode(host, fmt, S.flags(fmt))
    rng = np.random.default_rng(7000 * seed + FAMILIES.index(fmt))
    if fmt == "bayer_grbg":
        host = rng.integers(0, 256, (h, w), dtype=np.uint8)
        bgr = BR.demosaic(host, "grbg")
    else:
        samples = rng.integers(0, 1024, (h, w))
        host = WR.pack(samples, 10)
        bgr = np.ascontiguousarray(WR.process(samples, 10, "rggb", PIPE)).astype(np.uint8)
    host.setflags(write=False)
    return host, bgr


def flags(fmt):
    return S.flags(fmt) if fmt in S.DESC else ("bt601", "limited")


def desc(fmt, w):
    """image_desc's keywords for a source of `fmt` that is w pixels wide."""
    d = dict(DESC[fmt])
    if fmt == "raw_rggb10p":
        d["width"] = w
    return d


def depth(dfmt, w, h):
    """(host array, scale)"""
    return (S.depth_u16(w, h), 1.0) if dfmt == "u16" else (S.depth_f32(w, h), 1000.0)


def source_size(slot, ratio, extra):
    """The smallest source side whose reduced side is slot + extra, plus one pixel where that leaves the reduced side unchanged: a tail."""
    num, den = ratio
    n = -(-(slot + extra) * num // den)
    return n + 1 if ((n + 1) * den) // num == slot + extra else n
