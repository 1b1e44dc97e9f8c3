"""The reference of the high-bit raw ingest formats and of the raw pipeline (include/linemod_hip.h, DESIGN.md section 13 "High-bit raw
sources and the raw pipeline"), in numpy int64, vectorised and written from the header's text: how samples lie in u16 containers and in
PFNC-packed rows (pack, unpack, container, uncontainer), and process(): black level -> bilinear demosaic of the WHOLE source on N-bit
samples (mono: R = G = B) -> shift to 16 bits -> gains -> matrix -> tone table, as [H, W, 3] uint8 B, G, R; then slot(): the window,
mirror and shift of that image as a slot holds it.  Patterns are "rggb", "grbg", "gbrg", "bggr" (the top-left 2 x 2 tile in reading
order) and "mono".  A pipeline is a dict(black, gain [3], ccm [3, 3], tone [4096]) of integers, Q10.  No GPU, no library."""
import numpy as np

PATTERNS = ("rggb", "grbg", "gbrg", "bggr")
MONO = "mono"


def pattern_index(pattern):
    """The format's pattern field: red_x | red_y << 1, or 4 for mono."""
    return 4 if pattern == MONO else PATTERNS.index(pattern)


def identity():
    return dict(black=0, gain=np.full(3, 1024, np.int64), ccm=1024 * np.eye(3, dtype=np.int64), tone=(np.arange(4096) >> 4).astype(np.uint8))


def pack(samples, bits):
    """[H, W] samples below 2^bits -> [H, ceil(W * bits / 8)] uint8: sample c of a row is bits [bits * c, bits * c + bits) of the row read
    as a little-endian bit string."""
    s = np.asarray(samples).astype(np.int64)
    assert s.ndim == 2 and s.min() >= 0 and s.max() < (1 << bits)
    H, W = s.shape
    bitplane = ((s[:, :, None] >> np.arange(bits)) & 1).reshape(H, W * bits)            # bit b of the row
    nbytes = (W * bits + 7) // 8
    bitplane = np.concatenate([bitplane, np.zeros((H, nbytes * 8 - W * bits), np.int64)], axis=1)
    return (bitplane.reshape(H, nbytes, 8) << np.arange(8)).sum(axis=2).astype(np.uint8)


def unpack(rows, bits, width):
    """The header's formula: ((b[k] | b[k+1] << 8) >> (bits * c & 7)) & (2^bits - 1), k = bits * c >> 3."""
    b = np.asarray(rows).astype(np.int64)
    c = np.arange(width)
    k, ph = (bits * c) >> 3, (bits * c) & 7
    return (((b[:, k] | (b[:, k + 1] << 8)) >> ph) & ((1 << bits) - 1)).astype(np.int64)


def container(samples):
    """[H, W] -> little-endian u16, the sample in the low bits."""
    return np.asarray(samples).astype("<u2")


def uncontainer(words, bits):
    """A sample is min(s, 2^bits - 1): stray high bits clamp."""
    return np.minimum(np.asarray(words).astype(np.int64), (1 << bits) - 1)


def demosaic_channels(s, pattern):
    """Step 2: [H, W] int64 -> (R, G, B) int64 by the bilinear rule of the 8-bit Bayer formats (reflection -1 -> 1, w -> w - 2)."""
    H, W = s.shape
    if pattern == MONO:
        return s, s, s
    assert H % 2 == 0 and W % 2 == 0 and H >= 2 and W >= 2
    S = np.pad(s, 1, mode="reflect")
    c = S[1:-1, 1:-1]
    left, right, up, down = S[1:-1, :-2], S[1:-1, 2:], S[:-2, 1:-1], S[2:, 1:-1]
    h, v = (left + right + 1) >> 1, (up + down + 1) >> 1
    p = (left + right + up + down + 2) >> 2
    d = (S[:-2, :-2] + S[:-2, 2:] + S[2:, :-2] + S[2:, 2:] + 2) >> 2
    i = PATTERNS.index(pattern)
    y, x = np.mgrid[0:H, 0:W]
    dx, dy = (x ^ (i & 1)) & 1, (y ^ (i >> 1)) & 1
    sites = [(dx == 0) & (dy == 0), (dx == 1) & (dy == 1), (dx == 1) & (dy == 0), (dx == 0) & (dy == 1)]
    return np.select(sites, [c, d, h, v]), np.select(sites, [p, p, c, c]), np.select(sites, [d, c, v, h])


def pipeline_channels(R, G, B, bits, pipe):
    """Steps 3 - 6 on N-bit channels -> [.., 3] uint8 B, G, R.  int64, with the 32-bit bounds of the header asserted."""
    gain, ccm, tone = np.asarray(pipe["gain"], np.int64), np.asarray(pipe["ccm"], np.int64).reshape(3, 3), np.asarray(pipe["tone"], np.uint8)
    x = []
    for c, v in enumerate((R, G, B)):
        t = (v << (16 - bits)) * gain[c] + 512
        assert t.min() >= 0 and t.max() < 2 ** 32
        x.append(np.minimum(t >> 10, 65535))
    out = []
    for i in range(3):
        t = ccm[i, 0] * x[0] + ccm[i, 1] * x[1] + ccm[i, 2] * x[2] + 512
        assert t.min() >= -2 ** 31 and t.max() < 2 ** 31
        out.append(tone[np.clip(t >> 10, 0, 65535) >> 4])
    return np.stack([out[2], out[1], out[0]], axis=-1)


def process(samples, bits, pattern, pipe=None):
    """[H, W] unpacked samples (already clamped to N bits) -> the BGR image the rule yields from the whole source."""
    pipe = identity() if pipe is None else pipe
    s = np.asarray(samples).astype(np.int64)
    assert s.ndim == 2 and s.min() >= 0 and s.max() < (1 << bits)
    s = np.maximum(s - int(pipe["black"]), 0)
    R, G, B = demosaic_channels(s, pattern)
    return pipeline_channels(R, G, B, bits, pipe)


def slot(bgr, W, H, crop=(0, 0), flip_x=False, shift=(0, 0)):
    """The W x H slot: the window at `crop`, mirrored, translated by `shift` with zeros shifted in."""
    win = bgr[crop[1]:crop[1] + H, crop[0]:crop[0] + W]
    assert win.shape[:2] == (H, W)
    if flip_x:
        win = win[:, ::-1]
    out = np.zeros_like(win)
    sx, sy = shift
    if abs(sx) < W and abs(sy) < H:
        out[max(sy, 0):H + min(sy, 0), max(sx, 0):W + min(sx, 0)] = win[max(-sy, 0):H + min(-sy, 0), max(-sx, 0):W + min(-sx, 0)]
    return out
