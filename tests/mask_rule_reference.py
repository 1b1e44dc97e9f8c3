"""Reference for the mask rules (include/linemod_hip.h, lm_mask_rule), a plain numpy restatement of the contract: seed = the enabled gates
ANDed, dilated with a (2r + 1)^2 square whose window is clipped to the image, then cut to a rectangle; 255 inside, 0 outside.  Nothing
here is taken from csrc/lm_k_mask.hip: no bit words, no doubling steps; the dilation is a maximum over explicitly sliced windows, and the
HSV gate is color_check_reference's independent 8-bit HSV rule (exact rational division tables) with its inRange.

A rule is a dict with the keyword arguments of Detector.set_mask_rule:
    modalities, depth_range=(zmin, zmax) | None, keep_invalid, hsv_range=(lower[3], upper[3]) | None, grow, rect=(x, y, w, h) | None
"""
import numpy as np

import color_check_reference as ccr


def depth_gate(depth, zmin, zmax, keep_invalid):
    d = np.asarray(depth).astype(np.int64)
    return np.where(d == 0, bool(keep_invalid), (d >= int(zmin)) & (d <= int(zmax)))


def hsv_gate(bgr, lower, upper):
    h, s, v = ccr.hsv8_table(bgr)
    return ccr.inrange_mask(h, s, v, lower, upper)


def dilate(seed, r):
    """out[y, x] = any(seed[max(y - r, 0) : y + r + 1, max(x - r, 0) : x + r + 1]): the window clipped to the image."""
    seed = np.asarray(seed, bool)
    h, w = seed.shape
    rows = np.zeros_like(seed)
    for dy in range(-r, r + 1):                       # rows[y] |= seed[y + dy] where y + dy is a row of the image
        lo, hi = max(0, -dy), min(h, h - dy)
        if lo < hi:
            rows[lo:hi] |= seed[lo + dy:hi + dy]
    out = np.zeros_like(seed)
    for dx in range(-r, r + 1):
        lo, hi = max(0, -dx), min(w, w - dx)
        if lo < hi:
            out[:, lo:hi] |= rows[:, lo + dx:hi + dx]
    return out


def dilate_windows(seed, r):
    """The same by the definition, one window per pixel (slow: the CPU test compares the two on small images)."""
    seed = np.asarray(seed, bool)
    h, w = seed.shape
    out = np.zeros_like(seed)
    for y in range(h):
        for x in range(w):
            out[y, x] = seed[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].any()
    return out


def seed_of(rule, bgr, depth, shape):
    seed = np.ones(shape, bool)
    if rule.get("depth_range") is not None:
        seed &= depth_gate(depth, rule["depth_range"][0], rule["depth_range"][1], rule.get("keep_invalid", False))
    if rule.get("hsv_range") is not None:
        seed &= hsv_gate(bgr, rule["hsv_range"][0], rule["hsv_range"][1])
    return seed


def mask_of(rule, bgr, depth, shape=None):
    """The rule's level-0 mask, uint8 0 / 255, for the frame (bgr [h, w, 3] uint8 or None, depth [h, w] uint16 or None)."""
    if shape is None:
        shape = (bgr if bgr is not None else depth).shape[:2]
    m = dilate(seed_of(rule, bgr, depth, shape), int(rule.get("grow", 0)))
    if rule.get("rect") is not None:
        x, y, w, h = (int(v) for v in rule["rect"])
        if not (w == 0 and h == 0):
            inside = np.zeros(shape, bool)
            inside[y:y + h, x:x + w] = True
            m = m & inside
    return m.astype(np.uint8) * np.uint8(255)


# ---- the crafted inputs the CPU and the GPU tests share ---------------------------------------------------------------------------------
SIZES = [(80, 80), (160, 80), (400, 240), (640, 480)]          # (w, h); the GPU test adds (100, 80), a width that is no multiple of 8
GROWS = [0, 1, 2, 7, 16]
ZMIN, ZMAX = 700, 900                                          # the depth gate the crafted seeds are written for


def depth_from_seed(seed):
    """A depth frame whose gate [ZMIN, ZMAX] (keep_invalid off) is `seed`: inside pixels at ZMIN, ZMAX or between, the others at
    ZMIN - 1, ZMAX + 1, 0 or 65535, in a fixed pattern."""
    seed = np.asarray(seed, bool)
    yy, xx = np.mgrid[0:seed.shape[0], 0:seed.shape[1]]
    k = (xx + 3 * yy) % 4
    inside = np.choose(k, [ZMIN, ZMAX, (ZMIN + ZMAX) // 2, ZMIN + 1])
    outside = np.choose(k, [ZMIN - 1, ZMAX + 1, 0, 65535])
    return np.where(seed, inside, outside).astype(np.uint16)


def crafted_seeds(w, h, r):
    """(name, seed[h, w] bool) for the frame size and grow: single pixels at the corners, at x = 63, 64 and w - 1, at y = 0 and h - 1, pairs
    2r + 1 and 2r + 2 apart (merged / not merged by the dilation), full, empty, random at 10 % and 90 %."""
    def single(x, y):
        s = np.zeros((h, w), bool)
        s[y, x] = True
        return s
    out = [("corner00", single(0, 0)), ("corner0w", single(w - 1, 0)), ("cornerh0", single(0, h - 1)), ("cornerhw", single(w - 1, h - 1)),
           ("x63", single(63, h // 2)), ("x64", single(64, h // 2)), ("xw1", single(w - 1, h // 3)),
           ("y0", single(w // 2, 0)), ("yh1", single(w // 3, h - 1))]
    for gap in (2 * r + 1, 2 * r + 2):
        # horizontal: the pixels strictly between two seeds `gap` apart number gap - 1; each seed covers r of them: merged iff gap - 1 <= 2r
        s = np.zeros((h, w), bool)
        x0 = min(64 - r - 1, w - 1 - gap)               # the pair straddles the border between two 64-pixel words (where the frame is wide enough)
        s[h // 2, x0] = s[h // 2, x0 + gap] = True
        s[10, 5] = s[10 + gap, 5] = True                # and a vertical pair
        out.append(("pair%d" % gap, s))
    out.append(("full", np.ones((h, w), bool)))
    out.append(("empty", np.zeros((h, w), bool)))
    # random seeds: a band of 34 columns in the middle stays empty, wider than the 2 * 16 columns the largest dilation closes, so that the
    # mask is neither all 0 nor all 255 at any grow (a 90 % field dilated by 16 would otherwise be one full frame like `full`)
    rng = np.random.default_rng(w * 1000 + h + r)
    for name, density in (("rand10", 0.10), ("rand90", 0.90)):
        s = rng.random((h, w)) < density
        s[:, w // 2 - 17:w // 2 + 17] = False
        out.append((name, s))
    return out


def gap_is_merged(mask_row_or_col, a, b):
    """True when every pixel strictly between positions a < b is set."""
    return bool(np.asarray(mask_row_or_col)[a + 1:b].all())


def depth_edge_cases(w=80, h=80):
    """(depth frame, [rules]) around the gate's edges: columns of d = ZMIN - 1, ZMIN, ZMAX, ZMAX + 1, 0, 65535 (and values between), with
    keep_invalid off and on, and a gate with zmin == zmax."""
    vals = np.array([ZMIN - 1, ZMIN, ZMAX, ZMAX + 1, 0, 65535, ZMIN + 1, ZMAX - 1, 1, 65534], np.uint16)
    yy, xx = np.mgrid[0:h, 0:w]
    depth = vals[(xx + 7 * yy) % len(vals)]
    rules = [dict(modalities=3, depth_range=(ZMIN, ZMAX), keep_invalid=False), dict(modalities=3, depth_range=(ZMIN, ZMAX), keep_invalid=True),
             dict(modalities=3, depth_range=(ZMIN, ZMIN), keep_invalid=False), dict(modalities=3, depth_range=(ZMAX, ZMAX), keep_invalid=True),
             dict(modalities=3, depth_range=(0, 65535), keep_invalid=False), dict(modalities=3, depth_range=(65535, 65535), keep_invalid=False)]
    return depth, rules


HSV_LOWER, HSV_UPPER = (20, 60, 70), (90, 200, 220)


def hsv_edge_frame(w=160, h=80):
    """A frame of seeded random colours.  `hsv_edge_coverage` counts the pixels it holds on each edge of the gate [HSV_LOWER, HSV_UPPER]
    (the CPU test asserts that none is missing)."""
    rng = np.random.default_rng(2024)
    bgr = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    return bgr


def hsv_edge_coverage(bgr, lower=HSV_LOWER, upper=HSV_UPPER):
    """{(channel, which): count} of pixels whose channel value is exactly lower - 1, lower, upper, upper + 1 while the two other
    channels lie inside the range: the pixels on which an off-by-one of one bound shows."""
    hsv = ccr.hsv8_table(bgr)
    cov = {}
    for c in range(3):
        others = np.ones(hsv[0].shape, bool)
        for o in range(3):
            if o != c:
                others &= (hsv[o] >= lower[o]) & (hsv[o] <= upper[o])
        for which, val in (("lower-1", lower[c] - 1), ("lower", lower[c]), ("upper", upper[c]), ("upper+1", upper[c] + 1)):
            cov[(c, which)] = int(((hsv[c] == val) & others).sum())
    return cov


def rect_cases(w, h):
    """(name, seed, rule): rectangles in the interior, touching each edge of the frame, the whole frame, 1 x 1 on a set pixel, and a
    seed pixel just outside the rectangle whose dilation must not leak past it."""
    rng = np.random.default_rng(7 * w + h)
    seed = rng.random((h, w)) < 0.3
    seed[h // 2, w // 2] = True
    out = []
    for name, rect in (("interior", (w // 4, h // 4, w // 2, h // 2)), ("left", (0, 10, 20, 30)), ("top", (10, 0, 30, 20)),
                       ("right", (w - 20, 5, 20, 30)), ("bottom", (5, h - 20, 30, 20)), ("frame", (0, 0, w, h)),
                       ("one", (w // 2, h // 2, 1, 1)), ("corner", (w - 1, h - 1, 1, 1))):
        s = seed.copy()
        if name == "frame":
            s[0, 0] = False                                # (grow 0 below: the full-frame rectangle's mask is the seed, not all 255)
        if name == "corner":
            s[h - 1, w - 1] = True
            s[h - 3:h - 1, w - 3:w] = False; s[h - 1, w - 3:w - 1] = False      # its neighbours are off: only grow 0 keeps it a 1 x 1 answer
        out.append((name, s, dict(modalities=3, depth_range=(ZMIN, ZMAX), grow=0 if name in ("frame", "corner") else 1, rect=rect)))
    x0, y0 = w // 2, h // 2
    leak = np.zeros((h, w), bool)
    leak[y0, x0 - 1] = True                                # one pixel left of the rectangle's first column
    leak[y0 - 6, x0 + 4] = True                            # and one pixel above its first row
    out.append(("leak", leak, dict(modalities=3, depth_range=(ZMIN, ZMAX), grow=3, rect=(x0, y0 - 5, 20, 20))))
    return out
