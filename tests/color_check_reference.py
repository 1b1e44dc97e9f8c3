"""References for the colour check (f1: HSV in-range mask, hull of a template's level-0 features, polygon fill counts), written from
the definitions in numpy and Python integers.  Nothing here is taken from csrc/lm_k_post.hip or host/PostProcess.cpp -- no division
table built with lrint of a double, no per-row interval, no error-accumulating line walk -- with ONE exception that is named where it
occurs: the tie rule of the outline's line (see `line_pixels`).

    hsv8_table(bgr)                    OpenCV's 8-bit BGR -> HSV rule in int64, tables by exact rational rounding
    hsv_real(bgr)                      textbook real-valued HSV in float64, H in [0, 180), S and V in [0, 255]
    inrange_mask(h, s, v, lo, hi)      cv::inRange with double bounds: round half to even, then compare unbounded integers
    convex_hull(points)                counter-clockwise vertices without collinear ones (scipy + exact integer degenerate cases)
    hull_pixels(hull)                  the closed polygon's lattice points plus its 8-connected outline, pixel by pixel
    counts(hull, offset, mask, w, h)   (pixels of the placed hull inside the frame, of those set in mask)
"""
from fractions import Fraction

import numpy as np

HSV_SHIFT = 12


def _round_half_up(q):
    return (2 * q.numerator + q.denominator) // (2 * q.denominator)


def _round_half_even(q):
    return round(q)                                   # Fraction.__round__ rounds half to even, exactly


def division_tables(rounding=_round_half_up):
    """sdiv[i] = round((255 << 12) / i), hdiv[i] = round((180 << 12) / (6 i)), i = 1 .. 255, entry 0 = 0; in exact arithmetic."""
    sdiv = [0] + [rounding(Fraction(255 << HSV_SHIFT, i)) for i in range(1, 256)]
    hdiv = [0] + [rounding(Fraction(180 << HSV_SHIFT, 6 * i)) for i in range(1, 256)]
    return np.array(sdiv, np.int64), np.array(hdiv, np.int64)


def division_table_ties():
    """The i in 1 .. 255 at which one of the two quotients lies exactly half-way between two integers (none, asserted by the CPU test)."""
    return [i for i in range(1, 256)
            if (2 * Fraction(255 << HSV_SHIFT, i)).denominator == 1 and (2 * Fraction(255 << HSV_SHIFT, i)).numerator % 2
            or (2 * Fraction(180 << HSV_SHIFT, 6 * i)).denominator == 1 and (2 * Fraction(180 << HSV_SHIFT, 6 * i)).numerator % 2]


_SDIV, _HDIV = division_tables()


def hsv8_table(bgr, priority="rgb"):
    """(H, S, V) int64 arrays of OpenCV's 8-bit rule for bgr[..., 3] uint8: V = max; S = (diff * sdiv[V] + 2048) >> 12; H from the sector of
    the maximum (priority R, then G, then B): g - b, b - r + 2 diff, r - g + 4 diff, times hdiv[diff], same rounding (the shift is an
    arithmetic one: floor), plus 180 when negative.  `priority` names the order in which the channels are asked "are you the maximum?";
    the CPU test shows that no order changes any H (two equal maxima lie on a sector border, where both sectors' formulas agree)."""
    c = np.asarray(bgr).astype(np.int64)
    b, g, r = c[..., 0], c[..., 1], c[..., 2]
    v = np.maximum(b, np.maximum(g, r))
    diff = v - np.minimum(b, np.minimum(g, r))
    s = (diff * _SDIV[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    sector = {"r": (r, g - b), "g": (g, b - r + 2 * diff), "b": (b, r - g + 4 * diff)}
    p0, p1, p2 = (sector[k] for k in priority)
    h = np.where(v == p0[0], p0[1], np.where(v == p1[0], p1[1], p2[1]))
    h = (h * _HDIV[diff] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def hsv_real(bgr):
    """(H, S, V) float64: V = max, S = 255 (max - min) / max (0 for black), H = half the hue angle in degrees, in [0, 180) (0 for greys)."""
    c = np.asarray(bgr).astype(np.float64)
    b, g, r = c[..., 0], c[..., 1], c[..., 2]
    v = np.maximum(b, np.maximum(g, r))
    diff = v - np.minimum(b, np.minimum(g, r))
    safe = np.where(diff > 0, diff, 1.0)
    deg = np.where(v == r, 60.0 * (g - b) / safe, np.where(v == g, 120.0 + 60.0 * (b - r) / safe, 240.0 + 60.0 * (r - g) / safe))
    deg = np.where(diff > 0, deg, 0.0)
    deg = np.where(deg < 0, deg + 360.0, deg)
    s = np.where(v > 0, 255.0 * diff / np.where(v > 0, v, 1.0), 0.0)
    return deg / 2.0, s, v


def round_bound(x):
    """A double bound as cv::inRange means it for 8-bit data: the nearest integer, ties to even, in exact arithmetic (a Python int)."""
    return round(float(x))


def inrange_mask(h, s, v, lower, upper):
    """Boolean array: lo <= value <= hi on all three channels, bounds rounded by `round_bound`, compared as unbounded integers (the
    channel values are 0 .. 255, so each channel's verdicts are a table of 256 Python comparisons)."""
    out = None
    for val, lo, hi in zip((h, s, v), lower, upper):
        lo, hi = round_bound(lo), round_bound(hi)
        tab = np.array([lo <= x <= hi for x in range(256)], bool)
        val = np.asarray(val)
        assert val.min() >= 0 and val.max() <= 255
        if tab.all() and out is not None:
            continue                                  # (this channel excludes nothing)
        ok = tab[val]
        out = ok if out is None else out & ok
    return out


def sv_pair_colours():
    """Colours [n, 3] uint8 (n a multiple of 8) that hold every pair (V, diff = V - min) -- the two table indices of the 8-bit rule; S is a
    function of the pair alone -- with the third channel at the minimum, the maximum and half-way, in all six channel orders."""
    v, d = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    v, d = v[d <= v], d[d <= v]
    mn = v - d
    out = []
    for mid in (mn, v, (mn + v) // 2):
        for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
            c = (v, mid, mn)
            out.append(np.stack([c[order[0]], c[order[1]], c[order[2]]], axis=1))
    out = np.concatenate(out).astype(np.uint8)
    return out[:len(out) // 8 * 8] if len(out) % 8 == 0 else np.concatenate([out, np.repeat(out[-1:], 8 - len(out) % 8, axis=0)])


# ---- hull ------------------------------------------------------------------------------------------------------------------------
def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(points):
    """Vertices of the convex hull of integer points as a list of (x, y) Python ints: counter-clockwise in the (x, y) plane (cross product
    of consecutive edges > 0), no collinear vertex, as cv::convexHull returns them.  One distinct point: that point.  All points on one
    line: its two extreme points, smaller (x, y) first.  Otherwise scipy.spatial.ConvexHull, then verified exactly: every turn strictly
    left, every input point on or left of every edge.  The starting vertex is not specified (the fill does not depend on it)."""
    pts = sorted({(int(x), int(y)) for x, y in points})
    if len(pts) <= 1:
        return pts
    a, b = pts[0], pts[-1]
    if all(_cross(a, b, p) == 0 for p in pts):
        return [a, b]
    from scipy.spatial import ConvexHull
    arr = np.array(pts, np.float64)
    hull = [pts[i] for i in ConvexHull(arr).vertices]
    n = len(hull)
    if sum(hull[i][0] * hull[(i + 1) % n][1] - hull[(i + 1) % n][0] * hull[i][1] for i in range(n)) < 0:
        hull.reverse()
    hull = [hull[i] for i in range(n) if _cross(hull[i - 1], hull[i], hull[(i + 1) % n]) != 0]
    n = len(hull)
    assert n >= 3 and all(_cross(hull[i - 1], hull[i], hull[(i + 1) % n]) > 0 for i in range(n)), "not strictly convex"
    px = np.array([p[0] for p in pts], np.int64); py = np.array([p[1] for p in pts], np.int64)
    for i in range(n):
        (ax, ay), (bx, by) = hull[i], hull[(i + 1) % n]
        assert ((bx - ax) * (py - ay) - (by - ay) * (px - ax) >= 0).all(), "a point lies outside the hull"
    return hull


def hull_edges(hull):
    """The outline's directed edges: vertex i to vertex i + 1, cyclically (a two-vertex hull has both directions; one vertex, none)."""
    n = len(hull)
    return [(hull[i], hull[(i + 1) % n]) for i in range(n)] if n > 1 else []


def edge_has_tie(a, b):
    """True when the exact line a-b passes half-way between two pixels at some step of its major axis."""
    M, m = sorted((abs(b[0] - a[0]), abs(b[1] - a[1])), reverse=True)
    return any((2 * k * m) % (2 * M) == M for k in range(1, M))


def line_pixels(a, b):
    """The 8-connected line from a to b in closed form: one pixel per step k = 0 .. M of the major axis (M = max(|dx|, |dy|); the x axis when
    |dx| >= |dy|), minor coordinate = start + sign * (integer nearest to k m / M), in integers.

    THE TIE RULE -- the one thing this file takes from the product.  Where k m / M is exactly half-way, the pixel FARTHER from a (nearer
    to b along the minor axis) is taken: floor((2 k m + M) / (2 M)).  The line is therefore not symmetric: a-b and b-a differ at ties, and
    the outline walks each edge from vertex i to vertex i + 1 of the counter-clockwise hull.  Established on the CPU against the walk
    in host/PostProcess.cpp's hull_counts (tests/test_color_check_cpu.py: the hull families hold edges with ties walked in each direction); that
    cv::fillPoly's outline is this line with this rule is what tests/test_opencv_vectors.py pins, where OpenCV is available."""
    dx, dy = b[0] - a[0], b[1] - a[1]
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    adx, ady = abs(dx), abs(dy)
    if adx >= ady:
        return [(a[0] + sx * k, a[1] + sy * ((2 * k * ady + adx) // (2 * adx) if adx else 0)) for k in range(adx + 1)]
    return [(a[0] + sx * ((2 * k * adx + ady) // (2 * ady)), a[1] + sy * k) for k in range(ady + 1)]


def hull_pixels(hull):
    """(x0, y0, img): img[y - y0, x - x0] is True for every pixel of the filled hull -- the lattice points of the closed polygon (cross
    product >= 0 against every edge of the counter-clockwise hull, integers) and the outline (`line_pixels` of every edge).  One vertex:
    that pixel; two: the closed segment's lattice points and both directed lines."""
    xs = [p[0] for p in hull]; ys = [p[1] for p in hull]
    x0, y0 = min(xs), min(ys)
    gx, gy = np.meshgrid(np.arange(x0, max(xs) + 1, dtype=np.int64), np.arange(y0, max(ys) + 1, dtype=np.int64))
    if len(hull) == 1:
        img = np.ones(gx.shape, bool)
    elif len(hull) == 2:
        (ax, ay), (bx, by) = hull
        img = (bx - ax) * (gy - ay) - (by - ay) * (gx - ax) == 0          # (inside the bounding box: on the closed segment)
    else:
        img = np.ones(gx.shape, bool)
        for (ax, ay), (bx, by) in hull_edges(hull):
            img &= (bx - ax) * (gy - ay) - (by - ay) * (gx - ax) >= 0
    for a, b in hull_edges(hull):
        for x, y in line_pixels(a, b):
            img[y - y0, x - x0] = True
    return x0, y0, img


def rows_are_runs(img):
    """True when the set pixels of every row of a boolean image are contiguous (or the row is empty)."""
    d = np.diff(np.pad(img.astype(np.int8), ((0, 0), (1, 1))), axis=1)
    return bool(((d == 1).sum(axis=1) <= 1).all())


def counts_of_pixels(px, offset, mask, w, h):
    """`counts` for an already rasterised hull (the result of hull_pixels): the hull is placed at `offset` and clipped to the w x h frame."""
    x0, y0, img = px
    x0 += int(offset[0]); y0 += int(offset[1])
    cx0, cy0 = max(x0, 0), max(y0, 0)
    cx1, cy1 = min(x0 + img.shape[1], w), min(y0 + img.shape[0], h)
    if cx0 >= cx1 or cy0 >= cy1:
        return 0, 0
    sub = img[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
    return int(sub.sum()), int((sub & mask[cy0:cy1, cx0:cx1]).sum())


def counts(hull, offset, mask, w, h):
    """(pixels of the hull placed at offset that lie inside the w x h frame, of those the ones set in the boolean mask[h, w])."""
    return counts_of_pixels(hull_pixels(hull), offset, mask, w, h)


# ---- hull families shared by the CPU and the GPU tests --------------------------------------------------------------------------------
def circle_lattice_points(n):
    """n lattice points in convex position: the shortest primitive vectors, one per direction, sorted by angle and summed give a
    lattice polygon with an even number of edges and no collinear vertex (for an odd n one vertex of the (n + 1)-gon is left out);
    translated so that all coordinates are >= 0."""
    m = n + n % 2
    r, half = 1, []
    while len(half) < m // 2:
        r += 1
        half = [(x, y) for x in range(-r, r + 1) for y in range(0, r + 1)
                if (y > 0 or x > 0) and np.gcd(abs(x), abs(y)) == 1 and x * x + y * y <= r * r]
    half.sort(key=lambda v: (v[0] * v[0] + v[1] * v[1], v))
    half = half[:m // 2]
    vecs = sorted(half + [(-x, -y) for x, y in half], key=lambda v: np.arctan2(v[1], v[0]))
    pts, x, y = [], 0, 0
    for vx, vy in vecs:
        pts.append((x, y)); x += vx; y += vy
    assert (x, y) == (0, 0)
    mx, my = min(p[0] for p in pts), min(p[1] for p in pts)
    return [(p[0] - mx, p[1] - my) for p in pts][:n]


def hull_families(rng, n_random=120, n_sliver=60, n_flat=40):
    """Point sets (lists of (x, y) >= 0) of the families the issue names, generated from `rng` (numpy Generator).  Returns a list of
    (family name, points)."""
    out = []
    for _ in range(n_random):
        n = int(rng.integers(1, 12))
        out.append(("random", [(int(x), int(y)) for x, y in rng.integers(0, 40, (n, 2))]))
    for _ in range(n_sliver):                                     # within one pixel of a line of random rational slope, up to 120 long
        p, q = int(rng.integers(-12, 13)), int(rng.integers(1, 13))
        steep = bool(rng.integers(0, 2))
        length = int(rng.integers(8, 121))
        n = int(rng.integers(3, 12))
        pts = []
        for _k in range(n):
            t = int(rng.integers(0, length + 1))
            u = (t * p) // q + int(rng.integers(-1, 2))
            pts.append((u, t) if steep else (t, u))
        mx, my = min(a for a, _ in pts), min(b for _, b in pts)
        out.append(("sliver", [(a - mx, b - my) for a, b in pts]))
    for k in range(n_flat):
        bw, bh = ((200, 6), (5, 150))[k % 2]
        n = int(rng.integers(3, 12))
        out.append(("flat" if k % 2 == 0 else "tall", [(int(rng.integers(0, bw + 1)), int(rng.integers(0, bh + 1))) for _ in range(n)]))
    for _ in range(20):                                           # all collinear on a slanted line: a two-vertex hull
        p, q = int(rng.integers(1, 8)), int(rng.integers(1, 8))
        sgn = 1 if rng.integers(0, 2) else -1
        ks = rng.integers(0, 12, int(rng.integers(2, 7)))
        if len(set(int(k) for k in ks)) < 2:
            ks = np.array([0, 5])
        pts = [(int(k) * p, sgn * int(k) * q) for k in ks]
        my = min(b for _, b in pts)
        out.append(("collinear", [(a, b - my) for a, b in pts]))
    out.append(("point", [(3, 4)]))
    out.append(("point", [(0, 0)]))
    out.append(("point_repeated", [(7, 2)] * 5))
    # edges with exact ties in the line, each in both directions (as a two-vertex hull both directions are walked; as a triangle's edge one)
    for (dx, dy) in [(2, 1), (1, 2), (6, 3), (3, 6), (2, -1), (1, -2), (6, -3), (10, 5), (4, 2), (14, 7), (6, 1), (1, 6), (10, 3), (3, 10)]:
        base = (0, max(0, -dy))
        a, b = base, (base[0] + dx, base[1] + dy)
        out.append(("tie_segment", [a, b]))
        for third in [(0, 20), (20, 0), (25, 25)]:
            if _cross(a, b, third) != 0:
                out.append(("tie_triangle", [a, b, third]))
    for _ in range(60):                                           # polygons of even-sided edges: many ties in every direction
        n = int(rng.integers(3, 9))
        out.append(("tie_even", [(2 * int(x), 2 * int(y)) for x, y in rng.integers(0, 16, (n, 2))]))
    return out


def placements(rng, bw, bh, w, h):
    """Offsets for a hull whose bounding box is [0, bw] x [0, bh]: well inside, straddling each border and corner, wholly outside on
    each side, far outside."""
    cx, cy = (w - bw) // 2 + int(rng.integers(-20, 21)), (h - bh) // 2 + int(rng.integers(-20, 21))
    sx0, sx1 = -(bw // 2) - 1, w - 1 - bw // 2
    sy0, sy1 = -(bh // 2) - 1, h - 1 - bh // 2
    far = 10 ** 6
    return [(cx, cy), (sx0, cy), (sx1, cy), (cx, sy0), (cx, sy1), (sx0, sy0), (sx1, sy0), (sx0, sy1), (sx1, sy1),
            (-bw - 1, cy), (w, cy), (cx, -bh - 1), (cx, h), (-bw, cy), (w - 1, cy), (cx, -bh), (cx, h - 1),
            (far, cy), (-far, cy), (cx, far), (cx, -far), (-far, far)]


def count_tie_edges(hulls):
    return sum(1 for hull in hulls for a, b in hull_edges(hull) if edge_has_tie(a, b))


# ---- the combined HSV ranges both test files use ------------------------------------------------------------------------------------
def combined_ranges():
    """(lower, upper) pairs: the range of the reference's shipped model, the one of test_color_check_counts_against_numpy_fill, bounds at
    0 / 179 / 180 / 255, fractional bounds (x.5 for even and odd x, x.49, x.51), lower > upper on one channel, and bounds outside 8 bits."""
    big = 1e12
    return [
        ([0, 0, 0], [255, 150, 255]),
        ([0, 0, 100], [180, 255, 255]),
        ([0, 0, 0], [0, 255, 255]), ([179, 0, 0], [179, 255, 255]), ([180, 0, 0], [255, 255, 255]), ([0, 0, 0], [179, 255, 255]),
        ([1, 0, 0], [178, 255, 255]), ([0, 255, 0], [255, 255, 255]), ([0, 0, 0], [255, 0, 255]), ([0, 0, 0], [255, 255, 0]),
        ([0, 0, 255], [255, 255, 255]), ([0, 1, 1], [180, 254, 254]),
        ([10.5, 0, 0], [20.5, 255, 255]), ([11.5, 0, 0], [21.5, 255, 255]),                 # ties: to even, 10 / 20 and 12 / 22
        ([0, 100.5, 0], [255, 200.5, 255]), ([0, 101.5, 0], [255, 201.5, 255]),
        ([0, 0, 50.5], [255, 255, 60.5]), ([0, 0, 51.5], [255, 255, 61.5]),
        ([30.49, 99.49, 50.49], [90.49, 199.49, 200.49]), ([30.51, 99.51, 50.51], [90.51, 199.51, 200.51]),
        ([0.5, 0.5, 0.5], [254.5, 254.5, 254.5]), ([-0.5, -0.5, -0.5], [178.5, 255.5, 255.5]),
        ([100, 0, 0], [50, 255, 255]), ([0, 200, 0], [255, 100, 255]), ([0, 0, 128], [255, 255, 127]),   # lower > upper: empty
        ([-1, -1, -1], [256, 256, 256]), ([-1, 0, 0], [-1, 255, 255]), ([0, 256, 0], [255, 256, 255]), ([0, 0, 0], [255, 255, -1]),
        ([0, 0, 0], [big, big, big]), ([-big, -big, -big], [255, 255, 255]), ([-big, 20, -big], [big, 180, big]),
        ([20, -big, 60], [160, big, 250]), ([big, 0, 0], [big, 255, 255]), ([0, 0, 0], [255, -big, 255]),
        ([0, 0, 0], [2147483648.0, 255, 4294967296.0]), ([-2147483649.0, -4294967296.0, 0], [255, 255, 255]),
    ]
