"""Numpy reference of the depth registration (include/linemod_hip.h "Raw depth registered onto the colour camera"),
written from the rule and not from the kernel: float32 arrays, ONE operation per statement (numpy rounds every ufunc call on its own and
cannot contract two of them), and a plain Python loop for the splat's minimum.

A camera is a dict(width, height, fx, fy, cx, cy, dist=(k1, k2, p1, p2, k3)); rays is the float32 [h, w, 2] table the detector returns
(Detector.registration_rays) or pinhole_rays' for a camera without distortion."""
import numpy as np

F = np.float32


def cam(width, height, fx, fy, cx, cy, dist=(0.0, 0.0, 0.0, 0.0, 0.0)):
    return dict(width=int(width), height=int(height), fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), dist=tuple(float(v) for v in dist))


def pinhole_rays(c):
    """The table of a camera with zero coefficients: float32((i - cx) / fx), float32((j - cy) / fy), the quotient taken in double with the
    float32 camera numbers the library holds."""
    i = np.arange(c["width"], dtype=np.float64)
    j = np.arange(c["height"], dtype=np.float64)
    rx = ((i - float(F(c["cx"]))) / float(F(c["fx"]))).astype(F)
    ry = ((j - float(F(c["cy"]))) / float(F(c["fy"]))).astype(F)
    out = np.zeros((c["height"], c["width"], 2), F)
    out[:, :, 0] = rx[None, :]
    out[:, :, 1] = ry[:, None]
    return out


def brown_forward(x, y, dist):
    """Normalised undistorted (x, y) -> distorted, in double: the model whose inverse the ray table holds."""
    k1, k2, p1, p2, k3 = dist
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y


def to_t(raw, scale=1.0):
    raw = np.asarray(raw)
    if raw.dtype == np.uint16:
        return raw.astype(F)
    assert raw.dtype == F
    with np.errstate(all="ignore"):
        return raw * F(scale)


def hits(t, rx, ry, colour, R, tr):
    """(dropped, u, v, m) per element of the float32 arrays t, rx, ry.  u, v: float32 whole numbers (meaningless where dropped), m uint32."""
    t, rx, ry = (np.asarray(a, F) for a in (t, rx, ry))
    R = np.asarray(R, F).reshape(3, 3)
    tr = np.asarray(tr, F).reshape(3)
    fx, fy, cx, cy = (F(colour[k]) for k in ("fx", "fy", "cx", "cy"))
    k1, k2, p1, p2, k3 = (F(v) for v in colour["dist"])
    one, two, half = F(1.0), F(2.0), F(0.5)
    with np.errstate(all="ignore"):
        ok = np.isfinite(t) & (t > 0)
        X = rx * t
        Y = ry * t
        P = []
        for r in range(3):
            s0 = R[r, 0] * X
            s1 = R[r, 1] * Y
            s01 = s0 + s1
            s2 = R[r, 2] * t
            s012 = s01 + s2
            P.append(s012 + tr[r])
        Xc, Yc, Zc = P
        ok &= np.isfinite(Zc) & (Zc > 0)
        a = Xc / Zc
        b = Yc / Zc
        aa = a * a
        bb = b * b
        ab = a * b
        r2 = aa + bb
        q = r2 * k3
        q = k2 + q
        q = r2 * q
        q = k1 + q
        q = r2 * q
        rad = one + q
        # ad = a * rad + ((2 * p1) * (a * b) + p2 * (r2 + 2 * (a * a)))
        t1 = (two * p1) * ab
        t2 = two * aa
        t2 = r2 + t2
        t2 = p2 * t2
        tang = t1 + t2
        ad = a * rad
        ad = ad + tang
        # bd = b * rad + (p1 * (r2 + 2 * (b * b)) + (2 * p2) * (a * b))
        t3 = two * bb
        t3 = r2 + t3
        t3 = p1 * t3
        t4 = (two * p2) * ab
        tang = t3 + t4
        bd = b * rad
        bd = bd + tang
        xf = fx * ad
        xf = xf + cx
        yf = fy * bd
        yf = yf + cy
        u = np.floor(xf + half)
        v = np.floor(yf + half)
        ok &= np.isfinite(u) & np.isfinite(v)
        m = np.minimum(np.rint(Zc), F(65535.0))
        ok &= m >= one
    assert all(x.dtype == F for x in (X, Xc, a, r2, rad, ad, bd, xf, u, m))
    mi = np.zeros(t.shape, np.uint32)
    mi[ok] = m[ok].astype(np.uint32)
    return ~ok, u, v, mi


def register(raw, scale, rays, colour, R, tr, splat=(0, 0), stats=False):
    """The registered image Rg, uint16 [colour height, colour width].  stats: also a dict of per-pixel arrays over Rg -- count (number of
    contributions), zmax (the farthest contribution, 0 without any), distinct (number of distinct contributed values) -- and n_valid,
    and (u, v) of the valid depth pixels."""
    rays = np.asarray(rays, F)
    dropped, u, v, m = hits(to_t(raw, scale), rays[:, :, 0], rays[:, :, 1], colour, R, tr)
    W, H = colour["width"], colour["height"]
    sx, sy = splat
    NONE = 1 << 32
    z = [[NONE] * W for _ in range(H)]
    contrib = {} if stats else None
    keep = ~dropped
    # compared as floats first: u, v may lie far outside the int range
    keep &= (u >= F(-sx)) & (u <= F(W - 1 + sx)) & (v >= F(-sy)) & (v <= F(H - 1 + sy))
    for uu, vv, mm in zip(u[keep].astype(np.int64).tolist(), v[keep].astype(np.int64).tolist(), m[keep].tolist()):
        for y in range(max(vv - sy, 0), min(vv + sy, H - 1) + 1):
            row = z[y]
            for x in range(max(uu - sx, 0), min(uu + sx, W - 1) + 1):
                if mm < row[x]:
                    row[x] = mm
                if stats:
                    contrib.setdefault((y, x), []).append(mm)
    Rg = np.array([[0 if q == NONE else q for q in row] for row in z], np.uint16).reshape(H, W)
    if not stats:
        return Rg
    count, zmax, distinct = (np.zeros((H, W), np.int64) for _ in range(3))
    for (y, x), lst in contrib.items():
        count[y, x], zmax[y, x], distinct[y, x] = len(lst), max(lst), len(set(lst))
    return Rg, dict(count=count, zmax=zmax, distinct=distinct, n_valid=int((~dropped).sum()), u=u[~dropped], v=v[~dropped])
