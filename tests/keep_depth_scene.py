"""The 160 x 80 scene of the keep-depth tests (tests/test_gpu_keep_depth.py): a window of the golden frame that holds the part, a second
depth image for it, and a colour-only bank LEARNED from the window by the CPU oracle (rectangular object masks, two classes), so that a
colour-only match finds real matches at every threshold the tests use.  Built once and left unchanged."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
W, H = 160, 80
X0, Y0 = 242, 254                     # the window's corner in the golden frame: the part's rim and the table around it
T = [2, 8]
# object masks of the learned templates, (x, y, w, h) in the window, per class
MASKS = [[(67, 27, 68, 47), (89, 17, 54, 40), (28, 9, 56, 58), (10, 4, 78, 48), (55, 13, 91, 55)],
         [(32, 28, 89, 41), (17, 18, 47, 40), (24, 19, 98, 34), (33, 13, 94, 36), (10, 8, 41, 55), (13, 29, 69, 46)]]
THRESHOLD = 60.0                      # the oracle finds 23 matches of the bank in the window at this threshold (asserted by the tests' fixture)
_cache = {}


def frame():
    """(bgr [80, 160, 3], depth [80, 160]) of the window."""
    if "frame" not in _cache:
        f = np.load(os.path.join(GOLDEN, "frame0.npz"))
        bgr = np.ascontiguousarray(f["bgr"][Y0:Y0 + H, X0:X0 + W])
        depth = np.ascontiguousarray(f["depth"][Y0:Y0 + H, X0:X0 + W])
        bgr.setflags(write=False); depth.setflags(write=False)
        _cache["frame"] = (bgr, depth)
    return _cache["frame"]


def other_depth(seed=5):
    """A depth image that differs from the window's everywhere it can: noise of 2 .. 3999 mm with 0 / 1 holes."""
    rng = np.random.default_rng(seed)
    d = rng.integers(2, 4000, (H, W)).astype(np.uint16)
    d[rng.random((H, W)) < 0.1] = 0
    d[rng.random((H, W)) < 0.05] = 1
    return d


def bank(orc):
    """[(class id, descs, features)] of the colour-only bank, learned by the oracle from the window."""
    if "bank" not in _cache:
        bgr, _ = frame()
        o = orc.Detector(color_only=True, T=T)
        out = []
        for c, masks in enumerate(MASKS):
            for (x, y, w, h) in masks:
                m = np.zeros((H, W), np.uint8)
                m[y:y + h, x:x + w] = 255
                tid, _bb = o.add_template("part%d" % c, bgr, None, m)
                assert tid >= 0, ("the oracle could not learn a template from mask", c, (x, y, w, h))
        for c in range(len(MASKS)):
            descs, feats = o.export_class(c)
            out.append(("part%d" % c, descs, feats))
        o.close()
        _cache["bank"] = out
    return _cache["bank"]


def bank_rgbd(orc):
    """(class id, descs, features) of a small RGB-D bank learned from the window: the RGB-D detector of the comparison needs one to match at all."""
    if "bank_rgbd" not in _cache:
        bgr, depth = frame()
        o = orc.Detector(color_only=False, T=[5, 8])
        for (x, y, w, h) in MASKS[0][:3]:
            m = np.zeros((H, W), np.uint8)
            m[y:y + h, x:x + w] = 255
            tid, _bb = o.add_template("part0", bgr, depth, m)
            assert tid >= 0
        descs, feats = o.export_class(0)
        o.close()
        _cache["bank_rgbd"] = ("part0", descs, feats)
    return _cache["bank_rgbd"]


def shifted(img, ox, oy):
    """img translated by (ox, oy) pixels, zeros shifted in (the uploads' shift)."""
    out = np.zeros_like(img)
    h, w = img.shape[:2]
    out[max(oy, 0):h + min(oy, 0), max(ox, 0):w + min(ox, 0)] = img[max(-oy, 0):h - max(oy, 0), max(-ox, 0):w - max(ox, 0)]
    return out
