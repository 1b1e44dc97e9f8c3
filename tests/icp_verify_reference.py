"""numpy restatement of the ICP branch's best-pose check (the reference's HighLevelLinemodIcp.cpp:93-137, estimateBestMatch): the mask of
valid pixels, cv::erode 3x3 twice with its default border value, the mean absolute depth difference over the eroded mask, and the rule
that picks a group's pose and accepts or rejects the group."""
import numpy as np

SCENE_MIN = 600
CORRECT_ESTIMATE_THRESHOLD = 35


def m0(render, scene, scene_min=SCENE_MIN):
    """render > 1 and scene > scene_min"""
    return (np.asarray(render, np.int64) > 1) & (np.asarray(scene, np.int64) > scene_min)


def erode3(mask):
    """One 3x3 erosion of a boolean image; a neighbour outside the image is ignored (cv::erode's default border value: the border
    does not erode)."""
    m = np.asarray(mask, bool)
    h, w = m.shape
    p = np.ones((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = m
    out = np.ones((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + h, dx:dx + w]
    return out


def erode3_border_erodes(mask):
    """The wrong erosion a zero border gives (what the tests must tell apart from erode3)."""
    m = np.asarray(mask, bool)
    h, w = m.shape
    p = np.zeros((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = m
    out = np.ones((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + h, dx:dx + w]
    return out


def window5(mask):
    """Every in-image pixel of the 5x5 window is set: the fused form of two erode3 on a rectangle, written per pixel."""
    m = np.asarray(mask, bool)
    h, w = m.shape
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            out[y, x] = m[max(y - 2, 0):min(y + 3, h), max(x - 2, 0):min(x + 3, w)].all()
    return out


def eroded_mask(render, scene, scene_min=SCENE_MIN):
    return erode3(erode3(m0(render, scene, scene_min)))


def verify(render, scene, scene_min=SCENE_MIN):
    """(count, sum, mean): the eroded mask's pixels, the integer sum of |scene - render| over them, sum / count (0.0 for an empty mask)"""
    mask = eroded_mask(render, scene, scene_min)
    diff = np.abs(np.asarray(scene, np.int64) - np.asarray(render, np.int64))
    count = int(mask.sum())
    total = int(diff[mask].sum())
    return count, total, (float(total) / float(count) if count else 0.0)


def select_best(means):
    """estimateBestMatch's loop on the means: pose i is kept if (mean < bestMean and mean != 0) or i == 0, bestMean being the kept mean
    truncated to uint16; accepted when bestMean <= 35 and the list is not empty.  Returns (accepted, best index)."""
    best_mean, best_pose = 0, 0
    for i, mean in enumerate(means):
        if (mean < best_mean and mean != 0) or i == 0:
            best_pose = i
            best_mean = int(mean) & 0xFFFF      # (uint16_t)mean of a non-negative mean below 2^16: the truncation
    return (best_mean <= CORRECT_ESTIMATE_THRESHOLD and len(means) > 0), best_pose
