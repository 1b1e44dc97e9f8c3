"""Crafted candidate lists for the feature selection (tests/test_select_cpu.py: numpy reference against the host's C++;
tests/test_gpu_select.py: lm_stage_select against the numpy reference).  A list is a dict: modality (0 colour, 1 depth), xy int16 [n, 2]
in row-major order, labels int32 [n], scores float32 [n], want, area (depth only).  Each list is built to break one wrong reading of
the rules: `>` for `>=` in the distance test (lattices whose neighbour distances hit d2 exactly), a key without the list index (equal
scores), a distance relaxed before the last candidate was visited (blocks that need many walks), a division by the wrong label's count
or by a reciprocal (scores that tie only after the division), an offset that is off by one (the batch)."""
import numpy as np


def _lst(modality, xy, labels, scores, want, area=None):
    xy = np.asarray(xy, np.int16).reshape(-1, 2)
    order = np.lexsort((xy[:, 0], xy[:, 1]))          # row-major: y, then x
    return {"modality": modality, "xy": np.ascontiguousarray(xy[order]), "labels": np.asarray(labels, np.int32)[order].copy(),
            "scores": np.asarray(scores, np.float32)[order].copy(), "want": int(want), "area": None if area is None else float(area)}


def _block(x0, y0, w, h):
    ys, xs = np.mgrid[y0:y0 + h, x0:x0 + w]
    return np.stack([xs.ravel(), ys.ravel()], 1)


def _random_positions(rng, n, width, height):
    p = rng.choice(width * height, size=n, replace=False)
    return np.stack([p % width, p // width], 1)


def _colour(rng, xy, want, values=None):
    n = len(xy)
    scores = (rng.choice(values, n) if values is not None else rng.integers(3100, 90000, n)).astype(np.float32)
    return _lst(0, xy, rng.integers(0, 8, n), scores, want)


def colour_cases():
    rng = np.random.default_rng(1511)
    c = {}
    c["n_eq_want_63"] = _colour(rng, _random_positions(rng, 63, 64, 48), 63)
    c["n_eq_want_31"] = _colour(rng, _random_positions(rng, 31, 40, 30), 31)
    c["n_eq_want_plus_1"] = _colour(rng, _random_positions(rng, 64, 64, 48), 63)
    c["n_eq_want_eq_1"] = _colour(rng, [[7, 9]], 1)
    # every score equal: the order is the list order
    c["stable_all_equal"] = _colour(rng, _block(3, 2, 20, 15), 20, values=[4000.0])
    c["stable_two_values"] = _colour(rng, _block(0, 0, 25, 12), 31, values=[4000.0, 4001.0])
    # an 8 x 8 block, want 63: distance 2, then 1 -- the lattice's neighbour distances 1, 2, 4 hit d2 exactly
    c["relax_8x8"] = _colour(rng, _block(10, 10, 8, 8), 63, values=[5000.0, 6000.0, 7000.0])
    # a dense 40 x 40 block, want 63: the initial distance is 1600 / 63 + 1 = 26, many walks before 63 fit
    c["relax_40x40"] = _colour(rng, _block(100, 50, 40, 40), 63)
    # two far clusters: the first walks keep one feature per cluster
    c["two_clusters"] = _colour(rng, np.concatenate([_block(5, 5, 9, 9), _block(500, 400, 9, 9)]), 63)
    for n in (1023, 1024, 1025):
        c["len_%d" % n] = _colour(rng, _random_positions(rng, n, 320, 240), 63)
    # many candidates per thread, many ties: 70 001 positions in 1280 x 960, scores from 16 values
    c["len_70001_ties"] = _colour(rng, _random_positions(rng, 70001, 1280, 960), 63, values=3200.0 + 97.0 * np.arange(16))
    c["too_few_want_minus_1"] = _colour(rng, _random_positions(rng, 62, 64, 48), 63)
    c["too_few_empty"] = _lst(0, np.zeros((0, 2)), np.zeros(0), np.zeros(0), 63)
    return c


def depth_cases():
    rng = np.random.default_rng(1512)
    c = {}
    # scores that tie only after the division: 2 / 4 against 3 / 6, 3 / 3 against 7 / 7; a label with one candidate (score 1 / 1).
    # 21 candidates on a 7 x 3 lattice, want 16, area 36: the distance starts at sqrtf(36) / sqrtf(16) + 1.5 = 3.0 exactly ...
    lab = np.array([0] * 4 + [1] * 6 + [2] * 3 + [3] * 7 + [4])
    sc = np.array([2.0] * 4 + [3.0] * 6 + [3.0] * 3 + [7.0] * 7 + [1.0])
    perm = rng.permutation(21)
    c["division_ties"] = _lst(1, _block(4, 4, 7, 3), lab[perm], sc[perm], 16, area=36.0)
    # ... and here, want 20 and area 50, it has a fractional part (3.08...), so the last walk runs at 0 < distance < 1
    perm = rng.permutation(21)
    c["fractional_last_pass"] = _lst(1, _block(4, 4, 7, 3), lab[perm], sc[perm], 20, area=50.0)
    # label counts that no reciprocal divides exactly: 3, 7, 11, 13, 23, 29, 41, 47 candidates, integer scores 2 .. 40
    lab = np.repeat(np.arange(8), [3, 7, 11, 13, 23, 29, 41, 47])
    xy = _random_positions(rng, len(lab), 60, 50)
    c["odd_label_counts"] = _lst(1, xy, rng.permutation(lab), rng.integers(2, 41, len(lab)), 63, area=2310.0)
    n = 6000
    c["interior_6000"] = _lst(1, _random_positions(rng, n, 160, 120), rng.integers(0, 8, n), rng.integers(2, 30, n), 63, area=9000.0)
    c["n_eq_want"] = _lst(1, _random_positions(rng, 31, 30, 30), rng.integers(0, 8, 31), rng.integers(2, 9, 31), 31, area=640.0)
    c["too_few_want_minus_1"] = _lst(1, _random_positions(rng, 30, 30, 30), rng.integers(0, 8, 30), rng.integers(2, 9, 30), 31, area=640.0)
    c["too_few_empty"] = _lst(1, np.zeros((0, 2)), np.zeros(0), np.zeros(0), 15, area=0.0)
    return c


def batch_lists(modality, count, seed):
    """`count` lists of mixed lengths for one call, empty and failing lists among them."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        want = int(rng.choice([63, 31, 15, 7]))
        n = [0, want - 1, want, want + 1, int(rng.integers(1, 40)), int(rng.integers(64, 3000))][k % 6]
        xy = _random_positions(rng, n, 96, 64) if n else np.zeros((0, 2))
        if modality == 0:
            out.append(_lst(0, xy, rng.integers(0, 8, n), rng.choice(3200.0 + 50.0 * np.arange(40), n) if n else np.zeros(0), want))
        else:
            out.append(_lst(1, xy, rng.integers(0, 8, n), rng.integers(2, 20, n), want, area=float(rng.integers(n, 4 * n + 2))))
    return out
