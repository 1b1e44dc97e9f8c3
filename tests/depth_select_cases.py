"""The depth check's sorted order statistic, as numpy states it, and the pixel patterns the CPU and GPU tests of the selection share
(tests/test_depth_select_cpu.py, tests/test_gpu_depth_select.py).  Nothing here is taken from the kernel or from PostProcess.cpp."""
import numpy as np


def rule(crop, k):
    """The element at 0-based index k of the ascending sort of t = (d <= 1) ? 65535 : d; an empty crop gives 65535."""
    d = np.asarray(crop, np.uint16)
    if d.size == 0:
        return 65535
    t = np.where(d <= 1, 65535, d).astype(np.uint16)
    return int(np.sort(t.ravel())[k])


def patterns(h, w, seed=0):
    """name -> [h, w] uint16: the value families of the issue, for a crop of h x w pixels whose depth-check rank is k = n // 5."""
    n = h * w
    k = n // 5
    rng = np.random.default_rng(seed + 1000 * h + w)
    out = {}

    def shuffled(flat):
        flat = np.asarray(flat, np.uint16).copy()
        rng.shuffle(flat)
        return flat.reshape(h, w)

    out["equal"] = np.full((h, w), 1234, np.uint16)                                     # contention and ties
    out["holes"] = shuffled(np.arange(n) % 2)                                           # all 0 or 1: 65535
    # 0x00FF and 0x0100 around the rank: k values of 0x00FF (index k is the first 0x0100) and k + 1 of them (index k is the last 0x00FF)
    out["straddle_above"] = shuffled([0x00FF] * k + [0x0100] * (n - k))
    out["straddle_below"] = shuffled([0x00FF] * min(k + 1, n) + [0x0100] * (n - min(k + 1, n)))
    out["first_bin"] = shuffled(2 + (np.arange(n) * 7) % 254)                           # every value below 256: the rank falls in bin 0
    # mostly holes and far values: the rank falls in the last bin; real 65535s among them
    far = np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 3 == 1, 65535, 0xFF00 + (np.arange(n) * 5) % 256))
    if n >= 10:
        far[: n // 10] = 700                                                            # a few near values, fewer than k
    out["last_bin"] = shuffled(far)
    out["real_65535_and_holes"] = shuffled(np.where(np.arange(n) % 4 == 0, 65535, np.where(np.arange(n) % 4 == 1, 1, 900 + np.arange(n) % 4)))
    step = max(1, 65000 // max(n, 1))
    out["gradient"] = shuffled(2 + np.arange(n) * step) if n <= 65000 else shuffled(2 + np.arange(n) % 65000)   # every value distinct (n <= 65000)
    smooth = 800 + (np.add.outer(np.arange(h), np.arange(w)) // 3) + rng.integers(0, 4, (h, w))
    smooth[rng.random((h, w)) < 0.1] = 0                                                # a smooth surface with holes
    out["smooth"] = smooth.astype(np.uint16)
    return out
