"""addTemplate's feature selection restated in numpy: lmh::select_color / lmh::select_depth and pick_scattered of csrc/lm_extract.cpp.

    select(modality, xy, labels, scores, want, area) -> FEATURE rows (x, y, label) in the host's order, or None for "fewer than want".

Every float is np.float32 and every operation is one IEEE single-precision operation, as in the C++: the depth scores' division by the
label count, the stable sort by score descending (equal scores keep the list order), the initial distance (colour: n / want + 1 in
integers; depth: sqrtf(area) / sqrtf(want) + 1.5f) and the walk -- cyclic over the sorted list, keep a candidate iff
(float)(dx * dx + dy * dy) >= d2 against everything kept, after the last candidate distance -= 1 and d2 = distance * distance.

The walk is written with one integer per candidate, the smallest squared distance to anything kept: "far enough from everything kept"
is (float)that >= d2, because the int -> float conversion is monotone.  Within one walk d2 is fixed and the kept set only grows, so a
candidate that failed stays failed; the next candidate the host keeps is the first one at or after its cursor that still passes.
tests/test_select_cpu.py holds this file to the C++ itself (tests/cpp/select_dump.cpp links lm_extract.cpp)."""
import numpy as np

F32 = np.float32


def initial_distance(modality, n, want, area=None):
    if modality == 0:
        return F32(n // want + 1)
    return F32(F32(np.sqrt(F32(area))) / F32(np.sqrt(F32(want))) + F32(1.5))


def sorted_order(modality, labels, scores):
    s = np.asarray(scores, F32)
    if modality == 1:
        cnt = np.bincount(np.asarray(labels, np.int64), minlength=8)
        s = (s / cnt[labels].astype(F32)).astype(F32)
    return np.argsort(-s, kind="stable")


def select(modality, xy, labels, scores, want, area=None):
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    labels = np.asarray(labels, np.int64)
    n = len(labels)
    if n < want:
        return None
    order = sorted_order(modality, labels, scores)
    x, y = xy[order, 0], xy[order, 1]
    distance = initial_distance(modality, n, want, area)
    d2 = F32(distance * distance)
    mind2 = np.full(n, np.iinfo(np.int64).max // 4, np.int64)
    kept = []
    while True:
        alive = mind2.astype(F32) >= d2 if kept else np.ones(n, bool)
        pos = 0
        while pos < n and alive[pos:].any():
            i = pos + int(np.argmax(alive[pos:]))
            kept.append(i)
            if len(kept) == want:
                k = order[np.array(kept)]
                return np.stack([xy[k, 0], xy[k, 1], labels[k]], 1).astype(np.int32)
            dd = (x - x[i]) ** 2 + (y - y[i]) ** 2
            mind2 = np.minimum(mind2, dd)
            alive &= dd.astype(F32) >= d2
            pos = i + 1
        distance = F32(distance - F32(1.0))
        d2 = F32(distance * distance)
        if distance < 0:
            raise ValueError("the host's walk does not end on this list (repeated positions)")
