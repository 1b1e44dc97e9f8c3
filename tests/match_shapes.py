"""Scenes and expected lists for tests/test_gpu_match_shapes.py: frame shapes whose level pitch W = width / T is no multiple of 4 (the
general k_refine<., false>), widths that are no multiple of 8, T outside {2, 4, 5, 8}, scanned levels without nibble memories.

Every expected list comes from TWO CPU references that must agree before the GPU is asked: the oracle (orc.Detector.match) and the numpy
restatement tests/masked_reference.py::match on the oracle's quantised pyramid.  Both are computed once per scene and kept.

Helper module (no test_ prefix): pytest does not collect it."""
import numpy as np

import masked_reference as mr
from conftest import assert_matches_equal


class Case:
    """One row of the shape table.  pitch_mod4: {level: W % 4 the row claims}; flags: further claims, checked by check_properties."""

    def __init__(self, name, M, size, T, pitch_mod4, flags=()):
        self.name, self.M, self.size, self.T, self.pitch_mod4, self.flags = name, M, size, list(T), dict(pitch_mod4), tuple(flags)
        self.L = len(self.T)

    def level_size(self, l):
        return self.size[0] >> l, self.size[1] >> l

    def pitch(self, l):
        return self.level_size(l)[0] // self.T[l]

    def refine_kernels(self):
        """The k_refine instantiations plan_match names, level L-2 down to 0: <LAST, W4> = (level == 0, pitch % 4 == 0)."""
        return ["k_refine<%s,%s>" % ("true" if l == 0 else "false", "true" if self.pitch(l) % 4 == 0 else "false")
                for l in range(self.L - 2, -1, -1)]


def nibble_rule(w, T):
    """lm_host.h nibble_supported(), restated: nibble-packed response memories exist for these scanned levels only."""
    return T in (2, 4, 5, 8) and w % 4 == 0 and (w // T) % 8 == 0


def check_properties(case):
    """The shape has what its row claims (asserted, not assumed), and lm_create's rule holds at every level."""
    for l in range(case.L):
        w, h = case.level_size(l)
        T = case.T[l]
        assert (w << l, h << l) == case.size, (case.name, l)                      # every level halves exactly
        assert w % T == 0 and h % T == 0 and (w * h) % 16 == 0, (case.name, l)
    for l, r in case.pitch_mod4.items():
        assert l < case.L - 1, (case.name, l)                                       # a level k_refine works at
        assert case.pitch(l) % 4 == r, (case.name, l, case.pitch(l))
    low_w = case.level_size(case.L - 1)[0]
    for f in case.flags:
        if f == "general_refine":          # at least one refined level takes k_refine<., false>
            assert any(case.pitch(l) % 4 != 0 for l in range(case.L - 1)), case.name
        elif f == "no_nibble":             # the byte scan without LM_FLAG_BYTE_RESPONSES
            assert not nibble_rule(low_w, case.T[-1]), case.name
        elif f == "nibble":                # k_scan4 / k_scan1 / k_scanl can run
            assert nibble_rule(low_w, case.T[-1]), case.name
        elif f == "width_not_8":           # the fallback quantisers and the generic k_linear_memories
            assert case.size[0] % 8 != 0, case.name
        elif f == "odd_pitch0":
            assert case.pitch(0) % 2 == 1, case.name
        elif f == "other_T":
            assert any(t not in (2, 4, 5, 8) for t in case.T), case.name
        elif f == "w4_behind_general":     # a W4 last level whose candidates come through a non-W4 level above it
            assert case.pitch(0) % 4 == 0 and case.pitch(1) % 4 != 0 and case.L == 3, case.name
        elif f == "both_general":          # k_refine<false,false> and k_refine<true,false> in one call
            assert case.L == 3 and case.pitch(0) % 4 != 0 and case.pitch(1) % 4 != 0, case.name
        else:
            raise AssertionError("unknown flag " + f)


CASES = [
    Case("rgbd-212x160-T4.2", 2, (212, 160), [4, 2], {0: 1}, ("general_refine", "no_nibble", "width_not_8", "odd_pitch0")),
    Case("rgbd-216x160-T4.4", 2, (216, 160), [4, 4], {0: 2}, ("general_refine",)),
    Case("color-220x160-T4.2", 1, (220, 160), [4, 2], {0: 3}, ("general_refine", "width_not_8", "odd_pitch0")),
    Case("rgbd-210x160-T5.5", 2, (210, 160), [5, 5], {0: 2}, ("general_refine", "width_not_8")),
    Case("color-210x160-T2.5", 1, (210, 160), [2, 5], {0: 1}, ("general_refine", "width_not_8", "odd_pitch0")),
    Case("rgbd-424x320-T4.4.2", 2, (424, 320), [4, 4, 2], {0: 2, 1: 1}, ("general_refine", "both_general")),
    Case("color-424x320-T2.2.2", 1, (424, 320), [2, 2, 2], {0: 0, 1: 2}, ("general_refine", "w4_behind_general")),
    Case("rgbd-240x168-T3.6", 2, (240, 168), [3, 6], {0: 0}, ("other_T", "no_nibble")),
    Case("color-224x224-T7.7", 1, (224, 224), [7, 7], {0: 0}, ("other_T", "no_nibble")),
    Case("rgbd-240x320-T8.5", 2, (240, 320), [8, 5], {0: 2}, ("general_refine", "nibble")),
    Case("color-240x320-T8.5", 1, (240, 320), [8, 5], {0: 2}, ("general_refine", "nibble")),
]
BY_NAME = {c.name: c for c in CASES}


class Scene:
    """Two frames of one shape (B = A rolled by odd offsets: the same edges at other positions and block phases, a seam where it wraps),
    the oracle's quantised pyramids, a bank, and the expected lists by (frame, threshold)."""

    def __init__(self, orc, synth, case, frame_seed, bank=None, two_frames=True):
        self.orc, self.case = orc, case
        w, h = case.size
        a = synth.make_frame(w, h, seed=frame_seed, n_shapes=14)
        self.frames = [a]
        if two_frames:
            self.frames.append(tuple(np.ascontiguousarray(np.roll(p, (7, 13), axis=(0, 1))) for p in a))
        self.o = orc.Detector(color_only=(case.M == 1), T=case.T)
        self.quant = []
        for f in range(len(self.frames)):
            self.o.prepare(self.bgr(f), self.depth(f))
            self.quant.append({(l, m): self.o.stage(0, l, m).reshape(h >> l, w >> l).copy() for l in range(case.L) for m in range(case.M)})
        self.descs, self.feats = bank(self) if bank is not None else (None, None)
        if self.descs is not None:
            self.o.add_class("c", self.descs, self.feats)
        self._lists, self._scans = {}, {}

    def bgr(self, f):
        return self.frames[f][0]

    def depth(self, f):
        return self.frames[f][1] if self.case.M == 2 else None

    def detector(self, lm, slots=16, **kw):
        w, h = self.case.size
        d = lm.Detector(lm.default_config(color_only=(self.case.M == 1), width=w, height=h, T=self.case.T, frame_slots=slots, **kw))
        d.add_class("c", self.descs, self.feats)
        return d

    def numpy_list(self, f, thr, **kw):
        return mr.match(self.orc, self.quant[f], [(self.descs, self.feats)], self.case.T, thr, **kw)

    def oracle_list(self, f, thr):
        return self.o.match(self.bgr(f), self.depth(f), thr, threads=8, cap=1 << 18)

    def expected(self, f, thr):
        """The list both references give; they are compared first, so a disagreement between them is reported as such."""
        key = (f, float(thr))
        if key not in self._lists:
            exp = self.oracle_list(f, thr)
            assert_matches_equal(self.numpy_list(f, thr), exp)
            exp.setflags(write=False)
            self._lists[key] = exp
        return self._lists[key]

    def scan_expected(self, f, thr):
        key = (f, float(thr))
        if key not in self._scans:
            self.o.prepare(self.bgr(f), self.depth(f))
            c = self.o.scan_candidates(thr, threads=8, cap=1 << 20)
            c.setflags(write=False)
            self._scans[key] = c
        return self._scans[key]


def table_scene(orc, synth, case):
    """The scene of the shape table: 40 templates, half of them crops of frame A's quantised images."""
    w, h = case.size

    def bank(s):
        descs, feats, crops = synth.make_bank(40, case.M, case.L, seed=7100 + w, quantized=s.quant[0], crop_fraction=0.5, frame_size=(w, h),
                                              T0=case.T[0], num_features=24, size_range=(24, 56))
        assert len(crops) >= 5
        return descs, feats
    return Scene(orc, synth, case, 7000 + w, bank)


def clamp_scene(orc, synth, case, tmpl_size):
    """Templates almost as large as the frame: max_x = w - tw - 8 T and max_y are negative, every candidate refines at (max_x, max_y)."""
    w, h = case.size

    def bank(s):
        descs, feats, _ = synth.make_bank(12, case.M, case.L, seed=7400 + w, fixed_l0_size=tmpl_size, num_features=24)
        return descs, feats
    return Scene(orc, synth, case, 7300 + w, bank, two_frames=False)


def floor_div(a, b):
    """The division a refinement must NOT use: equal to C's for a >= 0, one less for negative non-multiples."""
    return a // b
