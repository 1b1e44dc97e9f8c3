"""Route cases, frame contents and CPU references for tests/test_preprocess_routes_cpu.py and tests/test_gpu_preprocess_routes.py: every
pre-processing route (a3-a10) at its smallest shapes, with a different frame in every slot.

A row CLAIMS a route, the exact set of kernels its call launches (spelled as lmh::pre_kernel_name spells them) and geometric properties
(a partial last strip, a tall image, a row wider than one wave's 62 segments, ...).  Nothing is assumed: the CPU test asks the planner
(tests/cpp/preprocess_route_dump.cpp) for every row's plan and recomputes the geometry from the shape.

Expected planes come from TWO CPU references that must agree before the GPU is asked: orc.Detector (prepare + stage) and the same planes
composed from the oracle's single stages (composed_planes).

Helper module (no test_ prefix): pytest does not collect it."""
import zlib

import numpy as np

# LM_TUNE_* knobs of the pre-processing and their defaults as lm_set_tuning takes them.  The first two belong to a detector, the others are
# process-wide (a test restores them).
KNOB_DEFAULTS = {"BATCH_PHASES": 2, "PHASE_MAX_SLOTS": 15, "BLUR_PYR": 3, "BLUR_STRIP": 0, "CBLUR_VARIANT": 0, "CGRAD_VARIANT": 0,
                 "CGRAD_LEVELS": 1, "PYRDOWN_VARIANT": 0, "DMEDIAN_VARIANT": 0}
CONFIG_DEFAULTS = {"weak_threshold": 10.0, "distance_threshold": 2000, "difference_threshold": 50, "flags": 0}


class Case:
    """One row: a call of n_slots frames on slots [first_slot, first_slot + n_slots) of a detector of total_slots slots."""

    def __init__(self, name, M, size, T, n_slots, route, kernels, flags=(), knobs=None, config=None, lut="default", first_slot=0, total_slots=None, threshold=60.0):
        self.name, self.M, self.size, self.T, self.n_slots, self.route = name, M, tuple(size), list(T), n_slots, route
        self.kernels, self.flags = frozenset(kernels), tuple(flags)
        self.knobs = dict(KNOB_DEFAULTS, **(knobs or {}))
        self.config = dict(CONFIG_DEFAULTS, **(config or {}))
        self.lut, self.first_slot, self.threshold = lut, first_slot, float(threshold)      # threshold: of the match lists
        self.total_slots = total_slots if total_slots is not None else max(first_slot + n_slots, 2)
        self.L = len(self.T)
        assert set(self.knobs) == set(KNOB_DEFAULTS) and set(self.config) == set(CONFIG_DEFAULTS), name

    def level_size(self, l):
        return self.size[0] >> l, self.size[1] >> l

    def plan_line(self):
        """The row as tests/cpp/preprocess_route_dump.cpp reads it.  A lane's call with the other lanes idle (others_busy 0)."""
        w, h = self.size
        T = self.T + [8] * (4 - self.L)
        k = self.knobs
        v = [self.name, w, h, self.M, self.L] + T + [self.n_slots, k["PHASE_MAX_SLOTS"], k["BATCH_PHASES"], 0, 0 if self.lut == "bytes" else 1,
                                                    self.config["flags"] & 1, k["CBLUR_VARIANT"], k["CGRAD_VARIANT"], k["PYRDOWN_VARIANT"],
                                                    k["DMEDIAN_VARIANT"], k["BLUR_PYR"], k["BLUR_STRIP"], k["CGRAD_LEVELS"]]
        return " ".join(str(x) for x in v)

    def reference_key(self):
        """Rows with the same key share frames, oracle planes, bank and lists."""
        return (self.size, self.M, tuple(self.T), tuple(sorted(self.config.items())), self.lut, self.threshold)

    def content_seed(self):
        c = self.config
        return zlib.crc32(repr((self.size, self.M, c["weak_threshold"], c["distance_threshold"], c["difference_threshold"])).encode())


def parse_plan(text):
    """'kernel param grid [+lds] [nb/g]; ...' of the dump -> [(kernel, param, (gx, gy, gz))]"""
    steps = []
    for st in text.split(";"):
        f = st.split()
        if not f:
            continue
        g = [int(x) for x in f[2].split("x")]
        steps.append((f[0], int(f[1]), tuple(g + [1] * (3 - len(g)))))
    return steps


def lm_create_accepts(case):
    """lm_create's shape rule restated (cols % T == 0, rows % T == 0, rows x cols % 16 == 0 at every level; levels halve exactly)."""
    for l in range(case.L):
        w, h = case.level_size(l)
        if (w << l, h << l) != case.size or w % case.T[l] or h % case.T[l] or (w * h) % 16:
            return False
    return 1 <= case.total_slots <= 1024 and case.first_slot + case.n_slots <= case.total_slots


def _strip0(h):
    return 32 if h > 640 else 16


# geometric claims, each recomputed from the row (steps: the planner's launches of the row)
GEOMETRY = {
    "partial_strip0": lambda c, s: c.size[1] % _strip0(c.size[1]) != 0,            # level 0's last blur / gradient strip is short
    "partial_strip0_32": lambda c, s: c.size[1] % 32 != 0,                          # ... when 32-row strips are forced
    "whole_strips0": lambda c, s: c.size[1] % _strip0(c.size[1]) == 0,
    "partial_strip1": lambda c, s: (c.size[1] // 2) % 16 != 0,                     # level 1's last 16-row strip is short
    "half_strip1": lambda c, s: (c.size[1] // 2) % 16 == 8,
    "tall": lambda c, s: c.size[1] > 640,                                           # 32-row strips: the <.., 32, 32> and <1, 32> instantiations
    "not_tall": lambda c, s: c.size[1] <= 640,
    "one_band1": lambda c, s: (c.size[1] // 2) // c.T[1] == 1,                      # level 1 is one band of T rows
    "blur_row_gt62": lambda c, s: c.size[0] * 3 // 16 > 62,                         # a row of 16-byte blur lanes spans several waves
    "grad_row_gt62": lambda c, s: c.size[0] // 16 > 62,                             # a row of 16-pixel gradient lanes spans several waves
    "grad_row_le62": lambda c, s: c.size[0] // 16 <= 62,
    "n_not_mult4": lambda c, s: c.n_slots % 4 != 0,
    "n_mult16": lambda c, s: c.n_slots % 16 == 0,
    "n_odd": lambda c, s: c.n_slots % 2 == 1,
    "one_frame": lambda c, s: c.n_slots == 1,
    "first_slot_nonzero": lambda c, s: c.first_slot > 0 and c.first_slot + c.n_slots < c.total_slots,
    "lm_pitch80": lambda c, s: ((c.size[0] >> 1) // c.T[1]) % 80 == 0,
    "lm_pitch_not80": lambda c, s: ((c.size[0] >> 1) // c.T[1]) % 80 != 0,
    "row_bytes1_not32": lambda c, s: ((c.size[0] >> 1) * 3) % 32 != 0,             # no matrix-core blur at level 1
    "w_16_not_32": lambda c, s: c.size[0] % 16 == 0 and c.size[0] % 32 != 0,
    "w_8_not_16": lambda c, s: c.size[0] % 8 == 0 and c.size[0] % 16 != 0,
    "w_not_8": lambda c, s: c.size[0] % 8 != 0,
    "three_levels": lambda c, s: c.L == 3,
    "slots_gt256": lambda c, s: c.n_slots > 256,                                    # block-index ranges beyond 8 bits of slot
    "interleave": lambda c, s: any(k.startswith("k_blur_pyr<") and p == 1 for k, p, _ in s),
    "no_interleave": lambda c, s: any(k.startswith("k_blur_pyr<") and p == 0 for k, p, _ in s),
    "mx_strip96": lambda c, s: any(k in ("k_blur_mx_pyr", "k_cblur_mx") and p == 96 for k, p, _ in s),
    "lut_bytes": lambda c, s: c.lut == "bytes",
    "weak_off_integer": lambda c, s: float(c.config["weak_threshold"] ** 2) != int(c.config["weak_threshold"] ** 2),
    "depth_full_range": lambda c, s: c.config["distance_threshold"] > 65535,
    "per_pixel_taps": lambda c, s: c.config["difference_threshold"] > 5461,        # k_dnormal's body above the packed taps
    "double_products": lambda c, s: 250 <= c.config["difference_threshold"] <= 5461,
}


def check_claims(case, route, steps):
    """The planner's route and launches are what the row claims; its geometry is what the shape gives."""
    assert lm_create_accepts(case), case.name
    assert route == case.route, (case.name, route)
    planned = frozenset(k for k, _, _ in steps)
    assert planned == case.kernels, (case.name, "planned only: %s" % sorted(planned - case.kernels), "claimed only: %s" % sorted(case.kernels - planned))
    for f in case.flags:
        assert f in GEOMETRY, "unknown claim " + f
        assert GEOMETRY[f](case, steps), (case.name, f)


# ---- the table --------------------------------------------------------------------------------------------------------------------
PH5 = ("k_phase<1,5>", "k_phase<2,5>", "k_phase<3,5>", "k_phase<4,5>", "k_lm_fast<8,40>")
PH2 = ("k_phase<1,5>", "k_phase<2,5>", "k_phase<3,5>", "k_phase<4,2>", "k_lm_fast<8,40>")
LM40 = "k_lm_fast<8,40>"


def _bphase(T0, s, first):
    return tuple("k_bphase<%d,%d,%d,%d>" % (ph, T0, s, s) for ph in ((1, 2, 3) if first else (2, 3)))


def _bsplit(tall, *more):
    return ("k_bsplit<1,32>" if tall else "k_bsplit<1,16>", "k_bsplit<2,16>", "k_dmedian<16>", "k_cgrad<8>") + more


SEP5 = ("k_blur_mx_pyr", "k_cblur_mx", "k_dnormal", "k_dmedian<16>", "k_lm_spread5")      # + the gradient kernels + the level-1 memories


def _cases():
    v = []

    def add(*a, **k):
        v.append(Case(*a, **k))

    # ---- few frames: one launch per dependency level (k_phase)
    for n, fl in ((1, ("one_frame",)), (3, ("n_not_mult4",)), (15, ("n_not_mult4", "n_odd"))):
        add("few-rgbd-640x80-n%d" % n, 2, (640, 80), [5, 8], n, "phases", PH5, fl + ("partial_strip1", "blur_row_gt62"))
        add("few-rgbd-640x240-n%d" % n, 2, (640, 240), [5, 8], n, "phases", PH5, fl + ("half_strip1",))        # level 1: 120 rows = 7.5 strips of 16
        add("few-color-128x48-n%d" % n, 1, (128, 48), [2, 8], n, "phases", PH2, fl + ("partial_strip1",))
        add("few-color-256x16-n%d" % n, 1, (256, 16), [2, 8], n, "phases", PH2, fl + ("one_band1",))
    # ---- batches, colour only: k_bphase (launch 1 is k_blur_mx_pyr unless BLUR_PYR is 0)
    for n, fl in ((16, ("n_mult16",)), (19, ("n_not_mult4", "n_odd"))):
        for bp in (3, 0):
            first = bp == 0
            head = () if first else ("k_blur_mx_pyr",)
            kn = {"BLUR_PYR": bp}
            sfx = "-n%d%s" % (n, "-blurpyr0" if first else "")
            add("batch-color-T2-128x48" + sfx, 1, (128, 48), [2, 8], n, "batch_phases", head + _bphase(2, 16, first) + (LM40,),
                fl + ("not_tall", "partial_strip1", "whole_strips0"), kn)
            add("batch-color-T2-128x656" + sfx, 1, (128, 656), [2, 8], n, "batch_phases", head + _bphase(2, 32, first) + (LM40,),
                fl + ("tall", "partial_strip0", "partial_strip1"), kn)                                            # 20.5 strips of 32; level 1: 20.5 of 16
            add("batch-color-T5-640x80" + sfx, 1, (640, 80), [5, 8], n, "batch_phases", head + _bphase(5, 16, first) + (LM40,),
                fl + ("not_tall", "partial_strip1", "blur_row_gt62"), kn)
            add("batch-color-T5-640x720" + sfx, 1, (640, 720), [5, 8], n, "batch_phases", head + _bphase(5, 32, first) + (LM40,),
                fl + ("tall", "partial_strip0", "half_strip1"), kn)                                               # 22.5 strips of 32
    # ---- batches, RGB-D: k_bsplit between plain launches
    for n, fl in ((16, ("n_mult16",)), (19, ("n_not_mult4", "n_odd"))):
        add("batch-rgbd-640x80-n%d" % n, 2, (640, 80), [5, 8], n, "batch_phases", _bsplit(False, "k_blur_mx_pyr", "k_dnormal", LM40),
            fl + ("not_tall", "partial_strip1", "mx_strip96"))
        add("batch-rgbd-640x720-n%d" % n, 2, (640, 720), [5, 8], n, "batch_phases", _bsplit(True, "k_blur_mx_pyr", "k_dnormal", LM40),
            fl + ("tall", "partial_strip0", "half_strip1"))
        add("batch-rgbd-640x80-n%d-blurpyr0" % n, 2, (640, 80), [5, 8], n, "batch_phases", _bsplit(False, "k_bsplit<0,16>", "k_cblur_sh<16>", LM40),
            fl + ("not_tall", "partial_strip1"), {"BLUR_PYR": 0})
        add("batch-rgbd-640x720-n%d-blurpyr0" % n, 2, (640, 720), [5, 8], n, "batch_phases", _bsplit(True, "k_bsplit<0,16>", "k_cblur_sh<32>", LM40),
            fl + ("tall", "partial_strip0", "half_strip1"), {"BLUR_PYR": 0})
        add("batch-rgbd-1280x80-n%d" % n, 2, (1280, 80), [5, 8], n, "batch_phases", _bsplit(False, "k_blur_mx_pyr", "k_dnormal", "k_lm_fast<8,80>"),
            fl + ("grad_row_gt62", "lm_pitch80", "partial_strip1"))
    for strip, n, bp, fl in ((0, 16, 3, ("no_interleave",)), (32, 19, 2, ("interleave", "n_not_mult4")), (64, 16, 3, ("no_interleave",)), (0, 19, 2, ("interleave",))):
        add("batch-rgbd-640x80-n%d-cblur3-strip%d-blurpyr%d" % (n, strip, bp), 2, (640, 80), [5, 8], n, "batch_phases",
            _bsplit(False, "k_blur_pyr<%d>" % (strip or 16), "k_dnormal", LM40), fl + ("partial_strip1",),
            {"CBLUR_VARIANT": 3, "BLUR_STRIP": strip, "BLUR_PYR": bp})
    # the rules' edges inside the batch kernels: a weak threshold off the integers, the full depth range on both sides of k_dnormal's switch
    add("batch-rgbd-640x80-n16-weak3.5", 2, (640, 80), [5, 8], 16, "batch_phases", _bsplit(False, "k_blur_mx_pyr", "k_dnormal", LM40),
        ("weak_off_integer",), config={"weak_threshold": 3.5})
    add("few-rgbd-640x80-n3-weak3.5", 2, (640, 80), [5, 8], 3, "phases", PH5, ("weak_off_integer",), config={"weak_threshold": 3.5})
    add("batch-rgbd-640x80-n16-depth-full-250", 2, (640, 80), [5, 8], 16, "batch_phases", _bsplit(False, "k_blur_mx_pyr", "k_dnormal", LM40),
        ("depth_full_range", "double_products"), config={"distance_threshold": 70000, "difference_threshold": 250})
    add("batch-rgbd-640x80-n16-depth-full-5462", 2, (640, 80), [5, 8], 16, "batch_phases", _bsplit(False, "k_blur_mx_pyr", "k_dnormal", LM40),
        ("depth_full_range", "per_pixel_taps"), config={"distance_threshold": 70000, "difference_threshold": 5462})
    # ---- the separate launches at the same shapes (BATCH_PHASES 0: what a lane runs beside busy lanes)
    sep = {"BATCH_PHASES": 0}
    add("sep-rgbd-640x80-n16", 2, (640, 80), [5, 8], 16, "separate", SEP5 + ("k_cgrad_levels<8,8>", LM40), ("partial_strip1", "mx_strip96"), sep)
    add("sep-rgbd-640x720-n19", 2, (640, 720), [5, 8], 19, "separate", SEP5 + ("k_cgrad_levels<8,8>", LM40), ("tall", "n_not_mult4", "half_strip1"), sep)
    add("sep-rgbd-640x80-n16-cgrad3", 2, (640, 80), [5, 8], 16, "separate", SEP5 + ("k_cgrad_levels<32,8>", LM40), ("partial_strip1",), dict(sep, CGRAD_VARIANT=3))
    add("sep-rgbd-640x80-n19-levels0", 2, (640, 80), [5, 8], 19, "separate", SEP5 + ("k_cgrad<8>", LM40), ("n_not_mult4",), dict(sep, CGRAD_LEVELS=0))
    add("sep-rgbd-640x80-n16-levels0-cgrad3", 2, (640, 80), [5, 8], 16, "separate", SEP5 + ("k_cgrad<32>", LM40), ("partial_strip1",),
        dict(sep, CGRAD_LEVELS=0, CGRAD_VARIANT=3))
    add("sep-rgbd-640x80-n16-blurpyr0", 2, (640, 80), [5, 8], 16, "separate",
        ("k_cblur_mx", "k_pyrdown16", "k_cgrad<8>", "k_dnormal", "k_dmedian<16>", "k_lm_spread5", LM40), ("mx_strip96",), dict(sep, BLUR_PYR=0))
    add("sep-color-T2-128x48-n16", 1, (128, 48), [2, 8], 16, "separate", ("k_blur_mx_pyr", "k_cblur_mx", "k_cgrad_levels<8,8>", "k_lm_spread2", LM40), ("partial_strip1",), sep)
    add("sep-color-T5-640x80-n19", 1, (640, 80), [5, 8], 19, "separate", ("k_blur_mx_pyr", "k_cblur_mx", "k_cgrad_levels<8,8>", "k_lm_spread5", LM40), ("n_not_mult4",), sep)
    add("sep-rgbd-1280x80-n16", 2, (1280, 80), [5, 8], 16, "separate", SEP5 + ("k_cgrad_levels<8,8>", "k_lm_fast<8,80>"), ("grad_row_gt62", "lm_pitch80"), sep)
    # few frames through the separate launches (PHASE_MAX_SLOTS 0): the one-shot kernels on resident slots
    add("sep-rgbd-640x80-n3-phases-off", 2, (640, 80), [5, 8], 3, "separate",
        ("k_cblur", "k_corient", "k_cvote", "k_dnormal", "k_dmedian<4>", "k_pyrdown8", "k_lm_fast<5,128>", LM40), ("n_not_mult4",), {"PHASE_MAX_SLOTS": 0})
    # ---- the separate route at shapes outside phases_shape
    FEW44 = ("k_cblur", "k_corient", "k_cvote", "k_dnormal", "k_dmedian<4>", "k_pyrdown8", "k_lm_fast<4,64>")
    add("sep-rgbd-96x48-T4.4-n16", 2, (96, 48), [4, 4], 16, "separate",
        ("k_blur_mx_pyr", "k_cblur_sh<16>", "k_cgrad_levels<8,8>", "k_dnormal", "k_dmedian<16>", "k_lm_fast<4,64>"), ("row_bytes1_not32", "partial_strip1"))
    add("sep-rgbd-96x48-T4.4-n3", 2, (96, 48), [4, 4], 3, "separate", FEW44, ("n_not_mult4",))
    # (three levels: lm_debug_read rebuilds the depth modality's quantised image above level 0 by a k_nn_half of its own, so the call's
    # k_nn_half is pinned through level 2's depth memories, which read level 1's image at (2y, 2x))
    add("sep-rgbd-160x96-T4.4.4-n17", 2, (160, 96), [4, 4, 4], 17, "separate",
        ("k_blur_mx_pyr", "k_cgrad<8>", "k_dnormal", "k_dmedian<16>", "k_cblur_sh<16>", "k_pyrdown16", "k_color_quantize", "k_nn_half", "k_lm_fast<4,64>",
         "k_linear_memories"), ("three_levels", "n_not_mult4", "n_odd"))
    add("sep-rgbd-72x48-T4.4-n16", 2, (72, 48), [4, 4], 16, "separate", ("k_color_quantize", "k_pyrdown", "k_dnormal", "k_dmedian<16>", "k_linear_memories"), ("w_8_not_16",))
    add("sep-rgbd-84x48-T4.2-n17", 2, (84, 48), [4, 2], 17, "separate", ("k_color_quantize", "k_pyrdown", "k_depth_quantize", "k_linear_memories"), ("w_not_8", "n_odd"))
    # (RGB-D T {2, 8} at 128 x 48 takes k_lm_spread2 for BOTH modalities: the planner refutes k_lm_fast<2,128> there.  The nearest shapes that
    # reach it: a width that is no multiple of 32 at T0 = 2, and T = 2 on the scanned level.)
    add("sep-rgbd-80x48-T2.8-n16", 2, (80, 48), [2, 8], 16, "separate",
        ("k_blur_pyr<16>", "k_cgrad<8>", "k_dnormal", "k_dmedian<16>", "k_color_quantize", "k_lm_fast<2,128>", "k_linear_memories"), ("w_16_not_32", "no_interleave"))
    add("sep-rgbd-96x48-T4.2-n16", 2, (96, 48), [4, 2], 16, "separate",
        ("k_blur_mx_pyr", "k_cblur_sh<16>", "k_cgrad_levels<8,8>", "k_dnormal", "k_dmedian<16>", "k_lm_fast<4,64>", "k_lm_fast<2,128>"), ("row_bytes1_not32",))
    add("sep-rgbd-128x48-T2.8-n16", 2, (128, 48), [2, 8], 16, "separate",
        ("k_blur_mx_pyr", "k_cblur_mx", "k_cgrad_levels<8,8>", "k_dnormal", "k_dmedian<16>", "k_lm_spread2", LM40), ("partial_strip1",))
    add("sep-rgbd-640x80-n16-lut-bytes", 2, (640, 80), [5, 8], 16, "separate",
        ("k_blur_mx_pyr", "k_cblur_mx", "k_cgrad_levels<8,8>", "k_depth_quantize", "k_lm_spread5", LM40), ("lut_bytes",), lut="bytes")
    # ---- a slot range that does not start at 0
    add("batch-rgbd-640x80-slots3to19", 2, (640, 80), [5, 8], 16, "batch_phases", _bsplit(False, "k_blur_mx_pyr", "k_dnormal", LM40),
        ("first_slot_nonzero",), first_slot=3, total_slots=24)
    # ---- gradient strips of 16 rows are chosen from 1536 waves per call on; a detector has at most 1024 slots, so a call needs frames of two
    # waves: 64 x 248 (4 lanes x 16 strips = 64 lanes at level 0; level 1 is one wave), and 128 x 496 for two waves at level 1.  Threshold 90
    # keeps the candidates of 768 frames inside the detector's default buffers.
    m2 = ("k_blur_mx_pyr", "k_cblur_mx", "k_lm_spread2", "k_lm_fast<2,128>")
    add("many-color-64x248-n768", 1, (64, 248), [2, 2], 768, "separate", m2 + ("k_cgrad_levels<16,8>",), ("slots_gt256", "partial_strip0", "partial_strip1"), threshold=90.0)
    add("many-color-64x248-n768-levels0", 1, (64, 248), [2, 2], 768, "separate", m2 + ("k_cgrad<16>", "k_cgrad<8>"), ("slots_gt256", "partial_strip0"), {"CGRAD_LEVELS": 0}, threshold=90.0)
    add("many-color-128x496-n768", 1, (128, 496), [2, 2], 768, "separate", m2 + ("k_cgrad_levels<16,16>",), ("slots_gt256", "partial_strip1"), threshold=90.0)
    add("many-color-128x496-n768-cgrad3", 1, (128, 496), [2, 2], 768, "separate", m2 + ("k_cgrad_levels<32,16>",), ("slots_gt256", "partial_strip0_32"), {"CGRAD_VARIANT": 3}, threshold=90.0)
    return v


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Kernels of lmh::pre_kernel_name that no row runs: {name: (why no call of the table reaches it, the test that covers it, which diffs the
# quantised images of resident slots)}
EXCEPTIONS = {
    "mask_rules": ("not a kernel of the planner: the detector builds the step from the slots' mask rules, and a masked slot changes what the planes must hold",
                   "tests/test_gpu_mask_rules.py"),
    "match_masks": ("not a kernel of the planner: the detector builds the step from the slots' match masks, and a masked slot changes what the planes must hold",
                    "tests/test_gpu_match_masks.py"),
}


# ---- contents: a different frame in every slot ------------------------------------------------------------------------------------
COLOUR_KINDS = ("scene", "noise", "extremes", "blocks", "rect", "edge", "tie")
DEPTH_KINDS = ("scene", "noise", "steps", "lattice")
EDGE_MIN, TIE_MIN = 50, 200
TIE_DIFFERENT_MIN = 50      # of the ties, those between channels of different gradients (as many as an edge value has pixels)


def colour_kind(slot):
    return COLOUR_KINDS[slot % len(COLOUR_KINDS)]


def depth_kinds(case):
    return DEPTH_KINDS + (("full", "near") if case.config["distance_threshold"] > 65535 else ())


def depth_kind(case, slot):
    k = depth_kinds(case)
    return k[slot % len(k)]


def edge_values(t):
    """The squared gradient magnitudes at the weak threshold's edge: t * t itself when a gradient can have it, and the nearest attainable
    values on either side.  A 3 x 3 Sobel pair has dx = dy (mod 2) -- both are the sum of the four corner pixels mod 2 -- so dx^2 + dy^2 is
    a sum of two squares of equal parity: 98, 100, 104 around 10^2 (101 = 10^2 + 1 cannot occur), 10 and 16 around 3.5^2 = 12.25."""
    t2 = float(t) * float(t)
    r = int(t2 ** 0.5) + 8
    vals = sorted({a * a + b * b for a in range(r) for b in range(r) if (a - b) % 2 == 0})
    below, above = max(v for v in vals if v < t2), min(v for v in vals if v > t2)
    return [below] + ([int(t2)] if t2 == int(t2) and int(t2) in vals else []) + [above]


def edge_counts(orc, bgr, t):
    """Interior pixels (the border rows and columns are zeroed by rule) whose magnitude^2 equals each value of edge_values(t)."""
    _, mag = orc.color_quantize(bgr, t, want_magnitude=True)
    m = mag[1:-1, 1:-1]
    return [int((m == v).sum()) for v in edge_values(t)]


def tie_counts(orc, bgr, t):
    """(interior pixels above the weak threshold where two channels share the largest magnitude^2, those of them where the two channels'
    gradients DIFFER: which one the B, G, R cascade takes decides the orientation there)"""
    dx, dy = orc.sobel3(orc.gaussian7(bgr))
    dx, dy = dx.astype(np.int64)[1:-1, 1:-1], dy.astype(np.int64)[1:-1, 1:-1]
    m = dx * dx + dy * dy
    at = m == m.max(axis=2, keepdims=True)
    first, last = at.argmax(axis=2)[..., None], (2 - at[..., ::-1].argmax(axis=2))[..., None]
    pick = lambda a, i: np.take_along_axis(a, i, axis=2)[..., 0]
    differ = (pick(dx, first) != pick(dx, last)) | (pick(dy, first) != pick(dy, last))
    tie = (at.sum(axis=2) >= 2) & (m.max(axis=2) > t * t)
    return int(tie.sum()), int((tie & differ).sum())


def _edge_frame(orc, rng, w, h, t):
    """Searched on the CPU: low uniform noise around mid grey whose blurred gradients crowd around t."""
    base = max(1, int(round(1.2 * t)))
    amps = [a for a in (base, base + 2, base - 1, base + 4, base + 1) if a >= 1]
    for k in range(80):
        a = amps[k % len(amps)]
        bgr = (128 + rng.integers(-a, a + 1, (h, w, 3))).astype(np.uint8)
        if min(edge_counts(orc, bgr, t)) >= EDGE_MIN:
            return bgr
    raise AssertionError("no threshold-edge frame found for %d x %d at t = %g" % (w, h, t))


def _tie_pattern(rng, w, h):
    """Three bands, each with another pair of channels carrying a strong pattern over a weak third (B and G, G and R, B and R).  The pattern
    comes in 16 x 16 tiles.  The second channel of a pair holds two tiles of three TRANSPOSED: where the blur's rounding allows it, its gradient
    away from the tile edges is the first's with dx and dy exchanged -- the same magnitude, another orientation.  Every third tile is a plain copy."""
    th, tw = (h + 15) // 16, (w + 15) // 16
    tiles = np.kron(rng.integers(0, 256, (th, tw, 4, 4), dtype=np.uint8), np.ones((1, 1, 4, 4), np.uint8))      # [ty, tx, 16, 16]
    strong = tiles.transpose(0, 2, 1, 3).reshape(th * 16, tw * 16)[:h, :w]
    copy = ((np.arange(th)[:, None] * tw + np.arange(tw)[None, :]) % 3 == 2)[:, :, None, None]
    turned = np.where(copy, tiles, tiles.transpose(0, 1, 3, 2)).transpose(0, 2, 1, 3).reshape(th * 16, tw * 16)[:h, :w]
    weak = (128 + rng.integers(-2, 3, (h, w))).astype(np.uint8)
    bgr = np.empty((h, w, 3), np.uint8)
    cuts = [0, w // 3 // 16 * 16, 2 * w // 3 // 16 * 16, w]
    for band, odd in enumerate((2, 0, 1)):       # the channel that differs
        x0, x1 = cuts[band], cuts[band + 1]
        pair = [ch for ch in range(3) if ch != odd]
        bgr[:, x0:x1, odd] = weak[:, x0:x1]
        bgr[:, x0:x1, pair[0]] = strong[:, x0:x1]
        bgr[:, x0:x1, pair[1]] = turned[:, x0:x1]
    return bgr


def _tie_frame(orc, rng, w, h, t):
    for _ in range(40):
        bgr = _tie_pattern(rng, w, h)
        ties, different = tie_counts(orc, bgr, t)
        if ties >= TIE_MIN and different >= TIE_DIFFERENT_MIN:
            return bgr
    raise AssertionError("no tie frame found for %d x %d at t = %g" % (w, h, t))


def make_frame_of(orc, synth, case, slot):
    """(bgr, depth or None) of one slot: the kinds cycle with the slot, every slot has its own seed.  Edge and tie frames are checked as
    they are made, so every one of them has what it claims."""
    w, h = case.size
    t = case.config["weak_threshold"]
    rng = np.random.default_rng([case.content_seed(), slot])
    scene = None
    kind = colour_kind(slot)
    if kind == "scene" or (case.M == 2 and depth_kind(case, slot) == "scene"):
        sb, sd = synth.make_frame(max(w, 64), max(h, 64), seed=int(rng.integers(1 << 30)), n_shapes=14)
        scene = np.ascontiguousarray(sb[:h, :w]), np.ascontiguousarray(sd[:h, :w])
    if kind == "scene":
        bgr = scene[0]
    elif kind == "noise":
        bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "extremes":       # per channel 0 or 255: the largest blur, Sobel and pyrDown sums
        bgr = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    elif kind == "blocks":         # 8 x 8 blocks +- 3: votes that pass 5 of 9
        b = rng.integers(3, 253, ((h + 7) // 8, (w + 7) // 8, 3))
        bgr = (np.kron(b, np.ones((8, 8, 1), np.int64))[:h, :w] + rng.integers(-3, 4, (h, w, 3))).astype(np.uint8)
    elif kind == "rect":           # a constant frame, a rectangle touching the top and the right border
        bgr = np.empty((h, w, 3), np.uint8)
        bgr[:] = rng.integers(0, 256, 3)
        bgr[0:int(rng.integers(2, h - 1)), int(rng.integers(1, w - 2)):w] = rng.integers(0, 256, 3)
    elif kind == "edge":
        bgr = _edge_frame(orc, rng, w, h, t)
    else:
        bgr = _tie_frame(orc, rng, w, h, t)
    if case.M == 1:
        return np.ascontiguousarray(bgr), None
    dk = depth_kind(case, slot)
    diff = case.config["difference_threshold"]
    if dk == "scene":
        depth = scene[1]
    elif dk == "noise":            # hits d >= 2000, |delta| >= 50, zeros
        depth = rng.integers(0, 2600, (h, w)).astype(np.uint16)
    elif dk == "steps":            # right at the difference threshold
        depth = (600 + (diff - 1) * rng.integers(0, 3, (h, w))).clip(0, 65535).astype(np.uint16)
    elif dk == "lattice":          # zero-length normals: every tap 5 away crosses the gate; zeros; a flat patch
        yy, xx = np.mgrid[0:h, 0:w]
        depth = np.where(((yy // 5) + (xx // 5)) % 2 == 0, 300, 300 + 4 * diff).clip(0, 65535).astype(np.uint16)
        x0, y0 = int(rng.integers(0, w // 2)), int(rng.integers(0, h // 2))
        depth[y0:y0 + h // 3, x0:x0 + w // 4] = 0
        depth[h // 2:h // 2 + h // 4, w // 2 + x0 // 2:w // 2 + x0 // 2 + w // 8] = 700
    elif dk == "full":             # the whole u16 range: deltas that wrap as i16
        depth = rng.integers(0, 65536, (h, w)).astype(np.uint16)
    else:                          # "near": far depths within the gate of each other
        depth = (30000 + rng.integers(-diff, diff + 1, (h, w)).clip(-30000, 35535)).astype(np.uint16)
    return np.ascontiguousarray(bgr), np.ascontiguousarray(depth)


def normal_lut(orc, kind):
    if kind == "default":
        return None
    assert kind == "bytes"
    return np.random.default_rng(9).integers(0, 256, 8000).astype(np.uint8)      # arbitrary bytes: the median must be a true median


# ---- references -------------------------------------------------------------------------------------------------------------------
def plane_keys(case):
    return [(what, l, m) for what in (0, 2) for l in range(case.L) for m in range(case.M)]


def composed_planes(orc, case, bgr, depth):
    """Every plane of a frame from the oracle's single stages: the second reference."""
    c = case.config
    lut = normal_lut(orc, case.lut)
    out = {}
    img = bgr
    for l in range(case.L):
        if l > 0:
            img = orc.pyrdown(img)
        out[(0, l, 0)] = orc.color_quantize(img, c["weak_threshold"])
        if case.M == 2:
            out[(0, l, 1)] = orc.depth_quantize(depth, c["distance_threshold"], c["difference_threshold"], lut) if l == 0 else np.ascontiguousarray(out[(0, l - 1, 1)][::2, ::2])
        for m in range(case.M):
            resp = orc.response_maps(orc.spread(out[(0, l, m)], case.T[l]))
            out[(2, l, m)] = np.stack([orc.linearize(resp[o], case.T[l]) for o in range(8)])
    return {k: v.reshape(-1) for k, v in out.items()}


def oracle_detector(orc, case):
    c = case.config
    o = orc.Detector(color_only=(case.M == 1), T=case.T, weak_threshold=c["weak_threshold"], distance_threshold=c["distance_threshold"],
                     difference_threshold=c["difference_threshold"])
    lut = normal_lut(orc, case.lut)
    if lut is not None:
        o.set_normal_lut(lut)
    return o


def oracle_planes(o, case, bgr, depth):
    o.prepare(bgr, depth)
    return {k: o.stage(*k) for k in plane_keys(case)}


def small_bank(case, quant0, seed):
    """A handful of templates of 24 .. 40 px (less where the frame is smaller), their features picked from slot 0's quantised pyramid."""
    from oracle.oracle import DESC_DTYPE, FEATURE_DTYPE
    rng = np.random.default_rng(seed)
    w, h = case.size
    M, L = case.M, case.L
    step = 1 << (L - 1)
    descs, feats = [], []
    for _ in range(6):
        # inside the refinement's range (8 T0 <= x <= w - w0 - 8 T0) where the frame has one, so that the crops are found there; a frame of
        # 80 rows at T0 = 5 has none, every candidate refines at the clamped corner and its lists are short or empty
        b = 8 * case.T[0]
        wr, hr = w - 2 * b, h - 2 * b
        w0 = min(int(rng.integers(12, 21)) * 2, (wr if wr >= 16 else w - 4) // step * step)
        h0 = min(int(rng.integers(12, 21)) * 2, (hr if hr >= 16 else h - 4) // step * step)
        x0 = (b + int(rng.integers(0, wr - w0 + 1))) // step * step if wr >= 16 else int(rng.integers(0, (w - w0) // step)) * step
        y0 = (b + int(rng.integers(0, hr - h0 + 1))) // step * step if hr >= 16 else int(rng.integers(0, (h - h0) // step)) * step
        for l in range(L):
            wl, hl, nf = w0 >> l, h0 >> l, max(16 >> l, 4)
            for m in range(M):
                q = quant0[(0, l, m)].reshape(h >> l, w >> l)
                sub = q[(y0 >> l):(y0 >> l) + hl + 1, (x0 >> l):(x0 >> l) + wl + 1]
                ys, xs = np.nonzero(sub)
                f = np.zeros(nf, FEATURE_DTYPE)
                if ys.size >= nf:
                    pick = rng.choice(ys.size, nf, replace=False)
                    f["x"], f["y"] = xs[pick], ys[pick]
                    f["label"] = np.floor(np.log2(sub[ys[pick], xs[pick]].astype(np.float64))).astype(np.int32)
                else:           # too little structure under the crop: a random template
                    f["x"], f["y"], f["label"] = rng.integers(0, wl + 1, nf), rng.integers(0, hl + 1, nf), rng.integers(0, 8, nf)
                descs.append((wl, hl, l, nf))
                feats.append(f)
    return np.array(descs, DESC_DTYPE), np.concatenate(feats)


class Reference:
    """Frames, oracle planes, bank and lists of the rows that share a reference_key, slot by slot as they are first asked for."""

    def __init__(self, orc, synth, case):
        self.orc, self.synth, self.case = orc, synth, case
        self.o = oracle_detector(orc, case)
        self._slots = {}
        bgr, depth = make_frame_of(orc, synth, case, 0)
        self.descs, self.feats = small_bank(case, oracle_planes(self.o, case, bgr, depth), case.content_seed() & 0xFFFF)
        self.o.add_class("c", self.descs, self.feats)

    def _make(self, o, s):
        bgr, depth = make_frame_of(self.orc, self.synth, self.case, s)
        planes = oracle_planes(o, self.case, bgr, depth)
        matches = o.match_prepared(self.case.threshold, threads=1 if o is not self.o else 8, cap=1 << 16)
        for a in list(planes.values()) + [matches, bgr] + ([depth] if depth is not None else []):
            a.setflags(write=False)
        return bgr, depth, planes, matches

    def slot(self, s):
        """(bgr, depth, {plane key: bytes}, match list) of content slot s; read-only."""
        if s not in self._slots:
            self._slots[s] = self._make(self.o, s)
        return self._slots[s]

    def prefetch(self, slots, workers=8):
        """The slots of a call of hundreds of frames, made by `workers` threads, each with an oracle detector of its own (the same bank)."""
        from concurrent.futures import ThreadPoolExecutor
        todo = [s for s in slots if s not in self._slots]
        if len(todo) < 4 * workers:
            return

        def work(part):
            o = oracle_detector(self.orc, self.case)
            o.add_class("c", self.descs, self.feats)
            return [(s, self._make(o, s)) for s in part]
        with ThreadPoolExecutor(workers) as ex:
            for done in ex.map(work, [todo[k::workers] for k in range(workers)]):
                self._slots.update(done)


def first_difference(case, key, got, exp):
    """Where two planes first differ, as text: (y, x) of a quantised image; orientation, (y, x) of a linear memory."""
    what, l, m = key
    w, h = case.level_size(l)
    if got.size != exp.size:
        return "sizes %d and %d" % (got.size, exp.size)
    i = int(np.flatnonzero(got != exp)[0])
    n_bad = int((got != exp).sum())
    if what == 0:
        return "(y, x) = (%d, %d): got %d, expected %d; %d bytes differ" % (i // w, i % w, got[i], exp[i], n_bad)
    T = case.T[l]
    W = w // T
    ori, rem = divmod(i, w * h)
    cell, pos = divmod(rem, W * (h // T))
    return "orientation %d, (y, x) = (%d, %d): got %d, expected %d; %d bytes differ" % (ori, (pos // W) * T + cell // T, (pos % W) * T + cell % T, got[i], exp[i], n_bad)


def rows_by_kernel():
    """{kernel name: [rows that run it]}: the table's index (a row's kernel set is exact, the CPU test holds it to the planner)."""
    out = {}
    for c in CASES:
        for k in sorted(c.kernels):
            out.setdefault(k, []).append(c.name)
    return out


if __name__ == "__main__":      # python tests/preprocess_routes.py: which rows run which kernel
    for k, rows in sorted(rows_by_kernel().items()):
        print("%-24s %3d  %s" % (k, len(rows), " ".join(rows)))
