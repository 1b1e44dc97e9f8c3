"""Which kernels the pre-processing (a3-a10) launches, call by call, for the calls of tests/cpp/preprocess_plan_table.cpp that a detector
can make: resident synthetic frames, one lane, fixed seeds, plus the stage hooks.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/preprocess_launches.py > OUT/calls.txt
    python3 tools/preprocess_launches.py --reduce OUT/calls.txt OUT/<...>_kernel_trace.csv > profiles/preprocess_launches.txt

The first form makes the calls and prints one label per call; behind every call it launches a marker (lm_stage_pyrdown of a 2 x 2 image,
then lm_stage_color_quantize of one pixel: k_pyrdown and k_color_quantize on one workgroup each, in that order, which no call of the list launches).  The second form cuts the trace at the markers and prints, per call,
the ordered (kernel, grid in workgroups, workgroup, LDS bytes) of the pre-processing kernels.  Two builds launch the same kernels exactly
when their reductions are the same text: profiles/preprocess_launches.txt is the one of the commit before the host planner
(lm_host.cpp plan_preprocess) and of the planner, identical."""
import csv
import importlib
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE = ("k_pyrdown", "k_nn_half", "k_blur_", "k_cblur", "k_corient", "k_cvote", "k_cgrad", "k_color_quantize", "k_dnormal", "k_dmedian",
       "k_depth_quantize", "k_lm_", "k_linear_memories", "k_phase", "k_bphase", "k_bsplit", "k_match_mask", "k_mask_rule")


MARK = ("  k_pyrdown grid 1x1x1 ", "  k_color_quantize grid 1x1x1 ")
MARK_KERNELS = ("k_pyrdown", "k_color_quantize")


def short_name(name):
    """'void (anonymous namespace)::k_phase<1, 5>(LmPhaseArgs, LmPhaseGrid) [clone .kd]' -> 'k_phase<1, 5>'"""
    m = re.search(r"\bk_[a-z0-9_]+(<[^>(]*>)?", name)
    return m.group(0) if m else name


def reduce(calls_path, trace_path, prefixes=PRE):
    """prefixes: the kernels that count (tools/match_launches.py passes the match stages'); the two marker kernels always do."""
    labels = [ln[5:].strip() for ln in open(calls_path) if ln.startswith("CALL ")]
    rows = list(csv.DictReader(open(trace_path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))

    def dims(r, what):
        return tuple(int(r["%s_Size_%s" % (what, ax)]) for ax in "XYZ")
    segments, cur = [], []
    for r in rows:
        name = short_name(r["Kernel_Name"])
        if not name.startswith(prefixes) and name not in MARK_KERNELS:
            continue
        wg, grid = dims(r, "Workgroup"), dims(r, "Grid")
        blocks = tuple(g // max(w, 1) for g, w in zip(grid, wg))
        cur.append("  %s grid %dx%dx%d wg %d lds %s" % (name, blocks[0], blocks[1], blocks[2], wg[0] * wg[1] * wg[2], r.get("LDS_Block_Size", "?")))
        if len(cur) >= 2 and cur[-2].startswith(MARK[0]) and cur[-1].startswith(MARK[1]):
            segments.append(cur[:-2])
            cur = []
    if len(segments) != len(labels) or cur:
        sys.exit("trace and call list disagree: %d labels, %d segments, %d launches behind the last marker" % (len(labels), len(segments), len(cur)))
    for label, seg in zip(labels, segments):
        print(label)
        print("\n".join(seg))


class Session:
    """Makes labelled calls with a marker behind each.  root: the checkout whose package is imported (another build to compare with)."""

    def __init__(self, root=ROOT):
        sys.path.insert(0, root)
        self.lm = importlib.import_module("line-mod-pipeline_amd")
        self.synth = importlib.import_module("line-mod-pipeline_amd.synth")
        self.det = None

    def marker(self):
        self.det.stage_pyrdown(np.zeros((2, 2, 3), np.uint8))
        self.det.stage_color_quantize(np.zeros((1, 1, 3), np.uint8), 10.0, False)

    def call(self, label, fn):
        print("CALL " + label, flush=True)
        fn()
        self.marker()

    def detector(self, color_only, w, h, slots, templates=12, size_range=None, crop_fraction=0.3, tag="", **kw):
        """A detector with `slots` resident frames and a small bank cut from frame 0's quantised images (a call of the list like any other)."""
        lm, synth = self.lm, self.synth
        print("CALL set-up %s %dx%d%s: prepare slot 0, first match" % ("colour" if color_only else "rgbd", w, h, tag), flush=True)
        d = lm.Detector(lm.default_config(color_only=color_only, width=w, height=h, frame_slots=slots, **kw))
        M, L = d.num_modalities, d.pyramid_levels
        frames = [synth.make_frame(w, h, seed=1234 + i) for i in range(min(slots, 4))]
        for i in range(slots):
            f = frames[i % len(frames)]
            d.upload_frame(i, f[0], None if color_only else f[1])
        d.prepare_slot(0)
        q = {(l, m): d.debug_read(0, 0, l, m).reshape(h >> l, w >> l) for l in range(L) for m in range(M)}
        descs, feats, _ = synth.make_bank(templates, M, L, seed=7, size_range=size_range or (48, min(160, h // 2)), quantized=q, crop_fraction=crop_fraction, frame_size=(w, h), T0=d.get_T(0))
        d.add_class("c", descs, feats)
        d.match_batch_classes(0, 1, 90.0)
        self.det = d
        self.marker()
        return d


def preprocess_calls(s):
    lm, call, detector = s.lm, s.call, s.detector

    def match(d, n):
        return lambda: d.match_batch_classes(0, n, 90.0)

    T = lm
    # ---- RGB-D 640 x 480, T {5, 8}
    d = detector(False, 640, 480, 96)
    for n in (1, 15, 16, 24, 96):
        call("rgbd 640x480 n %d" % n, match(d, n))
    for bp in (0, 1, 2):
        d.set_tuning(T.TUNE_BATCH_PHASES, bp)
        call("rgbd 640x480 n 16 BATCH_PHASES %d" % bp, match(d, 16))
    d.set_tuning(T.TUNE_BATCH_PHASES, 0)       # the launches of a call beside busy lanes, on one lane
    for n in (24, 96):
        call("rgbd 640x480 n %d BATCH_PHASES 0" % n, match(d, n))
    for v in (0, 1):
        d.set_tuning(T.TUNE_CGRAD_LEVELS, v)
        call("rgbd 640x480 n 96 BATCH_PHASES 0 CGRAD_LEVELS %d" % v, match(d, 96))
    for bp in (0, 1, 2, 3):
        for bs in (0, 16, 32, 64):
            d.set_tuning(T.TUNE_BLUR_PYR, bp)
            d.set_tuning(T.TUNE_BLUR_STRIP, bs)
            call("rgbd 640x480 n 24 BATCH_PHASES 0 BLUR_PYR %d BLUR_STRIP %d" % (bp, bs), match(d, 24))
    d.set_tuning(T.TUNE_BLUR_PYR, 1)
    d.set_tuning(T.TUNE_BLUR_STRIP, 0)
    for key, name, values in ((T.TUNE_CBLUR_VARIANT, "CBLUR_VARIANT", (1, 3, 4)), (T.TUNE_CGRAD_VARIANT, "CGRAD_VARIANT", (1, 2, 3)),
                              (T.TUNE_PYRDOWN_VARIANT, "PYRDOWN_VARIANT", (1, 2)), (T.TUNE_DMEDIAN_VARIANT, "DMEDIAN_VARIANT", (1, 2))):
        for v in values:
            d.set_tuning(key, v)
            for pm in (15, 0):
                d.set_tuning(T.TUNE_PHASE_MAX_SLOTS, pm)
                for bp in (0, 2):
                    d.set_tuning(T.TUNE_BATCH_PHASES, bp)
                    call("rgbd 640x480 n 1 %s %d PHASE_MAX_SLOTS %d BATCH_PHASES %d" % (name, v, pm, bp), match(d, 1))
                    call("rgbd 640x480 n 24 %s %d PHASE_MAX_SLOTS %d BATCH_PHASES %d" % (name, v, pm, bp), match(d, 24))
        d.set_tuning(key, 0)
    d.set_tuning(T.TUNE_BATCH_PHASES, 2)
    d.set_tuning(T.TUNE_PHASE_MAX_SLOTS, 0)
    for n in (1, 16):
        call("rgbd 640x480 n %d PHASE_MAX_SLOTS 0" % n, match(d, n))
    d.set_tuning(T.TUNE_PHASE_MAX_SLOTS, 15)
    mask = np.zeros((480, 640), np.uint8)
    mask[100:300, 200:500] = 255
    d.upload_match_mask(0, mask)
    d.upload_wait()
    for n in (1, 16, 96):
        call("rgbd 640x480 n %d, slot 0 masked" % n, match(d, n))
    rng = np.random.default_rng(5)
    for w, h in ((37, 53), (16, 64), (8, 8), (17, 80), (23, 91), (33, 8), (64, 48), (640, 480)):
        bgr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        depth = rng.integers(0, 3000, (h, w), dtype=np.uint16)
        for mag in (False, True):
            call("stage colour %dx%d magnitude %d" % (w, h, mag), lambda: d.stage_color_quantize(bgr, 10.0, mag))
        call("stage pyrDown %dx%d" % (w, h), lambda: d.stage_pyrdown(bgr))
        call("stage depth %dx%d" % (w, h), lambda: d.stage_depth_quantize(depth))
    for w, h, t in ((640, 480, 2), (640, 480, 4), (640, 480, 5), (640, 480, 8), (320, 240, 8), (48, 36, 3), (40, 20, 5), (24, 24, 8), (66, 30, 6), (70, 35, 7), (160, 160, 16), (36, 36, 2)):
        q = (1 << rng.integers(0, 8, (h, w))).astype(np.uint8)
        call("stage linear memories %dx%d T %d" % (w, h, t), lambda: d.stage_linear_memories(q, t))
    lut = np.full(8000, 3, np.uint8)          # not one-hot: the LDS-tiled depth kernel
    d.set_normal_lut(lut)
    for n in (1, 24):
        call("rgbd 640x480 n %d, LUT not one-hot" % n, match(d, n))
    d.close()
    # ---- the other detectors
    for label, args, kw, ns in (("colour 640x480", (True, 640, 480, 96), {}, (1, 15, 16, 96)),
                                ("rgbd 320x240", (False, 320, 240, 96), {}, (24, 96)),
                                ("rgbd 640x480 three levels T 4 8 8", (False, 640, 480, 24), {"T": (4, 8, 8)}, (1, 24)),
                                ("rgbd 640x480 byte responses", (False, 640, 480, 24), {"flags": lm.FLAG_BYTE_RESPONSES}, (1, 24)),
                                ("rgbd 1280x960", (False, 1280, 960, 8), {}, (2, 8))):
        d = detector(*args, **kw)
        for n in ns:
            call("%s n %d" % (label, n), match(d, n))
        if label == "colour 640x480":
            d.set_tuning(T.TUNE_BATCH_PHASES, 0)
            call("%s n 96 BATCH_PHASES 0" % label, match(d, 96))
        d.close()
    d = detector(True, 1280, 960, 32)
    for ww in (1, 0):
        d.set_tuning(T.TUNE_WORK_WEIGHT, ww)
        for n in (1, 3, 4, 8):
            call("colour 1280x960 n %d WORK_WEIGHT %d" % (n, ww), match(d, n))
    d.set_tuning(T.TUNE_WORK_WEIGHT, 1)
    d.set_tuning(T.TUNE_BATCH_PHASES, 0)
    for n in (4, 8, 32):
        call("colour 1280x960 n %d BATCH_PHASES 0" % n, match(d, n))
    d.set_tuning(T.TUNE_BATCH_PHASES, 2)
    d.set_tuning(T.TUNE_BLUR_PYR, 0)
    for n in (8, 32):
        call("colour 1280x960 n %d BLUR_PYR 0" % n, match(d, n))
    d.set_tuning(T.TUNE_BLUR_PYR, 1)
    d.close()


def cli(calls, prefixes):
    """[--root DIR]: make the calls with DIR's build; --reduce CALLS TRACE: print the reduction."""
    if len(sys.argv) == 4 and sys.argv[1] == "--reduce":
        reduce(sys.argv[2], sys.argv[3], prefixes)
    else:
        calls(Session(os.path.abspath(sys.argv[2])) if len(sys.argv) == 3 and sys.argv[1] == "--root" else Session())


if __name__ == "__main__":
    cli(preprocess_calls, PRE)
