"""Which kernels the match stages (a11-a15: scan, refinement plan, refinement, sort, merge) launch, call by call, for the calls of
tests/cpp/match_plan_table.cpp that a detector can make: small banks on small resident frames, one lane, fixed seeds.  The machinery is
tools/preprocess_launches.py's (markers, reduction), with the match kernels' names and this call list:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/match_launches.py [--root CHECKOUT] > OUT/calls.txt
    python3 tools/match_launches.py --reduce OUT/calls.txt OUT/<...>_kernel_trace.csv > profiles/match_launches.txt

profiles/match_launches.txt is the reduction of the commit before the host planner of the match stages (lm_host.cpp plan_match) and of the
planner, identical.  The runtime's fill kernel is kept too: the stream memsets in front of a k_scan1 launch show up as it.  (The trace's
LDS column is a kernel's static LDS; a launch's dynamic bytes are not in it -- tests/cpp/match_plan_table.cpp holds those.)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_launches as P  # noqa: E402

MATCH = ("k_scan", "k_refine", "k_emit_unrefined", "k_sort_unique", "k_merge_unique", "__amd_rocclr_fillBuffer")
NS = (1, 7, 8, 16, 24)
THR = 90.0


def match_calls(s):
    lm, call = s.lm, s.call

    def detector(color_only, w, h, slots=24, crops=True, **kw):
        # (crops: templates cut from frame 0, 8 T0 + 8 pixels inside it -- where the frame has the room)
        return s.detector(color_only, w, h, slots, size_range=(min(48, h // 6), min(160, h // 3)), crop_fraction=0.3 if crops else 0.0, tag=" " + " ".join("%s %s" % kv for kv in sorted(kw.items())), **kw)

    def fresh(d, n, classes=None):
        return lambda: d.match_batch_classes(0, n, THR, classes)

    def prepared(d, n, classes=None):
        return lambda: d.match_prepared(0, n, THR, classes)

    def forms(d, label, forms_, ns=NS):
        """Per scan form: a call of n frames that pre-processes them, for every n; then, on the slots the 24-frame call left, a11-a15 alone."""
        for f in forms_:
            d.set_tuning(lm.TUNE_SCAN_FORM, f)
            for n in ns:
                call("%s form %d n %d" % (label, f, n), fresh(d, n))
            for n in ns:
                call("%s form %d n %d prepared by n %d" % (label, f, n, ns[-1]), prepared(d, n))
        d.set_tuning(lm.TUNE_SCAN_FORM, 0)

    # ---- colour 128 x 96, T {2, 8}: every form, every settable variant, the debug callers
    d = detector(True, 128, 96, T=(2, 8))
    forms(d, "colour 128x96", (0, 1, 2, 3))
    for v in (1, 2, 3, 4, 8, 16, 32, 256, 9, 18):
        d.set_scan_variant(v)
        for f in (1, 2):
            d.set_tuning(lm.TUNE_SCAN_FORM, f)
            for n in (1, 8):
                call("colour 128x96 form %d n %d variant %d" % (f, n, v), fresh(d, n))
    d.set_scan_variant(0)
    for f, variants in ((1, (0, 8, 64 | 8)), (2, (0, 128, 256))):
        d.set_tuning(lm.TUNE_SCAN_FORM, f)
        d.match_batch_classes(0, 8, THR)
        d.prepare_slot(0)
        call("colour 128x96 form %d stage_scan" % f, lambda: d.stage_scan(0, THR))
        d.match_batch_classes(0, 8, THR)
        for v in variants:
            call("colour 128x96 form %d time_scan variant %d" % (f, v), lambda: d.time_scan(0, THR, iters=2, variant=v))
            call("colour 128x96 form %d time_scan_batch n 8 variant %d" % (f, v), lambda: d.time_scan_batch(0, 8, THR, iters=2, variant=v))
        call("colour 128x96 form %d n 8 after the timing calls" % f, fresh(d, 8))
    d.close()
    # ---- RGB-D 128 x 96: two modalities (the other default pruning rule), sort modes, a class list of two ranges
    d = detector(False, 128, 96, T=(2, 8))
    forms(d, "rgbd 128x96", (0, 1, 2, 3))
    for v in (8, 16, 32, 256):
        d.set_scan_variant(v)
        for f in (1, 2):
            d.set_tuning(lm.TUNE_SCAN_FORM, f)
            call("rgbd 128x96 form %d n 8 variant %d" % (f, v), fresh(d, 8))
    d.set_scan_variant(0)
    for mode in (0, 1):                          # (still form 2)
        d.set_tuning(lm.TUNE_SORT_SPLIT, mode)
        for n in (1, 8):
            call("rgbd 128x96 form 2 n %d SORT_SPLIT %d" % (n, mode), fresh(d, n))
    d.set_tuning(lm.TUNE_SORT_SPLIT, 2)
    for k in (2, 3):
        descs, feats, _ = s.synth.make_bank(5, 2, 2, seed=20 + k, size_range=(16, 32), frame_size=(128, 96), T0=2)
        d.add_class("c%d" % k, descs, feats)
    for f in (1, 2):
        d.set_tuning(lm.TUNE_SCAN_FORM, f)
        for classes in ([0, 2], [1], [-1]):
            call("rgbd 128x96 form %d n 8 classes %s" % (f, classes), fresh(d, 8, classes))
    d.close()
    # ---- the other shapes
    d = detector(True, 64, 48, crops=False, T=(2, 4))
    forms(d, "colour 64x48", (0, 1, 2, 3))
    d.close()
    d = detector(False, 320, 240, T=(4, 4))
    forms(d, "rgbd 320x240", (0, 1, 2, 3))
    d.close()
    d = detector(False, 640, 480)                # level 1's planes of both modalities: exactly k_scanl's LDS image
    forms(d, "rgbd 640x480", (0, 1, 2, 3), ns=(1, 24))
    d.close()
    # ---- byte responses (k_scan): every slot -> XCD mapping, the unroll variants, the plain mapping
    d = detector(True, 128, 96, T=(2, 8), flags=lm.FLAG_BYTE_RESPONSES)
    for v in (0, 1, 2, 4):
        d.set_scan_variant(v)
        for n in (1, 2, 3, 4, 7, 8, 16, 24):
            call("colour 128x96 byte responses n %d variant %d" % (n, v), fresh(d, n))
    d.close()
    # ---- one and three levels
    d = detector(True, 128, 96, crops=False, T=(8,))
    forms(d, "colour 128x96 one level", (0, 2))
    d.close()
    d = detector(False, 320, 240, T=(4, 8, 2))
    forms(d, "rgbd 320x240 three levels", (0, 2))
    d.close()


if __name__ == "__main__":
    P.cli(match_calls, MATCH)
