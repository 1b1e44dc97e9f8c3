"""Timing of the mask rules: a 96-frame 640 x 480 RGB-D lm_match_batch on bench.py's config-2 workload (seeded frames,
fixed-geometry bank) -- unmasked, with uploaded masks (resident, and with the 192 mask uploads counted), and with a rule on every
slot (depth range + HSV range, grow 0 and 8; the uploaded masks are that rule's masks) -- as the median of --repeat timed calls after
warm-up, each call ending in the lists' collection.  Prints one JSON object; --out also writes it.
usage: python tools/mask_rule_timing.py [--repeat N] [--templates N] [--out PATH] [--only unmasked|uploaded|rule0|rule8]
(--only: that case alone, for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/mask_rule_timing.py --only rule8)"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, B, THR = 640, 480, 96, 80.0


def _median_ms(fn, repeat, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts = 1e3 * np.array(ts)
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "p90_ms": float(np.percentile(ts, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=100)
    ap.add_argument("--templates", type=int, default=3000)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=("", "unmasked", "uploaded", "rule0", "rule8"))
    a = ap.parse_args()
    lm = importlib.import_module("line-mod-pipeline_amd")
    synth = importlib.import_module("line-mod-pipeline_amd.synth")
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=B)
    frames = [synth.make_frame(W, H, seed=1234 + i) for i in range(B)]
    d.upload_frame(0, *frames[0])
    d.prepare_slot(0)
    q = {(l, m): d.debug_read(0, 0, l, m).reshape(H >> l, W >> l) for l in range(2) for m in range(2)}
    descs, feats, _ = synth.make_bank(a.templates, 2, 2, seed=4321, fixed_l0_size=(96, 96), quantized=q, crop_fraction=0.1, frame_size=(W, H),
                                      T0=d.get_T(0))
    d.add_class("synthetic.ply", descs, feats)
    out = np.zeros((B, 4096), lm.MATCH_DTYPE)
    cnt = np.zeros(B, np.int32)

    def upload_frames():
        for i, (bgr, depth) in enumerate(frames):
            d.upload_frame(i, bgr, depth)

    def batch():
        d.match_batch(B, THR, 0, cap_per_frame=4096, out=out, counts=cnt)

    def rule(r):
        return lm.make_mask_rule(3, depth_range=(600, 900), hsv_range=([0, 0, 0], [255, 150, 255]), grow=r)

    res = {"frames": B, "width": W, "height": H, "templates": a.templates, "threshold": THR, "repeat": a.repeat}
    upload_frames()
    if a.only in ("", "unmasked"):
        res["unmasked"] = _median_ms(batch, a.repeat)
        res["unmasked"]["matches"] = int(cnt.sum())
    lists = {}
    for r in (0, 8):
        if a.only not in ("", "rule%d" % r):
            continue
        d.set_mask_rule(0, B, rule=rule(r))
        res["rule_grow%d" % r] = _median_ms(batch, a.repeat)
        res["rule_grow%d" % r]["matches"] = int(cnt.sum())
        lists[r] = [out[i, :cnt[i]].tobytes() for i in range(B)]
        d.clear_mask_rule()
    if a.only in ("", "uploaded"):
        masks = [d.stage_mask_rule(bgr, depth, rule(8)) for bgr, depth in frames]
        cov = float(np.mean([m.mean() / 255.0 for m in masks]))

        def upload_masks():
            for i, m in enumerate(masks):
                d.upload_match_mask(i, m, modality=-1)

        upload_masks()
        res["uploaded_resident"] = _median_ms(batch, a.repeat)
        res["uploaded_resident"]["matches"] = int(cnt.sum())
        res["uploaded_resident"]["mask_coverage"] = cov
        if 8 in lists:
            res["rule_grow8_lists_equal_uploaded"] = lists[8] == [out[i, :cnt[i]].tobytes() for i in range(B)]

        def with_uploads():
            upload_masks()
            batch()

        res["uploaded_with_mask_uploads"] = _median_ms(with_uploads, a.repeat)
    d.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
