"""Timing of learning from resident frames: 8 masked 640 x 480 RGB-D frames learned with ONE
lm_add_templates_slots call from slots that already hold them, beside 8 lm_add_template calls on host copies of the same frames and
masks (what a caller does without the call) in the same process: the median of --repeat timed runs after warm-up.  The frames are
frame0, the masks the first 8 of the seeded crop windows from which a template can be extracted; both ways add the same templates
(checked).  Writes profiles/learn_slots_timing.json (or --out) and prints it.
usage: python tools/learn_slots_timing.py [--repeat N] [--out PATH] [--gpu-only]     (--gpu-only: for a kernel trace of the slot call alone)"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import crop_masks  # noqa: E402

N, W, H = 8, 640, 480


def _median_ms(fn, repeat, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_slots_timing.json"))
    ap.add_argument("--gpu-only", action="store_true")
    a = ap.parse_args()
    lm = importlib.import_module("line-mod-pipeline_amd")
    f0 = np.load(os.path.join(ROOT, "tests", "golden", "frame0.npz"))
    bgr, depth = np.ascontiguousarray(f0["bgr"]), np.ascontiguousarray(f0["depth"])
    probe = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    masks = [m for m in crop_masks(W, H, 11, 48) if probe.add_template("probe", bgr, depth, m)[0] >= 0][:N]
    probe.close()
    assert len(masks) == N
    slots = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    host = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    for k in range(N):
        slots.upload_frame(k, bgr, depth)
    slots.upload_wait(-1)
    copies = [slots.read_frame(k) for k in range(N)]
    state = {}

    def one_call():
        state["slots"] = slots.add_templates_slots("obj", 0, masks)

    def per_frame():
        state["host"] = [host.add_template("obj", copies[k][0], copies[k][1], masks[k]) for k in range(N)]

    out = {"frames": N, "width": W, "height": H, "repeat": a.repeat}
    ms = _median_ms(one_call, a.repeat)
    out["add_templates_slots_ms"], out["add_templates_slots_min_ms"], out["add_templates_slots_max_ms"] = ms
    if not a.gpu_only:
        ms = _median_ms(per_frame, a.repeat)
        out["add_template_x8_ms"], out["add_template_x8_min_ms"], out["add_template_x8_max_ms"] = ms
        out["speedup"] = out["add_template_x8_ms"] / out["add_templates_slots_ms"]
        ids, bbs = state["slots"]
        assert [int(t) for t in ids] == [t for t, _ in state["host"]] and [tuple(int(v) for v in b) for b in bbs] == [b for _, b in state["host"]]
        for tid in ids:
            for level in range(2):
                for mod in range(2):
                    x, y = slots.get_template(0, int(tid), level, mod), host.get_template(0, int(tid), level, mod)
                    assert x[:2] == y[:2] and np.array_equal(x[2], y[2])
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    slots.close()
    host.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
