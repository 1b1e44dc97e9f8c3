"""What does the depth check's sorted order statistic cost on the GPU?  HIP events on the colour-check stream around ONE
kernel launch (lm_time_depth_select), the median of 50 calls after 10 warm-ups with p10 and p90, one process, nothing else on the device:

  1. k_depth_select against k_depth_counts -- the r06 kernel, untouched, as the yard-stick -- for the same query list: 96 resident 640 x 480
     frames (the golden frame's depth), 16 queries per frame whose crops are the bounding boxes of the shipped bank's level-0 templates
     (tests/golden/frame0_golden.npz) at seeded places, clipped to the frame as the depth check clips them, rank n / 5.
  2. the chosen histogram scheme (a run counted in registers, histograms private to a wave) against the naive one (one shared LDS histogram,
     one atomic per pixel) on all-equal crops: the contention decision.  Both are checked against numpy before anything is timed.
  3. is not taken here: the per-frame wall time of the streamed detectBatchBegin / End on config 5's end-to-end set-up comes from
     tools/pose_e2e_bench.cpp with LM_E2E_DEPTH_STATISTIC=1 (sorted, GPU selections) and =0 (the reference's element) on the files
     bench.py --config 5 keeps under LM_POSE_E2E_KEEP; `--e2e sorted.json reference.json` folds the two outputs into the result.

    python tools/time_depth_select.py [out.json] [--e2e sorted.json reference.json]      -> profiles/depth_select_times.json"""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
lm = importlib.import_module("line-mod-pipeline_amd")

W, H, N, PER_FRAME = 640, 480, 96, 16
WARMUP, RUNS = 10, 50


def stats(us):
    us = np.sort(np.asarray(us, np.float64))
    return {"median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)), "p90_us": float(np.percentile(us, 90))}


def timed(d, q, what):
    for _ in range(WARMUP):
        d.time_depth_select(q, what)
    return stats([d.time_depth_select(q, what) * 1e3 for _ in range(RUNS)])


def rule(depth, e):
    crop = depth[e["y0"]:e["y1"], e["x0"]:e["x1"]]
    return 65535 if crop.size == 0 else int(np.sort(np.where(crop <= 1, 65535, crop).ravel())[e["rank"]])


def main():
    args = sys.argv[1:]
    e2e = None
    if "--e2e" in args:
        i = args.index("--e2e")
        e2e = (args[i + 1], args[i + 2])
        del args[i:i + 3]
    g = np.load(os.path.join(HERE, "tests", "golden", "frame0_golden.npz"))
    f = np.load(os.path.join(HERE, "tests", "golden", "frame0.npz"))
    bgr, depth = f["bgr"], f["depth"]
    descs = g["rgbd_descs"]
    boxes = sorted({(int(r["width"]), int(r["height"])) for r in descs if r["pyramid_level"] == 0})
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    flat = np.full((H, W), 1234, np.uint16)
    for s in range(N):
        d.upload_frame(s, bgr, depth if s else flat)           # slot 0: the all-equal frame of comparison 2
    d.upload_wait(-1)
    rng = np.random.default_rng(3)
    q = []
    for s in range(1, N):
        for k in range(PER_FRAME):
            bw, bh = boxes[(s * PER_FRAME + k) % len(boxes)]
            x, y = int(rng.integers(-bw // 4, W - bw // 2)), int(rng.integers(-bh // 4, H - bh // 2))
            x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + bw, W), min(y + bh, H)
            q.append((x0, y0, x1, y1, ((x1 - x0) * (y1 - y0)) // 5, s))
    q = np.array(q, lm.DEPTH_SELECT_QUERY_DTYPE)
    got = d.depth_select(q)
    assert all(int(v) == rule(depth, e) for v, e in zip(got[::37], q[::37])), "k_depth_select differs from the numpy rule"
    px = int(((q["x1"] - q["x0"]) * (q["y1"] - q["y0"])).sum())
    res = {"runs": RUNS, "warmup": WARMUP, "version": d.lib.lm_version().decode().split(" (")[0], "frames": N - 1, "queries": len(q), "crop_pixels": px,
           "boxes": [list(b) for b in boxes],
           "bank_boxes": {"k_depth_select": timed(d, q, 0), "k_depth_counts": timed(d, q, 2)}}
    # 2: all-equal crops, the worst case of one shared histogram: 64 crops of 160 x 120 and one whole frame
    eq = np.array([(8 * k, 4 * k, 8 * k + 160, 4 * k + 120, (160 * 120) // 5, 0) for k in range(60)] + [(0, 0, W, H, (W * H) // 5, 0)], lm.DEPTH_SELECT_QUERY_DTYPE)
    assert (d.depth_select(eq) == 1234).all()
    res["all_equal_crops"] = {"queries": len(eq), "crop_pixels": int(((eq["x1"] - eq["x0"]) * (eq["y1"] - eq["y0"])).sum()),
                              "chosen_run_in_registers_per_wave_histograms": timed(d, eq, 0), "naive_one_shared_histogram": timed(d, eq, 1),
                              "k_depth_counts": timed(d, eq, 2)}
    res["bank_boxes"]["naive_one_shared_histogram"] = timed(d, q, 1)
    d.close()
    if e2e:
        out = {}
        for name, path in zip(("sorted_gpu_selections", "reference_element"), e2e):
            j = json.load(open(path))
            out[name] = {leg: {"us_per_frame": j[leg]["us_per_frame"], "post_us_per_frame": j[leg]["post_us_per_frame"],
                               "depth_check_cpu_us_per_frame": j[leg]["post_cpu_us_per_frame_by_part"]["depth_check"]} for leg in ("serial", "pipelined", "pipelined_pinned")}
            out[name]["depth_checks_per_frame"] = j["serial"]["per_frame_counts"]["depth_checks"]
            out[name]["poses_identical_across_passes"] = j["poses_identical_across_passes"]
        res["config5_e2e_streamed"] = out
    print(json.dumps(res, indent=1))
    out_path = next((a for a in args if a.endswith(".json")), os.path.join(HERE, "profiles", "depth_select_times.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
