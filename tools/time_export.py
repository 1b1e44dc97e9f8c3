"""What does lm_export_frames cost?  96 frames of 640 x 480 in ONE launch to BGR8 and to NV12, without primitives and
with about 200 per frame (a detection overlay: 180 feature rings, three poses' axes and boxes; and the same list moved off the frames, which
keeps the host's share of the call and the table copy but leaves the kernel's primitive loop nothing to do), beside
    - a device-to-device hipMemcpy of the same output bytes: what a pure copy costs, the yard-stick no export can beat;
    - what the library offered for the job before: lm_read_frame per slot (a synchronous copy of dense BGR to the host, nothing drawn).
The call is synchronous and runs on a stream of its own, so events of the tool's cannot bracket its launch alone: an export's figure is
the host's wall clock around the whole call -- checks, the planner, the one table copy, the launch, the wait -- the median of 50 calls
after 10 warm-ups with p10 / p90, the descriptor arrays built beforehand.  The copy is timed the same way (hipMemcpyAsync +
hipStreamSynchronize).  Writes profiles/export_times.json (or the path given as the first argument)."""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lm = importlib.import_module("line-mod-pipeline_amd")

W, H, N = 640, 480, 96
WARMUP, RUNS = 10, 50


def hip_runtime():
    """The HIP runtime the library has mapped (no second runtime enters the process)"""
    lm.load_library()
    for line in open("/proc/self/maps"):
        p = line.split(None, 5)[-1].strip() if "/" in line else ""
        if os.path.basename(p).startswith("libamdhip64.so"):
            lib = C.CDLL(p, mode=os.RTLD_NOLOAD | os.RTLD_NOW)
            lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            lib.hipStreamSynchronize.argtypes = [C.c_void_p]
            return lib
    raise RuntimeError("libamdhip64.so is not mapped")


def timed(fn):
    t = []
    for k in range(WARMUP + RUNS):
        t0 = time.perf_counter()
        fn()
        if k >= WARMUP:
            t.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": float(np.median(t)), "p10_us": float(np.percentile(t, 10)), "p90_us": float(np.percentile(t, 90))}


def overlay(rng, frame):
    """About 200 primitives: a template's feature rings around three detections, each with its axes and its box"""
    rows = []
    for _ in range(3):
        cx, cy = int(rng.integers(100, W - 100)), int(rng.integers(100, H - 100))
        for _ in range(60):
            rows.append((lm.DRAW_RING, frame, cx + int(rng.integers(-60, 60)), cy + int(rng.integers(-60, 60)), 1, 0, 1, 255, 0, 0, 255))
        for k, col in enumerate(((0, 0, 255), (0, 255, 0), (255, 0, 0))):
            rows.append((lm.DRAW_SEGMENT, frame, cx, cy, cx + int(rng.integers(-70, 70)), cy + int(rng.integers(-70, 70)), 2) + col + (255,))
        rows.append((lm.DRAW_BOX, frame, cx - 70, cy - 70, cx + 70, cy + 70, 1, 0, 255, 255, 255))
    return rows


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "export_times.json")
    hip = hip_runtime()
    d = lm.Detector(color_only=True, width=W, height=H, frame_slots=N)
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(4)]
    for s in range(N):
        d.upload_frame(s, frames[s % 4])
    d.upload_wait()
    rows = []
    for f in range(N):
        rows += overlay(rng, f)
    prims = np.zeros(len(rows), lm.DRAW_PRIM_DTYPE)
    for k, r in enumerate(rows):
        prims[k] = r
    # the same list moved off the frames: every check, every record and the table copy, but no tile lists anything -- what of the
    # annotated call's cost is NOT the kernel's primitive loop
    away = prims.copy()
    for k in ("x0", "y0"):
        away[k] += 4000
    for k in ("x1", "y1"):
        away[k][away["kind"] != lm.DRAW_RING] += 4000
    res = {"frames": N, "width": W, "height": H, "runs": RUNS, "warmup": WARMUP, "primitives_per_frame": len(rows) // N, "rows": {}}
    for name, px_bytes, layout in (("bgr8", 3.0, "hwc"), ("nv12", 1.5, "nv12")):
        fb = int(W * H * px_bytes)
        dst, src = lm.DeviceBuffer(N * fb), lm.DeviceBuffer(N * fb)
        desc = (lm.ImageDesc * N)()
        for i in range(N):
            view = dst.view(np.uint8, (H, W, 3), offset=i * fb) if layout == "hwc" else dst.view(np.uint8, (H * 3 // 2, W), offset=i * fb)
            desc[i] = lm.image_desc(view, layout=layout)

        def export(p):
            ptr, n = (p.ctypes.data_as(C.c_void_p), len(p)) if p is not None else (None, 0)
            return lambda: d._check(d.lib.lm_export_frames(d.h, 0, N, desc, None, ptr, n))

        def copy():
            if hip.hipMemcpyAsync(dst.ptr, src.ptr, N * fb, 3, None) or hip.hipStreamSynchronize(None):
                raise RuntimeError("hipMemcpyAsync failed")

        row = {"bytes_written": N * fb, "plain": timed(export(None)), "annotated": timed(export(prims)),
               "annotated_off_frame": timed(export(away)), "copy_d2d": timed(copy)}
        for k in ("plain", "annotated", "annotated_off_frame", "copy_d2d"):
            # bytes moved: the frame read (3 bytes per pixel; the copy reads what it writes) and the destination written
            moved = N * fb + (N * fb if k == "copy_d2d" else N * W * H * 3)
            row[k]["GBps"] = moved / row[k]["median_us"] / 1e3
        row["annotated_over_plain"] = row["annotated"]["median_us"] / row["plain"]["median_us"]
        row["plain_over_copy"] = row["plain"]["median_us"] / row["copy_d2d"]["median_us"]
        res["rows"][name] = row
        dst.close()
        src.close()
    # what there was before: a synchronous copy of every slot's dense BGR to the host, nothing drawn, no conversion
    res["read_frame_per_slot"] = timed(lambda: [d.read_frame(s) for s in range(N)])
    d.close()
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
