"""What does the area-averaged reduction cost at ingest?  96 frames in ONE call into 640 x 480 RGB-D slots, every
frame from device addresses of its own (796 MB of BGRA: nothing is served from a cache twice), the depth image uint16 of the colour
image's size:
    reduced_bgra / reduced_nv12    1920 x 1080 at 9/4 -> 853 x 480, the window at crop 106     (k_reduce / k_reduce_conv)
    reduced_bgr                    1280 x 960 at 2/1 -> 640 x 480                              (k_reduce)
    plain_*                        lm_ingest_frames of the same sources: a 640 x 480 crop, the path that moves bytes
HIP events on a stream S of the tool's own, as tools/time_rectify.py takes them: copies that keep the GPU busy while the host enqueues,
event, ingest (it waits for S), lm_ingest_release(S), event -- the median of 50 runs after 10 warm-ups, with p10 and p90, the descriptor
arrays built beforehand.  Slot 0 of every reduced leg is compared with tests/reduce_reference.py first.  Beside each time: the bytes the
leg has to read once (the source pixels under the window, and the depth rows the nearest rule touches) and that over the time, as a
fraction of the 6.3 TB/s a streaming kernel reaches on this part.  One process.

    python tools/time_reduce.py [out.json]         -> profiles/reduce_times.json   (under a kernel trace: the kernels' times)"""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.join(HERE, "tools"))
lm = importlib.import_module("line-mod-pipeline_amd")
T = importlib.import_module("time_ingest_yuv")
RR = importlib.import_module("reduce_reference")
QR = importlib.import_module("rectify_reference")

W, H, N = 640, 480, 96
K = 4               # distinct host images per leg, uploaded to N places
HBM = 6.3e12        # bytes per second a float4 copy reaches
T.WARMUP, T.RUNS = 10, 50
LEGS = [("bgra", 1920, 1080, (9, 4), (106, 0), (640, 300)), ("nv12", 1920, 1080, (9, 4), (106, 0), (640, 300)), ("bgr", 1280, 960, (2, 1), (0, 0), (320, 240))]


def main():
    hip = T.Hip()
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    rng = np.random.default_rng(1)
    scratch = lm.DeviceBuffer(64 << 20)
    opts = (lm.IngestOpts * N)()
    res = {"frames": N, "runs": T.RUNS, "warmup": T.WARMUP, "version": d.lib.lm_version().decode().split(" (")[0], "hbm_bytes_per_s": HBM}

    def busy():        # (80 copies of 32 MB: well over a millisecond of GPU work, enqueued faster than it runs -- the call's host time hides behind it)
        for _ in range(80):
            hip.ok(hip.lib.hipMemcpyAsync(scratch.ptr, C.c_void_p(scratch.ptr.value + (32 << 20)), 32 << 20, 3, hip.stream))

    def call(fn, col, dep):
        def run():
            d._check(fn(d.h, 0, N, col, dep, opts, hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        return run

    for fmt, sw, sh, ratio, crop, plain_crop in LEGS:
        shape = {"bgra": (sh, sw, 4), "nv12": (sh * 3 // 2, sw), "bgr": (sh, sw, 3)}[fmt]
        layout = dict(layout="nv12") if fmt == "nv12" else {}
        host = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(K)]
        depth = [rng.integers(400, 3000, (sh, sw)).astype(np.uint16) for _ in range(K)]
        cbuf, dbuf = lm.DeviceBuffer(N * host[0].nbytes), lm.DeviceBuffer(N * depth[0].nbytes)
        for i in range(N):
            cbuf.upload(host[i % K], i * host[0].nbytes)
            dbuf.upload(depth[i % K], i * depth[0].nbytes)
        col, dep, pcol, pdep = (lm.ImageDesc * N)(), (lm.ImageDesc * N)(), (lm.ImageDesc * N)(), (lm.ImageDesc * N)()
        for i in range(N):
            cv, dv = cbuf.view(np.uint8, shape, offset=i * host[0].nbytes), dbuf.view(np.uint16, (sh, sw), offset=i * depth[0].nbytes)
            col[i], pcol[i] = lm.image_desc(cv, crop=crop, **layout), lm.image_desc(cv, crop=plain_crop, **layout)
            dep[i], pdep[i] = lm.image_desc(dv, depth=True, crop=crop), lm.image_desc(dv, depth=True, crop=plain_crop)
        d.set_reduction(ratio)
        reduced, plain = call(d.lib.lm_ingest_frames_reduced, col, dep), call(d.lib.lm_ingest_frames, pcol, pdep)
        # slot 0 against the reference before anything is timed
        bgr = QR.decode(host[0], fmt)
        exp = (RR.slot_colour(RR.reduce_colour(bgr, ratio), W, H, crop), RR.slot_depth(RR.reduce_depth(depth[0], ratio), W, H, crop))
        reduced()
        got = d.read_frame(0)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), "%s: slot 0 differs from the reference" % fmt
        # what the leg has to read once: the source pixels under the window (every row of the chroma plane's share included), and for the
        # depth image the rows the nearest rule touches, each over the window's columns
        nx, dx, ny, dy = RR.ratio(ratio)
        cols = -(-(crop[0] + W) * nx // dx) - crop[0] * nx // dx
        rows = -(-(crop[1] + H) * ny // dy) - crop[1] * ny // dy
        bpp = {"bgra": 4.0, "nv12": 1.5, "bgr": 3.0}[fmt]
        read = N * (cols * rows * bpp + cols * 2 * H)
        leg = {"source": "%d x %d %s + u16" % (sw, sh, fmt), "ratio": "%d/%d" % ratio, "crop": list(crop), "bytes_read_once": int(read)}
        s = T.stats(hip.time_us(reduced, busy))
        s["bytes_per_s"] = read / (s["median_us"] * 1e-6)
        s["fraction_of_hbm"] = s["bytes_per_s"] / HBM
        leg["reduced"] = s
        leg["plain_crop_only"] = T.stats(hip.time_us(plain, busy))
        if fmt == "bgra":
            d.set_reduction(ratio, depth_rule="min_valid")
            leg["reduced_depth_min_valid"] = T.stats(hip.time_us(reduced, busy))
            d.set_reduction(ratio, depth=False)
            leg["reduced_colour_only_depth_plain"] = T.stats(hip.time_us(call(d.lib.lm_ingest_frames_reduced, col, pdep), busy))
        res["reduced_" + fmt] = leg
        hip.ok(hip.lib.hipStreamSynchronize(hip.stream))
        d.upload_wait(-1)
        cbuf.close()
        dbuf.close()
    d.close()
    scratch.close()
    print(json.dumps(res, indent=1))
    out_path = next((a_ for a_ in sys.argv[1:] if a_.endswith(".json")), os.path.join(HERE, "profiles", "reduce_times.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
