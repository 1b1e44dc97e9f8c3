"""What does the lens map in front of the box cost at ingest?  96 frames in ONE call into 640 x 480 RGB-D slots,
every frame from device addresses of its own (796 MB of BGRA: nothing of a source is served from a cache twice), 1920 x 1080 through a
Brown-Conrady lens, reduced 9/4 -> 853 x 480, the window at crop 106:
    bgra / nv12            lm_ingest_frames_rectified_reduced, the depth image uint16 of the source camera, DEPTH_ALIGNED, NEAREST
    bgra_min_valid         the same with the MIN_VALID depth rule
    bgra_registered        DEPTH_REGISTERED from an 848 x 480 raw depth image onto the slot's camera
and on the same sources, in the same session, the two routes that existed as yard-sticks:
    reduced_*              lm_ingest_frames_reduced at 9/4 -- the floor: the same reads, no map, no blend
    rectified_*            lm_ingest_frames_rectified into a 640 x 480 window of the ideal geometry -- a ninth of the work per slot pixel
Every rectified-and-reduced leg is timed in both grid orders (LM_TUNE_RECTIFY_REDUCE_GRID).  HIP events on a stream S of the tool's own,
as tools/time_reduce.py takes them: copies that keep the GPU busy while the host enqueues, event, ingest (it waits for S),
lm_ingest_release(S), event -- the median of 50 runs after 10 warm-ups, with p10 and p90, the descriptor arrays built beforehand.  Slot 0
of every leg is compared with the composed reference (tests/rectify_reduce_scenes.py; the registered depth: tests/register_reference.py)
before anything is timed.  Beside each time: the bytes the leg has to read once -- the source pixels under the window, the depth rows the
nearest rule touches, and ONE pass over the map entries under the window -- and that over the time, as a fraction of the 6.3 TB/s a
streaming kernel reaches on this part.  One process.

    python tools/time_rectify_reduce.py [out.json]         -> profiles/rectify_reduce_times.json"""
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
GR = importlib.import_module("register_reference")
X = importlib.import_module("rectify_reduce_scenes")

W, H, N = 640, 480, 96
SW, SH = 1920, 1080
K = 4               # distinct host images per leg, uploaded to N places
HBM = 6.3e12        # bytes per second a float4 copy reaches
T.WARMUP, T.RUNS = 10, 50
RATIO, CROP, RECT_CROP = (9, 4), (106, 0), (640, 300)
SOURCE = QR.cam(SW, SH, 1050.0, 1052.0, 965.5, 533.5, (-0.12, 0.03, 0.001, -0.001, 0.0))
IDEAL = QR.cam(SW, SH, 1000.0, 1000.0, 959.5, 539.5)
RAW_W, RAW_H = 848, 480
ROT = np.eye(3, dtype=np.float32)
TRANS = np.array([52.0, -4.0, 3.0], np.float32)


def to_cam(c):
    return lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])


def main():
    hip = T.Hip()
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    rng = np.random.default_rng(1)
    scratch = lm.DeviceBuffer(64 << 20)
    opts = (lm.IngestOpts * N)()
    res = {"frames": N, "runs": T.RUNS, "warmup": T.WARMUP, "version": d.lib.lm_version().decode().split(" (")[0], "hbm_bytes_per_s": HBM,
           "source": "%d x %d" % (SW, SH), "ratio": "%d/%d" % RATIO, "crop": list(CROP)}
    d.set_rectification(to_cam(SOURCE), to_cam(IDEAL))
    qmap = QR.build_map(SOURCE, IDEAL)
    assert np.array_equal(d.rectification_map(), qmap)

    def busy():        # (80 copies of 32 MB: well over a millisecond of GPU work, enqueued faster than it runs -- the call's host time hides behind it)
        for _ in range(80):
            hip.ok(hip.lib.hipMemcpyAsync(scratch.ptr, C.c_void_p(scratch.ptr.value + (32 << 20)), 32 << 20, 3, hip.stream))

    def call(fn, col, dep, route=None):
        def run():
            if route is None:
                d._check(fn(d.h, 0, N, col, dep, opts, hip.stream))
            else:
                d._check(fn(d.h, 0, N, col, dep, opts, route, hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        return run

    def both_orders(run):
        out = {}
        for order, name in ((0, "grid_frame_on_y"), (1, "grid_frame_fastest")):
            d.set_tuning(lm.TUNE_RECTIFY_REDUCE_GRID, order)
            out[name] = T.stats(hip.time_us(run, busy))
        d.set_tuning(lm.TUNE_RECTIFY_REDUCE_GRID, 0)
        return out

    nx, dx, ny, dy = RR.ratio(RATIO)
    cols = -(-(CROP[0] + W) * nx // dx) - CROP[0] * nx // dx
    rows = -(-(CROP[1] + H) * ny // dy) - CROP[1] * ny // dy
    depth = [rng.integers(400, 3000, (SH, SW)).astype(np.uint16) for _ in range(K)]
    dbuf = lm.DeviceBuffer(N * depth[0].nbytes)
    for i in range(N):
        dbuf.upload(depth[i % K], i * depth[0].nbytes)
    dviews = [dbuf.view(np.uint16, (SH, SW), offset=i * depth[0].nbytes) for i in range(N)]
    dep, rdep = (lm.ImageDesc * N)(), (lm.ImageDesc * N)()
    for i in range(N):
        dep[i], rdep[i] = lm.image_desc(dviews[i], depth=True, crop=CROP), lm.image_desc(dviews[i], depth=True, crop=RECT_CROP)
    Rd = QR.rectify_depth(depth[0], qmap)
    exp_d = RR.slot_depth(RR.reduce_depth(Rd, RATIO), W, H, CROP)

    for fmt in ("bgra", "nv12"):
        shape = {"bgra": (SH, SW, 4), "nv12": (SH * 3 // 2, SW)}[fmt]
        layout = dict(layout="nv12") if fmt == "nv12" else {}
        host = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(K)]
        cbuf = lm.DeviceBuffer(N * host[0].nbytes)
        for i in range(N):
            cbuf.upload(host[i % K], i * host[0].nbytes)
        col, rcol = (lm.ImageDesc * N)(), (lm.ImageDesc * N)()
        for i in range(N):
            cv = cbuf.view(np.uint8, shape, offset=i * host[0].nbytes)
            col[i], rcol[i] = lm.image_desc(cv, crop=CROP, **layout), lm.image_desc(cv, crop=RECT_CROP, **layout)
        bpp = {"bgra": 4.0, "nv12": 1.5}[fmt]
        # what a leg has to read once: the source pixels under the window (taken as the ideal pixels under it: the lens moves them, it
        # does not multiply them), the depth rows the nearest rule touches, and the map entries under the window ONCE per call
        read = N * (cols * rows * bpp + cols * 2 * H) + cols * rows * 8
        Ac = RR.reduce_colour(QR.rectify_colour(QR.decode(host[0], fmt), qmap), RATIO)
        exp_c = RR.slot_colour(Ac, W, H, CROP)
        d.set_reduction(RATIO)
        run = call(d.lib.lm_ingest_frames_rectified_reduced, col, dep, lm.RECTIFY_DEPTH_ALIGNED)
        for order in (0, 1):
            d.set_tuning(lm.TUNE_RECTIFY_REDUCE_GRID, order)
            run()
            got = d.read_frame(0)
            assert np.array_equal(got[0], exp_c), "%s, grid order %d: slot 0's colour differs from the composed reference" % (fmt, order)
            assert np.array_equal(got[1], exp_d), "%s: slot 0's depth differs" % fmt
        leg = {"source": "%d x %d %s + u16" % (SW, SH, fmt), "bytes_read_once": int(read), "map_bytes_under_window": int(cols * rows * 8)}
        leg.update(both_orders(run))
        for name in ("grid_frame_on_y", "grid_frame_fastest"):
            leg[name]["bytes_per_s"] = read / (leg[name]["median_us"] * 1e-6)
            leg[name]["fraction_of_hbm"] = leg[name]["bytes_per_s"] / HBM
        leg["reduced_yardstick"] = T.stats(hip.time_us(call(d.lib.lm_ingest_frames_reduced, col, dep), busy))
        leg["rectified_window_yardstick"] = T.stats(hip.time_us(call(d.lib.lm_ingest_frames_rectified, rcol, rdep, lm.RECTIFY_DEPTH_ALIGNED), busy))
        res[fmt] = leg
        if fmt == "bgra":
            d.set_reduction(RATIO, depth_rule="min_valid")
            run()
            got = d.read_frame(0)
            assert np.array_equal(got[0], exp_c) and np.array_equal(got[1], RR.slot_depth(RR.reduce_depth(Rd, RATIO, "min_valid"), W, H, CROP)), "min_valid: slot 0 differs"
            res["bgra_min_valid"] = both_orders(run)
            res["bgra_min_valid"]["reduced_yardstick"] = T.stats(hip.time_us(call(d.lib.lm_ingest_frames_reduced, col, dep), busy))
            # the registered depth: an 848 x 480 raw image onto the slot's camera, the reduced ideal one
            d.set_reduction(RATIO)
            cc = lm.reduced_camera(to_cam(IDEAL), RATIO)
            dc = GR.cam(RAW_W, RAW_H, 420.0, 420.0, 423.5, 239.5)
            d.set_registration(to_cam(dc), cc, ROT, TRANS, splat=(1, 1))
            raw = [rng.integers(700, 2500, (RAW_H, RAW_W)).astype(np.uint16) for _ in range(K)]
            rbuf = lm.DeviceBuffer(N * raw[0].nbytes)
            rawd = (lm.ImageDesc * N)()
            for i in range(N):
                rbuf.upload(raw[i % K], i * raw[0].nbytes)
                rawd[i] = lm.image_desc(rbuf.view(np.uint16, (RAW_H, RAW_W), offset=i * raw[0].nbytes), depth=True, crop=CROP)
            Rg = GR.register(raw[0], 1.0, d.registration_rays(), GR.cam(cc.width, cc.height, cc.fx, cc.fy, cc.cx, cc.cy), ROT, TRANS, (1, 1))
            run = call(d.lib.lm_ingest_frames_rectified_reduced, col, rawd, lm.RECTIFY_DEPTH_REGISTERED)
            run()
            got = d.read_frame(0)
            assert np.array_equal(got[0], exp_c) and np.array_equal(got[1], RR.slot_depth(Rg, W, H, CROP)), "registered: slot 0 differs"
            res["bgra_registered"] = both_orders(run)
            res["bgra_registered"]["raw_depth"] = "%d x %d u16" % (RAW_W, RAW_H)
            hip.ok(hip.lib.hipStreamSynchronize(hip.stream))
            d.upload_wait(-1)
            d.set_registration(None, None, None, None)
            rbuf.close()
        hip.ok(hip.lib.hipStreamSynchronize(hip.stream))
        d.upload_wait(-1)
        cbuf.close()
    dbuf.close()
    d.close()
    scratch.close()
    print(json.dumps(res, indent=1))
    out_path = next((a_ for a_ in sys.argv[1:] if a_.endswith(".json")), os.path.join(HERE, "profiles", "rectify_reduce_times.json"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
