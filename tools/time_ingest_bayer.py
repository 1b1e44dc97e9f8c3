"""What does the raw Bayer source format of lm_ingest_frames cost ("Bayer sources")?  96 frames in ONE call into
640 x 480 RGB-D slots, the window at (640, 300) of a 1920 x 1080 sensor (a multiple of 16 columns in: the kernels' fast path), the
depth image 1920 x 1080 uint16 aligned to the colour image:
    plain_bayer         LM_PIX_BAYER_RGGB8   k_ingest_bayer: 1 source byte per colour pixel, three source rows per output row
    plain_gray8         LM_PIX_GRAY8         k_ingest_yuv: the same bytes per pixel, one row -- the byte-moving floor
    plain_bgra          LM_PIX_BGRA8         k_ingest: what a caller who demosaics in front of the ingest would hand over
    plain_bayer_odd     the Bayer source with the window at (641, 301): the general path (unaligned spans, the other colour phase)
    rectified_bayer / rectified_bgra         lm_ingest_frames_rectified of the same sources (k_rectify_bayer / k_rectify), the lens of
                                             tools/time_rectify.py
HIP events on a stream S of the tool's own, as tools/time_rectify.py takes them: copies that keep the GPU busy while the host enqueues,
event, ingest (it waits for S), lm_ingest_release(S), event -- the median of 50 runs after 10 warm-ups, with p10 and p90, the descriptor
arrays built beforehand.  Slot 0 of every leg is compared with the references of tests/ first.  One process.

    python tools/time_ingest_bayer.py [out.json]         -> profiles/ingest_bayer_times.json   (under a kernel trace: the kernels' shares)"""
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
BR = importlib.import_module("ingest_bayer_reference")
IR = importlib.import_module("ingest_reference")
QR = importlib.import_module("rectify_reference")

W, H, N = 640, 480, 96
SW, SH = 1920, 1080
CROP, ODD = (640, 300), (641, 301)
T.WARMUP, T.RUNS = 10, 50


def main():
    hip = T.Hip()
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    k = lm.yaml_numbers(os.path.join(HERE, "tests", "golden", "reference_data", "linemod_settings.yml"), "distortion parameters")
    source = QR.cam(SW, SH, 1044.87 * 3, 1045.69141 * 3, 959.5, 539.5, tuple(float(v) for v in k))
    d.set_rectification(lm.camera(SW, SH, source["fx"], source["fy"], source["cx"], source["cy"], source["dist"]))
    qmap = QR.build_map(source, QR.pinhole_of(source))
    rng = np.random.default_rng(1)
    K = 4           # distinct depth images, taken in turns
    raw = [rng.integers(0, 256, (SH, SW), dtype=np.uint8) for _ in range(2)]
    bgra = [rng.integers(0, 256, (SH, SW, 4), dtype=np.uint8) for _ in range(2)]
    depth = [rng.integers(400, 3000, (SH, SW)).astype(np.uint16) for _ in range(K)]
    rbuf, abuf, dbuf = lm.DeviceBuffer(2 * raw[0].nbytes), lm.DeviceBuffer(2 * bgra[0].nbytes), lm.DeviceBuffer(K * depth[0].nbytes)
    for i in range(2):
        rbuf.upload(raw[i], i * raw[0].nbytes)
        abuf.upload(bgra[i], i * bgra[0].nbytes)
    for i in range(K):
        dbuf.upload(depth[i], i * depth[0].nbytes)
    scratch = lm.DeviceBuffer(64 << 20)
    arrays = lambda: (lm.ImageDesc * N)()
    col_b, col_g, col_a, col_o, dep, dep_o, opts = arrays(), arrays(), arrays(), arrays(), arrays(), arrays(), (lm.IngestOpts * N)()
    for i in range(N):
        rview = rbuf.view(np.uint8, (SH, SW), offset=(i % 2) * raw[0].nbytes)
        dview = dbuf.view(np.uint16, (SH, SW), offset=(i % K) * depth[0].nbytes)
        col_b[i] = lm.image_desc(rview, layout="bayer_rggb", crop=CROP)
        col_o[i] = lm.image_desc(rview, layout="bayer_rggb", crop=ODD)
        col_g[i] = lm.image_desc(rview, layout="gray", crop=CROP)
        col_a[i] = lm.image_desc(abuf.view(np.uint8, (SH, SW, 4), offset=(i % 2) * bgra[0].nbytes), crop=CROP)
        dep[i] = lm.image_desc(dview, depth=True, crop=CROP)
        dep_o[i] = lm.image_desc(dview, depth=True, crop=ODD)

    def rectified(col):
        def fn():
            d._check(d.lib.lm_ingest_frames_rectified(d.h, 0, N, col, dep, opts, lm.RECTIFY_DEPTH_ALIGNED, hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        return fn

    def plain(col, dep_=dep):
        def fn():
            d._check(d.lib.lm_ingest_frames(d.h, 0, N, col, dep_, opts, hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        return fn

    def busy():        # (80 copies of 32 MB: well over a millisecond of GPU work, enqueued faster than it runs -- the call's host time hides behind it)
        for _ in range(80):
            hip.ok(hip.lib.hipMemcpyAsync(scratch.ptr, C.c_void_p(scratch.ptr.value + (32 << 20)), 32 << 20, 3, hip.stream))

    # slot 0 of every leg against the references
    demosaiced = BR.demosaic(raw[0], "rggb")
    grey = np.stack([raw[0]] * 3, axis=-1)
    plain_legs = {"plain_bayer": (col_b, dep, demosaiced, CROP), "plain_gray8": (col_g, dep, grey, CROP),
                  "plain_bgra": (col_a, dep, np.ascontiguousarray(bgra[0][:, :, :3]), CROP), "plain_bayer_odd": (col_o, dep_o, demosaiced, ODD)}
    for name, (col, dep_, img, crop) in plain_legs.items():
        plain(col, dep_)()
        got = d.read_frame(0)
        assert np.array_equal(got[0], IR.colour(img, W, H, crop=crop)) and np.array_equal(got[1], IR.depth(depth[0], W, H, crop)), name + ": slot 0 differs from the reference"
    Rd = QR.slot_depth(QR.rectify_depth(depth[0], qmap), W, H, CROP)
    rect_legs = {"rectified_bayer": (col_b, demosaiced), "rectified_bgra": (col_a, np.ascontiguousarray(bgra[0][:, :, :3]))}
    for name, (col, img) in rect_legs.items():
        rectified(col)()
        got = d.read_frame(0)
        assert np.array_equal(got[0], QR.slot_colour(QR.rectify_colour(img, qmap), W, H, CROP)) and np.array_equal(got[1], Rd), name + ": slot 0 differs from the reference"

    res = {"frames": N, "runs": T.RUNS, "warmup": T.WARMUP, "version": d.lib.lm_version().decode().split(" (")[0], "source": [SW, SH], "window_at": list(CROP)}
    for name, (col, dep_, _, _) in plain_legs.items():
        res[name] = T.stats(hip.time_us(plain(col, dep_), busy))
    for name, (col, _) in rect_legs.items():
        res[name] = T.stats(hip.time_us(rectified(col), busy))
    res["plain_bayer_again"] = T.stats(hip.time_us(plain(col_b), busy))           # the spread of the same leg within the session
    for name in ("plain_bayer", "plain_bayer_odd"):
        res[name]["ratio_to_gray8"] = res[name]["median_us"] / res["plain_gray8"]["median_us"]
        res[name]["ratio_to_bgra"] = res[name]["median_us"] / res["plain_bgra"]["median_us"]
    res["rectified_bayer"]["ratio_to_bgra"] = res["rectified_bayer"]["median_us"] / res["rectified_bgra"]["median_us"]
    hip.ok(hip.lib.hipStreamSynchronize(hip.stream))
    d.upload_wait(-1)
    d.close()
    for b in (rbuf, abuf, dbuf, scratch):
        b.close()
    print(json.dumps(res, indent=1))
    out_path = next((a_ for a_ in sys.argv[1:] if a_.endswith(".json")), os.path.join(HERE, "profiles", "ingest_bayer_times.json"))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
