"""What does rectifying at ingest cost?  96 frames in ONE call into 640 x 480 RGB-D slots, the window at (640, 300) of
a 1920 x 1080 sensor whose lens has the reference's distortion coefficients (linemod_settings.yml) at that sensor's focal length, the
depth image 1920 x 1080 uint16 aligned to the colour image:
    rectified_bgra / rectified_nv12   lm_ingest_frames_rectified (k_rectify / k_rectify_yuv: map read, four taps, blend; depth nearest)
    plain_bgra / plain_nv12           lm_ingest_frames of the same sources (k_ingest / k_ingest_yuv: the path that moves bytes)
HIP events on a stream S of the tool's own, as tools/time_register.py takes them: copies that keep the GPU busy while the host enqueues,
event, ingest (it waits for S), lm_ingest_release(S), event -- the median of 50 runs after 10 warm-ups, with p10 and p90, the descriptor
arrays built beforehand.  Slot 0 of both rectified legs is compared with tests/rectify_reference.py first.  One process.

    python tools/time_rectify.py [out.json]         -> profiles/rectify_times.json   (under a kernel trace: the kernels' shares)"""
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
QR = importlib.import_module("rectify_reference")

W, H, N = 640, 480, 96
SW, SH = 1920, 1080
CROP = (640, 300)
T.WARMUP, T.RUNS = 10, 50


def main():
    hip = T.Hip()
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    k = lm.yaml_numbers(os.path.join(HERE, "tests", "golden", "reference_data", "linemod_settings.yml"), "distortion parameters")
    source = QR.cam(SW, SH, 1044.87 * 3, 1045.69141 * 3, 959.5, 539.5, tuple(float(v) for v in k))
    ideal = QR.pinhole_of(source)
    d.set_rectification(lm.camera(SW, SH, source["fx"], source["fy"], source["cx"], source["cy"], source["dist"]))
    qmap = QR.build_map(source, ideal)
    assert np.array_equal(d.rectification_map(), qmap)
    rng = np.random.default_rng(1)
    K = 4           # distinct depth images, taken in turns
    bgra = [rng.integers(0, 256, (SH, SW, 4), dtype=np.uint8) for _ in range(2)]
    nv12 = [rng.integers(0, 256, (SH * 3 // 2, SW), dtype=np.uint8) for _ in range(2)]
    depth = [rng.integers(400, 3000, (SH, SW)).astype(np.uint16) for _ in range(K)]
    abuf, nbuf, dbuf = lm.DeviceBuffer(2 * bgra[0].nbytes), lm.DeviceBuffer(2 * nv12[0].nbytes), lm.DeviceBuffer(K * depth[0].nbytes)
    for i in range(2):
        abuf.upload(bgra[i], i * bgra[0].nbytes)
        nbuf.upload(nv12[i], i * nv12[0].nbytes)
    for i in range(K):
        dbuf.upload(depth[i], i * depth[0].nbytes)
    scratch = lm.DeviceBuffer(64 << 20)
    col_a, col_n, dep, opts = (lm.ImageDesc * N)(), (lm.ImageDesc * N)(), (lm.ImageDesc * N)(), (lm.IngestOpts * N)()
    for i in range(N):
        col_a[i] = lm.image_desc(abuf.view(np.uint8, (SH, SW, 4), offset=(i % 2) * bgra[0].nbytes), crop=CROP)
        col_n[i] = lm.image_desc(nbuf.view(np.uint8, (SH * 3 // 2, SW), offset=(i % 2) * nv12[0].nbytes), layout="nv12", crop=CROP)
        dep[i] = lm.image_desc(dbuf.view(np.uint16, (SH, SW), offset=(i % K) * depth[0].nbytes), depth=True, crop=CROP)

    def rectified(col):
        def fn():
            d._check(d.lib.lm_ingest_frames_rectified(d.h, 0, N, col, dep, opts, lm.RECTIFY_DEPTH_ALIGNED, hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        return fn

    def plain(col):
        def fn():
            d._check(d.lib.lm_ingest_frames(d.h, 0, N, col, dep, opts, hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        return fn

    def busy():        # (80 copies of 32 MB: well over a millisecond of GPU work, enqueued faster than it runs -- the call's host time hides behind it)
        for _ in range(80):
            hip.ok(hip.lib.hipMemcpyAsync(scratch.ptr, C.c_void_p(scratch.ptr.value + (32 << 20)), 32 << 20, 3, hip.stream))

    Rd = QR.slot_depth(QR.rectify_depth(depth[0], qmap), W, H, CROP)
    for col, img in ((col_a, np.ascontiguousarray(bgra[0][:, :, :3])), (col_n, QR.decode(nv12[0], "nv12"))):
        rectified(col)()
        got = d.read_frame(0)
        assert np.array_equal(got[0], QR.slot_colour(QR.rectify_colour(img, qmap), W, H, CROP)) and np.array_equal(got[1], Rd), "slot 0 differs from the reference"
    win = qmap[CROP[1]:CROP[1] + H, CROP[0]:CROP[0] + W].astype(np.float64) / 32.0
    i, j = np.meshgrid(np.arange(CROP[0], CROP[0] + W), np.arange(CROP[1], CROP[1] + H))
    res = {"frames": N, "runs": T.RUNS, "warmup": T.WARMUP, "version": d.lib.lm_version().decode().split(" (")[0],
           "largest_displacement_in_the_window_px": float(np.hypot(win[:, :, 0] - i, win[:, :, 1] - j).max()),
           "rectified_bgra": T.stats(hip.time_us(rectified(col_a), busy)), "plain_bgra": T.stats(hip.time_us(plain(col_a), busy)),
           "rectified_nv12": T.stats(hip.time_us(rectified(col_n), busy)), "plain_nv12": T.stats(hip.time_us(plain(col_n), busy))}
    res["rectified_bgra_again"] = T.stats(hip.time_us(rectified(col_a), busy))
    hip.ok(hip.lib.hipStreamSynchronize(hip.stream))
    d.upload_wait(-1)
    d.close()
    for b in (abuf, nbuf, dbuf, scratch):
        b.close()
    print(json.dumps(res, indent=1))
    out_path = next((a_ for a_ in sys.argv[1:] if a_.endswith(".json")), os.path.join(HERE, "profiles", "rectify_times.json"))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
