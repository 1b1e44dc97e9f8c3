"""What do the high-bit raw source formats and the raw pipeline of lm_ingest_frames cost ("High-bit raw sources and
the raw pipeline")?  tools/time_ingest_bayer.py's protocol: 96 frames in ONE call into 640 x 480 RGB-D slots, the window at (640, 300) of
a 1920 x 1080 sensor, the depth image 1920 x 1080 uint16 aligned to the colour image:
    bayer_rggb8         LM_PIX_BAYER_RGGB8, nothing set     k_ingest_bayer, the unprocessed kernel: the yardstick
    rggb8_hard          the same source under the hard pipeline   k_ingest_raw, N = 8: what the pipeline itself costs
    rggb12              LM_PIX_BAYER_RGGB12    2 source bytes per pixel
    rggb12p             LM_PIX_BAYER_RGGB12P   1.5 bytes per pixel and the unpacking
    rggb10p             LM_PIX_BAYER_RGGB10P   1.25 bytes per pixel, four bit phases
    mono12              LM_PIX_MONO12          one source row per output row, no stencil
    rectified_rggb12    lm_ingest_frames_rectified of the RGGB12 source (k_rectify_raw), the lens of tools/time_rectify.py
Every raw leg runs under the hard pipeline (a saturating gain, negative matrix entries, a random tone table: lookups without locality).
HIP events on a stream S of the tool's own, as tools/time_rectify.py takes them: copies that keep the GPU busy while the host enqueues,
event, ingest (it waits for S), lm_ingest_release(S), event -- the median of 50 runs after 10 warm-ups, with p10 and p90, the descriptor
arrays built beforehand.  Slot 0 of every leg is compared with the references of tests/ first.  One process.

    python tools/time_ingest_raw.py [out.json]         -> profiles/ingest_raw_times.json   (under a kernel trace: the kernels' shares)"""
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
RR = importlib.import_module("ingest_raw_reference")
IR = importlib.import_module("ingest_reference")
QR = importlib.import_module("rectify_reference")

W, H, N = 640, 480, 96
SW, SH = 1920, 1080
CROP = (640, 300)
T.WARMUP, T.RUNS = 10, 50


def hard_pipe():
    return dict(black=60, gain=np.array([30000, 1100, 700]), ccm=np.array([[1900, -700, -300], [-5000, 2500, -400], [3000, 4000, 6000]]),
                tone=np.random.default_rng(5).integers(0, 256, 4096).astype(np.uint8))


def set_pipe(d, pipe):
    if pipe is None:
        d.set_raw_processing(None)
    else:
        d.set_raw_processing(black=pipe["black"], gains=pipe["gain"] / 1024.0, ccm=pipe["ccm"] / 1024.0, tone=pipe["tone"])


def window_reference(samples, bits, pattern, pipe):
    """The slot's colour image: the rule on the window and a ring of two samples around it (an even origin keeps the pattern's phase; a
    pixel reads its 3 x 3 neighbourhood alone and the window lies inside the source)."""
    x0, y0 = CROP[0] - 2, CROP[1] - 2
    return RR.process(samples[y0:y0 + H + 4, x0:x0 + W + 4], bits, pattern, pipe)[2:-2, 2:-2]


def main():
    hip = T.Hip()
    k = lm.yaml_numbers(os.path.join(HERE, "tests", "golden", "reference_data", "linemod_settings.yml"), "distortion parameters")
    source = QR.cam(SW, SH, 1044.87 * 3, 1045.69141 * 3, 959.5, 539.5, tuple(float(v) for v in k))
    qmap = QR.build_map(source, QR.pinhole_of(source))
    rng = np.random.default_rng(1)
    K = 4           # distinct depth images, taken in turns
    depth = [rng.integers(400, 3000, (SH, SW)).astype(np.uint16) for _ in range(K)]
    dbuf = lm.DeviceBuffer(K * depth[0].nbytes)
    for i in range(K):
        dbuf.upload(depth[i], i * depth[0].nbytes)
    scratch = lm.DeviceBuffer(64 << 20)
    pipe = hard_pipe()
    # name -> (bits, packed, pattern, two images of samples)
    sources = {"rggb8": (8, False, "rggb"), "rggb12": (12, False, "rggb"), "rggb12p": (12, True, "rggb"), "rggb10p": (10, True, "rggb"), "mono12": (12, False, "mono")}
    samples, bufs, views = {}, {}, {}
    for name, (bits, packed, _) in sources.items():
        samples[name] = [rng.integers(0, 1 << bits, (SH, SW)) for _ in range(2)]
        rows = [s.astype(np.uint8) if bits == 8 else RR.pack(s, bits) if packed else RR.container(s) for s in samples[name]]
        bufs[name] = lm.DeviceBuffer(2 * rows[0].nbytes)
        for i in range(2):
            bufs[name].upload(rows[i], i * rows[0].nbytes)
        views[name] = [bufs[name].view(rows[0].dtype.type, rows[0].shape, offset=i * rows[0].nbytes) for i in range(2)]
    arrays = lambda: (lm.ImageDesc * N)()
    col, dep, opts = {name: arrays() for name in sources}, arrays(), (lm.IngestOpts * N)()
    for i in range(N):
        dep[i] = lm.image_desc(dbuf.view(np.uint16, (SH, SW), offset=(i % K) * depth[0].nbytes), depth=True, crop=CROP)
        for name, (bits, packed, pattern) in sources.items():
            layout = "mono" if pattern == "mono" else "bayer_" + pattern
            col[name][i] = lm.image_desc(views[name][i % 2], layout=layout, crop=CROP, bits=bits, packed=packed, width=SW if packed else None)

    def busy():        # (80 copies of 32 MB: well over a millisecond of GPU work, enqueued faster than it runs -- the call's host time hides behind it)
        for _ in range(80):
            hip.ok(hip.lib.hipMemcpyAsync(scratch.ptr, C.c_void_p(scratch.ptr.value + (32 << 20)), 32 << 20, 3, hip.stream))

    res = {"frames": N, "runs": T.RUNS, "warmup": T.WARMUP, "source": [SW, SH], "window_at": list(CROP)}
    ed = IR.depth(depth[0], W, H, CROP)
    legs = [("bayer_rggb8", "rggb8", None), ("rggb8_hard", "rggb8", pipe), ("rggb12", "rggb12", pipe), ("rggb12p", "rggb12p", pipe), ("rggb10p", "rggb10p", pipe),
            ("mono12", "mono12", pipe)]
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    res["version"] = d.lib.lm_version().decode().split(" (")[0]
    d.set_rectification(lm.camera(SW, SH, source["fx"], source["fy"], source["cx"], source["cy"], source["dist"]))

    def plain(c):
        def fn():
            d._check(d.lib.lm_ingest_frames(d.h, 0, N, c, dep, opts, hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        return fn

    def rectified(c):
        def fn():
            d._check(d.lib.lm_ingest_frames_rectified(d.h, 0, N, c, dep, opts, lm.RECTIFY_DEPTH_ALIGNED, hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        return fn

    for name, src, p in legs:
        bits, _, pattern = sources[src]
        set_pipe(d, p)
        plain(col[src])()
        got = d.read_frame(0)
        want = IR.colour(BR.demosaic(samples[src][0].astype(np.uint8), pattern), W, H, crop=CROP) if p is None else window_reference(samples[src][0], bits, pattern, p)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], ed), name + ": slot 0 differs from the reference"
        res[name] = T.stats(hip.time_us(plain(col[src]), busy))
    whole = RR.process(samples["rggb12"][0], 12, "rggb", pipe)
    rectified(col["rggb12"])()
    got = d.read_frame(0)
    assert np.array_equal(got[0], QR.slot_colour(QR.rectify_colour(whole, qmap), W, H, CROP)), "rectified_rggb12: slot 0 differs from the reference"
    assert np.array_equal(got[1], QR.slot_depth(QR.rectify_depth(depth[0], qmap), W, H, CROP)), "rectified_rggb12: depth differs"
    res["rectified_rggb12"] = T.stats(hip.time_us(rectified(col["rggb12"]), busy))
    set_pipe(d, None)
    res["bayer_rggb8_again"] = T.stats(hip.time_us(plain(col["rggb8"]), busy))          # the spread of the same leg within the session
    hip.ok(hip.lib.hipStreamSynchronize(hip.stream))
    d.upload_wait(-1)
    d.close()
    for name in res:
        if isinstance(res[name], dict) and name != "bayer_rggb8":
            res[name]["ratio_to_rggb8"] = res[name]["median_us"] / res["bayer_rggb8"]["median_us"]
    for b in list(bufs.values()) + [dbuf, scratch]:
        b.close()
    print(json.dumps(res, indent=1))
    out_path = next((a_ for a_ in sys.argv[1:] if a_.endswith(".json")), os.path.join(HERE, "profiles", "ingest_raw_times.json"))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
