"""What do the float colour sources of lm_ingest_frames and the float destinations of lm_export_frames cost (DESIGN.md sections 13 and 23)?
96 frames of 640 x 480, colour only, in ONE call, all sources 16-byte aligned and without geometry (the kernels' fast path):
    bgr8              k_ingest: 3 source bytes per pixel
    bgr_f32_planar    k_ingest_float: 12 source bytes per pixel, three planes (a torch tensor [3, H, W])
    rgba_f16          k_ingest_float: 8 source bytes per pixel (a renderer's RGBA16F target)
    rgba_f32          k_ingest_float: 16 source bytes per pixel (RGBA32F)
    bgr8_again        the first case once more behind the others: the run-to-run spread of this very measurement
HIP events on a stream S of the tool's own, as tools/time_ingest_yuv.py takes them (its Hip class): copies that keep the GPU busy while
the host enqueues, event, ingest (it waits for S), lm_ingest_release(S), event -- the median of 60 runs after 10 warm-ups, the descriptor
arrays built beforehand.  Every case's slots are compared with tests/ingest_float_reference.py before it is timed.  bytes moved = the
source bytes read + the 3 bytes per pixel written.
The export is synchronous on a stream of its own: as in tools/time_export.py its figure is the host's wall clock around the whole call
(median of 50 after 10 warm-ups), to BGR8 and to RGB_F32_PLANAR at 1 / 255 (a network's input), no primitives.

    python tools/time_ingest_float.py [out.json]          -> profiles/ingest_float_times.json"""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.join(HERE, "tools"))
lm = importlib.import_module("line-mod-pipeline_amd")
FR = importlib.import_module("ingest_float_reference")
from time_ingest_yuv import Hip, stats          # noqa: E402  (the event timing, shared)

W, H, N = 640, 480, 96


def main():
    out_path = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(HERE, "profiles", "ingest_float_times.json"))
    hip = Hip()
    d = lm.Detector(color_only=True, width=W, height=H, frame_slots=N)
    rng = np.random.default_rng(5)
    px = W * H
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(4)]
    unit = [f.astype(np.float32) / np.float32(255.0) for f in frames]
    assert all(np.array_equal(FR.to_u8(u, 255.0), f) for u, f in zip(unit, frames))
    # name -> (host frames in the producer's layout, image_desc's keywords, source bytes per pixel)
    rgba = [np.concatenate([u[..., ::-1], np.ones((H, W, 1), np.float32)], axis=-1) for u in unit]
    cases = {"bgr8": (frames, dict(), 3),
             "bgr_f32_planar": ([np.ascontiguousarray(np.transpose(u, (2, 0, 1))) for u in unit], dict(layout="chw", float_scale=255.0), 12),
             "rgba_f16": ([r.astype(np.float16) for r in rgba], dict(order="rgb", float_scale=255.0), 8),
             "rgba_f32": (rgba, dict(order="rgb", float_scale=255.0), 16)}
    assert all(np.array_equal(FR.to_u8(r.astype(np.float16)[..., 2::-1], 255.0), f) for r, f in zip(rgba, frames))
    busy_src, busy_dst = lm.DeviceBuffer(N * px * 3), lm.DeviceBuffer(N * px * 3)

    def busy():
        for _ in range(10):
            hip.ok(hip.lib.hipMemcpyAsync(busy_dst.ptr, busy_src.ptr, N * px * 3, 3, hip.stream))

    res = {"frames": N, "width": W, "height": H, "runs": 60, "warmup": 10, "version": d.lib.lm_version().decode().split(" (")[0], "ingest": {}, "export": {}}
    opts = (lm.IngestOpts * N)()
    for name in ("bgr8", "bgr_f32_planar", "rgba_f16", "rgba_f32", "bgr8"):
        host, kw, spp = cases[name]
        fb = host[0].nbytes
        buf = lm.DeviceBuffer(N * fb)
        for i in range(N):
            buf.upload(host[i % 4], i * fb)
        col = (lm.ImageDesc * N)()
        for i in range(N):
            col[i] = lm.image_desc(buf.view(host[0].dtype.type, host[0].shape, offset=i * fb), **kw)

        def fn():
            d._check(d.lib.lm_ingest_frames(d.h, 0, N, col, None, opts, hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        fn()
        for i in (0, 1, N - 1):
            assert np.array_equal(d.read_frame(i)[0], frames[i % 4]), "%s: slot %d differs from the reference" % (name, i)
        t = hip.time_us(fn, busy)
        key = name if name not in res["ingest"] else name + "_again"
        res["ingest"][key] = dict(stats(t), source_bytes_per_pixel=spp, GBps=(spp + 3) * px * N / float(np.median(t)) / 1e3,
                                  source_GBps=spp * px * N / float(np.median(t)) / 1e3)
        hip.ok(hip.lib.hipStreamSynchronize(hip.stream))
        d.upload_wait(-1)
        buf.close()

    # the way out: BGR8 beside RGB_F32_PLANAR
    scale = float(np.float32(1.0) / np.float32(255.0))
    for name, dtype, shape, kw, bpp in (("bgr8", np.uint8, (H, W, 3), dict(), 3), ("rgb_f32_planar", np.float32, (3, H, W), dict(layout="chw", order="rgb", float_scale=scale), 12),
                                        ("bgr8_again", np.uint8, (H, W, 3), dict(), 3)):
        fb = px * bpp
        dst = lm.DeviceBuffer(N * fb)
        desc = (lm.ImageDesc * N)()
        for i in range(N):
            desc[i] = lm.image_desc(dst.view(dtype, shape, offset=i * fb), **kw)
        call = lambda: d._check(d.lib.lm_export_frames(d.h, 0, N, desc, None, None, 0))
        call()
        got = dst.download(dtype, shape, offset=(N - 1) * fb)
        want = frames[(N - 1) % 4] if bpp == 3 else FR.from_u8(np.transpose(frames[(N - 1) % 4][..., ::-1], (2, 0, 1)), scale, False).view(np.float32)
        assert np.array_equal(got, want), "export %s differs from the reference" % name
        t = []
        for k in range(60):
            t0 = time.perf_counter()
            call()
            if k >= 10:
                t.append((time.perf_counter() - t0) * 1e6)
        res["export"][name] = dict(stats(np.array(t)), bytes_written_per_pixel=bpp, GBps=(3 + bpp) * px * N / float(np.median(t)) / 1e3)
        dst.close()
    d.close()
    busy_src.close()
    busy_dst.close()
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
