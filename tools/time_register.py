"""What does registering raw depth on the GPU cost?  96 frames in ONE call into 640 x 480 slots, the colour image
1920 x 1080 BGRA, the window at (640, 300):
    registered   lm_ingest_frames_registered: 512 x 424 float depth (metres, scale 1000) in the depth camera's geometry, splat (2, 1)
    plain        lm_ingest_frames: a 1920 x 1082 float depth image that is registered already (what a host pass delivers today)
HIP events on a stream S of the tool's own, as tools/time_ingest_yuv.py takes them: copies that keep the GPU busy while the host enqueues,
event, ingest (it waits for S), lm_ingest_release(S), event -- the median of 50 runs after 10 warm-ups, the descriptor arrays built
beforehand.  Slot 0 of the registered leg is compared with tests/register_reference.py first.

    python tools/time_register.py [out.json]         -> profiles/register_times.json   (under a kernel trace: the kernels' shares)"""
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
RR = importlib.import_module("register_reference")
IR = importlib.import_module("ingest_reference")

W, H, N = 640, 480, 96
CW, CH, DW, DH = 1920, 1080, 512, 424
CROP = (640, 300)
SPLAT = (2, 1)
T.WARMUP, T.RUNS = 10, 50


def main():
    hip = T.Hip()
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    dc = RR.cam(DW, DH, 365.0, 365.0, 255.5, 211.5, (0.09, -0.27, 0.0, 0.0, 0.1))
    cc = RR.cam(CW, CH, 1060.0, 1060.0, 959.5, 539.5, (0.03, -0.05, 0.001, -0.001, 0.0))
    a = np.deg2rad(0.5)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    t = np.array([52.0, 0.5, -1.0], np.float32)
    d.set_registration(lm.camera(DW, DH, dc["fx"], dc["fy"], dc["cx"], dc["cy"], dc["dist"]),
                       lm.camera(CW, CH, cc["fx"], cc["fy"], cc["cx"], cc["cy"], cc["dist"]), R, t, splat=SPLAT)
    rng = np.random.default_rng(1)
    K = 8           # distinct images, taken in turns
    yy, xx = np.mgrid[0:DH, 0:DW]
    raws = []
    for k in range(K):
        z = (1.2 + 0.3 * np.sin(xx / 37.0 + k) * np.cos(yy / 29.0) + rng.uniform(-0.002, 0.002, (DH, DW))).astype(np.float32)
        z[150:300, 180 + 10 * k:330 + 10 * k] = np.float32(0.6)
        z[rng.random((DH, DW)) < 0.02] = 0.0
        raws.append(z)
    colour = [rng.integers(0, 256, (CH, CW, 4), dtype=np.uint8) for _ in range(2)]
    cbuf = lm.DeviceBuffer(2 * colour[0].nbytes)
    rbuf = lm.DeviceBuffer(K * raws[0].nbytes)
    pbuf = lm.DeviceBuffer(K * CW * (CH + 2) * 4)
    pre = [rng.uniform(0.5, 2.0, (CH + 2, CW)).astype(np.float32) for _ in range(K)]
    for k in range(2):
        cbuf.upload(colour[k], k * colour[0].nbytes)
    for k in range(K):
        rbuf.upload(raws[k], k * raws[0].nbytes)
        pbuf.upload(pre[k], k * pre[0].nbytes)
    cviews = [cbuf.view(np.uint8, (CH, CW, 4), offset=k * colour[0].nbytes) for k in range(2)]
    col, raw, dep, opts = (lm.ImageDesc * N)(), (lm.ImageDesc * N)(), (lm.ImageDesc * N)(), (lm.IngestOpts * N)()
    for i in range(N):
        col[i] = lm.image_desc(cviews[i % 2], crop=CROP)
        raw[i] = lm.image_desc(rbuf.view(np.float32, (DH, DW), offset=(i % K) * raws[0].nbytes), depth=True, crop=CROP, scale=1000.0)
        dep[i] = lm.image_desc(pbuf.view(np.float32, (CH + 2, CW), offset=(i % K) * pre[0].nbytes), depth=True, crop=CROP, scale=1000.0)

    def leg(call, depth):
        def fn():
            d._check(call(d.h, 0, N, col, depth, opts, hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        return fn

    def busy():        # (80 copies of 33 MB: well over a millisecond of GPU work, enqueued faster than it runs -- the call's host time hides behind it)
        for _ in range(80):
            hip.ok(hip.lib.hipMemcpyAsync(pbuf.ptr, C.c_void_p(pbuf.ptr.value + 4 * pre[0].nbytes), 4 * pre[0].nbytes, 3, hip.stream))

    registered, plain = leg(d.lib.lm_ingest_frames_registered, raw), leg(d.lib.lm_ingest_frames, dep)
    registered()
    exp = IR.depth(RR.register(raws[0], 1000.0, d.registration_rays(), cc, R, t, SPLAT), W, H, CROP)
    got = d.read_frame(0)
    assert np.array_equal(got[1], exp) and np.array_equal(got[0], colour[0][CROP[1]:CROP[1] + H, CROP[0]:CROP[0] + W, :3]), "slot 0 differs from the reference"
    res = {"frames": N, "runs": T.RUNS, "warmup": T.WARMUP, "version": d.lib.lm_version().decode().split(" (")[0],
           "holes_in_slot_0": int((exp == 0).sum()),
           "registered_512x424_f32": T.stats(hip.time_us(registered, busy)),
           "plain_1920x1082_f32_already_registered": T.stats(hip.time_us(plain, busy))}
    res["registered_again"] = T.stats(hip.time_us(registered, busy))
    hip.ok(hip.lib.hipStreamSynchronize(hip.stream))
    d.upload_wait(-1)
    d.close()
    for b in (cbuf, rbuf, pbuf):
        b.close()
    print(json.dumps(res, indent=1))
    out_path = next((a_ for a_ in sys.argv[1:] if a_.endswith(".json")), os.path.join(HERE, "profiles", "register_times.json"))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
