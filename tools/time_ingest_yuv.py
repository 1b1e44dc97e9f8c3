"""What do the grey and YUV source formats of lm_ingest_frames cost?  96 frames of 640 x 480 RGB-D in ONE call, all
sources 16-byte aligned and without geometry (the kernels' fast path), the depth image LM_PIX_DEPTH_U16:
    (a)     BGR8          k_ingest, case (a) of tools/time_ingest.py: 3 source bytes per colour pixel
    nv12    NV12          k_ingest_yuv: 1.5 source bytes per colour pixel
    yuy2    YUY2          k_ingest_yuv: 2 source bytes
    gray    GRAY8         k_ingest_yuv: 1 source byte
    nv12_odd              NV12 with the window one column and one row into the source (the general path, 9 chroma pairs per lane)
    mixed                 BGR8 and NV12 frames taking turns in one call: both kernels launched, each leaving half the frames at once
and, for the host-fed pipeline whose camera delivers NV12: 96 pinned NV12 frames copied to a device buffer and ingested, against
lm_upload_frames_pinned of the same frames as BGR8 + U16 (host clock around the call and lm_upload_wait).
HIP events on a stream S of the tool's own, as tools/time_ingest.py takes them: ten copies that keep the GPU busy while the host
enqueues, event, ingest (it waits for S), lm_ingest_release(S), event -- the median of 60 runs after 10 warm-ups, the descriptor arrays
built beforehand.  Every case's slots are compared with tests/ingest_yuv_reference.py before it is timed.

    python tools/time_ingest_yuv.py [out.json]            all cases -> profiles/ingest_yuv_times.json
    python tools/time_ingest_yuv.py --only-a [--root DIR] case (a) alone, with nothing the 0.11 ABI lacks, as one JSON line on stdout; DIR:
                                                          another checkout whose built package is measured instead of this one -- to
                                                          compare two builds in one session, taking turns"""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONLY_A = "--only-a" in sys.argv
ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv else HERE
sys.path.insert(0, ROOT)
lm = importlib.import_module("line-mod-pipeline_amd")
synth = importlib.import_module("line-mod-pipeline_amd.synth")

W, H, N = 640, 480, 96
WARMUP, RUNS = 10, 60


class Hip:
    """The HIP runtime the library has mapped (no second runtime): a stream and two events."""

    def __init__(self):
        lm.load_library()
        path = None
        for line in open("/proc/self/maps"):
            p = line.split(None, 5)[-1].strip() if "/" in line else ""
            if os.path.basename(p).startswith("libamdhip64.so"):
                path = p
                break
        self.lib = lib = C.CDLL(path, mode=os.RTLD_NOLOAD | os.RTLD_NOW)
        vp = C.c_void_p
        lib.hipStreamCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
        lib.hipEventCreate.argtypes = [C.POINTER(vp)]
        lib.hipEventRecord.argtypes = [vp, vp]
        lib.hipEventSynchronize.argtypes = [vp]
        lib.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
        lib.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
        lib.hipStreamSynchronize.argtypes = [vp]
        s, e0, e1 = vp(), vp(), vp()
        self.ok(lib.hipStreamCreateWithFlags(C.byref(s), 1))
        self.ok(lib.hipEventCreate(C.byref(e0)))
        self.ok(lib.hipEventCreate(C.byref(e1)))
        self.stream, self.e0, self.e1 = s, e0, e1

    @staticmethod
    def ok(rc):
        if rc:
            raise RuntimeError("hipError %d" % rc)

    def time_us(self, fn, busy):
        """fn() enqueues work that stream S ends up waiting for: the event times around it over RUNS runs, in microseconds.  busy() first
        enqueues a few hundred microseconds of other work on S, so that the host has finished enqueuing fn's work before the GPU reaches
        the first event: the events then bracket GPU time alone."""
        t = []
        for k in range(WARMUP + RUNS):
            busy()
            self.ok(self.lib.hipEventRecord(self.e0, self.stream))
            fn()
            self.ok(self.lib.hipEventRecord(self.e1, self.stream))
            self.ok(self.lib.hipEventSynchronize(self.e1))
            ms = C.c_float()
            self.ok(self.lib.hipEventElapsedTime(C.byref(ms), self.e0, self.e1))
            if k >= WARMUP:
                t.append(ms.value * 1e3)
        return np.array(t)


def stats(t):
    return {"median_us": float(np.median(t)), "mean_us": float(np.mean(t)), "min_us": float(np.min(t)), "p10_us": float(np.percentile(t, 10)),
            "p90_us": float(np.percentile(t, 90))}


def bgr_to_yuv(bgr):
    """A camera's side: BT.601 limited range in float, full-resolution Y, U, V planes (uint8)."""
    b, g, r = (bgr[:, :, k].astype(np.float64) for k in range(3))
    q = lambda c: np.clip(np.rint(c), 0, 255).astype(np.uint8)
    return (q(16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255), q(128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255),
            q(128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255))


def main():
    hip = Hip()
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=N)
    frames = [synth.make_frame(W, H, seed=500 + i) for i in range(8)]
    px = W * H
    res = {"frames": N, "width": W, "height": H, "runs": RUNS, "warmup": WARMUP, "version": d.lib.lm_version().decode().split(" (")[0]}

    # the depth images and the BGR8 sources of case (a): [colour | depth] per frame, as tools/time_ingest.py lays them out
    fb = px * 5
    src = lm.DeviceBuffer(N * fb + 64)
    dst = lm.DeviceBuffer(N * fb)
    for i in range(N):
        b, z = frames[i % 8]
        src.upload(b, 16 + i * fb)
        src.upload(z, 16 + i * fb + px * 3)
    depth_view = [src.view(np.uint16, (H, W), offset=16 + i * fb + px * 3) for i in range(N)]
    bgr_frames = [dict(colour=src.view(np.uint8, (H, W, 3), offset=16 + i * fb), depth=depth_view[i]) for i in range(N)]

    def prepared(frames_):
        """The descriptor arrays of a call, built once: the timed region is the library's call, not the binding's Python."""
        col, dep, opts = (lm.ImageDesc * N)(), (lm.ImageDesc * N)(), (lm.IngestOpts * N)()
        for k, f in enumerate(frames_):
            kw = {n: f[n] for n in ("layout", "matrix", "range") if n in f}
            col[k] = lm.image_desc(f["colour"], crop=f.get("crop", (0, 0)), **kw)
            dep[k] = lm.image_desc(f["depth"], depth=True, crop=f.get("crop", (0, 0)))
        return col, dep, opts

    def ingest(arrs):
        def fn():
            d._check(d.lib.lm_ingest_frames(d.h, 0, N, arrs[0], arrs[1], arrs[2], hip.stream))
            d._check(d.lib.lm_ingest_release(d.h, 0, N, hip.stream))
        return fn

    def busy():
        for _ in range(10):
            hip.ok(hip.lib.hipMemcpyAsync(dst.ptr, C.c_void_p(src.ptr.value + 16), N * fb, 3, hip.stream))

    def measure(frames_, expect):
        """expect(i) -> the BGR frame slot i must hold: checked for the first and the last slots, then the timing."""
        fn = ingest(prepared(frames_))
        fn()
        for i in (0, 1, N - 1):
            got = d.read_frame(i)
            assert np.array_equal(got[0], expect(i)) and np.array_equal(got[1], frames[i % 8][1]), "slot %d differs from the reference" % i
        return hip.time_us(fn, busy)

    a = measure(bgr_frames, lambda i: frames[i % 8][0])
    res["a_bgr8_u16"] = dict(stats(a), source_bytes_per_pixel=5, GBps=(5 + 5) * px * N / float(np.median(a)) / 1e3)
    if ONLY_A:
        print(json.dumps(dict(res["a_bgr8_u16"], version=res["version"], root=ROOT)))
        d.close()
        src.close()
        dst.close()
        return

    sys.path.insert(0, os.path.join(HERE, "tests"))
    YR = importlib.import_module("ingest_yuv_reference")
    IR = importlib.import_module("ingest_reference")
    out_path = next((a_ for a_ in sys.argv[1:] if a_.endswith(".json")), os.path.join(HERE, "profiles", "ingest_yuv_times.json"))
    yuv = [bgr_to_yuv(b) for b, _ in frames]
    sub2 = lambda c: c[0::2, 0::2]
    packed = {"nv12": [YR.pack_nv(y, sub2(u), sub2(v), "nv12") for y, u, v in yuv],
              "yuy2": [YR.pack_422(y, u[:, 0::2], v[:, 0::2], "yuy2") for y, u, v in yuv],
              "gray": [y for y, _, _ in yuv]}
    bytes_per_frame = {"nv12": px * 3 // 2, "yuy2": px * 2, "gray": px}
    shape = {"nv12": (H * 3 // 2, W), "yuy2": (H, W, 2), "gray": (H, W)}
    ref = {fmt: [YR.yuv_to_bgr(p, fmt) for p in packed[fmt]] for fmt in packed}
    bufs = {}
    for fmt, nb in bytes_per_frame.items():
        bufs[fmt] = buf = lm.DeviceBuffer(N * nb)
        for i in range(N):
            p = packed[fmt][i % 8]
            buf.upload(np.concatenate([q.reshape(-1) for q in p]) if isinstance(p, tuple) else p, i * nb)

    def yuv_frames(fmt, **kw):
        return [dict(colour=bufs[fmt].view(np.uint8, shape[fmt], offset=i * bytes_per_frame[fmt]), depth=depth_view[i], layout=fmt, **kw) for i in range(N)]

    for fmt in ("nv12", "yuy2", "gray"):
        t = measure(yuv_frames(fmt), lambda i, fmt=fmt: ref[fmt][i % 8])
        spp = bytes_per_frame[fmt] / px + 2
        res["%s_u16" % fmt] = dict(stats(t), source_bytes_per_pixel=spp, GBps=(spp + 5) * px * N / float(np.median(t)) / 1e3,
                                   ratio_to_a=float(np.median(t) / np.median(a)))
    # (a) again, behind the others: the spread of the same case within the session
    a2 = measure(bgr_frames, lambda i: frames[i % 8][0])
    res["a_bgr8_u16_again"] = stats(a2)
    # the general path: an NV12 source one column wider and two rows higher than the window would need, the window at (1, 1)
    big = lm.DeviceBuffer(N * (W + 16) * (H + 2) * 3 // 2)
    bw, bh = W + 16, H + 2
    ref_odd = []
    for i in range(8):
        y, u, v = yuv[i]
        Y = np.zeros((bh, bw), np.uint8)
        Y[1:H + 1, 1:W + 1] = y
        U, V = np.full((bh // 2, bw // 2), 128, np.uint8), np.full((bh // 2, bw // 2), 128, np.uint8)
        U[:H // 2, :W // 2], V[:H // 2, :W // 2] = sub2(u), sub2(v)
        p = YR.pack_nv(Y, U, V, "nv12")
        ref_odd.append(IR.colour(YR.yuv_to_bgr(p, "nv12"), W, H, crop=(1, 1)))
        for k in range(i, N, 8):
            big.upload(np.concatenate([q.reshape(-1) for q in p]), k * bw * bh * 3 // 2)
    odd_frames = [dict(colour=big.view(np.uint8, (bh * 3 // 2, bw), offset=i * bw * bh * 3 // 2), depth=depth_view[i], layout="nv12", crop=(1, 1))
                  for i in range(N)]
    # (the depth image keeps crop (0, 0): prepared() gives both images the frame's crop, so the depth descriptors are set apart here)
    arrs = prepared(odd_frames)
    for k in range(N):
        arrs[1][k] = lm.image_desc(depth_view[k], depth=True)
    fn = ingest(arrs)
    fn()
    got = d.read_frame(N - 1)
    assert np.array_equal(got[0], ref_odd[(N - 1) % 8]) and np.array_equal(got[1], frames[(N - 1) % 8][1])
    res["nv12_odd_window_u16"] = dict(stats(hip.time_us(fn, busy)))
    # both kernels in one call
    nv = yuv_frames("nv12")
    mixed = [bgr_frames[i] if i % 2 else nv[i] for i in range(N)]
    t = measure(mixed, lambda i: frames[i % 8][0] if i % 2 else ref["nv12"][i % 8])
    res["mixed_bgr8_nv12_u16"] = dict(stats(t), ratio_to_a=float(np.median(t) / np.median(a)))

    # the host-fed leg: pinned NV12 + U16 frames -> device buffer -> ingest, against lm_upload_frames_pinned of BGR8 + U16
    nvb = bytes_per_frame["nv12"]
    pin_nv, pin_bgr = lm.PinnedBuffer(N * (nvb + px * 2)), lm.PinnedBuffer(N * fb)
    for i in range(N):
        y, uv = packed["nv12"][i % 8]
        pin_nv.view(np.uint8, (nvb,), offset=i * (nvb + px * 2))[...] = np.concatenate([y.reshape(-1), uv.reshape(-1)])
        pin_nv.view(np.uint16, (H, W), offset=i * (nvb + px * 2) + nvb)[...] = frames[i % 8][1]
        pin_bgr.view(np.uint8, (H, W, 3), offset=i * fb)[...] = ref["nv12"][i % 8]
        pin_bgr.view(np.uint16, (H, W), offset=i * fb + px * 3)[...] = frames[i % 8][1]
    stage = lm.DeviceBuffer(N * (nvb + px * 2))
    host_arrs = prepared([dict(colour=stage.view(np.uint8, shape["nv12"], offset=i * (nvb + px * 2)),
                               depth=stage.view(np.uint16, (H, W), offset=i * (nvb + px * 2) + nvb), layout="nv12") for i in range(N)])

    def host_clock(fn):
        t = []
        for k in range(3 + 15):
            t0 = time.perf_counter()
            fn()
            d.upload_wait(-1)
            if k >= 3:
                t.append((time.perf_counter() - t0) * 1e6)
        return np.array(t)

    def nv12_leg():
        hip.ok(hip.lib.hipMemcpyAsync(stage.ptr, pin_nv.ptr, N * (nvb + px * 2), 1, hip.stream))
        d._check(d.lib.lm_ingest_frames(d.h, 0, N, host_arrs[0], host_arrs[1], host_arrs[2], hip.stream))

    def bgr_leg():
        d.upload_frames_pinned(0, N, pin_bgr.ptr.value)

    t_nv = host_clock(nv12_leg)
    got_nv = d.read_frame(N - 1)
    t_bgr = host_clock(bgr_leg)
    got_bgr = d.read_frame(N - 1)
    assert np.array_equal(got_nv[0], got_bgr[0]) and np.array_equal(got_nv[1], got_bgr[1])
    res["host_fed_nv12_copy_and_ingest"] = dict(stats(t_nv), bytes_over_the_link=N * (nvb + px * 2))
    res["host_fed_bgr8_upload_frames_pinned"] = dict(stats(t_bgr), bytes_over_the_link=N * fb)

    hip.ok(hip.lib.hipStreamSynchronize(hip.stream))
    d.close()
    for b in [src, dst, big, stage, pin_nv, pin_bgr] + list(bufs.values()):
        b.close()
    print(json.dumps(res, indent=1))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
