"""What does lm_ingest_frames cost?  96 frames of 640 x 480 RGB-D in ONE launch, against a device-to-device
hipMemcpyAsync of the same 96 x 1 536 000 bytes:
    (a) BGR8 + U16, 16-byte aligned, no geometry          (the kernel's fast path; 10 bytes per pixel moved, 295 MB per launch)
    (b) the Kinect shape at full size: BGRA 1920 x 1080 + F32 1920 x 1082, window at (640, 301), mirrored, shifted by (3, -2)
    (c) (a) with the colour source misaligned by one byte (the depth source by one element)
and the effect on a lane-step (96 frames, 3000 templates) when the ingest of step k + 1 runs beside the match of step k.
HIP events on a stream S of the tool's own: ten copies that keep the GPU busy while the host enqueues, event, ingest (it waits for S),
lm_ingest_release(S), event -- the median of 60 runs after 10 warm-ups, in one process, the descriptor arrays built beforehand.  The events come from the HIP runtime the library has mapped (no second runtime).
Writes profiles/ingest_times.json (or the path given as the first argument)."""
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
synth = importlib.import_module("line-mod-pipeline_amd.synth")

W, H, N = 640, 480, 96
WARMUP, RUNS = 10, 60


class Hip:
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
        """fn() enqueues work that stream S ends up waiting for; the median (and minimum) over RUNS of the event time around it.  busy()
        first enqueues a few hundred microseconds of other work on S, so that the host has finished enqueuing fn's work before the GPU
        reaches the first event: the events then bracket GPU time alone.  Also the median host time of fn() itself."""
        t, host = [], []
        for k in range(WARMUP + RUNS):
            busy()
            self.ok(self.lib.hipEventRecord(self.e0, self.stream))
            h0 = time.perf_counter()
            fn()
            h1 = time.perf_counter()
            self.ok(self.lib.hipEventRecord(self.e1, self.stream))
            self.ok(self.lib.hipEventSynchronize(self.e1))
            ms = C.c_float()
            self.ok(self.lib.hipEventElapsedTime(C.byref(ms), self.e0, self.e1))
            if k >= WARMUP:
                t.append(ms.value * 1e3)
                host.append((h1 - h0) * 1e6)
        return float(np.median(t)), float(np.min(t)), float(np.median(host))


def replicate(buf, one, n):
    """n copies of the byte block `one` (host) in the DeviceBuffer: one upload, then device-to-device doubling."""
    nb = one.nbytes
    buf.upload(one)
    have = 1
    while have < n:
        k = min(have, n - have)
        rc = buf.lib.lm_device_copy(C.c_void_p(buf.ptr.value + have * nb), buf.ptr, k * nb, 2)
        if rc:
            raise RuntimeError(buf.lib.lm_last_error().decode())
        have += k


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ingest_times.json")
    hip = Hip()
    S = hip.stream.value
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=2 * N)
    rng = np.random.default_rng(5)
    res = {"frames": N, "width": W, "height": H, "runs": RUNS, "warmup": WARMUP, "bytes_written_per_launch": N * W * H * 5}

    # (a) and (c): [colour | depth] per frame, one byte (colour) / one element (depth) of slack in front for (c)
    frames = [synth.make_frame(W, H, seed=500 + i) for i in range(8)]
    fb = W * H * 5
    src = lm.DeviceBuffer(N * fb + 64)
    dst = lm.DeviceBuffer(N * fb)
    for i in range(N):
        b, z = frames[i % 8]
        src.upload(b, 16 + i * fb)
        src.upload(z, 16 + i * fb + W * H * 3)

    def plain(shift):
        return [dict(colour=src.view(np.uint8, (H, W, 3), offset=16 + i * fb + shift),
                     depth=src.view(np.uint16, (H, W), offset=16 + i * fb + W * H * 3 + 2 * shift)) for i in range(N)]

    def prepared(frames_):
        """The descriptor arrays of a call, built once: the timed region is the library's call, not the binding's Python."""
        col, dep, opts = (lm.ImageDesc * N)(), (lm.ImageDesc * N)(), (lm.IngestOpts * N)()
        for k, f in enumerate(frames_):
            col[k] = lm.image_desc(f["colour"], crop=f.get("crop", (0, 0)))
            dep[k] = lm.image_desc(f["depth"], depth=True, crop=f.get("crop", (0, 0)))
            sh = f.get("shift", (0, 0))
            opts[k].flip_x, opts[k].shift_x, opts[k].shift_y = int(f.get("flip_x", False)), sh[0], sh[1]
        return col, dep, opts

    def ingest(arrs, first=0, stream=hip.stream):
        def fn():
            d._check(d.lib.lm_ingest_frames(d.h, first, N, arrs[0], arrs[1], arrs[2], stream))
            if stream is not None:
                d._check(d.lib.lm_ingest_release(d.h, first, N, stream))
        return fn

    def copy():
        hip.ok(hip.lib.hipMemcpyAsync(dst.ptr, C.c_void_p(src.ptr.value + 16), N * fb, 3, hip.stream))

    def busy():
        for _ in range(10):
            copy()

    a_arrs, c_arrs = prepared(plain(0)), prepared(plain(1))
    res["a_bgr8_u16_aligned_us"], res["a_min_us"], res["a_host_call_us"] = hip.time_us(ingest(a_arrs), busy)
    got = d.read_frame(N - 1)
    assert np.array_equal(got[0], frames[(N - 1) % 8][0]) and np.array_equal(got[1], frames[(N - 1) % 8][1])
    res["copy_d2d_us"], res["copy_min_us"], _ = hip.time_us(copy, busy)
    res["c_misaligned_by_one_us"], res["c_min_us"], _ = hip.time_us(ingest(c_arrs), busy)
    res["ratio_a_over_copy"] = res["a_bgr8_u16_aligned_us"] / res["copy_d2d_us"]
    res["a_GBps"] = 2 * N * fb / res["a_bgr8_u16_aligned_us"] / 1e3

    # (b) the Kinect shape at full size
    kb, kd = 1920 * 1080 * 4, 1920 * 1082 * 4
    bgra = rng.integers(0, 256, (1080, 1920, 4), dtype=np.uint8)
    depthf = rng.uniform(400.0, 4500.0, (1082, 1920)).astype(np.float32)
    depthf[rng.random(depthf.shape) < 0.1] = np.inf
    kc, kz = lm.DeviceBuffer(N * kb), lm.DeviceBuffer(N * kd)
    replicate(kc, bgra, N)
    replicate(kz, depthf, N)
    k_frames = [dict(colour=kc.view(np.uint8, (1080, 1920, 4), offset=i * kb), depth=kz.view(np.float32, (1082, 1920), offset=i * kd),
                     crop=(640, 301), flip_x=True, shift=(3, -2)) for i in range(N)]
    res["b_kinect_bgra_f32_us"], res["b_min_us"], _ = hip.time_us(ingest(prepared(k_frames)), busy)
    res["b_bytes_read_per_launch"] = N * W * H * 8
    kc.close()
    kz.close()

    # the lane-step: 96 frames against 3000 templates on lane 0, slots [0, 96) and [96, 192) taking turns
    descs, feats, _ = synth.make_bank(3000, 2, 2, seed=4321, fixed_l0_size=(96, 96), frame_size=(W, H), T0=d.get_T(0))
    d.add_class("c", descs, feats)
    beside_fn = [ingest(a_arrs, first=r * N, stream=None) for r in range(2)]
    beside_fn[0]()
    beside_fn[1]()
    d.upload_wait(-1)

    out, counts = np.zeros((N, 4096), lm.MATCH_DTYPE), np.zeros(N, np.int32)

    def steps(beside, n=14):
        t = []
        d.match_begin(0, 0, N, 80.0, 0)
        for k in range(1, n + 1):
            r = k & 1
            t0 = time.perf_counter()
            if beside:
                beside_fn[r]()                         # step k's frames, while step k - 1 computes
            d.match_end(0, out=out, counts=counts, n_slots=N)
            d.match_begin(0, r * N, N, 80.0, 0)
            t.append((time.perf_counter() - t0) * 1e6)
        d.match_end(0, out=out, counts=counts, n_slots=N)
        return float(np.median(t[2:]))

    steps(False, 4)
    res["lane_step_resident_us"] = steps(False)
    res["lane_step_ingest_beside_us"] = steps(True)
    res["lane_step_resident_again_us"] = steps(False)
    d.upload_wait(-1)
    hip.ok(hip.lib.hipStreamSynchronize(hip.stream))
    d.close()
    src.close()
    dst.close()
    print(json.dumps(res, indent=1))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
