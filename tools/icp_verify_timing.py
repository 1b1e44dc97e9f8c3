"""Timing of the ICP branch's best-pose check: the host's meanDepthDifference per pose (tests/cpp/icp_verify_facade.cpp
with its timing flag) beside lm_stage_icp_verify_host and lm_icp_verify per pose at batch 1, 8 and 64, on frame0 at 640 x 480 with the
shipped mesh: the median of --repeat timed calls after warm-up.  Writes profiles/icp_verify_timing.json (or --out) and prints it.
usage: python tools/icp_verify_timing.py [--repeat N] [--out PATH] [--gpu-only]     (--gpu-only: for a kernel trace of the GPU calls alone)"""
import argparse
import ctypes as C
import importlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_error_reference as R  # noqa: E402


def _median_ms(fn, repeat, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def _host_ms(lm, depth, repeat):
    import pathlib
    import test_gpu_icp_verify_facade as T
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        T.write_inputs(depth, tmp)
        exe = T.build_driver(lm, tmp)
        out = subprocess.run([exe, "mesh.bin", "depth.raw", "gt.txt", "time", str(repeat)], cwd=tmp, capture_output=True, text=True, check=True).stdout
    return float(re.search(r"median ms (\S+)", out).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_verify_timing.json"))
    ap.add_argument("--gpu-only", action="store_true")
    a = ap.parse_args()
    lm = importlib.import_module("line-mod-pipeline_amd")
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    f0 = np.load(os.path.join(ROOT, "tests", "golden", "frame0.npz"))
    bgr, depth = f0["bgr"], np.ascontiguousarray(f0["depth"])
    W, H = 640, 480
    d = lm.Detector(color_only=False, width=W, height=H)
    d.set_render_mesh(0, g["vertices"], g["faces"])
    d.upload_frame(0, bgr, depth)
    rng = np.random.default_rng(1)
    qg = R.mat3_to_quat(g["gt_rotation"])
    tg = np.asarray(g["gt_position"])
    P = R.projection()
    out = {"width": W, "height": H, "vertices": int(len(g["vertices"])), "repeat": a.repeat}
    for n in (1, 8, 64):
        q = (lm.IcpVerifyQuery * n)()
        for k in range(n):
            q[k].frame, q[k].mesh_idx = 0, 0
            q[k].view_proj[:] = [float(v) for v in R.view_proj_mat4(P, R.view_mat(qg, tg + (rng.normal(0, 5, 3) if k else 0)))]
        res = np.zeros(n, lm.ICP_VERIFY_RESULT_DTYPE)
        rp, dp = res.ctypes.data_as(C.c_void_p), depth.ctypes.data_as(C.c_void_p)

        def host_form():
            d._check(d.lib.lm_stage_icp_verify_host(d.h, dp, 1, W, H, q, n, 600, rp))

        def slot_form():
            d._check(d.lib.lm_icp_verify(d.h, q, n, 600, rp))
        ms = _median_ms(host_form, a.repeat)
        first = res.copy()
        out["verify_host_batch%d_ms_per_call" % n] = ms
        out["verify_host_batch%d_ms_per_pose" % n] = ms / n
        ms = _median_ms(slot_form, a.repeat)
        assert res.tobytes() == first.tobytes()
        out["verify_slot_batch%d_ms_per_call" % n] = ms
        out["verify_slot_batch%d_ms_per_pose" % n] = ms / n
        if n == 1:
            out["gt_pose_count"], out["gt_pose_mean"] = int(res[0]["count"]), float(res[0]["mean"])
    d.close()
    if not a.gpu_only:
        out["host_meanDepthDifference_ms_per_pose"] = _host_ms(lm, depth, a.repeat)
        for n in (1, 8, 64):
            out["host_over_gpu_per_pose_batch%d" % n] = out["host_meanDepthDifference_ms_per_pose"] / out["verify_host_batch%d_ms_per_pose" % n]
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
