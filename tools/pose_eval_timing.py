"""Timing of the pose-error evaluation: Hodan queries/s at 640x480 (batch 256), ADD-S microseconds per query at
step 1 and step 40 on the shipped mesh, and the numpy restatement's time beside them (tests/pose_error_reference.py; for the Hodan error
that is the counting alone, on renders made beforehand).  Prints one JSON line.
usage: python tools/pose_eval_timing.py [--repeat N]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_error_reference as R  # noqa: E402


def _best(fn, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    lm = importlib.import_module("line-mod-pipeline_amd")
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    depth = np.load(os.path.join(ROOT, "tests", "golden", "frame0.npz"))["depth"]
    W, H = 640, 480
    d = lm.Detector(color_only=True, width=W, height=H)
    d.set_render_mesh(0, g["vertices"], g["faces"])
    rng = np.random.default_rng(1)
    qg = R.mat3_to_quat(g["gt_rotation"])
    tg = np.asarray(g["gt_position"])
    P = R.projection()
    n = 256
    vg = [R.view_proj_mat4(P, R.view_mat(qg, tg))] * n
    ve = [R.view_proj_mat4(P, R.view_mat(qg, tg + rng.normal(0, 10, 3))) for _ in range(n)]
    d.pose_error_vsd(depth, 0, 0, vg, ve)                                   # warm-up (allocations, code objects)
    t_vsd = _best(lambda: d.pose_error_vsd(depth, 0, 0, vg, ve), a.repeat)
    _, dg = d.render(0, vg[0], W, H)
    _, de = d.render(0, ve[0], W, H)
    t_np_vsd = _best(lambda: R.vsd_counts(dg, de, depth), a.repeat)
    out = {"hodan_batch": n, "hodan_queries_per_s": n / t_vsd, "hodan_us_per_query": 1e6 * t_vsd / n,
           "numpy_hodan_counts_us_per_query": 1e6 * t_np_vsd}
    v = g["vertices"]
    eye = np.eye(3, dtype=np.float32)
    for step, nq in ((1, 16), (40, 256)):
        Re = np.stack([R.quat_to_mat3(q / np.linalg.norm(q)) for q in rng.normal(size=(nq, 4))])
        t = np.tile(tg.astype(np.float32), (nq, 1))
        d.pose_error_add(0, eye, t, Re, t, step=step, symmetric=True)
        ts = _best(lambda: d.pose_error_add(0, eye, t, Re, t, step=step, symmetric=True), a.repeat)
        m = len(v[::step])
        out["adds_step%d_vertices" % step] = m
        out["adds_step%d_batch" % step] = nq
        out["adds_step%d_us_per_query" % step] = 1e6 * ts / nq
        out["adds_step%d_pairs_per_s" % step] = m * m * nq / ts
        t_np = _best(lambda: R.adds_per_vertex(v, step, eye, t[0], Re[0], t[0]), 1 if step == 1 else a.repeat)
        out["numpy_adds_step%d_us_per_query" % step] = 1e6 * t_np
    d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
