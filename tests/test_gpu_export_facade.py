"""PoseDetection::exportResults (host/Draw.h) through one C++ driver (tests/cpp/export_facade.cpp): detectBatchSlots on
two frames ingested from device memory with the principal-point shift in the ingest's opts, then exportResults -- the axes and the
bounding box of every final pose drawn on the GPU, the shift undone, dense BGR8 into device memory.  The exported bytes equal the numpy
reference (tests/export_reference.py) fed with the same poses: the driver prints them with %.9g (exact for a float), the Python builders
draw_axes / draw_box make the primitives from them."""
import os
import subprocess

import numpy as np
import pytest

import export_reference as ER
import keep_depth_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_export_results_equal_the_reference(lm, frame0, tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    bgr, depth = frame0
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(np.array([len(g["vertices"]), len(g["faces"])], np.uint32).tobytes())
        fh.write(g["vertices"].astype(np.float32).tobytes())
        fh.write(g["faces"].astype(np.int32).tobytes())
    bgr.tofile(tmp_path / "bgr.raw")
    depth.tofile(tmp_path / "depth.raw")
    host = os.path.join(ROOT, "line-mod-pipeline_amd", "host")
    libdir = os.path.dirname(lm.LIB_PATH)
    exe = str(tmp_path / "export_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "export_facade.cpp"),
                           os.path.join(host, "HighLevelLinemod.cpp"), os.path.join(host, "PoseDetection.cpp"),
                           os.path.join(host, "PostProcess.cpp"), os.path.join(host, "TemplateGenerator.cpp"),
                           "-L" + libdir, "-llinemod_hip", "-lpthread", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, "mesh.bin", "bgr.raw", "depth.raw", "55", "50", "export.raw"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert "run pd_slots 1 ''" in lines and "run export 1 ''" in lines, r.stdout[-3000:]
    cam = [l.split() for l in lines if l.startswith("camera ")][0]
    f32 = lambda s: float(np.float32(s))           # (%.9g names one float; the facade computes in double FROM that float)
    fx, fy, W, H, ox, oy = f32(cam[1]), f32(cam[2]), int(cam[3]), int(cam[4]), int(cam[6]), int(cam[7])
    assert (W, H, ox, oy) == (640, 480, -12, 10)
    prims, per_frame = [], [0, 0]
    for l in lines:
        if not l.startswith("final "):
            continue
        v = l.split()
        frame = int(v[1])
        t = [f32(x) for x in v[4:7]]
        R = np.array([f32(x) for x in v[8:17]]).reshape(3, 3)
        bb = [int(x) for x in v[18:22]]
        prims += [lm.draw_axes(R, t, fx, fy, W, H, 75.0, frame), lm.draw_box(bb, (0, 255, 255), 1, frame)]
        per_frame[frame] += 1
    assert per_frame[0] > 0, r.stdout[-3000:]
    prims = np.concatenate(prims)
    assert "prims %d" % len(prims) in lines
    assert (prims["kind"] == lm.DRAW_SEGMENT).sum() == 3 * sum(per_frame)           # every axis of every pose lies in front of the camera
    got = np.fromfile(tmp_path / "export.raw", np.uint8).reshape(2, H, W, 3)
    F = S.shifted(bgr, ox, oy)                  # the frame as it lies in both slots: the colour image is the same, the depth differs
    for i in range(2):
        A = ER.annotate(F, prims, i)
        assert (A != F).any() == (per_frame[i] > 0)
        want = ER.undo(A, False, (ox, oy))
        assert np.array_equal(got[i], want), "frame %d: %d bytes differ" % (i, int((got[i] != want).sum()))
        # where the shift kept the picture and nothing is drawn, the export is the camera's image again
        v, u = np.mgrid[0:H, 0:W]
        kept = (u + ox >= 0) & (u + ox < W) & (v + oy >= 0) & (v + oy < H) & (ER.undo((A == F).all(axis=2).astype(np.uint8), False, (ox, oy)) == 1)
        assert np.array_equal(got[i][kept], bgr[kept]) and kept.mean() > 0.9
    refusal = [l for l in lines if l.startswith("refused gray ")]
    assert refusal == ["refused gray 1 'destination image of frame 0: LM_PIX_GRAY8 is a source format: not served as a destination'"], refusal
