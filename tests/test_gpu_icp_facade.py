"""PoseDetection with "use icp" = 1 (tests/cpp/icp_facade.cpp): the reference's fixture benchmark/img0.png + depth0.png, the shipped
1950-template bank, the ICP branch of detect() (GPU refinement + estimateBestMatch), the Hodan error against pose0.yml, and the
frames estimateBestMatch rejects."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_pose_detection_use_icp_on_pose0(lm, frame0, tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    xyzn = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse_normals.npz"))["xyzn"]
    assert np.allclose(xyzn[:, :3], g["vertices"])
    bgr, depth = frame0
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(np.array([len(g["vertices"]), len(g["faces"])], np.uint32).tobytes())
        fh.write(g["vertices"].astype(np.float32).tobytes())
        fh.write(g["faces"].astype(np.int32).tobytes())
        fh.write(xyzn[:, 3:].astype(np.float32).tobytes())
    bgr.tofile(tmp_path / "bgr.raw")
    depth.tofile(tmp_path / "depth.raw")
    with open(tmp_path / "gt.txt", "w") as fh:
        fh.write(" ".join("%.17g" % v for v in list(g["gt_rotation"].reshape(-1)) + list(g["gt_position"])))
    exe = str(tmp_path / "icp_facade")
    libdir = os.path.dirname(lm.LIB_PATH)
    host = os.path.join(ROOT, "line-mod-pipeline_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "icp_facade.cpp"),
                           os.path.join(host, "HighLevelLinemod.cpp"), os.path.join(host, "PostProcess.cpp"),
                           os.path.join(host, "TemplateGenerator.cpp"), os.path.join(host, "PoseDetection.cpp"),
                           "-L" + libdir, "-llinemod_hip", "-lpthread", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, "mesh.bin", "bgr.raw", "depth.raw", "gt.txt"], cwd=tmp_path, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = [l for l in r.stdout.splitlines() if not l.startswith("ERROR")]
    print("\n".join(out))
    assert out[0] == "templates 1950"
    assert "detect error ''" in out
    assert "accepted 1" in out
    without_icp = [l for l in out if l.startswith("without icp:")][0].split()
    with_icp = [l for l in out if l.startswith("with icp:")][0].split()
    assert float(without_icp[3]) < 0.3, without_icp                                          # the template pose, as hodan_pose0.cpp
    # The refined pose is reported, not bounded: under the contract the full model, back faces included, is
    # registered to the visible surface and every level stops after two rounds, which moves this pose away from pose0.yml.
    assert 0.0 <= float(with_icp[3]) <= 1.0 and np.isfinite(float(with_icp[6])), with_icp
    assert [l for l in out if l.startswith("final pose mean")][0].endswith("accepted 1")
    assert [l for l in out if l.startswith("displaced 100 mm")][0].endswith("accepted 0")
    assert [l for l in out if l.startswith("part removed")][0].endswith("accepted 0")
    # the reference's rule on an empty mask: mean 0, pose 0 kept with mean 0 <= 35 (HighLevelLinemodIcp.cpp:121-129)
    assert [l for l in out if l.startswith("part zeroed")][0] == "part zeroed: mean 0.000 accepted 1"
    batch = [l for l in out if l.startswith("batch ")][0]
    assert batch.startswith("batch 0 'use icp is set"), batch
