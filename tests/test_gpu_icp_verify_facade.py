"""The facade's best-pose check on the GPU against the host's (tests/cpp/icp_verify_facade.cpp): HighLevelLinemodIcp's
meanDepthDifferencesGpu / estimateBestMatchGpu against meanDepthDifference / estimateBestMatch with SoftRender on frame0 -- the means
equal to the last bit, the verdicts and best indices equal, and the frames the check must reject."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(lm, tmp_path):
    exe = str(tmp_path / "icp_verify_facade")
    libdir = os.path.dirname(lm.LIB_PATH)
    host = os.path.join(ROOT, "line-mod-pipeline_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "icp_verify_facade.cpp"),
                           os.path.join(host, "HighLevelLinemod.cpp"), os.path.join(host, "PostProcess.cpp"),
                           os.path.join(host, "TemplateGenerator.cpp"), "-L" + libdir, "-llinemod_hip", "-lpthread",
                           "-Wl,-rpath," + libdir])
    return exe


def write_inputs(depth, tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    xyzn = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse_normals.npz"))["xyzn"]
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(np.array([len(g["vertices"]), len(g["faces"])], np.uint32).tobytes())
        fh.write(g["vertices"].astype(np.float32).tobytes())
        fh.write(g["faces"].astype(np.int32).tobytes())
        fh.write(xyzn[:, 3:].astype(np.float32).tobytes())
    depth.tofile(tmp_path / "depth.raw")
    with open(tmp_path / "gt.txt", "w") as fh:
        fh.write(" ".join("%.17g" % v for v in list(g["gt_rotation"].reshape(-1)) + list(g["gt_position"])))


@pytest.mark.gpu
def test_gpu_check_equals_the_host_check_on_frame0(lm, frame0, tmp_path):
    _, depth = frame0
    write_inputs(depth, tmp_path)
    exe = build_driver(lm, tmp_path)
    r = subprocess.run([exe, "mesh.bin", "depth.raw", "gt.txt"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = [l for l in r.stdout.splitlines() if not l.startswith("ERROR")]
    print("\n".join(out))
    means, verdicts = {}, {}
    for l in out:
        m = re.match(r"(.+) pose (\d+): host (\S+) gpu (\S+)$", l)
        if m:
            assert m.group(3) == m.group(4), l                   # %.17g of both: the same double
            means.setdefault(m.group(1), []).append(float(m.group(4)))
        m = re.match(r"(.+) verdict: host (\d) best (\d+) gpu (\d) best (\d+) error '(.*)'$", l)
        if m:
            assert m.group(2, 3) == m.group(4, 5), l
            assert m.group(6) == "", l
            verdicts[m.group(1)] = (int(m.group(4)), int(m.group(5)))
    assert [len(means[k]) for k in ("gt", "displaced 100 mm", "part removed", "part zeroed", "group")] == [1, 1, 1, 1, 5]
    assert set(verdicts) == {"gt", "displaced 100 mm", "part removed", "part zeroed", "group", "empty group"}
    assert means["gt"][0] > 0
    assert verdicts["displaced 100 mm"][0] == 0 and means["displaced 100 mm"][0] > 35
    assert verdicts["part removed"][0] == 0 and means["part removed"][0] == 150.0
    # the reference's rule on an empty mask: mean 0, pose 0 kept with mean 0 <= 35 (HighLevelLinemodIcp.cpp:121-129)
    assert means["part zeroed"] == [0.0] and verdicts["part zeroed"] == (1, 0)
    assert verdicts["empty group"] == (0, 65535)
    assert len(set(means["group"])) == 5                         # five different renders
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import icp_verify_reference as V
    ok, best = V.select_best(means["group"])
    assert verdicts["group"] == (1 if ok else 0, best if ok else 65535)
    no_mesh = [l for l in out if l.startswith("no mesh:")][0]
    assert no_mesh.startswith("no mesh: 0 '") and len(no_mesh) > len("no mesh: 0 ''"), no_mesh
