""""use icp" in PoseDetection's batch, stream and slot forms (tests/cpp/icp_batch_facade.cpp): on the golden frame, a
copy moved along the optical axis and a copy with the part pushed 150 mm back, with an off-centre principal point, the sorted depth
statistic and templates made on the GPU, the final poses of detect() frame by frame, of the class-list detectBatch, of two batches in
flight through Begin / End and of detectBatchSlots on the frames ingested from device memory are equal as printed with %.9g; over the
batch at least one group is accepted and at least one rejected; the refusals say why, and the single-class detectBatch still refuses."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def output(lm, frame0, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("icp_batch_facade")
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    xyzn = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse_normals.npz"))["xyzn"]
    bgr, depth = frame0
    with open(tmp / "mesh.bin", "wb") as fh:
        fh.write(np.array([len(g["vertices"]), len(g["faces"])], np.uint32).tobytes())
        fh.write(g["vertices"].astype(np.float32).tobytes())
        fh.write(g["faces"].astype(np.int32).tobytes())
        fh.write(xyzn[:, 3:].astype(np.float32).tobytes())
    bgr.tofile(tmp / "bgr.raw")
    depth.tofile(tmp / "depth.raw")
    host = os.path.join(ROOT, "line-mod-pipeline_amd", "host")
    libdir = os.path.dirname(lm.LIB_PATH)
    exe = str(tmp / "icp_batch_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "icp_batch_facade.cpp"),
                           os.path.join(host, "HighLevelLinemod.cpp"), os.path.join(host, "PoseDetection.cpp"),
                           os.path.join(host, "PostProcess.cpp"), os.path.join(host, "TemplateGenerator.cpp"),
                           "-L" + libdir, "-llinemod_hip", "-lpthread", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, "mesh.bin", "bgr.raw", "depth.raw", "55", "50"], cwd=tmp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    print(r.stdout)
    lines = r.stdout.splitlines()
    finals = {}
    for line in lines:
        parts = line.split()
        if parts and parts[0] == "final":
            finals.setdefault(parts[1], []).append(" ".join(parts[2:]))
    return lines, finals


def ran(lines, run):
    return [l for l in lines if l.startswith("run %s " % run)]


def test_the_four_forms_give_the_same_final_poses(output):
    lines, finals = output
    for k in range(3):
        assert ran(lines, "detect_%d" % k) == ["run detect_%d 1 ''" % k]
    assert ran(lines, "batch") == ["run batch 1 ''"]
    assert ran(lines, "stream") == ["run stream 1 1 1 1 '' ''"]
    assert ran(lines, "slots") == ["run slots 1 ''"] and ran(lines, "slots_again") == ["run slots_again 1 '' in_flight 0"]
    want = finals["detect"]
    assert want
    for form in ("batch", "stream", "slots", "slots_again"):
        assert finals.get(form) == want, form
    # the test cannot pass on empty lists: over the batch a group is accepted, and a group is rejected
    groups = [[int(v) for v in l.split()[1:]] for l in lines if l.startswith("groups ")]
    assert len(groups) == 3
    assert sum(a for _, n, a in groups) >= 1, groups
    assert any(a < 4 and n > a for _, n, a in groups), groups
    assert [l for l in lines if l.startswith("pushed back ")] and int([l for l in lines if l.startswith("pushed back ")][0].split()[2]) > 1000


def test_refusals_say_why(output):
    lines, _ = output
    ref = {l.split()[1]: l for l in lines if l.startswith("refused ")}
    # the single-class detectBatch keeps its refusal and its text
    assert ref["single_class"].startswith("refused single_class 1 'use icp is set: the ICP refinement runs in detect() only, not in the batch and stream forms'")
    for what in ("host_colour_check_batch", "host_colour_check_slots"):
        assert ref[what].startswith("refused %s 1 'use icp is set: with the host colour check" % what), ref[what]
    for what in ("colour_only_batch", "colour_only_slots"):
        assert ref[what].startswith("refused %s 1 'use icp is set: a colour-only detector keeps no depth frame" % what), ref[what]
    assert ref["crosses_set"].startswith("refused crosses_set 1 'slots 14 .. 17 cross a slot set")      # what detectTemplatesSlots refuses
    assert ref["unknown_class"].startswith("refused unknown_class 1 'unknown class name: no-such-class'")
