"""The shipped mode through the facade (tests/cpp/keep_depth_facade.cpp): the reference's own settings file --
`only use color modality: 1` with `use depth improvement: 1`, threshold 80 -- plus `depth statistic: 1`, read with readSettings, makes a
colour-only detector that keeps the depth frame on the device.  With templates of the shipped model made on the GPU, on the golden frame
and three copies moved along the optical axis,
  - the poses of detect() frame by frame equal, as %.9g strings, those of detectTemplatesBatch, of the streamed form with two batches
    in flight, and of detectTemplatesSlots on uploaded and on ingested frames;
  - the depth checks of the batch were decided on GPU-selected values, at least one inside and one outside the window;
  - with `use icp: 1` beside it the class-list detectBatch and detectBatchSlots give the final poses of detect()."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = os.path.join(ROOT, "tests", "golden", "reference_data", "linemod_settings.yml")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def program(lm, frame0, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("keep_depth_facade")
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
    shipped = open(SETTINGS).read()
    assert "only use color modality: 1" in shipped and "use depth improvement: 1" in shipped and "use icp: 0" in shipped
    (tmp / "statistic.yml").write_text(shipped + "depth statistic: 1\n")
    (tmp / "icp.yml").write_text(shipped.replace("use icp: 0", "use icp: 1") + "depth statistic: 1\n")
    host = os.path.join(ROOT, "line-mod-pipeline_amd", "host")
    libdir = os.path.dirname(lm.LIB_PATH)
    exe = str(tmp / "keep_depth_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "keep_depth_facade.cpp"),
                           os.path.join(host, "HighLevelLinemod.cpp"), os.path.join(host, "PoseDetection.cpp"),
                           os.path.join(host, "PostProcess.cpp"), os.path.join(host, "TemplateGenerator.cpp"),
                           "-L" + libdir, "-llinemod_hip", "-lpthread", "-Wl,-rpath," + libdir])

    def run(mode):
        r = subprocess.run([exe, mode + ".yml", "mesh.bin", "bgr.raw", "depth.raw", mode], cwd=tmp, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        print(r.stdout)
        lines = r.stdout.splitlines()
        runs = {}
        for line in lines:
            parts = line.split()
            if parts and parts[0] in ("pose", "final", "matches"):
                runs.setdefault(parts[1], []).append(" ".join(parts[:1] + parts[2:]))
        return lines, runs
    return run


@pytest.fixture(scope="module")
def statistic(program):
    return program("statistic")


@pytest.fixture(scope="module")
def icp(program):
    return program("icp")


def ran(lines, run):
    return [l for l in lines if l.startswith("run %s " % run)]


def test_settings_file_makes_a_colour_only_detector_that_keeps_depth(statistic):
    lines, _ = statistic
    assert lines[0] == "settings colourOnly 1 depthImprovement 1 threshold 80 statistic 1 icp 0 keep 1"
    assert lines[1] == "detector modalities 1 keeps_depth 1 facade 1"


def test_every_batch_form_gives_the_poses_of_detect(statistic):
    lines, runs = statistic
    for k in range(4):
        assert ran(lines, "detect_%d" % k) == ["run detect_%d 1 ''" % k]
    assert ran(lines, "batch") == ["run batch 1 ''"]
    assert ran(lines, "stream") == ["run stream 1 1 1 1 in_flight 2 ''"]
    assert ran(lines, "slots_up") == ["run slots_up 1 ''"] and ran(lines, "slots_in") == ["run slots_in 1 ''"]
    poses = lambda run: [l for l in runs[run] if l.startswith("pose ")]
    want = poses("detect")
    assert len(want) >= 1 and len({l.split()[1] for l in want}) >= 2, want          # poses on at least two of the four frames
    for run in ("batch", "stream", "slots_up", "slots_in"):
        assert poses(run) == want, run


def test_the_depth_checks_were_decided_on_gpu_selected_values(statistic):
    lines, _ = statistic
    sel = {l.split()[1]: (int(l.split()[3]), int(l.split()[5]), int(l.split()[7])) for l in lines if l.startswith("selected ")}
    for run in ("batch", "slots_up"):
        passed, failed, checks = sel[run]
        assert passed >= 1 and failed >= 1 and passed + failed == checks, (run, sel)


def test_match_gate_with_a_depth_range_on_the_colour_modality(statistic):
    """setMatchGate's depth range is served from the kept depth frame: detect() and the batch form give the same gated lists and poses;
    the gate leaves the part's own frame its matches and takes matches from the frame moved 90 mm out of the range (the colour images
    are the same, so ungated the two frames have the same list); without the frame on the device the library refuses the gate."""
    lines, runs = statistic
    assert ran(lines, "gate_detect_0") == ["run gate_detect_0 1 ''"] and ran(lines, "gate_detect_3") == ["run gate_detect_3 1 ''"]
    assert ran(lines, "gate_batch") == ["run gate_batch 1 ''"]
    assert runs["gate_batch"] and sorted(runs["gate_batch"]) == sorted(runs["gate_detect"])
    count = lambda run, frame: [int(l.split()[2]) for l in runs[run] if l.startswith("matches %d " % frame)][0]
    assert count("detect", 0) == count("detect", 3) > 0
    assert 0 < count("gate_detect", 0) <= count("detect", 0) and count("gate_detect", 3) < count("gate_detect", 0)
    ref = [l for l in lines if l.startswith("refused gate_without_depth_frame ")]
    assert len(ref) == 1 and ref[0].startswith("refused gate_without_depth_frame 1 '") and "colour-only" in ref[0]


def test_a_slot_without_depth_is_refused_by_its_number(statistic):
    lines, _ = statistic
    ref = [l for l in lines if l.startswith("refused no_depth_in_slot ")]
    assert len(ref) == 1 and ref[0].startswith("refused no_depth_in_slot 1 '") and "slot 9" in ref[0] and "without a depth image" in ref[0]
    assert ref[0].endswith("poses 0 in_flight 0")


def test_use_icp_in_the_batch_and_slot_forms(icp):
    lines, runs = icp
    assert lines[0] == "settings colourOnly 1 depthImprovement 1 threshold 80 statistic 1 icp 1 keep 1"
    assert lines[1] == "detector modalities 1 keeps_depth 1 facade 1"
    for k in range(4):
        assert ran(lines, "detect_%d" % k) == ["run detect_%d 1 ''" % k]
    assert ran(lines, "batch") == ["run batch 1 ''"] and ran(lines, "slots") == ["run slots 1 ''"]
    want = runs["detect"]
    assert len(want) >= 1, lines
    assert runs["batch"] == want and runs["slots"] == want
