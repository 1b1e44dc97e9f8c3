"""CPU tests of LM_FLAG_KEEP_DEPTH (ABI 0.13 additive): the flag's value in the header and the binding, lm_create and
lm_keeps_depth for both modality counts, the version string, the settings key `keep depth on device` with the combinations that imply it
(tests/cpp/keep_depth_settings.cpp), what an ingest call does with its depth descriptors with and without "keeps depth"
(tests/cpp/keep_depth_check_host.cpp, plain and under ASan / UBSan: host code alone), and the refusal to compute without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SETTINGS = os.path.join(ROOT, "tests", "golden", "reference_data", "linemod_settings.yml")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
REGISTERED_REFUSAL = "lm_ingest_frames_registered needs an RGB-D detector: a colour-only detector holds no depth frame"


def test_flag_value_agrees_between_header_and_binding(lm):
    header = open(os.path.join(ROOT, "include", "linemod_hip.h")).read()
    flags = {name: int(v) for name, v in re.findall(r"^#define LM_FLAG_(\w+) (\d+)$", header, re.M)}
    assert flags == {"BYTE_RESPONSES": 1, "BLOCKING_SYNC": 2, "KEEP_DEPTH": 4}
    assert (lm.FLAG_BYTE_RESPONSES, lm.FLAG_BLOCKING_SYNC, lm.FLAG_KEEP_DEPTH) == (1, 2, 4)
    assert "lm_keeps_depth" in lm.EXPORTS and re.search(r"^int lm_keeps_depth\(const lm_detector\* det\);", header, re.M)
    # no struct of the ABI changed: the flag lives in lm_config.flags, the last of its 22 int32 / float words
    assert C.sizeof(lm.Config) == 88 and lm.Config.flags.offset == 84


@pytest.mark.parametrize("color_only", [True, False], ids=["M1", "M2"])
@pytest.mark.parametrize("flags", [0, 4, 2, 6], ids=["plain", "keep", "other", "keep_and_other"])
def test_create_and_keeps_depth(lm, color_only, flags):
    lib = lm.load_library()
    d = lm.Detector(color_only=color_only, width=160, height=80, flags=flags)
    assert d.num_modalities == (1 if color_only else 2)
    want = (not color_only) or bool(flags & 4)
    assert lib.lm_keeps_depth(d.h) == (1 if want else 0) and d.keeps_depth is want
    assert d.cfg.flags == flags
    d.close()


def test_keep_depth_keyword_and_null(lm):
    lib = lm.load_library()
    assert lib.lm_keeps_depth(None) == -1
    d = lm.Detector(color_only=True, keep_depth=True, width=160, height=80)
    assert d.cfg.flags & lm.FLAG_KEEP_DEPTH and d.keeps_depth and d.num_modalities == 1 and d.get_T(0) == 2
    d.close()
    d = lm.Detector(color_only=True, width=160, height=80)
    assert d.cfg.flags == 0 and not d.keeps_depth
    d.close()
    d = lm.Detector(color_only=False, keep_depth=True, width=160, height=80)
    assert d.keeps_depth and d.num_modalities == 2 and d.get_T(0) == 5
    d.close()
    assert lm.default_config(color_only=True, keep_depth=True, flags=lm.FLAG_BLOCKING_SYNC).flags == lm.FLAG_BLOCKING_SYNC | lm.FLAG_KEEP_DEPTH
    assert lm.default_config(color_only=True).flags == 0


def test_version_string(lm):
    v = lm.load_library().lm_version()
    assert v.startswith(b"linemod_hip 0.13 ")
    assert b"0.13 additive: LM_FLAG_KEEP_DEPTH and lm_keeps_depth" in v
    for earlier in (b"0.13 additive: the ICP refinement batched across slots, lm_icp_refine_slots", b"lm_depth_select_begin and lm_depth_select_end",
                    b"0.13 additive: rectification and reduction in one ingest pass", b"0.13 = the 0.12 ABI plus the depth registration",
                    b"0.12 = the 0.11 ABI plus the YUV and grey ingest formats", b"0.5 = the 0.4 ABI plus lm_icp_*"):
        assert earlier in v, earlier


def test_settings_key_and_the_implied_combinations(lm, tmp_path):
    exe = str(tmp_path / "keep_depth_settings")
    libdir = os.path.dirname(lm.LIB_PATH)
    host = os.path.join(ROOT, "line-mod-pipeline_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "keep_depth_settings.cpp"),
                           os.path.join(host, "HighLevelLinemod.cpp"), os.path.join(host, "PostProcess.cpp"),
                           os.path.join(host, "TemplateGenerator.cpp"), "-L" + libdir, "-llinemod_hip", "-lpthread", "-Wl,-rpath," + libdir])
    shipped = open(SETTINGS).read()
    assert "only use color modality: 1" in shipped and "use icp: 0" in shipped and "keep depth on device" not in shipped and "depth statistic" not in shipped
    files = {
        "shipped": shipped,
        "key": shipped + "keep depth on device: 1\n",
        "key_off": shipped + "keep depth on device: 0\n",
        "statistic": shipped + "depth statistic: 1\n",
        "statistic_off": shipped + "depth statistic: 0\n",
        "icp": shipped.replace("use icp: 0", "use icp: 1"),
        "statistic_key_off": shipped + "depth statistic: 1\nkeep depth on device: 0\n",
        "icp_key_off": shipped.replace("use icp: 0", "use icp: 1") + "keep depth on device: 0\n",
        "rgbd_statistic_icp": shipped.replace("only use color modality: 1", "only use color modality: 0").replace("use icp: 0", "use icp: 1") + "depth statistic: 1\n",
        "rgbd_key": shipped.replace("only use color modality: 1", "only use color modality: 0") + "keep depth on device: 1\n",
    }
    for name, text in files.items():
        (tmp_path / (name + ".yml")).write_text(text)
    out = subprocess.run([exe] + [str(tmp_path / (n + ".yml")) for n in files], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0] == "defaults key 0 keeps 0"
    got = dict(zip(files, out[1:1 + len(files)]))
    assert got["shipped"] == "read 1 colourOnly 1 statistic 0 icp 0 key 0 keeps 0"
    assert got["key"] == "read 1 colourOnly 1 statistic 0 icp 0 key 1 keeps 1"
    assert got["key_off"] == "read 1 colourOnly 1 statistic 0 icp 0 key 0 keeps 0"
    assert got["statistic"] == "read 1 colourOnly 1 statistic 1 icp 0 key 1 keeps 1"
    assert got["statistic_off"] == "read 1 colourOnly 1 statistic 0 icp 0 key 0 keeps 0"
    assert got["icp"] == "read 1 colourOnly 1 statistic 0 icp 1 key 1 keeps 1"
    assert got["statistic_key_off"] == "read 1 colourOnly 1 statistic 1 icp 0 key 0 keeps 0"             # (an explicit 0 wins over what the file implies)
    assert got["icp_key_off"] == "read 1 colourOnly 1 statistic 0 icp 1 key 0 keeps 0"
    assert got["rgbd_statistic_icp"] == "read 1 colourOnly 0 statistic 1 icp 1 key 0 keeps 0"          # (an RGB-D detector keeps depth anyway: nothing to opt into)
    assert got["rgbd_key"] == "read 1 colourOnly 0 statistic 0 icp 0 key 1 keeps 0"
    assert out[-1] == "struct plain 0 key 1 statistic 0 icp 0 rgbd 0"          # (code that fills the struct itself: the field alone decides)


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def check_table(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("keep_depth_check_host") / "keep_depth_check_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + request.param +
                          ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "keep_depth_check_host.cpp"), os.path.join(CSRC, "lm_ingest_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    table = {}
    for line in r.stdout.splitlines()[1:]:
        key, flags, refusal = line.split(" | ", 2) if line.count(" | ") == 2 else (line.split(" | ") + [""])[:3]
        table[tuple(int(v) for v in key.split())] = (tuple(int(v) for v in flags.split()), refusal.strip())
    return table


def test_ingest_depth_descriptors_with_and_without_keeps_depth(check_table):
    """The table written out: (modalities, flags, registered, depth descriptors given) -> (keeps depth, depth required, the call takes
    the descriptors), refusal."""
    assert len(check_table) == 2 * 4 * 2 * 2
    for other in (0, 3):                    # a colour-only detector without the flag: as before -- descriptors ignored, the registered route refused
        for given in (0, 1):
            assert check_table[(1, other, 0, given)] == ((0, 0, 0), "")
            assert check_table[(1, other, 1, given)] == ((0, 0, 0), REGISTERED_REFUSAL)
    for flags in (4, 6):                    # ... with it: the descriptors are optional, but the registered route needs its raw depth images
        assert check_table[(1, flags, 0, 0)] == ((1, 0, 0), "")
        assert check_table[(1, flags, 0, 1)] == ((1, 0, 1), "")
        assert check_table[(1, flags, 1, 0)] == ((1, 1, 0), "")
        assert check_table[(1, flags, 1, 1)] == ((1, 1, 1), "")
    for flags in (0, 3, 4, 6):              # an RGB-D detector: required, whatever the flag says
        for registered in (0, 1):
            assert check_table[(2, flags, registered, 0)] == ((1, 1, 0), "")
            assert check_table[(2, flags, registered, 1)] == ((1, 1, 1), "")


def _has_gpu(lm):
    d = lm.Detector(color_only=True, width=64, height=64, T=[2, 8])
    try:
        d.stage_pyrdown(np.zeros((8, 8, 3), np.uint8))
        return True
    except lm.LinemodError:
        return False
    finally:
        d.close()


def test_compute_entry_points_fail_loudly_without_gpu(lm):
    if _has_gpu(lm):
        pytest.skip("a HIP device is present")
    d = lm.Detector(color_only=True, keep_depth=True, width=160, height=80)
    bgr, depth = np.zeros((80, 160, 3), np.uint8), np.zeros((80, 160), np.uint16)
    q = np.array([(0, 0, 8, 8, 3, 0)], lm.DEPTH_SELECT_QUERY_DTYPE)
    cq = np.array([(0, 0, 8, 8, 100, 200, 0, 0)], lm.DEPTH_QUERY_DTYPE)
    calls = (lambda: d.upload_frame(0, bgr, depth), lambda: d.upload_frame(0, bgr), lambda: d.read_frame(0), lambda: d.depth_select(q),
             lambda: d.depth_counts(cq), lambda: d.match(bgr, depth, 80.0), lambda: d.set_mask_rule(0, 1, modalities=1, depth_range=(500, 900)),
             lambda: d.stage_reserve(0, 1))
    for call in calls:
        with pytest.raises(lm.LinemodError) as e:
            call()
        assert e.value.code == lm.LM_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    d.close()
