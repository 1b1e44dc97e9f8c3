"""The scan planner on the CPU: lm_host.cpp's plan_layout / plan_scan -- which layout the pre-processing writes for the scanned level and
which similarity scan (k_scan4, k_scan1, k_scanl, or a refusal) then runs -- against the decision table of tests/cpp/scan_plan_table.cpp,
built with g++ as it is and under ASan / UBSan.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_scan_plan_table(tmp_path, flags):
    exe = str(tmp_path / "scan_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "scan_plan_table.cpp"), os.path.join(CSRC, "lm_host.cpp"), "-lz"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[1]) >= 80
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
