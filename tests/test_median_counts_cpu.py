"""The word arithmetic of k_dmedian's counting median on the CPU: lm_median_counts.h's host-callable functions (rank code -> cumulative
word, the two partial window counts -> flag word -> label) against their definitions, exhaustively per counter position
(tests/cpp/median_counts_check.cpp), built with g++ as it is and under ASan / UBSan.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_median_counts_check(tmp_path, flags):
    exe = str(tmp_path / "median_counts_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "median_counts_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    # 8 positions x 16 x 11 pairs x 4 neighbour settings, ten checks each, are the least it runs
    assert int(r.stdout.split()[1]) >= 8 * 16 * 11 * 4 * 10
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
