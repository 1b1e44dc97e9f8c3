"""The four resource owners of csrc/lm_own.h on the CPU: tests/cpp/own_test.cpp compiles the header alone against the stub runtime of
tests/cpp/hip_stub (malloc, a table of live handles, a k-th-call failure) and holds construction, moves, reset, grow's release-before-
allocate order and the fill-a-dozen-owners-and-fail-at-call-k shape of ensure_device / ensure_lane to the table and to the header's own
live counts.  Built with g++ as it is and under ASan / UBSan (leaks included).  A stand-alone program; nothing is loaded into Python.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
STUB = os.path.join(ROOT, "tests", "cpp", "hip_stub")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_owners(tmp_path, flags):
    exe = str(tmp_path / "own_test")
    # the stub first on the include path: lm_own.h's <hip/hip_runtime.h> is the stub's
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", STUB, "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "own_test.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[1]) >= 200
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_header_stands_alone():
    """lm_own.h includes the HIP runtime header and the standard library, nothing of the detector."""
    inc = [ln.split()[1] for ln in open(os.path.join(CSRC, "lm_own.h")) if ln.startswith("#include")]
    assert inc and all(i.startswith("<") for i in inc), inc
