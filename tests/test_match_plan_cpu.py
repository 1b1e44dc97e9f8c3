"""The match-stage planner on the CPU: lm_host.cpp's plan_match -- which kernels a11-a15 launch for a range of classes, in which order, on
which grids, and the numbers the kernels' argument structs derive from the call -- against the decision table of
tests/cpp/match_plan_table.cpp (expectations: the launch code of the commit the planner replaced, tests/cpp/match_plan_expect.inc), built
with g++ as it is and under ASan / UBSan.  A stand-alone program; nothing is loaded into Python.  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SOURCES = [os.path.join(ROOT, "tests", "cpp", "match_plan_table.cpp"), os.path.join(CSRC, "lm_host.cpp")]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_match_plan_table(tmp_path, flags):
    exe = str(tmp_path / "match_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, "-o", exe] + SOURCES + ["-lz"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[1]) >= 316
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def _trace_calls():
    """profiles/match_launches.txt (tools/match_launches.py: the launches traced on the GPU, the same for the code before the planner and
    for the planner) as {label: [(kernel, grid, workgroup)]}; the runtime's fill kernel reads surv_reset.  (The trace has no column for the
    dynamic LDS of a launch, only the kernel's static LDS: the dynamic bytes are the table's alone to hold.)"""
    calls, cur = {}, None
    for ln in open(os.path.join(ROOT, "profiles", "match_launches.txt")):
        if ln.startswith("#"):
            continue
        if not ln.startswith("  "):
            cur = calls.setdefault(ln.strip(), [])
            continue
        m = re.match(r"  (\S+?)(?:<([^>]*)>)? grid (\d+)x(\d+)x(\d+) wg (\d+) lds (\d+)", ln)
        name, targs = m.group(1), [t.strip() for t in (m.group(2) or "").split(",") if t.strip()]
        if name.startswith("__amd_rocclr_fillBuffer"):
            cur.append(("surv_reset", None, None))
            continue
        if name == "k_scan4" and targs[3:] == ["false"]:
            targs = targs[:3]       # (the no-shift-undo flag's default)
        cur.append((name + ("<%s>" % ",".join(targs) if targs else ""), tuple(int(m.group(k)) for k in (3, 4, 5)), int(m.group(6))))
    return calls


def _table_rows(exe):
    """The table's rows as the planner plans them (--dump; test_match_plan_table holds them to the expectations): {what: [steps]}"""
    rows = {}
    for ln in subprocess.run([exe, "--dump"], capture_output=True, text=True, timeout=300).stdout.splitlines():
        if ln.count("|") < 3:
            continue
        _, what, _, steps = ln.split("|", 3)
        plan = []
        for st in steps.split(";"):
            f = st.split()
            if not f:
                continue
            if f[0] == "surv_reset":
                plan.append(("surv_reset", None, None))
                continue
            g = [int(x) for x in f[1].split("x")]
            plan.append((f[0], tuple(g + [1] * (3 - len(g))), int(f[2][1:])))
        rows[what] = plan
    return rows


def test_table_rows_match_the_traced_launches(tmp_path):
    """Every row of the table that is named after a call of tools/match_launches.py: the planner's steps for the row are the kernels, grids
    and workgroups the GPU trace recorded for the call."""
    exe = str(tmp_path / "match_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, "-o", exe] + SOURCES + ["-lz"])
    calls, rows = _trace_calls(), _table_rows(exe)
    shared = sorted(set(calls) & set(rows))
    assert len(shared) >= 99, len(shared)
    bad = ["%s:\n  planned %s\n  traced  %s" % (label, rows[label], calls[label]) for label in shared if rows[label] != calls[label]]
    assert not bad, "\n".join(bad)
