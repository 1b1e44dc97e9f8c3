"""The pre-processing planner on the CPU: lm_host.cpp's plan_preprocess and single-stage planners -- which kernels a call's a3-a10 launch, in
which order and on which grids -- against the decision table of tests/cpp/preprocess_plan_table.cpp (expectations: the launches of the code
the planner replaced, tests/cpp/preprocess_plan_expect.inc), built with g++ as it is and under ASan / UBSan.  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def test_preprocess_plan_table(tmp_path, flags):
    exe = str(tmp_path / "preprocess_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "preprocess_plan_table.cpp"), os.path.join(CSRC, "lm_host.cpp"), "-lz"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[1]) >= 220
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def _trace_calls():
    """profiles/preprocess_launches.txt (tools/preprocess_launches.py: the launches traced on the GPU, the same for the code before the
    planner and for the planner) as {label: [(kernel, grid)]}, the mask kernels left out."""
    calls, cur = {}, None
    for ln in open(os.path.join(ROOT, "profiles", "preprocess_launches.txt")):
        if ln.startswith("#"):
            continue
        if not ln.startswith("  "):
            cur = calls.setdefault(ln.strip(), [])
            continue
        m = re.match(r"  (k_\w+)(?:<([^>]*)>)? grid (\d+)x(\d+)x(\d+) ", ln)
        name, targs = m.group(1), [t.strip() for t in (m.group(2) or "").split(",") if t.strip()]
        if name in ("k_match_mask", "k_mask_rule"):
            continue
        if name == "k_lm_fast":
            targs = targs[:2]
        if name in ("k_pyrdown16", "k_linear_memories"):
            targs = []
        cur.append((name + ("<%s>" % ",".join(targs) if targs else ""), tuple(int(m.group(k)) for k in (3, 4, 5))))
    return calls


def _table_rows(exe):
    """The table's rows as the planner plans them (--dump; test_preprocess_plan_table holds them to the expectations): {(what, w x h, n): [plans]}"""
    rows = {}
    for ln in subprocess.run([exe, "--dump"], capture_output=True, text=True, timeout=300).stdout.splitlines():
        if "|" not in ln:
            continue
        _, what, shape, n, steps = ln.split("|", 4)
        plan = []
        for st in steps.split(";"):
            f = st.split()
            if not f or f[0] in ("mask_rules", "match_masks"):
                continue
            g = [int(x) for x in f[2].split("x")]
            plan.append((f[0], tuple(g + [1] * (3 - len(g)))))
        rows.setdefault((what, shape, int(n)), []).append(plan)
    return rows


def test_table_rows_match_the_traced_launches(tmp_path):
    """Every row of the table that a detector call reaches is also a call of tools/preprocess_launches.py: the planner's steps for the row are
    the kernels and grids the GPU trace recorded for the call."""
    exe = str(tmp_path / "preprocess_plan_table")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "preprocess_plan_table.cpp"),
                           os.path.join(CSRC, "lm_host.cpp"), "-lz"])
    calls, rows = _trace_calls(), _table_rows(exe)
    pairs = []      # (trace label, table row key, which of the rows with that key)
    V = "640x480"
    for n in (1, 15, 16, 24, 96):
        pairs.append(("rgbd 640x480 n %d" % n, ("rgbd vga", V, n), 0))
    for bp in (0, 1, 2):
        pairs.append(("rgbd 640x480 n 16 BATCH_PHASES %d" % bp, ("rgbd vga, BATCH_PHASES x busy lanes", V, 16), 2 * bp))
    for v in (0, 1):
        pairs.append(("rgbd 640x480 n 96 BATCH_PHASES 0 CGRAD_LEVELS %d" % v, ("CGRAD_LEVELS", V, 96), v))
    for bp in (0, 1, 2, 3):
        for k, bs in enumerate((0, 16, 32, 64)):
            pairs.append(("rgbd 640x480 n 24 BATCH_PHASES 0 BLUR_PYR %d BLUR_STRIP %d" % (bp, bs), ("BLUR_PYR x BLUR_STRIP", V, 24), 4 * bp + k))
    for n in (1, 16):
        pairs.append(("rgbd 640x480 n %d PHASE_MAX_SLOTS 0" % n, ("PHASE_MAX_SLOTS 0", V, n), 0))
    for n in (1, 16, 96):
        pairs.append(("rgbd 640x480 n %d, slot 0 masked" % n, ("a masked slot", V, n), 0))
    for n in (1, 24):
        pairs.append(("rgbd 640x480 n %d, LUT not one-hot" % n, ("LUT not one-hot", V, n), 0))
        pairs.append(("rgbd 640x480 three levels T 4 8 8 n %d" % n, ("three levels", V, n), 0))
        pairs.append(("rgbd 640x480 byte responses n %d" % n, ("LM_FLAG_BYTE_RESPONSES", V, n), 0))
    for n in (1, 15, 16, 96):
        pairs.append(("colour 640x480 n %d" % n, ("colour vga", V, n), 0))
    pairs.append(("colour 640x480 n 96 BATCH_PHASES 0", ("colour vga, busy lanes", V, 96), 0))
    for n in (24, 96):
        pairs.append(("rgbd 320x240 n %d" % n, ("rgbd 320 x 240", "320x240", n), 0))
    for n in (2, 8):
        pairs.append(("rgbd 1280x960 n %d" % n, ("rgbd 1280 x 960", "1280x960", n), 0))
    for k, ww in enumerate((1, 0)):
        for n in (1, 3, 4, 8):
            pairs.append(("colour 1280x960 n %d WORK_WEIGHT %d" % (n, ww), ("colour 1280 x 960, WORK_WEIGHT", "1280x960", n), k))
    for n in (4, 8, 32):
        pairs.append(("colour 1280x960 n %d BATCH_PHASES 0" % n, ("colour 1280 x 960, busy lanes", "1280x960", n), 0))
    for n in (8, 32):
        pairs.append(("colour 1280x960 n %d BLUR_PYR 0" % n, ("colour 1280 x 960, BLUR_PYR 0", "1280x960", n), 0))
    for w, h in ((37, 53), (16, 64), (8, 8), (17, 80), (23, 91), (33, 8), (64, 48), (640, 480)):
        shape = "%dx%d" % (w, h)
        for mag in (0, 1):
            pairs.append(("stage colour %s magnitude %d" % (shape, mag), ("stage colour", shape, 1), mag))
        pairs.append(("stage pyrDown " + shape, ("stage pyrDown", shape, 1), 0))
        pairs.append(("stage depth " + shape, ("stage depth", shape, 1), 0))
    for w, h, ts in ((640, 480, (2, 4, 5, 8)), (320, 240, (8,)), (48, 36, (3,)), (40, 20, (5,)), (24, 24, (8,)), (66, 30, (6,)), (70, 35, (7,)), (160, 160, (16,)), (36, 36, (2,))):
        for k, t in enumerate(ts):
            pairs.append(("stage linear memories %dx%d T %d" % (w, h, t), ("stage linear memories", "%dx%d" % (w, h), 1), k))
    assert len(pairs) >= 100
    bad = []
    for label, key, k in pairs:
        assert label in calls, label
        assert key in rows and k < len(rows[key]), key
        if rows[key][k] != calls[label]:
            bad.append("%s:\n  planned %s\n  traced  %s" % (label, rows[key][k], calls[label]))
    assert not bad, "\n".join(bad)
