"""The plan of a batched ICP refinement on the CPU (lm_host.cpp plan_icp_batch / plan_icp_levels), dumped by
tests/cpp/icp_batch_plan.cpp (g++, no HIP) for crafted query lists: the per-query level records against tests/icp_reference.py's
level_schedule plus the rule that a level iterates only with at least 6 sampled rows on both sides, the rounds enqueued per level,
the scratch regions, the grids, and the chunking rules.  The scene sizes are frame0's (tests/test_gpu_icp_batch.py has them on the
GPU): 13 and 11 points, 1 712 and 2 979 points (one and two 1-NN chunks), models of 1 767 and 883 rows."""
import os
import subprocess

import pytest

import icp_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "icp_batch_plan.cpp"), os.path.join(CSRC, "lm_host.cpp")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
TILE = 256
MB = 1 << 20


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("icp_batch_plan") / "icp_batch_plan")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g"] + SAN + ["-I", CSRC, "-o", out] + SOURCES + ["-lz"])
    return out


def plan(exe, queries, step=2, iterations=6, levels=8, tolerance=0.1, budget=512 * MB):
    """queries: (npx, nm, first_pose, np, rows).  Returns the chunks as dicts."""
    args = [exe, str(step), str(iterations), str(levels), repr(float(tolerance)), str(budget)] + [",".join(str(v) for v in q) for q in queries]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    chunks = []
    for ln in r.stdout.splitlines():
        f = ln.split()
        if f[0] == "chunk":
            chunks.append(dict(bytes=int(f[3]), np=int(f[5]), nlevels=int(f[7]), g_px=int(f[9]), g_normals=int(f[11]), regions=[], queries=[],
                               pose0={}, lev={}, launch={}))
        elif f[0] == "region":
            chunks[-1]["regions"].append((f[1], int(f[2]), int(f[3]), int(f[4])))
        elif f[0] == "query":
            chunks[-1]["queries"].append(dict(query=int(f[1]), **{f[i]: int(f[i + 1]) for i in range(2, len(f), 2)}))
        elif f[0] == "poses":
            chunks[-1]["poses"] = int(f[1])
        elif f[0] == "pose0":
            chunks[-1]["pose0"][int(f[1])] = int(f[2])
        elif f[0] == "lev":
            d = {f[i]: f[i + 1] for i in range(3, len(f), 2)}
            chunks[-1]["lev"][(int(f[1]), int(f[2]))] = dict(level=int(d["level"]), s=int(d["s"]), nL=int(d["nL"]), ndL=int(d["ndL"]),
                                                              rounds=int(d["rounds"]), max_it=int(d["max_it"]), tolp=float(d["tolp"]))
        elif f[0] == "launch":
            chunks[-1]["launch"][int(f[1])] = dict(rounds=int(f[3]), g_src=int(f[5]), g_chunks=int(f[7]), g_dst=int(f[9]))
    assert r.stdout.splitlines()[-1] == "OK %d" % len(chunks)
    return chunks


def expected_levels(nm, rows, levels, iterations, tolerance):
    out = []
    for level, s, max_it, rounds, tolp in R.level_schedule(nm, levels, iterations, tolerance):
        nL, ndL = nm // s, rows // s
        out.append(dict(level=level, s=s, nL=nL, ndL=ndL, rounds=rounds if nL >= 6 and ndL >= 6 else 0, max_it=max_it, tolp=tolp))
    return out


def nn_chunks(ndL):
    return max(1, min(32, (ndL + 2047) // 2048))


def tiles(n):
    return (n + TILE - 1) // TILE


def check_chunk(c, queries, step, levels, iterations, tolerance):
    """Everything that must hold of one chunk, whatever its queries are."""
    # regions: 256-byte aligned, inside the chunk, no two overlapping
    regs = sorted(c["regions"], key=lambda r: r[2])
    assert len(regs) == 7 + 11 * len(c["queries"])
    for name, q, off, size in regs:
        assert off % 256 == 0 and off + size <= c["bytes"], (name, q, off, size)
    for a, b in zip(regs, regs[1:]):
        assert a[2] + max(a[3], 1) <= b[2], (a, b)
    by = {(name, q): size for name, q, off, size in regs}
    assert c["np"] == sum(e["np"] for e in c["queries"])
    live_np = 0
    for e in c["queries"]:
        npx, nm, first, np_, rows = queries[e["query"]]
        assert (e["npx"], e["nm"], e["np"]) == (npx, nm, np_) and np_ > 0
        ns_cap = max(npx // step, 1)
        assert e["nb"] == tiles(npx) and e["ns_cap"] == ns_cap and e["nch_cap"] == nn_chunks(ns_cap) and e["nblk_cap"] == max(1, tiles(ns_cap))
        assert rows <= ns_cap
        # the regions hold what the kernels index: the largest case the query can meet
        assert by[("z", e["query"])] >= npx * 4 and by[("cloud", e["query"])] >= (ns_cap + 1) * 24
        assert by[("blockcnt", e["query"])] >= tiles(npx) * 4 and by[("blockoff", e["query"])] >= tiles(npx) * 4
        assert by[("src0", e["query"])] >= np_ * nm * 48 and by[("srcL", e["query"])] >= np_ * nm * 48
        assert by[("part", e["query"])] >= np_ * nn_chunks(ns_cap) * nm * 16
        assert by[("nd", e["query"])] >= np_ * nm * 4 and by[("nidx", e["query"])] >= np_ * nm * 4
        assert by[("keys", e["query"])] >= np_ * ns_cap * 8 and by[("acc", e["query"])] >= np_ * max(1, tiles(ns_cap)) * 29 * 8
        # the scene grids cover the query
        assert c["g_px"] >= tiles(npx) and c["g_normals"] >= tiles(ns_cap)
        exp = expected_levels(nm, max(rows, 0), levels, iterations, tolerance)
        for l in range(levels):
            got = c["lev"][(e["query"], l)]
            if rows < 0:
                assert got["rounds"] == 0
                continue
            # TolP: tolerance (level + 1) (level + 1) in the library, tolerance (level + 1)^2 in the reference -- one rounding apart
            assert got.pop("tolp") == pytest.approx(exp[l].pop("tolp"), rel=1e-15, abs=0)
            assert got == exp[l], (e["query"], l, got, exp[l])
        assert c["pose0"][e["query"]] == (live_np if rows >= 0 else -1)
        live_np += np_ if rows >= 0 else 0
    assert c["poses"] == live_np
    assert by[("st", -1)] >= c["np"] * 360 and by[("out", -1)] >= c["np"] * 128 and by[("levels", -1)] >= len(c["queries"]) * levels * 32
    # per level: the rounds enqueued are the maximum over the queries, and every grid covers every query that iterates
    for l in range(levels):
        lv = [c["lev"][(e["query"], l)] for e in c["queries"]]
        g = c["launch"][l]
        assert g["rounds"] == max(v["rounds"] for v in lv)
        for v in lv:
            if v["rounds"]:
                assert g["g_src"] >= tiles(v["nL"]) and g["g_chunks"] >= nn_chunks(v["ndL"]) and g["g_dst"] >= max(1, tiles(v["ndL"]))
        it = [v for v in lv if v["rounds"]]
        if it:      # ... and no larger than the largest needs
            assert g["g_src"] == max(tiles(v["nL"]) for v in it) and g["g_chunks"] == max(nn_chunks(v["ndL"]) for v in it)
            assert g["g_dst"] == max(max(1, tiles(v["ndL"])) for v in it)


# (npx, model rows, first pose, poses, scene rows): the queries of tests/test_gpu_icp_batch.py and their neighbours
Q_1712 = (3600, 1767, 0, 2, 1712)
Q_883 = (5000, 883, 2, 1, 2400)
Q_13 = (26, 1767, 3, 1, 13)
Q_2979 = (6144, 1767, 4, 1, 2979)
Q_NONE = (100, 1767, 5, 0, 0)
Q_11 = (22, 1767, 5, 1, 11)
Q_SHORT = (16, 883, 6, 2, -1)


def test_level_records_of_the_frame0_cases(exe):
    queries = [Q_1712, Q_883, Q_13, Q_2979, Q_NONE, Q_11, Q_SHORT]
    chunks = plan(exe, queries)
    assert len(chunks) == 1
    c = chunks[0]
    assert [e["query"] for e in c["queries"]] == [0, 1, 2, 3, 5, 6]          # the query without poses takes no part
    check_chunk(c, queries, 2, 8, 6, 0.1)
    rounds = lambda q: [c["lev"][(q, l)]["rounds"] for l in range(8)]        # noqa: E731  (coarsest level first: levels 7 .. 0)
    assert rounds(0) == [0, 0, 0, 0, 0, 2, 3, 6]
    # 13 points against 1 767 rows: level 2 samples 3 scene rows and never iterates, levels 1 and 0 do
    assert c["lev"][(2, 5)]["ndL"] == 3 and rounds(2) == [0, 0, 0, 0, 0, 0, 3, 6]
    # 11 points: levels 2 and 1 never iterate
    assert rounds(5) == [0, 0, 0, 0, 0, 0, 0, 6]
    assert rounds(6) == [0] * 8
    # one and two 1-NN chunks at level 0, and the launch takes the larger
    assert nn_chunks(c["lev"][(0, 7)]["ndL"]) == 1 and nn_chunks(c["lev"][(3, 7)]["ndL"]) == 2 and c["launch"][7]["g_chunks"] == 2
    assert [c["launch"][l]["rounds"] for l in range(8)] == [0, 0, 0, 0, 0, 2, 3, 6]
    assert c["lev"][(1, 7)]["nL"] == 883 and c["lev"][(0, 7)]["nL"] == 1767


@pytest.mark.parametrize("params", [dict(), dict(tolerance=0.01, iterations=10), dict(levels=3, tolerance=0.001), dict(levels=1, iterations=1),
                                    dict(step=3)], ids=lambda p: ",".join("%s=%s" % kv for kv in sorted(p.items())) or "shipped")
def test_plans_hold_under_other_parameters(exe, params):
    queries = [Q_1712, Q_883, Q_13, Q_2979, Q_NONE, Q_11, Q_SHORT, (76800, 14136, 8, 3, 20000)]
    step, levels = params.get("step", 2), params.get("levels", 8)
    queries = [(npx, nm, f, n, min(rows, max(npx // step, 1))) for npx, nm, f, n, rows in queries]
    for c in plan(exe, queries, **params):
        check_chunk(c, queries, step, levels, params.get("iterations", 6), params.get("tolerance", 0.1))


def test_chunks_respect_the_budget_and_never_split_a_query(exe):
    queries = [Q_1712, Q_883, Q_13, Q_2979, Q_NONE, Q_11, Q_SHORT] + [(1600, 883, 8 + 14 * k, 14, 700) for k in range(9)]
    alone = [plan(exe, [q])[0]["bytes"] if q[3] else 0 for q in queries]
    for budget in (MB, 2 * MB, 3 * MB + 12345, 512 * MB):
        chunks = plan(exe, queries, budget=budget)
        seen = [e["query"] for c in chunks for e in c["queries"]]
        assert seen == [k for k, q in enumerate(queries) if q[3]]               # every query once, in order: none split, none dropped
        for c in chunks:
            check_chunk(c, queries, 2, 8, 6, 0.1)
            assert c["bytes"] <= budget or len(c["queries"]) == 1
        # greedy: a chunk ends only where the next query would not have fitted
        for c, nxt in zip(chunks, chunks[1:]):
            ks = [e["query"] for e in c["queries"]] + [nxt["queries"][0]["query"]]
            assert plan(exe, [queries[k] for k in ks], budget=1 << 40)[0]["bytes"] > budget
        if budget == MB:
            assert len(chunks) > 3
            assert any(len(c["queries"]) == 1 and c["bytes"] > budget for c in chunks) == any(b > budget for b in alone)
        if budget == 512 * MB:
            assert len(chunks) == 1


def test_a_chunk_breaks_at_an_overlapping_pose_range(exe):
    # queries 0 and 1 disjoint; 2 overlaps 0; 3 touches nothing; 4 overlaps 3's range by one pose; an empty range overlaps nothing
    queries = [(400, 883, 0, 4, 150), (400, 883, 4, 2, 150), (400, 883, 3, 1, 150), (400, 883, 10, 3, 150), (400, 883, 12, 5, 150),
               (400, 883, 11, 0, 150), (400, 883, 17, 1, 150)]
    chunks = plan(exe, queries)
    assert [[e["query"] for e in c["queries"]] for c in chunks] == [[0, 1], [2, 3], [4, 6]]
    for c in chunks:
        check_chunk(c, queries, 2, 8, 6, 0.1)
