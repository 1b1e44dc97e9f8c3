"""Fuzzer (kept under tests/ because it drives the oracle; not collected by pytest): stage kernels and whole matches against the oracle on random shapes and
contents.  usage: python tests/fuzz_parity.py [seconds] [seed]"""
import importlib, sys, os, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
lm = importlib.import_module("line-mod-pipeline_amd")
synth = importlib.import_module("line-mod-pipeline_amd.synth")
from oracle import oracle as orc
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_check_reference as ccref

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
det = lm.Detector(color_only=False)
t0 = time.time()
n_stage = n_match = n_scan = n_batch = n_colour = 0


def rand_bgr(h, w):
    k = rng.integers(0, 4)
    if k == 0:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if k == 1:   # blocks with sharp edges
        b = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8)
        return np.ascontiguousarray(np.kron(b, np.ones((8, 8, 1), np.uint8))[:h, :w])
    if k == 2:   # extremes
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    f, _ = synth.make_frame(max(w, 64), max(h, 64), seed=int(rng.integers(1 << 30)))
    return np.ascontiguousarray(f[:h, :w])


def rand_depth(h, w):
    k = rng.integers(0, 3)
    if k == 0:
        return rng.integers(0, 2600, (h, w)).astype(np.uint16)
    if k == 1:
        return (600 + 49 * rng.integers(0, 3, (h, w))).astype(np.uint16)
    _, d = synth.make_frame(max(w, 64), max(h, 64), seed=int(rng.integers(1 << 30)))
    return np.ascontiguousarray(d[:h, :w])


while time.time() - t0 < budget * 0.5:
    w = int(rng.choice([16, 32, 48, 64, 80, 96, 128, 160, 192, 320, 640, 24, 40, 56, 37, 53, 70]))
    h = int(rng.integers(8, 130))
    bgr = rand_bgr(h, w)
    thr = float(rng.choice([10.0, 0.0, 30.0, 200.0]))
    kb, kg = int(rng.choice([0, 1, 3, 4])), int(rng.integers(0, 4))      # blur / gradient kernels: by batch size, few-frame, batch; blur 4 = matrix cores
    det.set_tuning(lm.TUNE_CBLUR_VARIANT, kb); det.set_tuning(lm.TUNE_CGRAD_VARIANT, kg)
    assert np.array_equal(det.stage_color_quantize(bgr, thr), orc.color_quantize(bgr, thr)), ("colour", h, w, thr, kb, kg)
    if h % 2 == 0 and w % 2 == 0 and h >= 4:
        kp = int(rng.integers(0, 3))
        det.set_tuning(lm.TUNE_PYRDOWN_VARIANT, kp)
        assert np.array_equal(det.stage_pyrdown(bgr), orc.pyrdown(bgr)), ("pyrdown", h, w, kp)
    dep = rand_depth(h, w)
    det.set_tuning(lm.TUNE_DMEDIAN_VARIANT, int(rng.integers(0, 3)))   # median: 4 or 16 output rows per lane
    assert np.array_equal(det.stage_depth_quantize(dep), orc.depth_quantize(dep)), ("depth", h, w)
    n_stage += 1
det.set_tuning(lm.TUNE_CBLUR_VARIANT, 0); det.set_tuning(lm.TUNE_CGRAD_VARIANT, 0); det.set_tuning(lm.TUNE_PYRDOWN_VARIANT, 0)
det.set_tuning(lm.TUNE_DMEDIAN_VARIANT, 0)
det.close()

while time.time() - t0 < budget:
    color_only = bool(rng.integers(0, 2))
    awkward = bool(rng.integers(0, 2))
    if awkward:
        # the shape families of tests/test_gpu_match_shapes.py: any multiple of the smallest unit lm_create can take (level l's columns
        # and rows divide by T[l]), so that pitches W = width / T with W % 4 = 1, 2, 3, widths that are no multiple of 8, T = 3, 6, 7 and
        # three levels occur; lm_create refuses the draws whose rows x columns are no multiple of 16
        T = [[4, 2], [4, 4], [5, 5], [2, 5], [4, 4, 2], [2, 2, 2], [3, 6], [7, 7], [8, 5]][int(rng.integers(0, 9))]
        unit = int(np.lcm.reduce([t << l for l, t in enumerate(T)]))
        w, h = unit * int(rng.integers(1, 1 + 640 // unit)), unit * int(rng.integers(1, 1 + 480 // unit))
        w, h = max(w, unit * -(-200 // unit)), max(h, unit * -(-160 // unit))
    else:
        T = [[5, 8], [2, 8], [4, 4], [8, 8]][int(rng.integers(0, 4))] if not color_only else [[2, 8], [4, 8], [2, 4]][int(rng.integers(0, 3))]
        unit = int(np.lcm.reduce([T[0], 2 * T[1], 8]))
        w, h = unit * int(rng.integers(1, 1 + 640 // unit)), unit * int(rng.integers(1, 1 + 480 // unit))
        w, h = max(w, 4 * unit), max(h, 4 * unit)
    L = len(T)
    try:
        nb = int(rng.choice([1, 1, 3, 8, 16, 19]))               # frames per call: phase launches below 16, batch kernels from 16
        d = lm.Detector(lm.default_config(color_only=color_only, width=w, height=h, T=T, flags=int(rng.integers(0, 2)),
                                          frame_slots=max(nb, 2)))
    except lm.LinemodError:
        continue
    o = orc.Detector(color_only=color_only, T=T)
    bgr, depth = synth.make_frame(w, h, seed=int(rng.integers(1 << 30)))
    o.prepare(bgr, None if color_only else depth)
    M = 1 if color_only else 2
    q = {(l, m): o.stage(0, l, m).reshape(h >> l, w >> l) for l in range(L) for m in range(M)}
    n = int(rng.integers(5, 120))
    try:
        nfeat = int(rng.choice([63, 63, 63, 42, 21, 9]))                # r06: also tail rounds of the bit-plane scans (63 is upstream's maximum per template)
        descs, feats, _ = synth.make_bank(n, M, L, seed=int(rng.integers(1 << 30)), quantized=q, crop_fraction=0.3,
                                          frame_size=(w, h), T0=T[0], num_features=nfeat, **({"size_range": (24, 56)} if awkward else {}))
    except Exception:
        d.close(); continue
    d.add_class("c", descs, feats); o.add_class("c", descs, feats)
    thr = float(rng.choice([60.0, 75.0, 85.0, 40.0]))
    variant = int(rng.choice([0, 0, 32, 8, 1, 34, 9, 16, 17, 18]))   # load-block sizes; per-lane pruning (default), none (bit 3), wave-level (bit 4)
    d.set_scan_variant(variant)
    d.set_tuning(lm.TUNE_SCAN_FORM, int(rng.choice([0, 1, 2, 3, 3])))        # r05 / r06: nibble scan / bit-plane scan / bit-plane scan with the planes in LDS (by cost, forced)
    got = d.match(bgr, None if color_only else depth, thr, cap=1 << 18)
    exp = o.match(bgr, None if color_only else depth, thr, threads=8, cap=1 << 18)
    assert got.tobytes() == exp.tobytes(), ("match", color_only, T, w, h, n, thr, variant, len(got), len(exp))
    if len(got):
        # the colour check of the first matches for a random HSV range (fractional, reversed and out-of-range bounds among them) against the
        # exact references: table-rule HSV, hull of the template's level-0 features of all modalities, pixel-by-pixel fill
        head = got[:500]
        a_, b_ = sorted(rng.uniform(-20, 200, 2)); c_, e_ = sorted(rng.uniform(-20, 280, 2)); f_, g_ = sorted(rng.uniform(-20, 280, 2))
        lo_hsv, hi_hsv = [a_, c_, f_], [b_, e_, g_]
        if rng.integers(0, 8) == 0:
            k_ = int(rng.integers(0, 3)); lo_hsv[k_], hi_hsv[k_] = hi_hsv[k_], lo_hsv[k_]
        if rng.integers(0, 4) == 0:
            hi_hsv[int(rng.integers(0, 3))] = float(rng.choice([1e12, 256, 255.5, 2.0 ** 32]))
        cmask = ccref.inrange_mask(*ccref.hsv8_table(bgr), lo_hsv, hi_hsv)
        ends = np.concatenate([[0], np.cumsum(descs["num_features"])])
        pix = {}
        for t in set(int(v) for v in head["template_id"]):
            pts = np.concatenate([feats[ends[k]:ends[k + 1]] for k in range(t * L * M, t * L * M + M)])      # level 0, every modality
            pix[t] = ccref.hull_pixels(ccref.convex_hull(zip(pts["x"], pts["y"])))
        d.upload_frame(0, bgr, None if color_only else depth)
        in_hull, in_both = d.color_check_counts(0, lo_hsv, hi_hsv, head)
        for k, m_ in enumerate(head):
            want = ccref.counts_of_pixels(pix[int(m_["template_id"])], (int(m_["x"]), int(m_["y"])), cmask, w, h)
            assert (in_hull[k], in_both[k]) == want, ("colour check", color_only, T, w, h, lo_hsv, hi_hsv, k, m_, (in_hull[k], in_both[k]), want)
        n_colour += 1
    if nb > 1:
        d.set_tuning(lm.TUNE_PHASE_MAX_SLOTS, int(rng.choice([15, 0])))
        d.set_tuning(lm.TUNE_BATCH_PHASES, int(rng.choice([0, 1, 2])))     # 16+ frames: level-fused batch launches or one per kernel
        d.set_tuning(lm.TUNE_BLUR_PYR, int(rng.choice([0, 1, 2, 3])))         # level-0 blur + pyrDown apart, in one launch back to back, or dealt out evenly
        d.set_tuning(lm.TUNE_BLUR_STRIP, int(rng.choice([0, 16, 32, 64])))      # rows per blur strip inside k_blur_pyr
        d.set_tuning(lm.TUNE_CGRAD_LEVELS, int(rng.choice([0, 1])))             # r06: the two levels' gradients of a batch in one launch or two
        d.set_tuning(lm.TUNE_SCAN_LIST_ORDER, int(rng.choice([0, 1, 2, 3])))    # order of the scan's feature lists (same sums)
        d.set_tuning(lm.TUNE_SCAN_FORM, int(rng.choice([0, 1, 2, 3, 3])))
        d.set_tuning(lm.TUNE_SURVIVOR_QUEUE, int(rng.choice([1 << 20, 1 << 20, 64, 200, 4096])))   # r06: k_scan1's survivor queues, also far too small (partial fits, the waves' own sums)
        # r05: every way a frame reaches a slot -- the one-call upload, the staged upload (rows in random pieces; a zero shift here, the
        # shifted forms are swept in tests/test_gpu_stream.py) -- and the lists once more through lm_match_collect
        staged = bool(rng.integers(0, 2))
        if staged:
            d.stage_reserve(0, nb)
        # a different frame in every slot (slot 0: the frame above; then random contents of every kind), so that a block that computes the
        # right pixels for the wrong slot shows; the oracle's lists and planes of each
        slot_frames = [(bgr, None if color_only else depth)] + [(rand_bgr(h, w), None if color_only else rand_depth(h, w)) for _ in range(nb - 1)]
        for k in range(nb):
            fb, fd = slot_frames[k]
            if staged:
                cut = sorted(set([0, h] + [int(v) for v in rng.integers(0, h + 1, 3)]))
                for a, b in zip(cut[:-1], cut[1:]):
                    d.stage_rows(k, fb, fd, 0, 0, a, b)
                d.upload_staged(k)
            else:
                d.upload_frame(k, fb, fd)
        exps, exp_planes = [], []
        for fb, fd in slot_frames:
            o.prepare(fb, fd)
            exp_planes.append({(what, l, m): o.stage(what, l, m) for what in (0, 2) for l in range(L) for m in range(M)})
            exps.append(o.match_prepared(thr, threads=8, cap=1 << 18))
        assert exps[0].tobytes() == exp.tobytes()
        o.prepare(bgr, None if color_only else depth)      # (the oracle holds the first frame again: the scan check below reads it)
        cap_b = max(max(len(e) for e in exps), 1)
        outb, cntb = d.match_batch(nb, thr, 0, cap_per_frame=cap_b)
        outc2, cntc2 = d.match_collect(0, nb, cap_per_frame=cap_b)
        assert np.array_equal(cntb, cntc2) and outb.tobytes() == outc2.tobytes(), ("collect", color_only, T, w, h, n, thr, nb)
        for k in range(nb):
            for key, plane in exp_planes[k].items():      # quantised images and linear memories of every slot, level and modality
                assert np.array_equal(d.debug_read(k, *key), plane), ("batch planes", color_only, T, w, h, nb, k, key)
            assert cntb[k] == len(exps[k]) and outb[k, :cntb[k]].tobytes() == exps[k].tobytes(), ("batch", color_only, T, w, h, n, thr, nb, k)
        n_batch += 1
    if n_match % 4 == 0:
        # a second class: Detector::match with a class list = the merged per-class lists, one pre-processing (lm_match_batch_classes),
        # and the prepared slot again per class (lm_match_prepared)
        try:
            d2, f2, _ = synth.make_bank(max(n // 2, 3), M, L, seed=int(rng.integers(1 << 30)), quantized=q, crop_fraction=0.3, frame_size=(w, h), T0=T[0],
                                       **({"size_range": (24, 56)} if awkward else {}))
        except Exception:
            d.close(); continue
        d.add_class("c2", d2, f2); o.add_class("c2", d2, f2)
        d.upload_frame(0, bgr, None if color_only else depth)
        exp2 = o.match(bgr, None if color_only else depth, thr, class_idx=-1, threads=8, cap=1 << 18)
        outc, cntc = d.match_batch_classes(0, 1, thr, [1, 0], cap_per_frame=max(len(exp2), 1))
        assert outc[0, :cntc[0]].tobytes() == exp2.tobytes(), ("class list", color_only, T, w, h, n, thr)
        for c in (0, 1):
            outp, cntp = d.match_prepared(0, 1, thr, [c], cap_per_frame=max(len(exp2), 1))
            # (std::unique removes ADJACENT duplicates: in the mixed list a template of the other class can sit between two
            # equal matches of this class, so the class's own list is the filtered mixed list made unique once more)
            sub = exp2[exp2["class_idx"] == c]
            keep = np.ones(len(sub), bool)
            if len(sub) > 1:
                same = (sub["x"][1:] == sub["x"][:-1]) & (sub["y"][1:] == sub["y"][:-1]) & (sub["similarity"][1:] == sub["similarity"][:-1])
                keep[1:] = ~same
            expc = o.match(bgr, None if color_only else depth, thr, class_idx=c, threads=8, cap=1 << 18)
            assert sub[keep].tobytes() == expc.tobytes(), ("filter + unique", color_only, T, w, h, n, thr, c)
            assert outp[0, :cntp[0]].tobytes() == expc.tobytes(), ("prepared", color_only, T, w, h, n, thr, c)
    # a11-a13 alone: the scan kernel's candidate list, record by record
    d.upload_frame(1, bgr, None if color_only else depth)
    d.prepare_slot(1)
    assert np.array_equal(d.stage_scan(1, thr, 0), o.scan_candidates(thr, 0, threads=8)), ("scan", color_only, T, w, h, n, thr, variant)
    d.close()
    n_match += 1
    n_scan += 1
print("fuzz ok: %d stage rounds, %d whole matches, %d scan candidate lists, %d multi-frame calls, %d colour checks in %.0f s (seed %s)" % (
    n_stage, n_match, n_scan, n_batch, n_colour, time.time() - t0, sys.argv[2] if len(sys.argv) > 2 else "1"))
