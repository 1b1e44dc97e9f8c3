"""Mask rules on the GPU (lm_set_mask_rule, k_mask_rule): the mask bytes equal the numpy reference (tests/mask_rule_reference.py), a
match with a rule equals -- quantised images and lists, byte for byte -- the match with the reference's mask uploaded through
lm_upload_match_mask (the path test_gpu_match_masks.py pins against the oracle), a rule survives every kind of frame upload and follows
the new frame, and the refusals of the contract."""
import os
import socket
import subprocess

import numpy as np
import pytest

import mask_rule_reference as mrr

pytestmark = pytest.mark.gpu

THR = 75.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _T(M, L):
    return ([5] if M == 2 else [2]) + [8] * (L - 1)


def _rule(lm, spec):
    return lm.make_mask_rule(spec["modalities"], spec.get("depth_range"), spec.get("keep_invalid", False), spec.get("hsv_range"),
                             spec.get("grow", 0), spec.get("rect"))


# ---- mask bytes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,T", [(80, 80, [5, 8]), (160, 80, [5, 8]), (400, 240, [5, 8]), (640, 480, [5, 8]), (100, 80, [5])])
def test_mask_bytes_equal_reference_on_crafted_seeds(lm, w, h, T):
    """(100 x 80, one level: a width that is no multiple of 8, so a lane's 8 pixels are loaded one by one and the last lane's are cut.)"""
    d = lm.Detector(color_only=False, width=w, height=h, T=T, frame_slots=1)
    for r in mrr.GROWS:
        spec = dict(modalities=3, depth_range=(mrr.ZMIN, mrr.ZMAX), grow=r)
        for name, seed in mrr.crafted_seeds(w, h, r):
            depth = mrr.depth_from_seed(seed)
            got = d.stage_mask_rule(None, depth, _rule(lm, spec))
            assert np.array_equal(got, mrr.mask_of(spec, None, depth)), (w, h, r, name)
    d.close()


def test_mask_bytes_depth_gate_edges(lm):
    depth, rules = mrr.depth_edge_cases()
    d = lm.Detector(color_only=False, width=depth.shape[1], height=depth.shape[0], frame_slots=1)
    for spec in rules:
        for r in (0, 2):
            spec = dict(spec, grow=r)
            assert np.array_equal(d.stage_mask_rule(None, depth, _rule(lm, spec)), mrr.mask_of(spec, None, depth)), spec
    d.close()


def test_mask_bytes_hsv_gate_edges(lm):
    bgr = mrr.hsv_edge_frame()
    h, w = bgr.shape[:2]
    depth = mrr.depth_from_seed(np.random.default_rng(3).random((h, w)) < 0.7)
    for color_only in (False, True):
        d = lm.Detector(color_only=color_only, width=w, height=h, frame_slots=1)
        specs = [dict(modalities=1, hsv_range=(mrr.HSV_LOWER, mrr.HSV_UPPER)),
                 dict(modalities=1, hsv_range=(mrr.HSV_LOWER, mrr.HSV_UPPER), grow=1),
                 dict(modalities=1, hsv_range=([19.5, 59.5, 69.5], [90.5, 200.5, 220.5])),          # ties round to even: 20 60 70 / 90 200 220
                 dict(modalities=1, hsv_range=([0, 0, 0], [255, 150, 255]))]
        if not color_only:
            specs.append(dict(modalities=3, hsv_range=(mrr.HSV_LOWER, mrr.HSV_UPPER), depth_range=(mrr.ZMIN, mrr.ZMAX), grow=2))
        for spec in specs:
            exp = mrr.mask_of(spec, bgr, depth)
            assert (exp == 0).any() and (exp == 255).any()
            assert np.array_equal(d.stage_mask_rule(bgr, None if color_only else depth, _rule(lm, spec)), exp), spec
        d.close()


@pytest.mark.parametrize("w,h", [(80, 80), (400, 240)])
def test_mask_bytes_rectangles(lm, w, h):
    d = lm.Detector(color_only=False, width=w, height=h, frame_slots=1)
    for name, seed, spec in mrr.rect_cases(w, h):
        depth = mrr.depth_from_seed(seed)
        assert np.array_equal(d.stage_mask_rule(None, depth, _rule(lm, spec)), mrr.mask_of(spec, None, depth)), name
    d.close()


# ---- matching with a rule = matching with the reference's mask uploaded -------------------------------------
class _Scene:
    """frame0, a bank with crop templates of it, and rules with their reference masks.  The crops are cut from the detector's own
    quantised images: they only have to give the bank real matches; what is compared is rule against uploaded mask."""

    def __init__(self, lm, synth, bgr, depth, M=2, L=2):
        self.bgr, self.depth, self.M, self.L = bgr, (depth if M == 2 else None), M, L
        self.h, self.w = bgr.shape[:2]
        self.T = _T(M, L)
        d = lm.Detector(color_only=(M == 1), T=self.T, frame_slots=1)
        d.upload_frame(0, bgr, self.depth)
        d.prepare_slot(0)
        q = {(l, m): d.debug_read(0, 0, l, m).reshape(self.h >> l, self.w >> l).copy() for l in range(L) for m in range(M)}
        d.close()
        self.classes = [synth.make_bank(10, M, L, seed=40 + k, quantized=q, crop_fraction=0.4, frame_size=(self.w, self.h), T0=self.T[0])[:2]
                        for k in range(2)]
        both = 3 if M == 2 else 1
        self.rules = {"left": dict(modalities=both, rect=(0, 0, self.w // 2, self.h)),
                      "right": dict(modalities=both, rect=(self.w // 2, 0, self.w // 2, self.h)),
                      "hsv": dict(modalities=1, hsv_range=([0, 0, 0], [255, 150, 255]), grow=2)}
        if M == 2:
            self.rules["depth"] = dict(modalities=3, depth_range=(600, 800), grow=8)
            self.rules["combo"] = dict(modalities=2, depth_range=(560, 900), keep_invalid=True, hsv_range=([0, 0, 0], [255, 200, 255]), grow=8,
                                       rect=(40, 40, self.w - 80, self.h - 80))
        self.ref = {}

    def mask(self, key, frame=None):
        bgr, depth = frame if frame is not None else (self.bgr, self.depth)
        if frame is not None:
            return mrr.mask_of(self.rules[key], bgr, depth)
        if key not in self.ref:
            m = mrr.mask_of(self.rules[key], bgr, depth)
            assert (m == 0).any() and (m == 255).any(), key
            self.ref[key] = m
        return self.ref[key]

    def detector(self, lm, slots=8, **kw):
        d = lm.Detector(color_only=(self.M == 1), width=self.w, height=self.h, T=self.T, frame_slots=slots, **kw)
        for k, (descs, feats) in enumerate(self.classes):
            d.add_class("m%d" % k, descs, feats)
        return d

    def upload(self, d, slot, frame=None):
        bgr, depth = frame if frame is not None else (self.bgr, self.depth)
        d.upload_frame(slot, bgr, depth if self.M == 2 else None)

    def upload_ref_mask(self, d, slot, key, frame=None, also=None):
        """The reference's mask of rule `key` through lm_upload_match_mask, on the modalities the rule names; `also`: a mask every
        modality is ANDed with as well."""
        m = self.mask(key, frame) if key is not None else None
        for mod in range(self.M):
            named = key is not None and (self.rules[key]["modalities"] >> mod) & 1
            eff = m if named else None
            if also is not None:
                eff = also if eff is None else (eff & ((also != 0) * np.uint8(255)))
            if eff is not None:
                d.upload_match_mask(slot, eff, modality=mod)

    def quant(self, d, slot):
        return b"".join(d.debug_read(slot, 0, l, m).tobytes() for l in range(self.L) for m in range(self.M))


def _same(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def scene(lm, synth, frame0):
    return _Scene(lm, synth, *frame0)


@pytest.fixture(scope="module")
def plain(lm, scene):
    """The unruled, unmasked lists of the shared scene, per scan form None (default detector)."""
    d = scene.detector(lm, slots=1)
    scene.upload(d, 0)
    out = d.match_slot(0, THR).copy()
    d.close()
    assert len(out) > 0
    return out


@pytest.mark.parametrize("M,L", [(2, 2), (1, 2), (2, 3), (1, 3)])
def test_rule_equals_uploaded_mask_images_and_lists(lm, synth, frame0, scene, plain, M, L):
    s = scene if (M, L) == (2, 2) else _Scene(lm, synth, *frame0, M=M, L=L)
    d = s.detector(lm, slots=2)
    fewer = 0
    for key, spec in s.rules.items():
        s.upload(d, 0)
        d.set_mask_rule(0, 1, rule=_rule(lm, spec))
        got = d.match_slot(0, THR).copy()
        q_got = s.quant(d, 0)
        s.upload(d, 1)
        s.upload_ref_mask(d, 1, key)
        exp = d.match_slot(1, THR).copy()
        assert q_got == s.quant(d, 1), key
        assert _same(got, exp), key
        if (M, L) == (2, 2):
            fewer += len(got) < len(plain)
        r = d.mask_rule(0)
        assert r is not None and bytes(r) == bytes(_rule(lm, spec)) and d.mask_rule(1) is None
    if (M, L) == (2, 2):
        assert fewer > 0                                  # (left + right: a frame with matches loses some in one half at least)
    # the single-frame call with rule=: slot 0 holds the rule for that call only
    key = "left"
    got = d.match(s.bgr, s.depth, THR, rule=s.rules[key])
    assert d.mask_rule(0) is None
    exp = d.match(s.bgr, s.depth, THR, masks=s.mask(key))
    assert _same(got, exp)
    d.close()


def _mixed(scene, lm, d, n):
    """Slots 0 .. n - 1 in turn: ruled, uploaded mask, both, neither; returns the plan [(kind, rule key)]."""
    keys = list(scene.rules)
    other = (mrr.mask_of(dict(rect=(100, 60, 400, 300)), scene.bgr, scene.depth) // 255).astype(np.uint8) * 7      # an uploaded mask of its own
    plan = []
    for i in range(n):
        kind, key = ("rule", "upload", "both", "none")[i % 4], keys[(i // 4) % len(keys)]
        scene.upload(d, i)
        if kind in ("rule", "both"):
            d.set_mask_rule(i, 1, rule=_rule(lm, scene.rules[key]))
        else:
            d.clear_mask_rule(i, 1)
        if kind == "upload":
            scene.upload_ref_mask(d, i, key)
        if kind == "both":
            d.upload_match_mask(i, other, modality=-1)
        plan.append((kind, key))
    return plan, other


def _expected_mixed(scene, lm, plan, other, **kw):
    """The same slots through uploaded masks alone, on a second detector."""
    d = scene.detector(lm, slots=len(plan), **kw)
    for i, (kind, key) in enumerate(plan):
        scene.upload(d, i)
        if kind in ("rule", "upload"):
            scene.upload_ref_mask(d, i, key)
        elif kind == "both":
            scene.upload_ref_mask(d, i, key, also=other)
    return d


@pytest.mark.parametrize("form", [0, 1, 2, 3, "byte"])
def test_mixed_batch_every_scan_form(lm, scene, plain, form):
    """16 frames -- ruled, uploaded mask, both, neither -- through the batch kernels, with the scan form forced (1 k_scan4, 2 k_scan1,
    3 k_scanl), by cost (0) and with the byte scan."""
    kw = dict(flags=lm.FLAG_BYTE_RESPONSES) if form == "byte" else {}
    d = scene.detector(lm, slots=16, **kw)
    e = None
    try:
        if form != "byte":
            d.set_tuning(lm.TUNE_SCAN_FORM, form)
        plan, other = _mixed(scene, lm, d, 16)
        out, cnt = d.match_batch(16, THR, -1, cap_per_frame=8192)
        e = _expected_mixed(scene, lm, plan, other, **kw)
        if form != "byte":
            e.set_tuning(lm.TUNE_SCAN_FORM, form)
        eout, ecnt = e.match_batch(16, THR, -1, cap_per_frame=8192)
        for i, (kind, key) in enumerate(plan):
            assert _same(out[i, :cnt[i]], eout[i, :ecnt[i]]), (i, kind, key)
            assert scene.quant(d, i) == scene.quant(e, i), (i, kind, key)
            if kind == "none":
                assert _same(out[i, :cnt[i]], plain), i
    finally:
        d.close()
        if e is not None:
            e.close()


def test_two_lanes(lm, scene):
    d = scene.detector(lm, slots=8)
    plan, other = _mixed(scene, lm, d, 8)
    e = _expected_mixed(scene, lm, plan, other)
    for det in (d, e):
        for lane in range(2):
            det.match_begin(lane, 4 * lane, 4, THR, -1)
    for lane in range(2):
        out, cnt = d.match_end(lane, n_slots=4)
        eout, ecnt = e.match_end(lane, n_slots=4)
        for j in range(4):
            assert _same(out[j, :cnt[j]], eout[j, :ecnt[j]]), (lane, j, plan[4 * lane + j])
    d.close()
    e.close()


def test_prepared_before_and_after_a_rule_change(lm, scene):
    d = scene.detector(lm, slots=2)
    e = scene.detector(lm, slots=2)
    for det in (d, e):
        scene.upload(det, 0)
    d.set_mask_rule(0, 1, rule=_rule(lm, scene.rules["left"]))
    scene.upload_ref_mask(e, 0, "left")
    for det in (d, e):
        det.match_batch_classes(0, 1, THR, [0, 1])
    out, cnt = d.match_prepared(0, 1, THR, [1])
    eout, ecnt = e.match_prepared(0, 1, THR, [1])
    assert _same(out[0, :cnt[0]], eout[0, :ecnt[0]])
    d.set_mask_rule(0, 1, rule=_rule(lm, scene.rules["depth"]))
    with pytest.raises(lm.LinemodError):                   # a rule change makes the slot's a3-a10 results stale ...
        d.match_prepared(0, 1, THR, [1])
    with pytest.raises(lm.LinemodError):                   # ... and drops its last lists
        d.match_collect(0, 1)
    scene.upload(e, 0)
    scene.upload_ref_mask(e, 0, "depth")
    for det in (d, e):
        det.match_batch_classes(0, 1, THR, [0, 1])
    out, cnt = d.match_prepared(0, 1, THR, [1])
    eout, ecnt = e.match_prepared(0, 1, THR, [1])
    assert _same(out[0, :cnt[0]], eout[0, :ecnt[0]])
    d.close()
    e.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_gathered_one_rank(lm, scene):
    d = scene.detector(lm, slots=4)
    plan, other = _mixed(scene, lm, d, 4)
    e = _expected_mixed(scene, lm, plan, other)
    eout, ecnt = e.match_batch(4, THR, -1, cap_per_frame=8192)
    d.comm_init(0, 1, "127.0.0.1", _free_port())
    out = np.zeros(1 << 16, lm.MATCH_DTYPE)
    cnt = np.zeros(4, np.int32)
    d.match_begin_gathered(0, 0, 4, THR, -1)
    f0, nf, tot = d.match_end_gathered(0, out, cnt)
    assert (f0, nf) == (0, 4)
    pos = 0
    for i in range(4):
        assert _same(out[pos:pos + cnt[i]], eout[i, :ecnt[i]]), (i, plan[i])
        pos += cnt[i]
    d.comm_destroy()
    d.close()
    e.close()


# ---- sticky behaviour ----------------------------------------------------------------------------------
def _shifted(img, sx, sy):
    out = np.zeros_like(img)
    h, w = img.shape[:2]
    out[max(sy, 0):min(h + sy, h), max(sx, 0):min(w + sx, w)] = img[max(-sy, 0):min(h - sy, h), max(-sx, 0):min(w - sx, w)]
    return out


@pytest.mark.parametrize("path", ["plain", "pinned", "staged", "shifted"])
def test_rule_follows_the_new_frame_through_every_upload_path(lm, synth, scene, path):
    key = "depth"
    d = scene.detector(lm, slots=2)
    e = scene.detector(lm, slots=2)
    scene.upload(d, 0)
    d.set_mask_rule(0, 1, rule=_rule(lm, scene.rules[key]))
    d.upload_match_mask(0, scene.mask("left"), modality=-1)          # an uploaded mask beside the rule: the next upload clears it, not the rule
    scene.upload(e, 0)
    scene.upload_ref_mask(e, 0, key, also=scene.mask("left"))
    assert _same(d.match_slot(0, THR), e.match_slot(0, THR))
    bgr2, depth2 = synth.make_frame(scene.w, scene.h, seed=99)
    sx, sy = 13, -7
    frame2 = (_shifted(bgr2, sx, sy), _shifted(depth2, sx, sy)) if path == "shifted" else (bgr2, depth2)
    if path == "plain":
        d.upload_frame(0, bgr2, depth2)
    elif path == "shifted":
        d.upload_frame_shifted(0, bgr2, depth2, sx, sy)
    elif path == "staged":
        d.stage_reserve(0, 1)
        d.stage_rows(0, bgr2, depth2, 0, 0, 0, scene.h)
        d.upload_staged(0)
    else:
        fb = scene.w * scene.h * 5
        pb = lm.PinnedBuffer(fb)
        pb.view(np.uint8, (scene.h, scene.w, 3), 0)[:] = bgr2
        pb.view(np.uint16, (scene.h, scene.w), scene.w * scene.h * 3)[:] = depth2
        d.upload_frames_pinned(0, 1, pb.ptr.value, fb)
    try:
        got = d.match_slot(0, THR).copy()
    finally:
        if path == "pinned":
            pb.close([d])
    ref2 = scene.mask(key, frame2)
    assert (ref2 == 0).any() and (ref2 == 255).any() and not np.array_equal(ref2, scene.mask(key))
    scene.upload(e, 1, frame2)
    scene.upload_ref_mask(e, 1, key, frame2)
    assert _same(got, e.match_slot(1, THR))                     # the rule of the NEW frame, and no uploaded mask any more
    assert scene.quant(d, 0) == scene.quant(e, 1)
    # clearing the rule restores the unmasked lists
    d.clear_mask_rule(0, 1)
    scene.upload(e, 0, frame2)
    assert _same(d.match_slot(0, THR), e.match_slot(0, THR))
    d.close()
    e.close()


# ---- refusals and interference ---------------------------------------------------------------------------
def test_refusals(lm, scene):
    d = scene.detector(lm, slots=4)
    ok = dict(modalities=3, depth_range=(600, 800), grow=16, rect=(0, 0, scene.w, scene.h))
    d.set_mask_rule(0, 4, rule=_rule(lm, ok))
    d.clear_mask_rule()
    for bad in (dict(ok, grow=17), dict(ok, grow=-1), dict(ok, depth_range=(801, 800)), dict(ok, modalities=0), dict(ok, modalities=4),
                dict(ok, rect=(1, 0, scene.w, scene.h)), dict(ok, rect=(0, 1, scene.w, scene.h)), dict(ok, rect=(-1, 0, 10, 10)),
                dict(ok, rect=(0, 0, 0, 10)), dict(ok, rect=(scene.w, 0, 1, 1))):
        with pytest.raises(lm.LinemodError) as ex:
            d.set_mask_rule(0, 1, rule=_rule(lm, bad))
        assert ex.value.code == lm.LM_ERR_INVALID, bad
        assert d.mask_rule(0) is None
        with pytest.raises(lm.LinemodError):
            d.stage_mask_rule(scene.bgr, scene.depth, _rule(lm, bad))
    with pytest.raises(lm.LinemodError):
        d.set_mask_rule(3, 2, rule=_rule(lm, ok))               # slot range past the end
    # busy slots
    for i in range(2):
        scene.upload(d, i)
    d.match_begin(1, 0, 2, THR, -1)
    with pytest.raises(lm.LinemodError) as ex:
        d.set_mask_rule(1, 1, rule=_rule(lm, ok))
    assert ex.value.code == lm.LM_ERR_INVALID
    with pytest.raises(lm.LinemodError):
        d.set_mask_rule(0, 4, rule=_rule(lm, ok))
    d.set_mask_rule(2, 2, rule=_rule(lm, ok))                   # (slots outside the lane's range are free)
    d.match_end(1, n_slots=2)
    with pytest.raises(lm.LinemodError):
        d.clear_mask_rule(0, 5)
    d.close()
    # a depth gate on a colour-only detector, and the depth modality named there
    c = lm.Detector(color_only=True, frame_slots=1)
    for bad in (dict(modalities=1, depth_range=(600, 800)), dict(modalities=2), dict(modalities=3)):
        with pytest.raises(lm.LinemodError) as ex:
            c.set_mask_rule(0, 1, rule=_rule(lm, bad))
        assert ex.value.code == lm.LM_ERR_INVALID
    c.set_mask_rule(0, 1, rule=_rule(lm, dict(modalities=1, hsv_range=([0, 0, 0], [255, 150, 255]))))
    c.close()


def test_a_detector_without_rules_is_unchanged(lm, scene, plain):
    d = scene.detector(lm, slots=16)
    for i in range(16):
        scene.upload(d, i)
    out, cnt = d.match_batch(16, THR, -1, cap_per_frame=8192)        # never ruled: the level-fused launches
    for i in range(16):
        assert _same(out[i, :cnt[i]], plain), i
    d.set_mask_rule(0, 16, rule=_rule(lm, scene.rules["depth"]))
    out2, cnt2 = d.match_batch(16, THR, -1, cap_per_frame=8192)
    assert cnt2[0] != cnt[0] or not _same(out2[0, :cnt2[0]], plain)
    d.clear_mask_rule()
    assert all(d.mask_rule(i) is None for i in range(16))
    out3, cnt3 = d.match_batch(16, THR, -1, cap_per_frame=8192)
    for i in range(16):
        assert _same(out3[i, :cnt3[i]], plain), i
    d.close()


# ---- C++ facade (tests/cpp/match_gate_facade.cpp) ------------------------------------------------------------
def test_facade_match_gate_equals_host_masks_in_every_form(lm, frame0, tmp_path):
    """setMatchGate (depth range around the part, grow 8, the class's colour range) on frame0: detect(), detectBatch and the streamed
    form give the same poses, the ones detect() gives for the reference's mask passed through the masks overload.  RGB-D templates
    rendered from the mesh (a depth gate needs the depth modality) at detector threshold 55: the gate confines the match to the part's
    surroundings, where that threshold leaves the rendered templates room against the sensor's depth normals."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "lagergehaeuse.npz"))
    bgr, depth = frame0
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(np.array([len(g["vertices"]), len(g["faces"])], np.uint32).tobytes())
        fh.write(g["vertices"].astype(np.float32).tobytes())
        fh.write(g["faces"].astype(np.int32).tobytes())
    bgr.tofile(tmp_path / "bgr.raw")
    depth.tofile(tmp_path / "depth.raw")
    z = float(g["gt_position"][2])
    zmin, zmax = int(z) - 60, int(z) + 70                       # the part is 54 mm across
    spec = dict(modalities=3, depth_range=(zmin, zmax), hsv_range=(g["lower_color_range"][:3], g["upper_color_range"][:3]), grow=8)
    mask = mrr.mask_of(spec, bgr, depth)
    assert (mask == 0).any() and (mask == 255).any()
    mask.tofile(tmp_path / "mask.raw")
    host = os.path.join(ROOT, "line-mod-pipeline_amd", "host")
    libdir = os.path.dirname(lm.LIB_PATH)
    exe = str(tmp_path / "match_gate_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "match_gate_facade.cpp"),
                           os.path.join(host, "HighLevelLinemod.cpp"), os.path.join(host, "PoseDetection.cpp"),
                           os.path.join(host, "PostProcess.cpp"), os.path.join(host, "TemplateGenerator.cpp"),
                           "-L" + libdir, "-llinemod_hip", "-lpthread", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, "mesh.bin", "bgr.raw", "depth.raw", "mask.raw", str(zmin), str(zmax), "55", "3"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    runs = {}
    for line in r.stdout.splitlines():
        if line.startswith(("pose ", "none ")):
            parts = line.split()
            runs.setdefault(parts[1], []).append(" ".join(parts[2:]))
    lines = r.stdout.splitlines()
    assert any(l.startswith("batch 1") for l in lines) and any(l.startswith("stream 1 1 1 1") for l in lines), r.stdout[-2000:]
    want = runs["masked"]
    assert any(l.startswith("pose masked") for l in lines), r.stdout[-2000:]     # the gate keeps the part: there is a pose to compare
    for run in ("detect", "detect_again", "batch0", "batch1", "batch2", "stream0_0", "stream0_1", "stream1_0"):
        assert runs[run] == want, (run, r.stdout[-3000:])
    assert any(l.startswith("refused 'mask rule: grow out of range") and l.endswith("poses 0") for l in lines), r.stdout[-2000:]
