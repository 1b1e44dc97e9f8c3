"""Detector::match's per-modality masks on the GPU (lm_match_masked, lm_upload_match_mask, k_match_mask): the quantised images of a
masked slot equal the oracle's ANDed with the mask pyramid, and the lists of masked frames equal the independent numpy reference
(tests/masked_reference.py) on those images -- through every scan form, the byte scan, mixed and split batches, prepared calls,
lanes and the gathered path."""
import socket

import numpy as np
import pytest

import masked_reference as mr
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

THR = 75.0


def _T(M, L):
    return ([5] if M == 2 else [2]) + [8] * (L - 1)


def _oracle_quant(orc, bgr, depth, M, T):
    o = orc.Detector(color_only=(M == 1), T=T)
    o.prepare(bgr, depth if M == 2 else None)
    q = {(l, m): o.stage(0, l, m).reshape(bgr.shape[0] >> l, bgr.shape[1] >> l) for l in range(len(T)) for m in range(M)}
    o.close()
    return q


def _stripes(h, w, kind):
    yy, xx = np.mgrid[0:h, 0:w]
    return {"xstripe": (xx % 2 == 0), "ystripe": (yy % 2 == 1), "checker": ((xx + yy) % 2 == 0),
            "xstripe_odd": (xx % 2 == 1), "checker4": (((xx >> 2) + (yy >> 2)) % 2 == 1)}[kind].astype(np.uint8) * 255


def _blobs(h, w, seed, n=6):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(n):
        cx, cy, r = rng.integers(0, w), rng.integers(0, h), rng.integers(h // 10, h // 3)
        m |= (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
    return m.astype(np.uint8) * np.uint8(rng.integers(1, 256))


# ---- stage equality -------------------------------------------------------------------------------
@pytest.mark.parametrize("M,L", [(2, 2), (1, 2), (2, 1), (2, 3), (1, 3)])
def test_masked_quantised_images_equal_oracle_and_mask_pyramid(lm, orc, frame0, M, L):
    bgr, depth = frame0
    h, w = bgr.shape[:2]
    T = _T(M, L)
    q = _oracle_quant(orc, bgr, depth, M, T)
    d = lm.Detector(color_only=(M == 1), T=T, frame_slots=2)
    for kc, kd in (("xstripe", "ystripe"), ("checker", "xstripe_odd"), ("checker4", "checker")):
        cm, dm = _stripes(h, w, kc), _stripes(h, w, kd)
        for slot in (0, 1):
            d.upload_frame(slot, bgr, depth if M == 2 else None)
        d.upload_match_mask(0, cm, modality=0)
        if M == 2:
            d.upload_match_mask(0, dm, modality=1)
        d.upload_match_mask(1, cm, modality=-1)
        for slot in (0, 1):
            d.prepare_slot(slot)
        exp0 = mr.masked_pyramid(q, [cm, dm] if M == 2 else [cm], L, M, orc)
        exp1 = mr.masked_pyramid(q, [cm, cm] if M == 2 else [cm], L, M, orc)
        for l in range(L):
            for m in range(M):
                assert np.array_equal(d.debug_read(0, 0, l, m).reshape(h >> l, w >> l), exp0[(l, m)]), (kc, l, m)
                assert np.array_equal(d.debug_read(1, 0, l, m).reshape(h >> l, w >> l), exp1[(l, m)]), (kc, l, m)
    d.close()


# ---- lists --------------------------------------------------------------------------------------
class _Scene:
    """A frame, its oracle pyramid, a bank with crop templates and expected lists per mask pair (computed once)."""

    def __init__(self, orc, synth, bgr, depth, M=2, n_classes=2):
        self.orc, self.bgr, self.depth, self.M = orc, bgr, depth, M
        self.h, self.w = bgr.shape[:2]
        self.T = _T(M, 2)
        self.q = _oracle_quant(orc, bgr, depth, M, self.T)
        self.classes = []
        for k in range(n_classes):
            descs, feats, _ = synth.make_bank(10, M, 2, seed=40 + k, quantized=self.q, crop_fraction=0.4, frame_size=(self.w, self.h),
                                              T0=self.T[0])
            self.classes.append((descs, feats))
        self.cache = {}
        top = self.expected(None)[0]
        tw, th = int(self.classes[top["class_idx"]][0][top["template_id"] * 2 * M]["width"]), \
            int(self.classes[top["class_idx"]][0][top["template_id"] * 2 * M]["height"])
        roi = np.zeros((self.h, self.w), np.uint8)
        roi[max(top["y"] - 24, 0):top["y"] + th + 24, max(top["x"] - 24, 0):top["x"] + tw + 24] = 1
        self.masks = {"roi": (roi, roi if M == 2 else None), "blobs": (_blobs(self.h, self.w, 3), _blobs(self.h, self.w, 3) if M == 2 else None)}
        if M == 2:
            self.masks["pair"] = (_blobs(self.h, self.w, 5, n=10), roi)

    def detector(self, lm, slots=8, **kw):
        d = lm.Detector(color_only=(self.M == 1), width=self.w, height=self.h, frame_slots=slots, **kw)
        for k, (descs, feats) in enumerate(self.classes):
            d.add_class("m%d" % k, descs, feats)
        return d

    def expected(self, key, class_idx=-1):
        if (key, class_idx) not in self.cache:
            quant = self.q if key is None else mr.masked_pyramid(self.q, list(self.masks[key]), 2, self.M, self.orc)
            self.cache[(key, class_idx)] = mr.match(self.orc, quant, self.classes, self.T, THR, class_idx=class_idx)
        return self.cache[(key, class_idx)]

    def upload(self, d, slot, key):
        d.upload_frame(slot, self.bgr, self.depth if self.M == 2 else None)
        if key is not None:
            cm, dm = self.masks[key]
            d.upload_match_mask(slot, cm, modality=0)
            if dm is not None:
                d.upload_match_mask(slot, dm, modality=1)


@pytest.fixture(scope="module")
def scene(orc, synth, frame0):
    s = _Scene(orc, synth, *frame0)
    assert len(s.expected(None)) > 0
    for k in s.masks:
        e = s.expected(k)
        assert 0 < len(e) < len(s.expected(None)), k          # the masks remove matches, and keep some
    return s


@pytest.fixture(scope="module")
def scene_color(orc, synth, frame0):
    return _Scene(orc, synth, frame0[0], None, M=1)


def test_all_ones_and_all_zero_masks(lm, scene):
    d = scene.detector(lm)
    plain = d.match(scene.bgr, scene.depth, THR)
    assert_matches_equal(plain, scene.expected(None))
    ones = np.full((scene.h, scene.w), 7, np.uint8)
    assert_matches_equal(d.match(scene.bgr, scene.depth, THR, masks=ones), plain)
    assert_matches_equal(d.match(scene.bgr, scene.depth, THR, masks=(ones, None)), plain)
    assert len(d.match(scene.bgr, scene.depth, THR, masks=np.zeros((scene.h, scene.w), np.uint8))) == 0
    d.close()


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_masked_lists_every_scan_form(lm, scene, form):
    """Single frames (lm_match_masked, the few-frame kernels) and a 16-frame batch (the batch kernels) of masked frames, with the
    scan form forced (1 k_scan4, 2 k_scan1, 3 k_scanl) or by cost (0)."""
    d = scene.detector(lm, slots=16)
    d.set_tuning(lm.TUNE_SCAN_FORM, form)
    for key in scene.masks:
        assert_matches_equal(d.match(scene.bgr, scene.depth, THR, masks=scene.masks[key]), scene.expected(key))
    keys = list(scene.masks) + [None]
    for i in range(16):
        scene.upload(d, i, keys[i % len(keys)])
    out, cnt = d.match_batch(16, THR, -1, cap_per_frame=8192)
    for i in range(16):
        assert_matches_equal(out[i, :cnt[i]], scene.expected(keys[i % len(keys)]))
    d.close()


def test_masked_lists_colour_only(lm, scene_color):
    s = scene_color
    d = s.detector(lm, slots=16)
    for key in s.masks:
        assert_matches_equal(d.match(s.bgr, None, THR, masks=s.masks[key][0]), s.expected(key))
    keys = list(s.masks) + [None]
    for i in range(16):
        s.upload(d, i, keys[i % len(keys)])
    out, cnt = d.match_batch(16, THR, -1, cap_per_frame=8192)
    for i in range(16):
        assert_matches_equal(out[i, :cnt[i]], s.expected(keys[i % len(keys)]))
    d.close()


def test_masked_lists_byte_scan(lm, scene):
    d = scene.detector(lm, flags=lm.FLAG_BYTE_RESPONSES)
    for key in scene.masks:
        assert_matches_equal(d.match(scene.bgr, scene.depth, THR, masks=scene.masks[key]), scene.expected(key))
    d.close()


def test_masked_lists_large_frames(lm, orc, synth):
    """1280 x 960: the unfused route's batch kernels already for four frames (a frame counts as four VGA frames)."""
    s = _Scene(orc, synth, *synth.make_frame(1280, 960, seed=77), n_classes=1)
    d = s.detector(lm, slots=4)
    keys = ["roi", None, "pair", "blobs"]
    for i, k in enumerate(keys):
        s.upload(d, i, k)
    out, cnt = d.match_batch(4, THR, -1, cap_per_frame=8192)
    for i, k in enumerate(keys):
        assert_matches_equal(out[i, :cnt[i]], s.expected(k))
    d.close()


# ---- mixed, split and prepared calls ------------------------------------------------------------
def test_mixed_batch_and_lanes(lm, scene):
    d = scene.detector(lm, slots=8)
    keys = ["roi", None, "pair", None, "blobs", "roi"]
    for i, k in enumerate(keys):
        scene.upload(d, i, k)
    out, cnt = d.match_batch(6, THR, -1)
    for i, k in enumerate(keys):
        assert_matches_equal(out[i, :cnt[i]], scene.expected(k))
    # the same six frames split over three lanes (the slots keep frames and masks: they are pre-processed again)
    for lane in range(3):
        d.match_begin(lane, 2 * lane, 2, THR, -1)
    for lane in range(3):
        out, cnt = d.match_end(lane, n_slots=2)
        for j in range(2):
            assert_matches_equal(out[j, :cnt[j]], scene.expected(keys[2 * lane + j]))
    d.close()


def test_prepared_class_list_before_and_after_a_mask_change(lm, scene):
    d = scene.detector(lm, slots=2)
    scene.upload(d, 0, "roi")
    out, cnt = d.match_batch_classes(0, 1, THR, [0, 1])
    assert_matches_equal(out[0, :cnt[0]], scene.expected("roi"))
    out, cnt = d.match_prepared(0, 1, THR, [1])
    assert_matches_equal(out[0, :cnt[0]], scene.expected("roi", class_idx=1))
    cm, dm = scene.masks["pair"]
    d.upload_match_mask(0, cm, modality=0)
    d.upload_match_mask(0, dm, modality=1)
    with pytest.raises(lm.LinemodError):          # a mask change makes the slot's a3-a10 results stale
        d.match_prepared(0, 1, THR, [1])
    out, cnt = d.match_batch_classes(0, 1, THR, [0, 1])
    assert_matches_equal(out[0, :cnt[0]], scene.expected("pair"))
    out, cnt = d.match_prepared(0, 1, THR, [1])
    assert_matches_equal(out[0, :cnt[0]], scene.expected("pair", class_idx=1))
    # clearing both masks: the unmasked lists again
    d.upload_match_mask(0, None, modality=-1)
    out, cnt = d.match_batch_classes(0, 1, THR, [0, 1])
    assert_matches_equal(out[0, :cnt[0]], scene.expected(None))
    d.close()


# ---- lifecycle ----------------------------------------------------------------------------------
def test_frame_upload_clears_the_mask_and_busy_slots_refuse_masks(lm, scene):
    d = scene.detector(lm, slots=4)
    scene.upload(d, 0, "roi")
    assert_matches_equal(d.match_slot(0, THR), scene.expected("roi"))
    d.upload_frame(0, scene.bgr, scene.depth)                         # the new frame has no mask
    assert_matches_equal(d.match_slot(0, THR), scene.expected(None))
    scene.upload(d, 1, "blobs")
    d.match_begin(1, 0, 2, THR, -1)
    with pytest.raises(lm.LinemodError):
        d.upload_match_mask(1, scene.masks["roi"][0], modality=0)
    with pytest.raises(lm.LinemodError):
        d.upload_match_mask(0, None)
    out, cnt = d.match_end(1, n_slots=2)
    assert_matches_equal(out[0, :cnt[0]], scene.expected(None))
    assert_matches_equal(out[1, :cnt[1]], scene.expected("blobs"))
    with pytest.raises(lm.LinemodError):                              # modality out of range
        d.upload_match_mask(0, scene.masks["roi"][0], modality=2)
    d.close()


def test_masked_lanes_twenty_rounds(lm, scene):
    """A fresh detector, three lanes, frames and masks uploaded again every round behind the previous round's ends."""
    d = scene.detector(lm, slots=12)
    keys = list(scene.masks) + [None]
    for rnd in range(20):
        plan = {}
        for lane in range(3):
            first = 4 * lane
            for j in range(4):
                k = keys[(rnd + lane + j) % len(keys)]
                scene.upload(d, first + j, k)
                plan[first + j] = k
            d.match_begin(lane, first, 4, THR, -1)
        for lane in range(3):
            out, cnt = d.match_end(lane, n_slots=4)
            for j in range(4):
                assert_matches_equal(out[j, :cnt[j]], scene.expected(plan[4 * lane + j]))
    d.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_gathered_one_rank(lm, scene):
    d = scene.detector(lm, slots=4)
    d.comm_init(0, 1, "127.0.0.1", _free_port())
    keys = ["pair", None, "roi", "blobs"]
    for i, k in enumerate(keys):
        scene.upload(d, i, k)
    out = np.zeros(1 << 16, lm.MATCH_DTYPE)
    cnt = np.zeros(4, np.int32)
    d.match_begin_gathered(0, 0, 4, THR, -1)
    f0, nf, tot = d.match_end_gathered(0, out, cnt)
    assert (f0, nf) == (0, 4)
    pos = 0
    for i, k in enumerate(keys):
        assert_matches_equal(out[pos:pos + cnt[i]], scene.expected(k))
        pos += cnt[i]
    d.comm_destroy()
    d.close()


def test_masked_quantised_images_narrow_levels(lm, orc, synth):
    """720 x 480: level 1 is 360 pixels wide, not a multiple of 16, so k_match_mask takes its per-byte form at every level."""
    bgr, depth = synth.make_frame(720, 480, seed=9)
    h, w = bgr.shape[:2]
    for M in (2, 1):
        T = _T(M, 2)
        q = _oracle_quant(orc, bgr, depth, M, T)
        d = lm.Detector(color_only=(M == 1), width=w, height=h, T=T, frame_slots=1)
        for kc, kd in (("xstripe", "ystripe"), ("checker", "checker4")):
            cm, dm = _stripes(h, w, kc), _stripes(h, w, kd)
            d.upload_frame(0, bgr, depth if M == 2 else None)
            d.upload_match_mask(0, cm, modality=0)
            if M == 2:
                d.upload_match_mask(0, dm, modality=1)
            d.prepare_slot(0)
            exp = mr.masked_pyramid(q, [cm, dm] if M == 2 else [cm], 2, M, orc)
            for l in range(2):
                for m in range(M):
                    assert np.array_equal(d.debug_read(0, 0, l, m).reshape(h >> l, w >> l), exp[(l, m)]), (M, kc, l, m)
        d.close()


def test_pinned_and_staged_uploads_clear_the_mask(lm, scene):
    d = scene.detector(lm, slots=4)
    fb = scene.w * scene.h * 5
    pb = lm.PinnedBuffer(2 * fb)
    try:
        for i in range(2):
            pb.view(np.uint8, (scene.h, scene.w, 3), i * fb)[:] = scene.bgr
            pb.view(np.uint16, (scene.h, scene.w), i * fb + scene.w * scene.h * 3)[:] = scene.depth
        for i in range(2):
            scene.upload(d, i, "roi")
        out, cnt = d.match_batch(2, THR, -1)
        for i in range(2):
            assert_matches_equal(out[i, :cnt[i]], scene.expected("roi"))
        d.upload_frames_pinned(0, 2, pb.ptr.value, fb)
        out, cnt = d.match_batch(2, THR, -1)
        for i in range(2):
            assert_matches_equal(out[i, :cnt[i]], scene.expected(None))
    finally:
        pb.close([d])
    scene.upload(d, 2, "blobs")
    assert_matches_equal(d.match_slot(2, THR), scene.expected("blobs"))
    d.stage_reserve(2, 1)
    d.stage_rows(2, scene.bgr, scene.depth, 0, 0, 0, scene.h)
    d.upload_staged(2)
    assert_matches_equal(d.match_slot(2, THR), scene.expected(None))
    # a mask change drops the slot's last lists (they belong to the old mask)
    d.upload_match_mask(2, scene.masks["roi"][0], modality=0)
    with pytest.raises(lm.LinemodError):
        d.match_collect(2, 1)
    d.close()


def test_python_masks_of_any_dtype_keep_nonzero_pixels(lm, scene):
    d = scene.detector(lm)
    roi = scene.masks["roi"][0]
    exp = scene.expected("roi")
    for m in (roi.astype(np.int32) * 256, roi.astype(np.float32) * 0.5, roi.astype(bool)):
        assert_matches_equal(d.match(scene.bgr, scene.depth, THR, masks=m), exp)
    d.close()


# ---- C++ facade (tests/cpp/masks_facade.cpp) -------------------------------------------------------
@pytest.fixture(scope="module")
def facade_exe(lm, tmp_path_factory):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "line-mod-pipeline_amd", "host")
    libdir = os.path.dirname(lm.LIB_PATH)
    exe = str(tmp_path_factory.mktemp("masks_facade") / "masks_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(root, "tests", "cpp", "masks_facade.cpp"),
                           os.path.join(host, "HighLevelLinemod.cpp"), os.path.join(host, "PoseDetection.cpp"),
                           os.path.join(host, "PostProcess.cpp"), os.path.join(host, "TemplateGenerator.cpp"),
                           "-L" + libdir, "-llinemod_hip", "-Wl,-rpath," + libdir])
    return exe


def test_facade_detect_template_with_masks(lm, frame0, golden0, facade_exe, tmp_path):
    import subprocess
    bgr, depth = frame0
    h, w = bgr.shape[:2]
    det = lm.Detector(color_only=False)
    det.add_class("lagergehaeuse.ply", golden0["rgbd_descs"], golden0["rgbd_features"])
    det.save_yaml(tmp_path / "linemod_templates.yml.gz")
    bgr.tofile(tmp_path / "bgr.raw")
    depth.tofile(tmp_path / "depth.raw")
    cm = _blobs(h, w, 11, n=12)
    dm = np.zeros((h, w), np.uint8)
    dm[150:420, 180:520] = 1
    cm.tofile(tmp_path / "cm.raw")
    dm.tofile(tmp_path / "dm.raw")
    for cmf, dmf, masks in (("cm.raw", "dm.raw", (cm, dm)), ("cm.raw", "-", (cm, None)), ("-", "-", None)):
        r = subprocess.run([facade_exe, "match", "0", "bgr.raw", "depth.raw", cmf, dmf, "80"], cwd=tmp_path, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("match ")]
        got = np.array([(int(a), int(b), np.float32(c), int(t), int(k)) for a, b, c, t, k in rows], lm.MATCH_DTYPE)
        exp = det.match(bgr, depth, 80.0, class_idx=0, masks=masks)
        assert len(exp) > 0 or masks is not None
        assert_matches_equal(got, exp)
    det.close()


def test_facade_pose_detection_with_masks(lm, frame0, facade_exe, tmp_path):
    """PoseDetection::detect with a mask in camera coordinates, the principal point shifting the frame by 60 pixels: a mask covering
    the object gives the unmasked pose, and under its complement no pose lies on the object -- the frame's weaker detections
    elsewhere may remain.  A mask shifted the wrong way (120 pixels off) or not at all would leave the object visible."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = np.load(os.path.join(root, "tests", "golden", "lagergehaeuse.npz"))
    bgr, depth = frame0
    with open(tmp_path / "mesh.bin", "wb") as fh:
        fh.write(np.array([len(g["vertices"]), len(g["faces"])], np.uint32).tobytes())
        fh.write(g["vertices"].astype(np.float32).tobytes())
        fh.write(g["faces"].astype(np.int32).tobytes())
    bgr.tofile(tmp_path / "bgr.raw")
    depth.tofile(tmp_path / "depth.raw")
    r = subprocess.run([facade_exe, "pose", "mesh.bin", "bgr.raw", "depth.raw", "60", "32"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    first = {}
    for l in lines:
        if l.startswith(("pose ", "none ")):
            first.setdefault(l.split()[1], l)
    assert first["plain"].startswith("pose "), r.stdout[-2000:]
    assert first["cover"].replace("cover", "plain") == first["plain"], r.stdout[-2000:]
    bb = [int(v) for v in first["plain"].split()[-4:]]                      # the object's box (translated frame)
    excluded = [[int(v) for v in l.split()[-4:]] for l in lines if l.startswith("pose exclude")]
    def overlaps(b):
        x, y, w, h = b
        return not (x + w <= bb[0] or bb[0] + bb[2] <= x or y + h <= bb[1] or bb[1] + bb[3] <= y)
    assert not any(overlaps(b) for b in excluded), r.stdout[-2000:]                         # no pose on the object
    misplaced = [[int(v) for v in l.split()[-4:]] for l in lines if l.startswith("pose misplaced")]
    assert any(overlaps(b) for b in misplaced), r.stdout[-2000:]                            # ... which a wrong-way shift would leave
