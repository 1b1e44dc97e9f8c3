"""LM_FLAG_KEEP_DEPTH on the GPU (ABI 0.13 additive): a colour-only detector that keeps the depth frame (K) beside a
plain colour-only one (C) and an RGB-D one (R), all at 160 x 80 with two levels (tests/keep_depth_scene.py).  The feature adds no kernel:
  - every upload and ingest form leaves in K's depth plane the bytes the same call leaves in R's, and in K's colour plane C's;
  - the depth consumers (counts, the sorted selection, a mask rule's depth gate, the ICP refinement and verification) give on K the
    bytes they give on R, and what the existing numpy references give;
  - the colour-only match beside the depth frame returns C's lists from C's quantised images and linear memories with C's launch counts;
  - a slot whose frame came without depth refuses the depth consumers, naming the slot, until an upload with depth restores them;
  - C refuses what it refused, in the same words, and R with the flag behaves as R."""
import numpy as np
import pytest

import depth_select_cases as DS
import keep_depth_scene as S
import mask_rule_reference as mrr

pytestmark = pytest.mark.gpu

W, H, THR = S.W, S.H, S.THRESHOLD
SHIFTS = [(0, 0), (7, -5)]
INVALID = 1
NSLOTS = 16


@pytest.fixture(scope="module")
def trio(lm, orc):
    """K, C, R with their banks; the window and a second depth image."""
    bgr, depth = S.frame()
    K = lm.Detector(color_only=True, keep_depth=True, width=W, height=H, T=S.T, frame_slots=NSLOTS)
    Cd = lm.Detector(color_only=True, width=W, height=H, T=S.T, frame_slots=NSLOTS)
    R = lm.Detector(color_only=False, width=W, height=H, frame_slots=NSLOTS)
    assert (K.keeps_depth, Cd.keeps_depth, R.keeps_depth) == (True, False, True) and (K.num_modalities, Cd.num_modalities, R.num_modalities) == (1, 1, 2)
    for name, descs, feats in S.bank(orc):
        K.add_class(name, descs, feats)
        Cd.add_class(name, descs, feats)
    R.add_class(*S.bank_rgbd(orc))
    o = orc.Detector(color_only=True, T=S.T)
    for name, descs, feats in S.bank(orc):
        o.add_class(name, descs, feats)
    assert len(o.match(bgr, None, THR)) == 23          # the scene is not empty: what the parity tests compare are real lists
    o.close()
    yield K, Cd, R, bgr, depth
    for d in (K, Cd, R):
        d.close()


def refused(lm, call, *words):
    with pytest.raises(lm.LinemodError) as e:
        call()
    assert e.value.code == INVALID, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def depth_consumers(lm, d, slot):
    """Calls that read the depth plane of `slot`, cheapest first (the ICP ones are test_icp_on_k_gives_r_bytes')."""
    sq = np.array([(0, 0, 8, 8, 12, slot)], lm.DEPTH_SELECT_QUERY_DTYPE)
    cq = np.array([(0, 0, 8, 8, 100, 900, slot, 0)], lm.DEPTH_QUERY_DTYPE)
    return [lambda: d.depth_select(sq), lambda: d.depth_counts(cq), lambda: d.time_depth_select(sq), lambda: d.read_frame(slot)]


# ---- 1. every upload form ----------------------------------------------------------------------------------
class Pinned:
    """[colour | depth] contiguous in one pinned block, and the two apart in a second one."""

    def __init__(self, lm, bgr, depth):
        self.lm = lm
        cb = W * H * 3
        self.pair = lm.PinnedBuffer(W * H * 5)
        self.apart = lm.PinnedBuffer(W * H * 5 + 4096)
        self.bgr, self.depth = self.pair.view(np.uint8, (H, W, 3)), self.pair.view(np.uint16, (H, W), offset=cb)
        self.bgr2, self.depth2 = self.apart.view(np.uint8, (H, W, 3)), self.apart.view(np.uint16, (H, W), offset=cb + 4096)
        for b, dd in ((self.bgr, self.depth), (self.bgr2, self.depth2)):
            b[...] = bgr
            dd[...] = depth

    def close(self, dets):
        self.pair.close(dets)
        self.apart.close(dets)


def _staged(d, slot, bgr, depth, sx, sy):
    d.stage_reserve(slot, 1)
    for r0, r1 in ((0, 33), (33, 34), (34, H)):           # three row ranges, as a pool of threads would fill them
        d.stage_rows(slot, bgr, depth, sx, sy, r0, r1)
    d.upload_staged(slot)


def _forms(lm, pin):
    """name -> call(detector, slot, bgr, depth or None, shift): every form of the issue's section 2.  A form without a shift of its own
    is handed the images translated on the host, so every form leaves the same frame."""
    def host_shift(img, sh):
        return None if img is None else S.shifted(img, *sh)

    def pinned_fill(contiguous, bgr, depth, sh):
        b, dd = (pin.bgr, pin.depth) if contiguous else (pin.bgr2, pin.depth2)
        return b, (dd if depth is not None else None)

    def pinned(contiguous):
        def call(d, slot, bgr, depth, sh):
            b, dd = pinned_fill(contiguous, bgr, depth, sh)
            if sh == (0, 0):
                d.upload_frame_pinned(slot, b, dd)
            else:
                d.upload_frame_pinned_shifted(slot, b, dd, *sh)
            d.upload_wait(slot)
        return call

    def matched(kind):
        def call(d, slot, bgr, depth, sh):
            assert slot == 0
            b, dd = host_shift(bgr, sh), host_shift(depth, sh)
            if d.num_modalities == 2 and dd is None:
                return
            thr = 99.0
            if kind == "match":
                d.match(b, dd, thr)
            elif kind == "classes":
                d.match_classes(b, dd, thr, [0])
            else:
                d.match(b, dd, thr, masks=(np.full((H, W), 255, np.uint8), None))
        return call

    return {
        "upload_frame": lambda d, s, b, dd, sh: d.upload_frame(s, host_shift(b, sh), host_shift(dd, sh)),
        "upload_frame_shifted": lambda d, s, b, dd, sh: d.upload_frame_shifted(s, b, dd, *sh),
        "pinned_pair": pinned(True),
        "pinned_apart": pinned(False),
        "staged": lambda d, s, b, dd, sh: _staged(d, s, b, dd, *sh),
        "match": matched("match"),
        "match_classes": matched("classes"),
        "match_masked": matched("masked"),
    }


FORMS = ["upload_frame", "upload_frame_shifted", "pinned_pair", "pinned_apart", "staged", "match", "match_classes", "match_masked"]


@pytest.fixture(scope="module")
def pinned_frames(lm, trio):
    K, Cd, R, bgr, depth = trio
    p = Pinned(lm, bgr, depth)
    yield p
    p.close((K, Cd, R))


@pytest.mark.parametrize("shift", SHIFTS, ids=["shift00", "shift7m5"])
@pytest.mark.parametrize("form", FORMS)
def test_every_upload_form_with_and_without_depth(lm, trio, pinned_frames, form, shift):
    K, Cd, R, bgr, depth = trio
    call = _forms(lm, pinned_frames)[form]
    slot = 0 if form.startswith("match") else 3
    exp_b, exp_d = S.shifted(bgr, *shift), S.shifted(depth, *shift)
    # an earlier frame with ANOTHER depth image in all three: what the call must replace
    for d in (K, R):
        d.upload_frame(slot, bgr[::-1].copy(), S.other_depth())
    Cd.upload_frame(slot, bgr[::-1].copy())
    # with depth
    for d in (K, Cd, R):
        call(d, slot, bgr, depth, shift)
    kb, kd = K.read_frame(slot)
    cb, cd = Cd.read_frame(slot)
    rb, rd = R.read_frame(slot)
    assert cd is None and np.array_equal(kb, cb) and np.array_equal(cb, exp_b)
    assert kd.tobytes() == rd.tobytes() and np.array_equal(rd, exp_d) and (exp_d != S.shifted(S.other_depth(), *shift)).any()
    for consumer in depth_consumers(lm, K, slot):
        consumer()
    # without depth: the colour frame arrives, the depth consumers refuse the slot by its number
    flipped = np.ascontiguousarray(bgr[:, ::-1])
    if form.startswith("pinned"):
        pinned_frames.bgr[...] = flipped
        pinned_frames.bgr2[...] = flipped
    call(K, slot, flipped, None, shift)
    call(Cd, slot, flipped, None, shift)
    kb, none = K.read_frame(slot, depth=False)
    assert none is None and np.array_equal(kb, Cd.read_frame(slot)[0]) and np.array_equal(kb, S.shifted(flipped, *shift))
    for consumer in depth_consumers(lm, K, slot):
        refused(lm, consumer, "slot %d" % slot, "without a depth image")
    refused(lm, lambda: K.icp_refine(slot, (10, 10, 40, 40), 0, np.eye(4)[None], (1044.87, 1045.69141, 80.0, 40.0)), "slot %d" % slot)
    # the plane's bytes were left alone, and a later upload with depth restores the consumers
    if form.startswith("pinned"):
        pinned_frames.bgr[...] = bgr
        pinned_frames.bgr2[...] = bgr
    call(K, slot, bgr, depth, shift)
    kb, kd = K.read_frame(slot)
    assert np.array_equal(kb, exp_b) and kd.tobytes() == rd.tobytes()
    for consumer in depth_consumers(lm, K, slot):
        consumer()


def test_upload_frames_pinned_takes_the_rgbd_layout(lm, trio):
    """[colour dense | depth dense] per frame, three frames in one transfer at a frame stride with a gap: K's planes are R's, the colour C's
    (which takes the colour-only layout), and every slot of the run holds depth."""
    K, Cd, R, bgr, depth = trio
    n, fb, stride = 3, W * H * 5, W * H * 5 + 256
    pin, pin_c = lm.PinnedBuffer(stride * n), lm.PinnedBuffer(W * H * 3 * n)
    frames = [(np.roll(bgr, 11 * k, axis=1), np.roll(depth, 5 * k, axis=0)) for k in range(n)]
    for k, (b, dd) in enumerate(frames):
        pin.view(np.uint8, (H, W, 3), offset=k * stride)[...] = b
        pin.view(np.uint16, (H, W), offset=k * stride + W * H * 3)[...] = dd
        pin_c.view(np.uint8, (H, W, 3), offset=k * W * H * 3)[...] = b
    K.upload_frame(5, bgr)                                  # slot 5 holds no depth before the run
    for d in (K, R):
        d.upload_frames_pinned(4, n, pin.ptr.value, stride)
    Cd.upload_frames_pinned(4, n, pin_c.ptr.value)
    for k, (b, dd) in enumerate(frames):
        kb, kd = K.read_frame(4 + k)
        rb, rd = R.read_frame(4 + k)
        assert np.array_equal(kb, Cd.read_frame(4 + k)[0]) and np.array_equal(kb, b) and kd.tobytes() == rd.tobytes() and np.array_equal(kd, dd)
    refused(lm, lambda: K.upload_frames_pinned(4, n, pin.ptr.value, W * H * 3), "frame stride smaller than a frame")     # (5 bytes per pixel)
    pin.close((K, R))
    pin_c.close((Cd,))


# ---- 2. match parity K against C ---------------------------------------------------------------------------
def _planes(d, slot):
    """The quantised images of every level, the spread memory of the refinement level, the response memories of the scanned one."""
    return b"".join([d.debug_read(slot, 0, l, 0).tobytes() for l in range(2)] + [d.debug_read(slot, 1, 0, 0).tobytes(), d.debug_read(slot, 2, 1, 0).tobytes()])


def test_match_parity_with_the_plain_colour_only_detector(lm, trio):
    K, Cd, R, bgr, depth = trio
    frames = [S.shifted(bgr, 3 * k - 20, (k % 5) - 2) for k in range(NSLOTS)]
    got = {}
    for name, d in (("K", K), ("C", Cd)):
        d.set_profiling(True)
        c0 = d.get_stage_counts()
        f0 = d.get_scan_form_stats()
        lists = [d.match(bgr, depth if name == "K" else None, THR).copy()]
        planes = [_planes(d, 0)]
        for k, f in enumerate(frames):
            d.upload_frame(k, f, S.other_depth(k) if name == "K" else None)
        lists.append(d.match_slot(2, THR).copy())
        planes.append(_planes(d, 2))
        out, counts = d.match_batch(NSLOTS, THR)
        lists += [out[k, :counts[k]].copy() for k in range(NSLOTS)]
        planes += [_planes(d, k) for k in range(NSLOTS)]
        c1 = d.get_stage_counts()
        f1 = d.get_scan_form_stats()
        got[name] = (lists, planes, {k: c1[k] - c0[k] for k in c1}, (f1[0] - f0[0], f1[1] - f0[1], f1[3]))
        d.set_profiling(False)
    kl, kp, kc, kf = got["K"]
    cl, cp, cc, cf = got["C"]
    assert len(kl[0]) == 23 and sum(len(l) for l in kl[2:]) > 50
    for a, b in zip(kl, cl):
        assert len(a) == len(b) and a.tobytes() == b.tobytes()
    assert kp == cp
    assert kc == cc and kc["preprocess_frames"] == 2 + NSLOTS and kc["scan_launches"] >= 3
    assert kf == cf                                         # the planner chose the same scan forms and lane counts


# ---- 3. depth consumers on K against R and the numpy references ---------------------------------------------
PLACES = [(3, 1, 1, 1), (5, 3, 37, 1), (1, 5, 1, 29), (4, 6, 7, 5), (13, 6, 8, 5), (23, 6, 9, 5), (34, 6, 2, 2), (38, 6, 5, 1), (45, 6, 1, 5),
          (4, 14, 11, 13), (127, 40, 33, 40)]


def test_depth_counts_and_selection_on_k(lm, trio):
    """The crop families of tests/depth_select_cases.py -- the 1-pixel and all-equal crops among them, and an empty one -- on K and R:
    numpy's values, and the same bytes on both.  The counts against numpy's count of the same crops."""
    K, Cd, R, bgr, depth = trio
    names = sorted(DS.patterns(2, 2))
    rng = np.random.default_rng(11)
    frames, q, cq = [], [], []
    for slot, name in enumerate(names):
        f = rng.integers(0, 4000, (H, W)).astype(np.uint16)
        for (x, y, w, h) in PLACES:
            f[y:y + h, x:x + w] = DS.patterns(h, w, seed=slot)[name]
            q.append((x, y, x + w, y + h, (w * h) // 5, slot))
            cq.append((x, y, x + w, y + h, 500, 1300, slot, 0))
        q.append((0, 0, W, H, (W * H) // 5, slot))
        q.append((9, 9, 9, 30, 0, slot))                    # an empty crop: 65535
        cq.append((0, 0, W, H, 2, 0x00FF, slot, 0))
        frames.append(f)
    assert len(frames) <= NSLOTS
    q, cq = np.array(q, lm.DEPTH_SELECT_QUERY_DTYPE), np.array(cq, lm.DEPTH_QUERY_DTYPE)
    for d in (K, R):
        for slot, f in enumerate(frames):
            d.upload_frame(slot, bgr, f)
    exp = np.array([DS.rule(frames[e["slot"]][e["y0"]:e["y1"], e["x0"]:e["x1"]], e["rank"]) for e in q], np.uint16)
    gk, gr = K.depth_select(q), R.depth_select(q)
    assert gk.tobytes() == gr.tobytes() == exp.tobytes()
    assert (exp == 65535).any() and (exp == 1234).any() and (exp == 0x00FF).any() and (exp == 0x0100).any()
    below, inside = [], []
    for e in cq:
        t = frames[e["slot"]][e["y0"]:e["y1"], e["x0"]:e["x1"]].astype(np.int64)
        t = np.where(t <= 1, 65535, t)
        below.append(int((t < e["lo"]).sum()))
        inside.append(int(((t >= e["lo"]) & (t <= e["hi"])).sum()))
    kb, ki = K.depth_counts(cq)
    rb, ri = R.depth_counts(cq)
    assert kb.tolist() == rb.tolist() == below and ki.tolist() == ri.tolist() == inside and max(inside) > 100 and max(below) > 100
    assert K.time_depth_select(q) > 0.0
    refused(lm, lambda: Cd.depth_select(q[:1]), "keeps no depth frame on the device")


def test_rule_with_a_depth_gate_masks_the_colour_modality(lm, trio):
    """Depth gate + grow 2 + rectangle on modality 1 (colour): K's ruled match equals C's match with the numpy reference's mask uploaded --
    lists and quantised images; the mask hides real matches; a frame without depth refuses the match and names the slot."""
    K, Cd, R, bgr, depth = trio
    spec = dict(modalities=1, depth_range=(640, 700), keep_invalid=False, grow=2, rect=(20, 6, 120, 70))
    mask = mrr.mask_of(spec, bgr, depth)
    assert (mask == 0).sum() > 1000 and (mask == 255).sum() > 1000
    slot = 6
    for d in (K, Cd):
        d.clear_mask_rule()
    K.upload_frame(slot, bgr, depth)
    K.set_mask_rule(slot, 1, **spec)
    Cd.upload_frame(slot, bgr)
    Cd.upload_match_mask(slot, mask, modality=0)
    a, b = K.match_slot(slot, THR).copy(), Cd.match_slot(slot, THR).copy()
    assert len(a) == len(b) and a.tobytes() == b.tobytes() and 0 < len(a) < 23, (len(a), len(b))       # (tests/masked_reference.py on the oracle's images: 6)
    for l in range(2):
        assert K.debug_read(slot, 0, l, 0).tobytes() == Cd.debug_read(slot, 0, l, 0).tobytes()
    refused(lm, lambda: K.set_mask_rule(slot, 1, **dict(spec, modalities=3)), "modalities must name at least one modality the detector has")
    # the rule is sticky: the next frame comes without depth, and the match on the ruled slot is refused before anything runs
    for k in range(slot):
        K.upload_frame(k, bgr, depth)
    c0 = K.get_stage_counts()
    K.upload_frame(slot, bgr)
    refused(lm, lambda: K.match_slot(slot, THR), "slot %d" % slot, "without a depth image")
    refused(lm, lambda: K.match_batch(slot + 1, THR), "slot %d" % slot)
    refused(lm, lambda: K.match_begin(1, slot, 1, THR), "slot %d" % slot)
    assert K.get_stage_counts() == c0
    # the host-frame match on slot 0: the rule there is served by the call's own depth image, refused without one
    K.set_mask_rule(0, 1, **spec)
    Cd.upload_frame(0, bgr)
    c = K.match(bgr, depth, THR)
    Cd.upload_match_mask(0, mask, modality=0)
    assert c.tobytes() == Cd.match_slot(0, THR).tobytes()
    refused(lm, lambda: K.match(bgr, None, THR), "slot 0", "without a depth image")
    K.clear_mask_rule()
    Cd.upload_frame(0, bgr)
    assert len(K.match(bgr, None, THR)) == 23                       # without the rule a frame without depth matches as ever
    refused(lm, lambda: Cd.set_mask_rule(slot, 1, **spec), "colour-only")


# ---- 4. ICP on K against R (640 x 480: the golden frame) ------------------------------------------------------
def test_icp_on_k_gives_r_bytes(lm):
    import icp_fixtures as F
    import test_gpu_icp_batch as B
    import test_gpu_icp_verify as TV
    bgr, depth = F.frame0()
    V, Fc, xyzn, G = F.mesh_model()
    mesh = np.load(F.GOLDEN + "/lagergehaeuse.npz")
    frames = {0: depth, 2: B.shifted(depth, -6, 4), 5: B.shifted(depth, 3, -2)}
    slots = [0, 2, 0, 5, 0]
    boxes = [B.BOX_1712, B.BOX_2979, B.BOX_13, B.BOX_2979, B.BOX_1712]
    classes = [0, 3, 0, 0, 0]
    counts = [2, 1, 1, 1, 0]
    poses = np.stack([F.perturbed(G, 0, 3, [4, -6, 10]), F.perturbed(G, 1, -4, [-8, 5, 12]), F.perturbed(G, 2, 2, [3, 3, -8]),
                      F.perturbed(G, 2, 2, [3, -2, 4]), F.perturbed(G, 0, 2, [3, 4, -5])])
    names, vps = TV._view_projs(mesh)
    vslots = [(0, 2, 5)[i % 3] for i in range(9)]
    vk = [(i * 2) % 5 for i in range(9)]
    out = {}
    for name, kw in (("K", dict(color_only=True, keep_depth=True)), ("R", dict(color_only=False))):
        d = lm.Detector(frame_slots=8, **kw)
        d.icp_set_model(0, xyzn, 8)
        d.icp_set_model(3, xyzn, 16)
        d.set_render_mesh(0, mesh["vertices"], mesh["faces"])
        for s, f in frames.items():
            d.upload_frame(s, bgr, f)
        one = d.icp_refine(0, B.BOX_1712, 0, poses[:2], F.K0)
        many, status, rc = d.icp_refine_slots(slots, boxes, classes, poses, F.K0, counts=counts, return_status=True)
        assert rc == lm.LM_OK and (status[[0, 1, 3]] == lm.LM_OK).all()
        count, total, mean = d.icp_verify(vslots, None, 0, vps[vk])
        out[name] = (one.tobytes(), many.tobytes(), status.tobytes(), count.tobytes(), total.tobytes(), mean.tobytes())
        if name == "K":
            assert not np.array_equal(one, poses[:2]) and count.max() > 500          # the refinement moved the poses, the verification saw the part
            d.upload_frame(2, bgr)                                                    # slot 2 now holds a frame without depth
            refused(lm, lambda: d.icp_refine(2, B.BOX_2979, 0, poses[:1], F.K0), "slot 2", "without a depth image")
            refused(lm, lambda: d.icp_refine_slots(slots, boxes, classes, poses, F.K0, counts=counts), "slot 2")
            refused(lm, lambda: d.icp_verify(vslots, None, 0, vps[vk]), "slot 2")
            d.icp_refine(0, B.BOX_1712, 0, poses[:2], F.K0)                            # nothing stayed claimed
        d.close()
    assert out["K"] == out["R"]
    c = lm.Detector(color_only=True, frame_slots=8)
    c.icp_set_model(0, xyzn, 8)
    c.upload_frame(0, bgr)
    refused(lm, lambda: c.icp_refine(0, B.BOX_1712, 0, poses[:2], F.K0), "colour-only", "lm_stage_icp_refine_host")
    c.close()


# ---- 5. ingest on K ---------------------------------------------------------------------------------------
class Sources:
    def __init__(self, lm):
        self.lm, self.bufs = lm, []

    def put(self, host, pad=0):
        """A device copy of a [h, w] or [h, w, c] array whose rows are `pad` bytes longer than their pixels -> the view image_desc wants."""
        import rectify_scenes as RS_
        data, rs = RS_.lay_out(host, pad)
        buf = self.lm.DeviceBuffer(len(data))
        buf.upload(data)
        self.bufs.append(buf)
        strides = (rs, host.shape[2], 1) if host.ndim == 3 else (rs, host.dtype.itemsize)
        return buf.view(host.dtype.type, host.shape, 0, strides)

    def close(self):
        for b in self.bufs:
            b.close()


@pytest.fixture(scope="module")
def sources(lm, trio):
    s = Sources(lm)
    yield s
    trio[0].upload_wait(-1); trio[1].upload_wait(-1); trio[2].upload_wait(-1)
    s.close()


def to_cam(lm, c):
    return lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])


def ingest_case(lm, trio, frame, setup, colour_only_frame=None, slot=9):
    """The same ingest_frames call on K, R and C: K's depth plane is R's, K's colour is C's; then the call without its depth descriptor on K:
    the colour arrives, the slot holds no depth.  colour_only_frame: what C is handed where it refuses the route itself."""
    K, Cd, R, bgr, depth = trio
    for d in (K, Cd, R):
        setup(d)
        d.upload_frame(slot, bgr, S.other_depth() if d is not Cd else None)
    for d in (K, R):
        d.ingest_frames(slot, [frame])
    Cd.ingest_frames(slot, [colour_only_frame or frame])
    kb, kd = K.read_frame(slot)
    rb, rd = R.read_frame(slot)
    assert np.array_equal(kb, Cd.read_frame(slot)[0]) and np.array_equal(kb, rb)
    assert kd.tobytes() == rd.tobytes() and (kd != 0).sum() > 1000 and (kd != S.other_depth()).mean() > 0.9
    return kb, kd


def test_plain_ingest_u16_and_f32(lm, trio, sources):
    K, Cd, R, bgr, depth = trio
    rng = np.random.default_rng(21)
    col = sources.put(rng.integers(0, 256, (97, 203, 3), dtype=np.uint8), pad=3)
    d16 = sources.put(rng.integers(0, 65536, (97, 203), dtype=np.uint16), pad=2)
    f32 = rng.uniform(-50.0, 70000.0, (97, 203)).astype(np.float32)
    f32[rng.random(f32.shape) < 0.1] = np.nan
    d32 = sources.put(f32, pad=4)
    for dep, scale in ((d16, 1.0), (d32, 0.5)):
        frame = dict(colour=col, depth=dep, order="rgb", crop=(3, 2), depth_crop=(11, 5), depth_scale=scale, flip_x=True, shift=(7, -5))
        kb, _ = ingest_case(lm, trio, frame, lambda d: None)
        # a frame without a depth descriptor is legal on K and clears the slot's depth
        K.ingest_frames(9, [dict(frame, depth=None, shift=(0, 0))])
        Cd.ingest_frames(9, [dict(frame, shift=(0, 0))])
        assert np.array_equal(K.read_frame(9, depth=False)[0], Cd.read_frame(9)[0])
        refused(lm, lambda: K.read_frame(9), "slot 9", "without a depth image")
        with pytest.raises(ValueError):
            K.ingest_frames(9, [frame, dict(frame, depth=None)])               # the binding: all frames of a call or none
        with pytest.raises(ValueError):
            R.ingest_frames(9, [dict(frame, depth=None)])


def test_registered_ingest(lm, trio, sources):
    import register_scenes as G
    K, Cd, R, bgr, depth = trio
    colour = sources.put(np.random.default_rng(3).integers(0, 256, (G.CH, G.CW, 3), dtype=np.uint8))
    raw = sources.put(G.scene_a())
    dc, cc = G.depth_cam_a(G.ZERO), G.colour_cam(G.ZERO)

    def setup(d):
        if d is not Cd:
            d.set_registration(to_cam(lm, dc), to_cam(lm, cc), G.ROT, G.TRANS, splat=(1, 1))
    frame = dict(colour=colour, depth=raw, crop=G.CROP, register_depth=True)
    ingest_case(lm, trio, frame, setup, colour_only_frame=dict(colour=colour, crop=G.CROP))
    refused(lm, lambda: Cd.ingest_frames(9, [frame]), "colour-only", "lm_ingest_frames_registered needs an RGB-D detector")
    for d in (K, R):
        d.set_registration(None, None, None, None)


def test_rectified_ingest(lm, trio, sources):
    import rectify_scenes as Q
    colour, dep = sources.put(Q.source("bgr"), pad=1), sources.put(Q.depth_u16(), pad=2)
    frame = dict(colour=colour, depth=dep, crop=(24, 20), flip_x=True, shift=(3, -2), rectified=True, **Q.DESC["bgr"])
    ingest_case(lm, trio, frame, lambda d: d.set_rectification(to_cam(lm, Q.source_cam()), to_cam(lm, Q.ideal_cam())))
    for d in trio[:3]:
        d.set_rectification(None)


def test_reduced_ingest(lm, trio, sources):
    import reduce_scenes as RS
    import test_gpu_reduce as TR
    r = (9, 4)
    w, h = TR.sides(W, H, r)
    colour, (dhost, scale) = sources.put(RS.colour("bgr", w, h)[0], pad=1), RS.depth("f32", w, h)
    frame = dict(colour=colour, depth=sources.put(dhost, pad=4), depth_scale=scale, crop=(3, 1), depth_crop=(2, 1), flip_x=True, shift=(3, -2), reduced=True,
                 **RS.desc("bgr", w))
    ingest_case(lm, trio, frame, lambda d: d.set_reduction(r, depth_rule="min_valid"))
    for d in trio[:3]:
        d.set_reduction(None)


def test_rectified_reduced_ingest(lm, trio, sources):
    import rectify_reduce_scenes as X
    import rectify_scenes as Q
    import reduce_scenes as RS
    r = (9, 4)
    source, ideal, _ = X.lens_map(*X.ideal_sides(W, H, r))

    def setup(d):
        d.set_rectification(to_cam(lm, source), to_cam(lm, ideal))
        d.set_reduction(r, depth_rule="nearest")
    colour, (dhost, scale) = sources.put(RS.colour("bgr", Q.SW, Q.SH)[0], pad=1), RS.depth("u16", Q.SW, Q.SH)
    frame = dict(colour=colour, depth=sources.put(dhost, pad=2), depth_scale=scale, crop=(2, 2), flip_x=False, shift=(-5, 4), rectify_reduce=True,
                 **RS.desc("bgr", Q.SW))
    ingest_case(lm, trio, frame, setup)
    for d in trio[:3]:
        d.set_reduction(None)
        d.set_rectification(None)


# ---- 6. what stays as it was -------------------------------------------------------------------------------
def test_plain_colour_only_refuses_what_it_refused_and_rgbd_ignores_the_flag(lm, orc, trio):
    K, Cd, R, bgr, depth = trio
    sq = np.array([(0, 0, 8, 8, 12, 1)], lm.DEPTH_SELECT_QUERY_DTYPE)
    cq = np.array([(0, 0, 8, 8, 100, 900, 1, 0)], lm.DEPTH_QUERY_DTYPE)
    Cd.upload_frame(1, bgr, depth)                          # (the depth image is ignored, as ever)
    no_plane = "the detector keeps no depth frame on the device (no depth modality)"
    refused(lm, lambda: Cd.depth_select(sq), no_plane)
    refused(lm, lambda: Cd.depth_counts(cq), no_plane)
    refused(lm, lambda: Cd.time_depth_select(sq), no_plane)
    refused(lm, lambda: Cd.set_mask_rule(1, 1, modalities=1, depth_range=(500, 900)), "a colour-only detector does not keep on the device")
    refused(lm, lambda: Cd.icp_refine(1, (10, 10, 40, 40), 0, np.eye(4)[None], (1044.87, 1045.69141, 80.0, 40.0)), "colour-only")
    refused(lm, lambda: Cd.read_frame(1, depth=True), "a colour-only detector holds no depth frame")
    assert Cd.read_frame(1)[1] is None
    # R with the flag: the same bytes, the same lists, the depth image still required
    R2 = lm.Detector(color_only=False, keep_depth=True, width=W, height=H, frame_slots=2)
    assert R2.keeps_depth and R2.num_modalities == 2 and R2.cfg.flags & lm.FLAG_KEEP_DEPTH
    R2.add_class(*S.bank_rgbd(orc))
    for d in (R, R2):
        d.upload_frame_shifted(1, bgr, depth, 7, -5)
    assert R2.read_frame(1)[1].tobytes() == R.read_frame(1)[1].tobytes()
    a, b = R.match(bgr, depth, 55.0), R2.match(bgr, depth, 55.0)
    assert a.tobytes() == b.tobytes()
    assert R2.depth_select(sq).tobytes() == R.depth_select(sq).tobytes()
    refused(lm, lambda: R2.upload_frame(1, bgr), "depth image missing")
    refused(lm, lambda: R.upload_frame(1, bgr), "depth image missing")
    R2.close()


# ---- 7. learning from resident frames with a depth-gated object mask -------------------------------------------
def test_learning_with_a_depth_gated_object_mask(lm):
    """lm_add_templates_slots with a rule as the object mask, the rule gating on depth: on K the rule reads the kept depth frame, and the
    templates -- ids, bounding boxes, the features of every level -- are those C learns from the same colour frames with the numpy
    reference's mask of the rule handed in as an array.  A slot whose frame came without depth is refused by its number before anything
    is learned; C refuses the rule in the words it always had."""
    bgr, depth = S.frame()
    specs = [dict(modalities=1, depth_range=(600, 680), grow=2), dict(modalities=1, depth_range=(560, 660), keep_invalid=True, grow=0, rect=(16, 4, 128, 72))]
    frames = [(bgr, depth), (S.shifted(bgr, 7, -5), S.shifted(depth, 7, -5))]
    K = lm.Detector(color_only=True, keep_depth=True, width=W, height=H, T=S.T, frame_slots=4)
    Cd = lm.Detector(color_only=True, width=W, height=H, T=S.T, frame_slots=4)
    masks = []
    for k, ((b, dd), spec) in enumerate(zip(frames, specs)):
        K.upload_frame(1 + k, b, dd)
        Cd.upload_frame(1 + k, b)
        m = mrr.mask_of(spec, b, dd)
        assert (m == 0).sum() > 1000 and (m == 255).sum() > 1000
        masks.append(m)
    rules = [lm.make_mask_rule(s["modalities"], s.get("depth_range"), s.get("keep_invalid", False), None, s.get("grow", 0), s.get("rect")) for s in specs]
    kid, kbb = K.add_templates_slots("learnt", 1, rules)
    cid, cbb = Cd.add_templates_slots("learnt", 1, masks)
    assert kid.tolist() == cid.tolist() == [0, 1] and np.array_equal(kbb, cbb), (kid, cid, kbb, cbb)
    for tid in (0, 1):
        for level in range(2):
            kw, kh, kf = K.get_template(0, tid, level, 0)
            cw, ch, cf = Cd.get_template(0, tid, level, 0)
            assert (kw, kh) == (cw, ch) and kf.tobytes() == cf.tobytes() and len(kf) > 0
    # the mask mattered: unmasked learning gives other templates
    uid, ubb = Cd.add_templates_slots("unmasked", 1, [None, None])
    assert not np.array_equal(ubb, cbb)
    # a frame without depth in a ruled slot: refused, nothing added
    K.upload_frame(2, frames[1][0])
    before = K.num_templates()
    refused(lm, lambda: K.add_templates_slots("learnt", 1, rules), "slot 2", "without a depth image")
    assert K.num_templates() == before
    kid2, _ = K.add_templates_slots("learnt", 1, [rules[0], None])          # ... while an unruled slot needs no depth
    assert kid2.tolist() == [2, 3]
    refused(lm, lambda: Cd.add_templates_slots("learnt", 1, rules), "colour-only")
    K.close()
    Cd.close()


def test_rows_staged_with_and_without_depth_are_refused(lm, trio):
    """The lm_stage_rows calls that fill one slot bring a depth image or none does: a slot staged both ways is refused by lm_upload_staged
    before anything is sent (the slot keeps its frame), and staging it again after a new reserve goes through."""
    K, Cd, R, bgr, depth = trio
    K.upload_frame(7, bgr, S.other_depth())
    before = K.read_frame(7)
    K.stage_reserve(7, 1)
    K.stage_rows(7, bgr[::-1].copy(), depth, 0, 0, 0, 40)
    K.stage_rows(7, bgr[::-1].copy(), None, 0, 0, 40, H)
    refused(lm, lambda: K.upload_staged(7), "slot 7", "a depth image for some rows and none for others")
    after = K.read_frame(7)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    _staged(K, 7, bgr, depth, 0, 0)
    kb, kd = K.read_frame(7)
    assert np.array_equal(kb, bgr) and np.array_equal(kd, depth)
    _staged(K, 7, bgr, None, 0, 0)
    refused(lm, lambda: K.read_frame(7), "slot 7", "without a depth image")
