"""lm_export_frames on the GPU: the slots' colour frames, with primitives drawn, into device memory in the consumer's
format -- byte for byte against tests/export_reference.py (numpy, written from the header's rule).  Every destination is allocated with 256
guard bytes of 0xA5 in front of it, behind it and between its planes, and random bytes everywhere else: a case compares the WHOLE
allocation with the reference's, so the guards, the surface outside the window and the window itself are all asserted.  Device memory
comes from DeviceBuffer; no second HIP runtime enters the process."""
import ctypes as C
import threading

import numpy as np
import pytest

import export_reference as ER
import keep_depth_scene as S

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID, OVERFLOW = 1, 4
MATRICES = [("bt601", "limited"), ("bt709", "limited"), ("bt601", "full"), ("bt709", "full")]
# layout, order, bytes per pixel, matrix, range
FORMATS = [("hwc", "bgr", 3, None, None), ("hwc", "rgb", 3, None, None), ("hwc", "bgr", 4, None, None), ("hwc", "rgb", 4, None, None),
           ("chw", "bgr", 1, None, None), ("chw", "rgb", 1, None, None)] + [("nv12", "bgr", 1, m, r) for m, r in MATRICES]
BGR8, BGRA8, NV12 = FORMATS[0], FORMATS[2], FORMATS[6]


class Target:
    """One destination surface in device memory, and the same bytes on the host (raw0: what was there before the export)."""

    def __init__(self, lm, rng, fmt, w, h, surface=None, window=(0, 0), offset=0, pad=0):
        layout, order, px, matrix, range_ = fmt
        sw, sh = surface or (w, h)
        rs = sw * px + pad
        plane = sh * rs
        if layout == "hwc":
            ps, body = 0, plane
        elif layout == "chw":
            ps, body = plane + GUARD, 3 * plane + 2 * GUARD
        else:
            ps, body = plane + GUARD, plane + GUARD + (sh // 2) * rs
        self.offset = GUARD + offset
        nbytes = self.offset + body + GUARD
        raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
        self.guards = np.zeros(nbytes, bool)
        self.guards[:self.offset] = True
        self.guards[self.offset + body:] = True
        if ps:
            for k in range(2 if layout == "chw" else 1):
                self.guards[self.offset + k * ps + plane:self.offset + (k + 1) * ps] = True
        raw[self.guards] = 0xA5
        self.raw0 = raw
        self.buf = lm.DeviceBuffer(nbytes)
        self.buf.upload(raw)
        self.surface = ER.Surface(layout, order, px, sw, sh, window, rs, ps, self.offset, nbytes, matrix or "bt601", range_ or "limited")
        if layout == "hwc":
            view = self.buf.view(np.uint8, (sh, sw, px), offset=self.offset, strides=(rs, px, 1))
        elif layout == "chw":
            view = self.buf.view(np.uint8, (3, sh, sw), offset=self.offset, strides=(ps, rs, 1))
        else:
            view = (self.buf.view(np.uint8, (sh, sw), offset=self.offset, strides=(rs, 1)),
                    self.buf.view(np.uint8, (sh // 2, sw), offset=self.offset + ps, strides=(rs, 1)))
        self.spec = dict(target=view, order=order, layout=layout, window=window, matrix=matrix or "bt601", range=range_ or "limited")

    def read(self):
        return self.buf.download(np.uint8, (self.buf.nbytes,))

    def check(self, E, what):
        """The allocation after an export of the W x H BGR image E"""
        got, want = self.read(), self.surface.write(self.raw0.copy(), E)
        assert np.array_equal(got[self.guards], self.raw0[self.guards]), "%s: %d guard bytes changed" % (what, int((got[self.guards] != 0xA5).sum()))
        assert np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))
        assert (want != self.raw0).any(), what         # (the export wrote something: the comparison is not of two untouched buffers)

    def close(self):
        self.buf.close()


def make_prims(lm, rows):
    p = np.zeros(len(rows), lm.DRAW_PRIM_DTYPE)
    for k, r in enumerate(rows):
        p[k] = r
    return p


def frames_for(rng, n, w, h):
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]


@pytest.mark.parametrize("size", [(16, 16), (48, 32), (160, 80)], ids=lambda s: "%dx%d" % s)
def test_plain_export_every_format(lm, size):
    """Every destination format and NV12 matrix, no primitives: the window at (0, 0) of a surface of the frame's size and in the
    bottom-right corner of a larger one, data offsets 0 .. 3 and a row stride that is no multiple of anything, four mixed formats per call.
    16 x 16 is narrower than a tile, 48 x 32 one ragged tile, 160 x 80 three tile columns and a ragged last tile row."""
    W, H = size
    d = lm.Detector(color_only=True, width=W, height=H, T=[2, 8], frame_slots=4)
    rng = np.random.default_rng(21 + W)
    frames = frames_for(rng, 4, W, H)
    for s, f in enumerate(frames):
        d.upload_frame(s, f)
    for s, f in enumerate(frames):
        assert np.array_equal(d.read_frame(s)[0], f)
    cases = [(fmt, corner, off) for corner in (False, True) for off in range(4) for fmt in FORMATS]
    assert len(cases) % 4 == 0
    for i in range(0, len(cases), 4):
        targets = []
        for fmt, corner, off in cases[i:i + 4]:
            surface, window = ((W + 8, H + 6), (8, 6)) if corner else ((W, H), (0, 0))
            targets.append(Target(lm, rng, fmt, W, H, surface, window, offset=off, pad=(3 if off else 0) + (2 if corner else 0)))
        assert len({(t.surface.layout, t.surface.order, t.surface.px, t.surface.matrix, t.surface.range) for t in targets}) > 1      # mixed formats in one call
        d.export_frames(0, [t.spec for t in targets])
        for s, (t, case) in enumerate(zip(targets, cases[i:i + 4])):
            t.check(frames[s], "%r" % (case,))
            t.close()
    # BGR8 with no undo is lm_read_frame's image
    t = Target(lm, rng, BGR8, W, H)
    d.export_frame(2, t.spec["target"])
    assert np.array_equal(t.read()[GUARD:GUARD + W * H * 3].reshape(H, W, 3), d.read_frame(2)[0])
    t.close()
    d.close()


@pytest.mark.parametrize("size", [(48, 32), (160, 80)], ids=lambda s: "%dx%d" % s)
def test_undo(lm, size):
    """The ingest's mirror and shift undone: shifts that are and are not multiples of four, odd (NV12's chroma blocks are the
    destination's, not the frame's), and by the whole width (all black), each with and without the mirror; then the ingest -> export
    round trip."""
    W, H = size
    d = lm.Detector(color_only=True, width=W, height=H, T=[2, 8], frame_slots=8)
    rng = np.random.default_rng(31 + W)
    frames = frames_for(rng, 8, W, H)
    for s, f in enumerate(frames):
        d.upload_frame(s, f)
    opts = [(flip, sh) for sh in ((0, 0), (7, -3), (-5, 4), (W, 0), (4, 2), (-8, -1)) for flip in (False, True)]
    for fmt in (BGR8, BGRA8, NV12, FORMATS[5], FORMATS[9]):
        for i in range(0, len(opts), 4):
            targets = [Target(lm, rng, fmt, W, H, (W + 2, H + 2), (2, 2), offset=1, pad=1) for _ in range(4)]
            d.export_frames(2, [t.spec for t in targets], undo=[dict(flip_x=f, shift=s) for f, s in opts[i:i + 4]])
            for k, (t, (flip, sh)) in enumerate(zip(targets, opts[i:i + 4])):
                E = ER.undo(frames[2 + k], flip, sh)
                if sh == (W, 0):
                    assert not E.any()
                t.check(E, "%s flip %s shift %r" % (fmt[0], flip, sh))
                t.close()
    # round trip: a BGR8 source ingested with opts and exported with the same opts as undo is the source wherever the shift kept it
    src = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
    sbuf = lm.DeviceBuffer(src.nbytes)
    sbuf.upload(src)
    for flip, (sx, sy) in ((False, (7, -3)), (True, (7, -3)), (True, (-5, 4)), (False, (0, 0)), (True, (0, 0))):
        d.ingest_frame(0, sbuf.view(np.uint8, (H, W, 3)), flip_x=flip, shift=(sx, sy))
        t = Target(lm, rng, BGR8, W, H)
        d.export_frame(0, t.spec["target"], undo=dict(flip_x=flip, shift=(sx, sy)))
        got = t.read()[GUARD:GUARD + W * H * 3].reshape(H, W, 3)
        # source pixel (u, v) went to frame pixel ((flip ? W - 1 - u : u) + sx, v + sy): kept iff that lies inside the frame
        v, u = np.mgrid[0:H, 0:W]
        x, y = np.where(flip, W - 1 - u, u) + sx, v + sy
        kept = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        assert np.array_equal(got[kept], src[kept]) and not got[~kept].any() and kept.any()
        assert (~kept).any() == ((sx, sy) != (0, 0))
        t.close()
    sbuf.close()
    d.close()


def primitive_rows(rng, W, H):
    """Frames 0 .. 2 of a 4-frame call, interleaved; frame 3 gets nothing"""
    rows = []
    for r in (0, 1, 2, 3, 4, 5, 40):
        for f in range(3):
            rows.append((0, f, int(rng.integers(0, W)), int(rng.integers(0, H)), r, 0, 1 + (r == 40) * f, *rng.integers(0, 256, 3), 255))
    c = (W // 2, H // 2)
    octants = [(50, 20), (20, 50), (-20, 50), (-50, 20), (-50, -20), (-20, -50), (20, -50), (50, -20), (70, 0), (0, 45), (-70, 0), (0, -45)]
    for k, (dx, dy) in enumerate(octants):
        for t in (1, 2, 3, 64):
            if t == 64 and k % 4:
                continue
            rows.append((1, k % 3, c[0] - dx // 2 + k, c[1] - dy // 2, c[0] + dx + k, c[1] + dy, t, *rng.integers(0, 256, 3), 255 if t < 64 else 90))
    rows += [(1, 1, -30, 10, W + 30, 60, 2, 10, 200, 30, 255), (1, 2, 63, -10, 65, H + 10, 3, 200, 10, 30, 255), (1, 0, 5, 31, W - 5, 33, 1, 1, 2, 3, 255)]
    rows += [(2, 0, 10, 10, 100, 60, 1, 0, 255, 255, 255), (2, 1, 60, 28, 70, 36, 5, 255, 0, 255, 200), (2, 2, -20, -20, W + 20, H + 20, 5, 9, 9, 9, 255),
             (2, 1, -3, -3, W + 2, H + 2, 5, 90, 19, 29, 255), (2, 0, 62, 30, 66, 34, 1, 255, 255, 255, 255)]
    # opacities 255, 128 and 1 stacked five deep on the same pixels
    for k, a in enumerate((255, 128, 1, 128, 255)):
        rows.append((2, 1, 20, 40, 45, 60, 64 if k % 2 == 0 else 3, 40 * k, 255 - 50 * k, 17 * k, a))
    return rows


def crowded_rows(rng):
    """2 000 one-pixel rings on the tile (1, 1) of frame 0 -- far more than one LDS chunk -- and 50 elsewhere"""
    rows = [(0, 0, int(rng.integers(64, 128)), int(rng.integers(32, 64)), 0, 0, 1, *rng.integers(0, 256, 3), int(rng.choice([255, 128, 1]))) for _ in range(2000)]
    rows += [(0, int(rng.integers(0, 3)), int(rng.integers(0, 160)), int(rng.integers(0, 80)), 0, 0, 1, *rng.integers(0, 256, 3), 255) for _ in range(50)]
    return rows


@pytest.fixture(scope="module")
def drawn(lm):
    """The 160 x 80 detector with four frames resident, the mixed primitive list and the reference's annotated frames (computed once)."""
    W, H = 160, 80
    d = lm.Detector(color_only=True, width=W, height=H, T=[2, 8], frame_slots=4)
    rng = np.random.default_rng(41)
    frames = frames_for(rng, 4, W, H)
    for s, f in enumerate(frames):
        d.upload_frame(s, f)
    prims = make_prims(lm, primitive_rows(rng, W, H))
    crowd = make_prims(lm, crowded_rows(rng))
    yield dict(d=d, rng=rng, frames=frames, prims=prims, crowd=crowd, A=[ER.annotate(frames[f], prims, f) for f in range(4)],
               A_crowd=[ER.annotate(frames[f], crowd, f) for f in range(4)], W=W, H=H)
    d.close()


def export_all(lm, w, fmt, prims, undo=None, first=0, n=4, **target):
    ts = [Target(lm, w["rng"], fmt, w["W"], w["H"], **target) for _ in range(n)]
    w["d"].export_frames(first, [t.spec for t in ts], prims, undo)
    return ts


@pytest.mark.parametrize("fmt", [BGR8, NV12, BGRA8, FORMATS[4]], ids=["bgr8", "nv12", "bgra8", "planar"])
def test_primitives_mixed_list(lm, drawn, fmt):
    w = drawn
    assert all((w["A"][f] != w["frames"][f]).any() for f in range(3)) and np.array_equal(w["A"][3], w["frames"][3])
    ts = export_all(lm, w, fmt, w["prims"], surface=(164, 84), window=(4, 2), offset=3, pad=1)
    for f, t in enumerate(ts):
        t.check(w["A"][f], "frame %d" % f)
        t.close()
    # with the mirror and a shift undone: the primitives stay in frame coordinates, the tiles are the exported image's
    undo = [dict(flip_x=True, shift=(7, -3)), dict(flip_x=False, shift=(-5, 4)), dict(flip_x=True, shift=(0, 0)), None]
    ts = export_all(lm, w, fmt, w["prims"], undo)
    for f, t in enumerate(ts):
        o = undo[f] or dict(flip_x=False, shift=(0, 0))
        t.check(ER.undo(w["A"][f], o["flip_x"], o["shift"]), "frame %d undone" % f)
        t.close()


def test_primitives_order_is_part_of_the_result(lm, drawn):
    w = drawn
    rev = w["prims"][::-1].copy()
    ts = export_all(lm, w, BGR8, rev)
    differs = 0
    for f, t in enumerate(ts):
        A = ER.annotate(w["frames"][f], rev, f)
        differs += int((A != w["A"][f]).any())
        t.check(A, "frame %d reversed" % f)
        t.close()
    assert differs >= 2


def test_primitives_more_than_one_chunk_on_a_tile(lm, drawn):
    w = drawn
    for fmt in (BGR8, NV12):
        ts = export_all(lm, w, fmt, w["crowd"])
        for f, t in enumerate(ts):
            t.check(w["A_crowd"][f], "frame %d crowded" % f)
            t.close()
    assert np.array_equal(w["A_crowd"][3], w["frames"][3])


def test_primitives_per_frame_calls_and_unrelated_primitives(lm, drawn):
    """The same call split into per-frame calls, and the same primitives with unrelated ones appended for other frames, give the same
    bytes per frame"""
    w, lmod = drawn, lm
    for f in range(3):
        mine = w["prims"][w["prims"]["frame"] == f].copy()
        mine["frame"] = 0
        ts = export_all(lmod, w, BGR8, mine, first=f, n=1)
        ts[0].check(w["A"][f], "frame %d alone" % f)
        ts[0].close()
    # frames 1 and 2 alone, as frames 0 and 1 of a call over slots 1 .. 2, with primitives of the OTHER frame appended behind each
    sub = w["prims"][w["prims"]["frame"] >= 1].copy()
    sub["frame"] -= 1
    extra = w["crowd"][w["crowd"]["frame"] == 0][:300].copy()
    extra["frame"] = 1
    both = np.concatenate([sub[sub["frame"] == 0], extra, sub[sub["frame"] == 1]])
    ts = export_all(lmod, w, NV12, both, first=1, n=2)
    ts[0].check(w["A"][1], "frame 1 beside a crowded neighbour")
    ts[1].check(ER.annotate(w["frames"][2], both, 1), "frame 2 with the extra primitives")
    for t in ts:
        t.close()


def refused(lm, call, code, *words):
    with pytest.raises(lm.LinemodError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for word in words:
        assert word in str(e.value), (word, str(e.value))


def test_refusals_and_overflow(lm, drawn):
    """The detector's own refusals (the descriptors' and primitives' are pinned without a GPU by tests/test_export_cpu.py); a refused call
    writes nothing, claims nothing, and the slots accept uploads afterwards"""
    w = drawn
    d, W, H = w["d"], w["W"], w["H"]
    ts = [Target(lm, w["rng"], BGR8, W, H) for _ in range(2)]
    specs = [t.spec for t in ts]
    one = make_prims(lm, [(0, 0, 5, 5, 3, 0, 1, 1, 2, 3, 255)])
    refused(lm, lambda: d.export_frames(3, specs), INVALID, "slot out of range")
    refused(lm, lambda: d.export_frames(-1, specs), INVALID, "slot out of range")
    refused(lm, lambda: d.export_frames(0, []), INVALID, "n_slots <= 0")
    bad = one.copy(); bad["frame"] = 2
    refused(lm, lambda: d.export_frames(0, specs, bad), INVALID, "primitive 0: frame 2 lies outside 0 .. 1")
    bad = np.concatenate([one, one]); bad["thickness"][1] = 65
    refused(lm, lambda: d.export_frames(0, specs, bad), INVALID, "primitive 1: thickness 65")
    refused(lm, lambda: d.export_frames(0, [specs[0], specs[0]]), INVALID, "destination images of frames 0 and 1 overlap in memory")
    refused(lm, lambda: d.export_frames(0, [specs[0], dict(specs[1], window=(1, 0))]), INVALID, "destination image of frame 1: window 160 x 80 at (1, 0)")
    refused(lm, lambda: d.export_frames(0, specs, np.zeros(65537, lm.DRAW_PRIM_DTYPE)), INVALID, "65537 primitives exceed 65536")
    # the tile-binning bound: 65536 boxes around the whole frame touch 9 tiles each, 589824 entries: fine; 8 frames' worth do not exist
    # here, so the bound is reached with a second detector of 640 x 480 frames (150 tiles: 27 963 such boxes fit, 30 000 do not)
    big = lm.Detector(color_only=True, width=640, height=480, frame_slots=1)
    big.upload_frame(0, np.zeros((480, 640, 3), np.uint8))
    bt = Target(lm, w["rng"], BGR8, 640, 480)
    boxes = make_prims(lm, [(2, 0, 0, 0, 639, 479, 1, 1, 2, 3, 0)] * 30000)
    refused(lm, lambda: big.export_frames(0, [bt.spec], boxes), OVERFLOW, "4500000 entries", "4194304")
    assert np.array_equal(bt.read(), bt.raw0)
    bt.close()
    fresh = lm.Detector(color_only=True, width=W, height=H, T=[2, 8], frame_slots=2)
    refused(lm, lambda: fresh.export_frames(0, specs), INVALID, "frame 0: no frame uploaded to slot")
    fresh.close()
    big.close()
    for t in ts:
        assert np.array_equal(t.read(), t.raw0)         # nothing was written by any refused call
    # nothing is claimed: uploads go through, and the export works
    for s in range(2):
        d.upload_frame(s, w["frames"][s])
    d.export_frames(0, specs, one)
    ts[0].check(ER.annotate(w["frames"][0], one, 0), "after the refusals")
    ts[1].check(w["frames"][1], "after the refusals")
    for t in ts:
        t.close()


def test_detections_drawn_on_the_scene(lm, orc):
    """The keep-depth tests' 160 x 80 scene: match, take the best match, draw its response and its box, export as BGR8 and as NV12"""
    bgr, _ = S.frame()
    d = lm.Detector(color_only=True, width=S.W, height=S.H, T=S.T, frame_slots=2)
    for name, descs, feats in S.bank(orc):
        d.add_class(name, descs, feats)
    d.upload_frame(0, bgr)
    out, counts = d.match_batch(1, S.THRESHOLD)
    assert counts[0] > 0
    best = out[0][:counts[0]][int(np.argmax(out[0][:counts[0]]["similarity"]))]
    tw, th, feats = d.get_template(int(best["class_idx"]), int(best["template_id"]), 0, 0)
    rings = lm.draw_response(d, best, 0)
    assert len(rings) == len(feats) > 0 and (rings["kind"] == lm.DRAW_RING).all() and (rings["x1"] == d.get_T(0) // 2).all()
    prims = np.concatenate([rings, lm.draw_box((int(best["x"]), int(best["y"]), tw, th), (0, 255, 255), 2, 0)])
    A = ER.annotate(bgr, prims, 0)
    assert (A != bgr).any()
    rng = np.random.default_rng(51)
    for fmt in (BGR8, NV12):
        t = Target(lm, rng, fmt, S.W, S.H)
        d.export_frame(0, t.spec["target"], prims, order=t.spec["order"], layout=t.spec["layout"])
        t.check(A, "the scene as %s" % fmt[0])
        t.close()
    d.close()


def test_match_in_flight_is_no_obstacle(lm, orc):
    """The export only reads the slots: a match in flight on them does not refuse it, and the match's lists are what they are without it"""
    bgr, _ = S.frame()
    d = lm.Detector(color_only=True, width=S.W, height=S.H, T=S.T, frame_slots=4)
    for name, descs, feats in S.bank(orc):
        d.add_class(name, descs, feats)
    rng = np.random.default_rng(52)
    for s in range(4):
        d.upload_frame(s, S.shifted(bgr, 2 * s, -s))
    want, want_counts = d.match_batch(4, S.THRESHOLD)
    assert want_counts.sum() > 0
    ts = [Target(lm, rng, NV12, S.W, S.H) for _ in range(4)]
    box = lm.draw_box((10, 10, 50, 30), (0, 0, 255), 3, 2)
    d.match_begin(1, 0, 4, S.THRESHOLD)
    d.export_frames(0, [t.spec for t in ts], box)
    got, got_counts = d.match_end(1, n_slots=4)
    assert np.array_equal(got_counts, want_counts)
    for s in range(4):
        assert got[s][:got_counts[s]].tobytes() == want[s][:want_counts[s]].tobytes()
        ts[s].check(ER.annotate(S.shifted(bgr, 2 * s, -s), box, s), "slot %d beside the match" % s)
        ts[s].close()
    d.close()


def test_upload_from_another_thread_is_refused_or_ordered(lm):
    """While an export runs, an upload into one of its slots from another thread is refused; one that got in before the claim is
    ordered in front of the export.  Never torn: the exported image is the old frame or the new one, whole.  The export is made long by
    27 000 thick, fully transparent segments across each tile of a 640 x 480 frame (opacity 0 leaves every byte as it was)."""
    W, H = 640, 480
    base = lm.live_resources()
    d = lm.Detector(color_only=True, width=W, height=H, frame_slots=2)
    rng = np.random.default_rng(61)
    old, new = frames_for(rng, 2, W, H)
    d.upload_frame(0, old)
    d.upload_frame(1, old)
    d.upload_wait()
    heavy = make_prims(lm, [(1, 0, -100, -100 + (k % 7), W + 100, H + 100, 64, 1, 2, 3, 0) for k in range(27000)])
    ts = [Target(lm, rng, BGR8, W, H) for _ in range(2)]
    done = []
    t = threading.Thread(target=lambda: done.append(d.export_frames(0, [x.spec for x in ts], heavy)))
    hits, accepted = 0, 0
    t.start()
    while t.is_alive():
        try:
            d.upload_frame(0, new)
            accepted += 1
        except lm.LinemodError as e:
            assert e.code == INVALID and "slot is read by an export in flight" in str(e), str(e)
            hits += 1
    t.join()
    assert len(done) == 1 and hits > 0
    got = ts[0].read()[GUARD:GUARD + W * H * 3].reshape(H, W, 3)
    assert np.array_equal(got, old) or (accepted > 0 and np.array_equal(got, new))
    ts[1].check(old, "the slot beside it")
    # the claim is gone with the call
    d.upload_frame(0, new)
    d.export_frames(0, [x.spec for x in ts])
    ts[0].check(new, "after the release")
    for x in ts:
        x.close()
    d.close()
    assert lm.live_resources() == base
