"""lm_ingest_frames on the GPU: frames that lie in device memory in their producer's format -> the slots, compared
byte for byte through read_frame with tests/ingest_reference.py (numpy, written from the definition), with the EXISTING shifted
upload, with the host composition of the reference's capture code, and end to end through the match.  Device memory comes from
DeviceBuffer; no second HIP runtime enters the process (tests/hip_runtime.py binds the one the library has mapped)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ingest_reference as IR
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

SW, SH = 203, 97          # source size of the sweep: odd, no multiple of anything
INVALID = 1
BUSY = "slot belongs to a match in flight"

COLOUR_FORMATS = [("bgr", "hwc", 3), ("rgb", "hwc", 3), ("bgr", "hwc", 4), ("rgb", "hwc", 4), ("bgr", "chw", 1), ("rgb", "chw", 1)]
# value at scale 1 -> u16: halves, the saturation edge, large, non-finite, non-positive, ordinary
SPECIAL = [(0.5, 0), (1.5, 2), (2.5, 2), (65534.5, 65534), (65535.5, 65535), (1e9, 65535), (3e9, 65535), (np.inf, 0), (-np.inf, 0),
           (np.nan, 0), (-0.0, 0), (-1.0, 0), (697.5, 698), (0.49999997, 0)]


class Source:
    """One source image: the bytes in a DeviceBuffer, the same bytes on the host as the strided array the reference reads."""

    def __init__(self, lm, raw, offset, dtype, shape, strides):
        self.buf = lm.DeviceBuffer(raw.nbytes)
        self.buf.upload(raw)
        self.view = self.buf.view(dtype, shape, offset=offset, strides=strides)
        item = np.dtype(dtype).itemsize
        flat = raw[offset:offset + (raw.nbytes - offset) // item * item].view(dtype)
        self.host = np.lib.stride_tricks.as_strided(flat, shape=shape, strides=strides, writeable=False)

    def close(self):
        self.buf.close()


def colour_source(lm, rng, order, layout, px, offset, w=SW, h=SH, pad=3):
    if layout == "hwc":
        rs = w * px + pad
        shape, strides, nbytes = (h, w, px), (rs, px, 1), offset + h * rs
    else:
        rs = w + pad
        ps = h * rs + (5 if pad else 0)
        shape, strides, nbytes = (3, h, w), (ps, rs, 1), offset + 3 * ps
    raw = rng.integers(0, 256, nbytes + 16, dtype=np.uint8)
    return Source(lm, raw, offset, np.uint8, shape, strides)


def depth_source(lm, rng, f32, w=SW, h=SH, pad=True):
    item = 4 if f32 else 2
    rs = w * item + (item if pad else 0)
    if f32:
        v = rng.uniform(-50.0, 70000.0, (h, rs // 4)).astype(np.float32)
        sp = np.array([a for a, _ in SPECIAL], np.float32)
        hit = rng.random(v.shape) < 0.2
        v[hit] = sp[rng.integers(0, len(sp), int(hit.sum()))]
    else:
        v = rng.integers(0, 65536, (h, rs // 2), dtype=np.uint16)
    raw = v.view(np.uint8).reshape(-1).copy()
    return Source(lm, raw, 0, np.float32 if f32 else np.uint16, (h, w), (rs, item))


def check_slot(d, slot, exp_bgr, exp_depth, what):
    bgr, depth = d.read_frame(slot)
    assert np.array_equal(bgr, exp_bgr), "%s: colour differs at %d bytes" % (what, int((bgr != exp_bgr).sum()))
    if exp_depth is not None:
        assert np.array_equal(depth, exp_depth), "%s: depth differs at %d pixels" % (what, int((depth != exp_depth).sum()))


@pytest.mark.parametrize("rgbd", [True, False], ids=["rgbd_160x80", "colour_48x32"])
def test_alignment_and_format_sweep(lm, rgbd):
    """Every colour format x both depth formats x base pointer offset 0..3 x crop_x {0, 1, 2, 3, max} x crop_y {0, max} x flip, row strides
    that are no multiple of 4 (u8) / of their element only (u16, f32), four mixed-format cases per ingest_frames call."""
    W, H = (160, 80) if rgbd else (48, 32)
    d = lm.Detector(color_only=not rgbd, width=W, height=H, frame_slots=4)
    rng = np.random.default_rng(11)
    col = {(k, off): colour_source(lm, rng, *COLOUR_FORMATS[k], off) for k in range(6) for off in range(4)}
    dep = {f32: depth_source(lm, rng, f32) for f32 in (False, True)} if rgbd else {False: None}
    cases = list(itertools.product(range(4), (0, 1, 2, 3, SW - W), (0, SH - H), (False, True), sorted(dep), range(6)))
    assert len(cases) % 4 == 0
    for i in range(0, len(cases), 4):
        frames = []
        for off, cx, cy, flip, f32, k in cases[i:i + 4]:
            order, layout, _ = COLOUR_FORMATS[k]
            frames.append(dict(colour=col[k, off].view, depth=dep[f32].view if rgbd else None, order=order, layout=layout, crop=(cx, cy),
                               depth_scale=1.0, flip_x=flip))
        assert len({f["order"] + f["layout"] + str(f["colour"].shape) for f in frames}) > 1      # mixed formats in one call
        d.ingest_frames(0, frames)
        for s, (off, cx, cy, flip, f32, k) in enumerate(cases[i:i + 4]):
            order, layout, _ = COLOUR_FORMATS[k]
            eb = IR.colour(col[k, off].host, W, H, order, layout, (cx, cy), flip)
            ed = IR.depth(dep[f32].host, W, H, (cx, cy), 1.0, flip) if rgbd else None
            check_slot(d, s, eb, ed, "format %d offset %d crop (%d, %d) flip %s f32 %s" % (k, off, cx, cy, flip, f32))
    d.close()
    for s in list(col.values()) + [s for s in dep.values() if s is not None]:
        s.close()


def test_shift_equals_the_existing_shifted_upload(lm):
    """BGR8 + U16 without crop: every shift gives the frame lm_upload_frame_shifted gives (an implementation of its own: the host staging
    pass); with a mirror and a crop it gives the numpy reference's."""
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    rng = np.random.default_rng(12)
    c0, d0 = colour_source(lm, rng, "bgr", "hwc", 3, 0, W, H, pad=0), depth_source(lm, rng, False, W, H, pad=False)
    bgr, depth = np.ascontiguousarray(c0.host), np.ascontiguousarray(d0.host)
    for sx, sy in ((0, 0), (7, -3), (-5, 11), (W - 1, 0), (-W, 0), (W + 5, 2)):
        d.upload_frame_shifted(1, bgr, depth, sx, sy)
        eb, ed = d.read_frame(1)
        d.ingest_frame(0, c0.view, d0.view, shift=(sx, sy))
        check_slot(d, 0, eb, ed, "shift (%d, %d)" % (sx, sy))
        assert np.array_equal(eb, IR.colour(bgr, W, H, shift=(sx, sy))) and np.array_equal(ed, IR.depth(depth, W, H, shift=(sx, sy)))
    c1, d1 = colour_source(lm, rng, "bgr", "hwc", 3, 1), depth_source(lm, rng, False)
    for sx, sy in ((0, 0), (7, -3), (-5, 11), (W - 1, 0), (-W, 0), (W + 5, 2)):
        d.ingest_frame(2, c1.view, d1.view, crop=(21, 9), flip_x=True, shift=(sx, sy))
        check_slot(d, 2, IR.colour(c1.host, W, H, crop=(21, 9), flip_x=True, shift=(sx, sy)),
                   IR.depth(d1.host, W, H, crop=(21, 9), flip_x=True, shift=(sx, sy)), "mirrored crop, shift (%d, %d)" % (sx, sy))
    d.close()
    for s in (c0, d0, c1, d1):
        s.close()


@pytest.mark.parametrize("scale", [1.0, 1000.0])
def test_float_depth_special_values(lm, scale):
    """One row of the special values (at scale 1000 divided by 1000 in float32 first): exactly the reference's u16, and at scale 1 the
    table's."""
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    v = np.zeros((H, W), np.float32)
    sp = np.array([a for a, _ in SPECIAL], np.float32)
    v[:, :] = np.resize(sp, W)[None, :]
    v[1] = np.resize(sp[::-1], W)
    if scale != 1.0:
        v = v / np.float32(scale)
    db = lm.DeviceBuffer(v.nbytes)
    db.upload(v)
    cb = lm.DeviceBuffer(W * H * 3)
    cb.upload(np.zeros((H, W, 3), np.uint8))
    for flip in (False, True):
        d.ingest_frame(0, cb.view(np.uint8, (H, W, 3)), db.view(np.float32, (H, W)), depth_scale=scale, flip_x=flip)
        _, got = d.read_frame(0)
        exp = IR.depth(v, W, H, scale=scale, flip_x=flip)
        assert np.array_equal(got, exp), (got[0, :16], exp[0, :16])
        if scale == 1.0 and not flip:
            assert list(got[0, :len(SPECIAL)]) == [b for _, b in SPECIAL]
    d.close()
    db.close()
    cb.close()


def test_the_kinect_shape(lm):
    """Kinect2::getKinectFrames + PoseDetection's translation, small: BGRA 240 x 100 and float depth 240 x 102 with +inf holes, the
    160 x 80 window at (40, 11) of both, mirrored, shifted by (3, -2).  The expectation is the reference's host composition in its
    order, written with slices: convertTo(CV_16UC1), crop both, BGRA2BGR, flip(.., 1), then translate with zeros shifted in."""
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    rng = np.random.default_rng(13)
    bgra = rng.integers(0, 256, (100, 240, 4), dtype=np.uint8)
    depthf = rng.uniform(400.0, 4500.0, (102, 240)).astype(np.float32)
    depthf[rng.random(depthf.shape) < 0.15] = np.inf
    cb, db = lm.DeviceBuffer(bgra.nbytes), lm.DeviceBuffer(depthf.nbytes)
    cb.upload(bgra)
    db.upload(depthf)
    d.ingest_frame(3, cb.view(np.uint8, bgra.shape), db.view(np.float32, depthf.shape), crop=(40, 11), flip_x=True, shift=(3, -2))
    # the host composition
    depth16 = np.zeros(depthf.shape, np.uint16)
    fin = np.isfinite(depthf)
    depth16[fin] = np.rint(depthf[fin]).astype(np.uint16)          # (400 .. 4500: no saturation; +inf -> 0)
    depth16 = depth16[11:11 + H, 40:40 + W]
    bgr = bgra[11:11 + H, 40:40 + W][:, :, :3]
    bgr, depth16 = bgr[:, ::-1], depth16[:, ::-1]
    eb, ed = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint16)
    eb[0:H - 2, 3:W] = bgr[2:H, 0:W - 3]
    ed[0:H - 2, 3:W] = depth16[2:H, 0:W - 3]
    check_slot(d, 3, eb, ed, "kinect shape")
    d.close()
    cb.close()
    db.close()


class Rig:
    """The 320 x 240 rig of test_gpu_upload_refusals.py: one frame, a 40-template bank cut from it, 4 slots, the oracle's list."""
    W, H, THR = 320, 240, 75.0

    def __init__(self, lm, orc, synth):
        W, H = self.W, self.H
        self.lm = lm
        self.d = d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
        self.bgr, self.depth = synth.make_frame(W, H, seed=500)
        o = orc.Detector(color_only=False)
        o.prepare(self.bgr, self.depth)
        q = {(l, m): o.stage(0, l, m).reshape(H >> l, W >> l) for l in range(2) for m in range(2)}
        descs, feats, _ = synth.make_bank(40, 2, 2, seed=99, size_range=(48, 120), quantized=q, crop_fraction=0.3, frame_size=(W, H),
                                          T0=d.get_T(0))
        d.add_class("c", descs, feats)
        o.add_class("c", descs, feats)
        self.exp = o.match(self.bgr, self.depth, self.THR, threads=8)
        # the producer's format: RGB planar and float metres, converted from the rig's frame on the host
        planar = np.ascontiguousarray(self.bgr[:, :, ::-1].transpose(2, 0, 1))
        metres = self.depth.astype(np.float32) / np.float32(1000)
        self.cb, self.db = lm.DeviceBuffer(planar.nbytes), lm.DeviceBuffer(metres.nbytes)
        self.cb.upload(planar)
        self.db.upload(metres)
        self.frame = dict(colour=self.cb.view(np.uint8, planar.shape), depth=self.db.view(np.float32, metres.shape), order="rgb", layout="chw",
                          depth_scale=1000.0)

    def close(self):
        self.d.close()
        self.cb.close()
        self.db.close()


@pytest.fixture(scope="module")
def rig(lm, orc, synth):
    r = Rig(lm, orc, synth)
    yield r
    r.close()


def test_end_to_end_match_after_ingest(rig):
    """match_slot and match_batch after ingest_frames (RGB planar + float metres) give the lists they give after upload_frame, which are the
    oracle's; a mask rule set on a slot survives the ingest as it survives an upload."""
    d, THR = rig.d, rig.THR
    assert len(rig.exp) > 0
    for s in range(4):
        d.upload_frame(s, rig.bgr, rig.depth)
    up_slot = d.match_slot(1, THR, 0)
    up_out, up_cnt = d.match_batch(4, THR, 0)
    up_frame = d.read_frame(2)
    d.ingest_frames(0, [rig.frame] * 4)
    got = d.read_frame(2)
    assert np.array_equal(got[0], up_frame[0]) and np.array_equal(got[1], up_frame[1])
    in_slot = d.match_slot(1, THR, 0)
    in_out, in_cnt = d.match_batch(4, THR, 0)
    assert_matches_equal(in_slot, up_slot)
    assert_matches_equal(in_slot, rig.exp)
    for s in range(4):
        assert_matches_equal(in_out[s, :in_cnt[s]], up_out[s, :up_cnt[s]])
        assert_matches_equal(in_out[s, :in_cnt[s]], rig.exp)
    # a rule belongs to the slot, not to the frame
    d.set_mask_rule(2, 1, modalities=3, depth_range=(400, 900))
    try:
        d.upload_frame(2, rig.bgr, rig.depth)
        ruled_up = d.match_slot(2, THR, 0)
        d.ingest_frames(2, [rig.frame])
        assert d.mask_rule(2) is not None and (d.mask_rule(2).zmin, d.mask_rule(2).zmax) == (400, 900)
        ruled_in = d.match_slot(2, THR, 0)
        assert_matches_equal(ruled_in, ruled_up)
    finally:
        d.clear_mask_rule()


def test_streams_and_reuse(lm):
    """The producer-stream path: the source is filled by an asynchronous copy on a stream S, ingested at once with stream=S, released
    to S, and overwritten on S -- the slot must hold the FIRST data.  This exercises the path (the event on S, the wait on the copy
    stream, the release); it cannot PROVE the ordering: a missing edge may still happen to give the right bytes.  Then the ticket rule:
    a slot ingested twice in a row, and a slot ingested behind a pending pinned upload, end with the last frame."""
    from hip_runtime import Runtime
    W, H = 160, 80
    d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    rng = np.random.default_rng(14)
    fb = W * H * 5
    pb = lm.PinnedBuffer(3 * fb)
    host = [(pb.view(np.uint8, (H, W, 3), offset=k * fb), pb.view(np.uint16, (H, W), offset=k * fb + W * H * 3)) for k in range(3)]
    for b, z in host:
        b[...] = rng.integers(0, 256, b.shape, dtype=np.uint8)
        z[...] = rng.integers(0, 65536, z.shape, dtype=np.uint16)
    src = [lm.DeviceBuffer(fb) for _ in range(2)]
    views = [(s.view(np.uint8, (H, W, 3)), s.view(np.uint16, (H, W), offset=W * H * 3)) for s in src]
    rt = Runtime()
    S = rt.stream_create()
    try:
        rt.memcpy_h2d_async(src[0].ptr.value, pb.ptr.value, fb, S)                 # frame 0 -> source, on S
        d.ingest_frames(0, [dict(colour=views[0][0], depth=views[0][1])], stream=S)
        d.ingest_release(0, 1, S)
        rt.memcpy_h2d_async(src[0].ptr.value, pb.ptr.value + fb, fb, S)            # frame 1 over the source, behind the release
        check_slot(d, 0, host[0][0], host[0][1], "first data")
        rt.stream_synchronize(S)
        assert np.array_equal(src[0].download(np.uint8, (H, W, 3)), host[1][0])
        # twice in a row into one slot: the second waits the first out and wins
        src[1].upload(pb.view(np.uint8, (fb,), offset=2 * fb))
        d.ingest_frame(1, *views[0])
        d.ingest_frame(1, *views[1], stream=S)
        check_slot(d, 1, host[2][0], host[2][1], "second ingest")
        # behind a pending pinned upload
        d.upload_frame_pinned(2, host[0][0], host[0][1])
        d.ingest_frame(2, *views[1])
        check_slot(d, 2, host[2][0], host[2][1], "ingest behind a pinned upload")
        d.ingest_frame(3, *views[0])
        d.upload_frame_pinned(3, host[0][0], host[0][1])
        check_slot(d, 3, host[0][0], host[0][1], "pinned upload behind an ingest")
        d.upload_wait(-1)
    finally:
        rt.stream_synchronize(S)
        rt.stream_destroy(S)
    d.close()
    for s in src:
        s.close()
    pb.close()


def test_refusals(rig):
    """Every validation of lm_ingest_frames with its words, argument checks before slot checks; a slot held by a lane in flight is refused with
    the existing words and taken after match_end."""
    lm, d, W, H = rig.lm, rig.d, rig.W, rig.H
    lib, h = d.lib, d.h
    good_c = lm.image_desc(rig.frame["colour"], order="rgb", layout="chw")
    good_d = lm.image_desc(rig.frame["depth"], depth=True, scale=1000.0)

    def call(first=3, n=1, colour=good_c, depth=good_d, edit_c=None, edit_d=None, null_c=False, null_d=False, frame=0):
        ca, da = (lm.ImageDesc * max(n, 1))(), (lm.ImageDesc * max(n, 1))()
        for k in range(max(n, 1)):
            for arr, src, edit in ((ca, colour, edit_c), (da, depth, edit_d)):
                C.memmove(C.byref(arr[k]), C.byref(src), C.sizeof(lm.ImageDesc))
                if k == frame:
                    for name, value in (edit or {}).items():
                        setattr(arr[k], name, value)
        rc = lib.lm_ingest_frames(h, first, n, None if null_c else ca, None if null_d else da, None, None)
        return rc, (lib.lm_last_error().decode() if rc else "")

    d.upload_wait(-1)
    assert call() == (0, "")
    assert call(null_c=True) == (INVALID, "bad argument")
    assert call(null_d=True) == (INVALID, "bad argument")
    assert call(n=0) == (INVALID, "bad argument")
    assert call(n=-2) == (INVALID, "bad argument")
    assert call(first=4) == (INVALID, "slot out of range")
    assert call(first=2, n=3) == (INVALID, "slot out of range")
    assert call(edit_c={"format": 99}) == (INVALID, "colour image of frame 0: unknown pixel format 99")
    assert call(edit_d={"format": -1}) == (INVALID, "depth image of frame 0: unknown pixel format -1")
    assert call(edit_c={"format": lm.PIX_DEPTH_U16}) == (INVALID, "colour image of frame 0: LM_PIX_DEPTH_U16 is a depth format")
    assert call(edit_d={"format": lm.PIX_BGRA8}) == (INVALID, "depth image of frame 0: LM_PIX_BGRA8 is a colour format")
    roi = "0 <= roi.x && roi.x + roi.width <= m.cols && 0 <= roi.y && roi.y + roi.height <= m.rows failed: window 320 x 240 at "
    assert call(edit_c={"crop_x": 1}) == (INVALID, "colour image of frame 0: " + roi + "(1, 0) in a 320 x 240 source")
    assert call(edit_c={"crop_y": -1}) == (INVALID, "colour image of frame 0: " + roi + "(0, -1) in a 320 x 240 source")
    assert call(first=2, n=2, edit_d={"height": 239}, frame=1) == (INVALID, "depth image of frame 1: " + roi + "(0, 0) in a 320 x 239 source")
    assert call(edit_d={"crop_x": 8, "width": 327}) == (INVALID, "depth image of frame 0: " + roi + "(8, 0) in a 327 x 240 source")
    assert call(edit_c={"row_stride": W - 1}) == (INVALID, "colour image of frame 0: row_stride smaller than a window row")
    assert call(edit_d={"row_stride": W * 4 - 4}) == (INVALID, "depth image of frame 0: row_stride smaller than a window row")
    assert call(edit_c={"plane_stride": 0}) == (INVALID, "colour image of frame 0: plane_stride must be positive")
    f32, u16 = "data and row_stride of a f32 source must be multiples of 4", "data and row_stride of a u16 source must be multiples of 2"
    assert call(edit_d={"data": good_d.data + 2}) == (INVALID, "depth image of frame 0: " + f32)
    assert call(edit_d={"row_stride": W * 4 + 2}) == (INVALID, "depth image of frame 0: " + f32)
    assert call(edit_d={"format": lm.PIX_DEPTH_U16, "data": good_d.data + 1}) == (INVALID, "depth image of frame 0: " + u16)
    assert call(edit_d={"format": lm.PIX_DEPTH_U16, "row_stride": W * 2 + 1}) == (INVALID, "depth image of frame 0: " + u16)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(edit_d={"scale": bad}) == (INVALID, "depth image of frame 0: scale must be finite and positive")
    assert call(edit_d={"format": lm.PIX_DEPTH_U16, "row_stride": W * 2, "scale": 0.0}) == (0, "")      # (scale belongs to f32 alone)
    # the slots: a lane in flight holds slot 1
    for s in range(4):
        d.upload_frame(s, rig.bgr, rig.depth)
    before = d.read_frame(1)
    d.match_begin(1, 1, 1, rig.THR, 0)
    try:
        assert call(first=1) == (INVALID, BUSY)
        assert call(first=0, n=2) == (INVALID, BUSY)
        assert call(first=1, n=3) == (INVALID, BUSY)
        assert call(first=1, edit_c={"format": 99}) == (INVALID, "colour image of frame 0: unknown pixel format 99")      # the first check wins
        assert call(first=1, null_c=True) == (INVALID, "bad argument")
        assert call(first=2, n=2) == (0, "")
        assert call(first=0) == (0, "")
    finally:
        out, cnt = d.match_end(1, n_slots=1)
    assert_matches_equal(out[0, :cnt[0]], rig.exp)
    after = d.read_frame(1)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert call(first=1) == (0, "")
    assert_matches_equal(d.match_slot(1, rig.THR, 0), rig.exp)
    # a colour check in flight: the existing words again
    m = d.match_slot(0, rig.THR, 0)[:3].copy()
    sl = np.zeros(len(m), np.int32)
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(180, 255, 255)
    d._check(lib.lm_color_check_begin_slots(h, sl.ctypes.data_as(C.c_void_p), lo, hi, m.ctypes.data_as(C.c_void_p), len(m)))
    try:
        assert call(first=0) == (INVALID, "slot is read by a colour check in flight: call lm_color_check_end first")
        assert call(first=1) == (0, "")
    finally:
        a, b = np.zeros(len(m), np.int64), np.zeros(len(m), np.int64)
        d._check(lib.lm_color_check_end(h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
    assert call(first=0) == (0, "")
