"""Raw depth registered onto the colour camera on the GPU (ABI 0.13): lm_ingest_frames_registered and
lm_stage_register_depth on a 160 x 80 RGB-D detector, compared byte for byte -- through read_frame or stage_register_depth -- with
tests/register_reference.py fed with the ray table the detector returns (registration_rays), and with ingest_reference's crop, mirror and
shift of the registered image.  The scenes (tests/register_scenes.py) are checked on the REFERENCE for holes, occlusion decided by the
minimum, collisions and depth pixels that leave the window, so that no comparison passes vacuously."""
import ctypes as C

import numpy as np
import pytest

import ingest_reference as IR
import register_reference as RR
import register_scenes as S
from conftest import assert_matches_equal

pytestmark = pytest.mark.gpu

W, H, CW, CH, CROP = S.W, S.H, S.CW, S.CH, S.CROP
INVALID = 1


def to_cam(lm, c):
    return lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["dist"])


class Stage:
    """The 160 x 80 RGB-D detector, a 208 x 120 BGR colour image in device memory, and device copies of raw depth images."""

    def __init__(self, lm):
        self.lm = lm
        self.d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
        self.bgr = np.random.default_rng(3).integers(0, 256, (CH, CW, 3), dtype=np.uint8)
        self.cbuf = lm.DeviceBuffer(self.bgr.nbytes)
        self.cbuf.upload(self.bgr)
        self.colour = self.cbuf.view(np.uint8, self.bgr.shape)
        self.bufs = []
        self._ref = {}

    def raw(self, image, pad=0):
        """A device copy of a raw depth image, rows `pad` elements longer than their pixels, that ends where the image ends."""
        h, w = image.shape
        item = image.dtype.itemsize
        rs = (w + pad) * item
        host = np.zeros((h, w + pad), image.dtype)
        host[:, :w] = image
        buf = self.lm.DeviceBuffer((h - 1) * rs + w * item)
        buf.upload(host.reshape(-1)[:(h - 1) * (w + pad) + w])
        self.bufs.append(buf)
        return buf.view(image.dtype.type, (h, w), strides=(rs, item))

    def register(self, dc, cc, splat=(0, 0), R=S.ROT, t=S.TRANS):
        self.d.set_registration(to_cam(self.lm, dc), to_cam(self.lm, cc), R, t, splat=splat)
        return self.d.registration_rays()

    def reference(self, key, make):
        """A reference image, computed once and shared."""
        if key not in self._ref:
            self._ref[key] = make()
        return self._ref[key]

    def close(self):
        self.d.close()
        self.cbuf.close()
        for b in self.bufs:
            b.close()


@pytest.fixture(scope="module")
def stage(lm):
    s = Stage(lm)
    yield s
    s.close()


def check_slot(d, slot, exp_bgr, exp_depth, what):
    bgr, depth = d.read_frame(slot)
    if exp_bgr is not None:
        assert np.array_equal(bgr, exp_bgr), "%s: colour differs at %d bytes" % (what, int((bgr != exp_bgr).sum()))
    assert np.array_equal(depth, exp_depth), "%s: depth differs at %d pixels" % (what, int((depth != exp_depth).sum()))


def scene_a_reference(stage, dist, splat, far=0.0):
    """Sets scene A's registration; (Rg, stats) of the reference with the detector's own ray table."""
    dc, cc = S.depth_cam_a(dist), S.colour_cam(dist)
    rays = stage.register(dc, cc, splat)
    return stage.reference(("A", dist, splat, far), lambda: RR.register(S.scene_a(far=far), 1.0, rays, cc, S.ROT, S.TRANS, splat, stats=True))


@pytest.mark.parametrize("dist", [S.ZERO, S.DIST], ids=["pinhole", "brown"])
@pytest.mark.parametrize("splat", [(0, 0), (1, 1), (2, 1)], ids=["splat00", "splat11", "splat21"])
def test_scene_a(stage, dist, splat):
    d = stage.d
    Rg, st = scene_a_reference(stage, dist, splat)
    win, cnt, zmax = S.window(Rg), S.window(st["count"]), S.window(st["zmax"])
    u, v = st["u"], st["v"]
    outside = int(((u < CROP[0]) | (u >= CROP[0] + W) | (v < CROP[1]) | (v >= CROP[1] + H)).sum())
    print("holes %d, pixels decided by occlusion %d, pixels with two or more contributors %d, valid depth pixels outside the window %d"
          % ((win == 0).sum(), ((zmax - win.astype(np.int64)) > 100).sum(), (cnt >= 2).sum(), outside))
    assert outside > 1000
    if splat == (0, 0):
        assert (win == 0).sum() > 5000
    if splat == (1, 1):
        assert ((zmax - win.astype(np.int64)) > 100).sum() >= 400 and (cnt >= 2).sum() > 5000
    raw = S.scene_a()
    assert np.array_equal(d.stage_register_depth(raw), Rg), "the whole registered image differs"
    src = stage.reference("A raw", lambda: stage.raw(raw))
    d.ingest_frame(1, stage.colour, src, crop=CROP, register_depth=True)
    check_slot(d, 1, IR.colour(stage.bgr, W, H, crop=CROP), win, "scene A %s %s" % (dist, splat))


def test_scene_b(stage):
    """Down-sampling: four u16 raw pixels per colour pixel, splat (0, 0)."""
    d = stage.d
    dc, cc = S.depth_cam_b(), S.colour_cam()
    rays = stage.register(dc, cc)
    Rg, st = stage.reference("B", lambda: RR.register(S.scene_b(), 1.0, rays, cc, S.ROT, S.TRANS, (0, 0), stats=True))
    assert (S.window(st["distinct"]) >= 3).sum() >= 1000
    assert np.array_equal(d.stage_register_depth(S.scene_b()), Rg)
    src = stage.raw(S.scene_b(), pad=3)         # rows that are no multiple of 4 bytes long
    d.ingest_frame(2, stage.colour, src, crop=CROP, register_depth=True)
    check_slot(d, 2, IR.colour(stage.bgr, W, H, crop=CROP), S.window(Rg), "scene B")


def test_geometry(stage):
    """Odd crops, the window flush with each edge of the colour geometry, mirror with odd shifts of both signs, a shift beyond the frame,
    and the colour window at another crop than the depth window."""
    d = stage.d
    Rg, _ = scene_a_reference(stage, S.DIST, (1, 1))
    src = stage.reference("A raw", lambda: stage.raw(S.scene_a()))
    cases = [((1, 3), False, (0, 0)), ((23, 7), False, (0, 0)), ((0, 0), False, (0, 0)), ((CW - W, 0), False, (0, 0)), ((0, CH - H), False, (0, 0)),
             ((CW - W, CH - H), True, (0, 0)), (CROP, True, (3, -1)), (CROP, True, (-5, 7)), ((7, 11), True, (1, 1)), (CROP, False, (-3, 5)),
             (CROP, False, (W, 0)), (CROP, True, (0, -H - 3)), (CROP, False, (W - 1, H - 1))]
    for k in range(0, len(cases), 4):
        group = cases[k:k + 4]
        d.ingest_frames(0, [dict(colour=stage.colour, depth=src, crop=crop, flip_x=flip, shift=shift, register_depth=True) for crop, flip, shift in group])
        for s, (crop, flip, shift) in enumerate(group):
            check_slot(d, s, IR.colour(stage.bgr, W, H, crop=crop, flip_x=flip, shift=shift), IR.depth(Rg, W, H, crop, 1.0, flip, shift),
                       "crop %s flip %s shift %s" % (crop, flip, shift))
    exp = IR.depth(Rg, W, H, CROP, 1.0, True, (3, -1))
    assert (exp != 0).sum() > 5000 and not np.array_equal(exp, S.window(Rg))
    assert not IR.depth(Rg, W, H, CROP, 1.0, False, (W, 0)).any()
    # the colour source is not the whole sensor image: its window lies elsewhere than the depth window
    d.ingest_frame(3, stage.colour, src, crop=(5, 33), depth_crop=(41, 9), flip_x=True, shift=(-1, 2), register_depth=True)
    check_slot(d, 3, IR.colour(stage.bgr, W, H, crop=(5, 33), flip_x=True, shift=(-1, 2)), IR.depth(Rg, W, H, (41, 9), 1.0, True, (-1, 2)), "two crops")


def test_stale_scratch(stage):
    """Two calls into the same slots, the second scene everywhere farther than the first: a z-buffer that kept the first call's minima
    would show them."""
    d = stage.d
    near, _ = scene_a_reference(stage, S.ZERO, (1, 1))
    far, _ = scene_a_reference(stage, S.ZERO, (1, 1), far=700.0)
    a, b = S.window(near), S.window(far)
    both = (a != 0) & (b != 0)
    assert both.sum() > 5000 and (b[both] > a[both]).all()
    src_near = stage.reference("A raw", lambda: stage.raw(S.scene_a()))
    src_far = stage.reference("A raw far", lambda: stage.raw(S.scene_a(far=700.0)))
    for slot in (0, 1):
        d.ingest_frames(slot, [dict(colour=stage.colour, depth=src_near, crop=CROP, register_depth=True)] * 2)
        d.ingest_frames(slot, [dict(colour=stage.colour, depth=src_far, crop=CROP, register_depth=True)] * 2)
        check_slot(d, slot, None, b, "the second call, slot %d" % slot)
        check_slot(d, slot + 1, None, b, "the second call, slot %d" % (slot + 1))


def test_batches(stage):
    """Three different raw images -- millimetres, another noise, metres with scale 1000 -- in one call equal three single calls and the
    reference."""
    d = stage.d
    dc, cc = S.depth_cam_a(S.DIST), S.colour_cam(S.DIST)
    rays = stage.register(dc, cc, (2, 1))
    metres = (S.scene_a(seed=9) / np.float32(1000.0)).astype(np.float32)
    raws = [(S.scene_a(), 1.0), (S.scene_a(seed=8, far=100.0), 1.0), (metres, 1000.0)]
    srcs = [stage.raw(r, pad=k) for k, (r, _) in enumerate(raws)]
    exp = [S.window(RR.register(r, sc, rays, cc, S.ROT, S.TRANS, (2, 1))) for r, sc in raws]
    assert not np.array_equal(exp[0], exp[1]) and not np.array_equal(exp[0], exp[2])
    d.ingest_frames(1, [dict(colour=stage.colour, depth=s, depth_scale=sc, crop=CROP, register_depth=True) for s, (_, sc) in zip(srcs, raws)])
    batch = [d.read_frame(1 + k)[1] for k in range(3)]
    for k in range(3):
        assert np.array_equal(batch[k], exp[k]), "frame %d of the batch" % k
        d.ingest_frame(0, stage.colour, srcs[k], depth_scale=raws[k][1], crop=CROP, register_depth=True)
        assert np.array_equal(d.read_frame(0)[1], batch[k]), "frame %d alone" % k


def test_producer_stream(stage):
    """The producer-stream form and ingest_release: the raw image is filled by an asynchronous copy on a stream, ingested at once with
    that stream, released to it and overwritten on it -- the slot holds the registration of the FIRST data.  (This exercises the path; it
    cannot prove the ordering.)"""
    from hip_runtime import Runtime
    lm, d = stage.lm, stage.d
    Rg, _ = scene_a_reference(stage, S.ZERO, (1, 1))
    first, second = S.scene_a(), S.scene_a(far=700.0)
    pb = lm.PinnedBuffer(2 * first.nbytes)
    host = [pb.view(np.float32, first.shape, offset=k * first.nbytes) for k in range(2)]
    host[0][...] = first
    host[1][...] = second
    src = lm.DeviceBuffer(first.nbytes)
    rt = Runtime()
    st = rt.stream_create()
    try:
        rt.memcpy_h2d_async(src.ptr.value, pb.ptr.value, first.nbytes, st)
        d.ingest_frame(2, stage.colour, src.view(np.float32, first.shape), crop=CROP, register_depth=True, stream=st)
        d.ingest_release(2, 1, st)
        rt.memcpy_h2d_async(src.ptr.value, pb.ptr.value + first.nbytes, first.nbytes, st)
        check_slot(d, 2, IR.colour(stage.bgr, W, H, crop=CROP), S.window(Rg), "first data")
        rt.stream_synchronize(st)
        assert np.array_equal(src.download(np.uint32, first.shape), second.view(np.uint32))        # (bits: the scene holds NaN)
        d.upload_wait(-1)
    finally:
        rt.stream_synchronize(st)
        rt.stream_destroy(st)
    src.close()
    pb.close()


def test_identity_reproduces_the_plain_ingest_and_its_matches(lm, orc, synth):
    """Equal cameras, identity extrinsics, splat 0: the registered ingest of a depth image is the plain ingest of it, byte for byte, and
    match_slot returns equal lists on both slots."""
    RW, RH, THR = 320, 240, 75.0
    d = lm.Detector(color_only=False, width=RW, height=RH, frame_slots=2)
    bgr, depth = synth.make_frame(RW, RH, seed=500)
    o = orc.Detector(color_only=False)
    o.prepare(bgr, depth)
    q = {(l, m): o.stage(0, l, m).reshape(RH >> l, RW >> l) for l in range(2) for m in range(2)}
    descs, feats, _ = synth.make_bank(40, 2, 2, seed=99, size_range=(48, 120), quantized=q, crop_fraction=0.3, frame_size=(RW, RH), T0=d.get_T(0))
    d.add_class("c", descs, feats)
    k = lm.camera(RW, RH, 300.0, 300.0, 159.5, 119.5)
    d.set_registration(k, k, np.eye(3), np.zeros(3))
    cb, db = lm.DeviceBuffer(bgr.nbytes), lm.DeviceBuffer(depth.nbytes)
    cb.upload(bgr)
    db.upload(depth)
    cv, dv = cb.view(np.uint8, bgr.shape), db.view(np.uint16, depth.shape)
    d.ingest_frame(0, cv, dv)
    d.ingest_frame(1, cv, dv, register_depth=True)
    plain, reg = d.read_frame(0), d.read_frame(1)
    assert (depth != 0).sum() > 1000
    assert np.array_equal(plain[1], depth) and np.array_equal(reg[1], depth) and np.array_equal(reg[0], plain[0])
    m0, m1 = d.match_slot(0, THR, 0), d.match_slot(1, THR, 0)
    assert len(m0) > 0
    assert_matches_equal(m1, m0)
    d.close()
    cb.close()
    db.close()


def test_refusals(stage):
    """Every refusal of lm_ingest_frames_registered with its words, before anything is enqueued: the slot holds what it held."""
    lm, d = stage.lm, stage.d
    lib = d.lib
    scene_a_reference(stage, S.ZERO, (1, 1))
    src = stage.reference("A raw", lambda: stage.raw(S.scene_a()))
    good_c = lm.image_desc(stage.colour, crop=CROP)
    good_d = lm.image_desc(src, depth=True, crop=CROP)

    def call(edit_c=None, edit_d=None, det=None, first=3):
        ca, da = (lm.ImageDesc * 1)(), (lm.ImageDesc * 1)()
        for arr, base, edit in ((ca, good_c, edit_c), (da, good_d, edit_d)):
            C.memmove(C.byref(arr[0]), C.byref(base), C.sizeof(lm.ImageDesc))
            for name, value in (edit or {}).items():
                setattr(arr[0], name, value)
        rc = lib.lm_ingest_frames_registered((det or d).h, first, 1, ca, da, None, None)
        return rc, (lib.lm_last_error().decode() if rc else "")

    who = "raw depth image of frame 0: "
    d.upload_wait(-1)
    d.ingest_frame(3, stage.colour, src, crop=CROP, register_depth=True)
    before = d.read_frame(3)
    assert call(first=2) == (0, "")
    # the detector
    plain = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
    assert call(det=plain) == (INVALID, "no registration set: lm_set_registration first")
    plain.close()
    mono = lm.Detector(color_only=True, width=W, height=H, T=[2, 8], frame_slots=4)
    assert call(det=mono) == (INVALID, "lm_ingest_frames_registered needs an RGB-D detector: a colour-only detector holds no depth frame")
    mono.close()
    # the raw image
    for w_, h_ in ((95, 64), (96, 65), (CW, CH)):
        assert call(edit_d={"width": w_, "height": h_}) == (INVALID, who + "a %d x %d image is not the registration's depth camera (96 x 64)" % (w_, h_))
    for cx, cy in ((-1, 0), (0, -1), (CW - W + 1, 0), (0, CH - H + 1), (1 << 30, 0)):
        assert call(edit_d={"crop_x": cx, "crop_y": cy}) == \
            (INVALID, who + "window %d x %d at (%d, %d) lies outside the %d x %d colour geometry" % (W, H, cx, cy, CW, CH))
    for name in ("BGR8", "BGRA8", "RGB8_PLANAR", "GRAY8", "NV12", "UYVY"):
        assert call(edit_d={"format": getattr(lm, "PIX_" + name)}) == (INVALID, who + "LM_PIX_%s is a colour format" % name)
    for bad in (99, -1, lm.PIX_DEPTH_F32 | lm.PIX_YUV_FULL):
        assert call(edit_d={"format": bad}) == (INVALID, who + "unknown pixel format %d" % bad)
    assert call(edit_d={"data": None}) == (INVALID, who + "null data pointer")
    assert call(edit_d={"row_stride": 96 * 4 - 4}) == (INVALID, who + "row_stride smaller than a raw row")
    assert call(edit_d={"row_stride": 96 * 4 + 2}) == (INVALID, who + "data and row_stride of a f32 source must be multiples of 4")
    assert call(edit_d={"data": good_d.data + 2}) == (INVALID, who + "data and row_stride of a f32 source must be multiples of 4")
    assert call(edit_d={"format": lm.PIX_DEPTH_U16, "data": good_d.data + 1}) == (INVALID, who + "data and row_stride of a u16 source must be multiples of 2")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(edit_d={"scale": bad}) == (INVALID, who + "scale must be finite and positive")
    # the colour image and the slots: lm_ingest_frames' own refusals
    assert call(edit_c={"format": lm.PIX_DEPTH_U16}) == (INVALID, "colour image of frame 0: LM_PIX_DEPTH_U16 is a depth format")
    assert call(edit_c={"crop_x": CW - W + 1})[0] == INVALID
    assert call(first=4) == (INVALID, "slot out of range")
    # the stage hook refuses the same images
    out = np.zeros((CH, CW), np.uint16)
    bad = lm.ImageDesc()
    C.memmove(C.byref(bad), C.byref(good_d), C.sizeof(lm.ImageDesc))
    bad.width = 95
    assert lib.lm_stage_register_depth(d.h, C.byref(bad), out.ctypes.data_as(C.c_void_p)) == INVALID
    assert lib.lm_last_error().decode() == who + "a 95 x 64 image is not the registration's depth camera (96 x 64)"
    # nothing was enqueued by any refusal: upload_wait has nothing to wait for and slot 3 holds what it held
    d.upload_wait(3)
    after = d.read_frame(3)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_resources(lm):
    """A detector that registered, on two copy streams and through the stage hook, gives everything back."""
    start = lm.live_resources()
    for cycle in range(2):
        d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
        d.set_registration(to_cam(lm, S.depth_cam_a(S.DIST)), to_cam(lm, S.colour_cam(S.DIST)), S.ROT, S.TRANS, splat=(1, 1))
        bgr = np.zeros((CH, CW, 3), np.uint8)
        cb, db = lm.DeviceBuffer(bgr.nbytes), lm.DeviceBuffer(S.scene_a().nbytes)
        cb.upload(bgr)
        db.upload(S.scene_a())
        frame = dict(colour=cb.view(np.uint8, bgr.shape), depth=db.view(np.float32, (64, 96)), crop=CROP, register_depth=True)
        d.ingest_frames(0, [frame])
        d.ingest_frames(1, [frame])
        d.ingest_frames(0, [frame] * 4)          # (the first stream's z-buffer grows)
        d.stage_register_depth(S.scene_a())
        d.upload_wait(-1)
        live = lm.live_resources()
        assert live[0] > start[0] + 2, (live, start)
        steady = lm.live_resources()
        d.ingest_frames(0, [frame] * 4)
        d.upload_wait(-1)
        assert lm.live_resources() == steady, "a registered ingest in the steady state created or released a resource"
        d.close()
        cb.close()
        db.close()
        assert lm.live_resources() == start, (cycle, lm.live_resources(), start)
