"""The float destinations of lm_export_frames on the GPU (0.13 additive): the twelve non-grey float formats, the window
offset inside a larger surface whose every byte was drawn beforehand, the surface at every misalignment class of its elements, the ingest's
mirror and an odd shift undone, a few primitives drawn.  A case compares the WHOLE allocation with the reference's: inside the window
tests/export_reference.py's 8-bit image through tests/ingest_float_reference.py's conversion, outside it the bytes that were there.
Then the round trip: exporting F32 at 1 / 255 and ingesting it again at 255 reproduces the slot's frame."""
import numpy as np
import pytest

import export_reference as ER
import ingest_float_reference as FR

pytestmark = pytest.mark.gpu

DESTINATIONS = [f for f in FR.FORMATS if f & 15 != 8]
W, H, SW, SH = 48, 32, 59, 39          # the frame (one ragged tile) and the larger surface; the window at (7, 5) reaches the surface's corner - 4


class Target:
    """A float surface in device memory (FR.Source lays it out: the allocation ends where the surface ends, rows and planes one element
    longer than dense, every byte drawn), and the same bytes on the host."""

    def __init__(self, lm, rng, fmt, offset, window):
        self.s = s = FR.Source(fmt, SW, SH, rng, offset=offset)
        self.fmt, self.window = fmt, window
        self.buf = lm.DeviceBuffer(len(s.raw))
        self.buf.upload(s.raw)
        self.view = self.buf.view(s.dtype, s.host.shape, offset=offset, strides=s.strides())

    def spec(self, scale):
        return dict(target=self.view, order=self.s.order, layout=self.s.layout, window=self.window, float_scale=scale)

    def want(self, E, scale):
        """The allocation after an export of the W x H BGR image E: the window's elements replaced, nothing else"""
        s = self.s
        half = s.es == 2
        raw = s.raw.copy()
        el = raw[s.offset:].view(np.uint16 if half else np.uint32)
        strided = np.lib.stride_tricks.as_strided
        C = E[..., ::-1] if s.order == "rgb" else E
        cx, cy = self.window
        if s.layout == "hwc":
            v = strided(el, (SH, SW, s.nch), s.strides())
            v[cy:cy + H, cx:cx + W, :3] = FR.from_u8(C, scale, half)
            if s.nch == 4:
                v[cy:cy + H, cx:cx + W, 3] = FR.from_u8(np.uint8(255), scale, half)
        else:
            v = strided(el, (3, SH, SW), s.strides())
            v[:, cy:cy + H, cx:cx + W] = FR.from_u8(np.transpose(C, (2, 0, 1)), scale, half)
        return raw

    def check(self, E, scale, what):
        got, want = self.buf.download(np.uint8, (len(self.s.raw),)), self.want(E, scale)
        assert np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))
        assert (want != self.s.raw).any(), what

    def close(self):
        self.buf.close()


def make_prims(lm, rows):
    p = np.zeros(len(rows), lm.DRAW_PRIM_DTYPE)
    for k, r in enumerate(rows):
        p[k] = r
    return p


@pytest.mark.parametrize("half", [0, 0x10], ids=["f32", "f16"])
def test_every_float_destination(lm, half):
    """Six layouts x every element multiple below 16 bytes x two windows, scales 1 / 255, 1 and 1 / 127.5; mirror and an odd shift undone,
    a ring, a segment and a box drawn; four frames of mixed layouts per call, one of them an 8-bit destination's neighbour in the same call."""
    d = lm.Detector(color_only=True, width=W, height=H, T=[2, 8], frame_slots=4)
    rng = np.random.default_rng(71 + half)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(4)]
    for s, f in enumerate(frames):
        d.upload_frame(s, f)
    rows = []
    for s in range(4):
        rows += [(lm.DRAW_BOX, s, 5, 4, 24, 16, 2, 0, 255, 0, 255), (lm.DRAW_RING, s, 30, 16, 6, 0, 1, 16, 32, 255, 128), (lm.DRAW_SEGMENT, s, 2, 29, 45, 3, 3, 255, 0, 0, 200)]
    prims = make_prims(lm, rows)
    undo = [dict(flip_x=True, shift=(3, -1)), None, dict(shift=(-5, 7)), dict(flip_x=True)]
    opts = [(True, (3, -1)), (False, (0, 0)), (False, (-5, 7)), (True, (0, 0))]
    E = [ER.undo(ER.annotate(frames[s], prims, s), *opts[s]) for s in range(4)]
    scales = (float(np.float32(1.0) / np.float32(255.0)), 1.0, float(np.float32(1.0) / np.float32(127.5)))
    formats = [f for f in DESTINATIONS if f & 0x10 == half]
    cases = [(fmt, off, window) for off in range(0, 16, 2 if half else 4) for window in ((7, 5), (0, 0)) for fmt in formats]
    assert len(cases) % 4 == 0
    for i in range(0, len(cases), 4):
        scale = scales[(i // 4) % 3]
        targets = [Target(lm, rng, fmt, off, window) for fmt, off, window in cases[i:i + 4]]
        d.export_frames(0, [t.spec(scale) for t in targets], prims, undo)
        for s, (t, case) in enumerate(zip(targets, cases[i:i + 4])):
            t.check(E[s], scale, "format 0x%x offset %d window %s scale %r" % (case + (scale,)))
            t.close()
    # an 8-bit and a float destination in one call: each kernel takes its own frames, and is launched only for them
    u8 = lm.DeviceBuffer(H * W * 3)
    t = Target(lm, rng, formats[3], 0, (7, 5))
    c0 = lm.launch_counts()
    d.export_frames(0, [u8.view(np.uint8, (H, W, 3)), t.spec(1.0)], prims[prims["frame"] < 2], undo[:2])
    c1 = lm.launch_counts()
    d.export_frames(0, [u8.view(np.uint8, (H, W, 3))])
    c2 = lm.launch_counts()
    d.export_frames(1, [t.spec(1.0)])
    c3 = lm.launch_counts()
    assert [(b["export"] - a["export"], b["export_float"] - a["export_float"]) for a, b in ((c0, c1), (c1, c2), (c2, c3))] == [(1, 1), (1, 0), (0, 1)]
    assert all(c3[k] == c0[k] for k in c0 if not k.startswith("export"))
    d.export_frames(0, [u8.view(np.uint8, (H, W, 3)), t.spec(1.0)], prims[prims["frame"] < 2], undo[:2])
    assert np.array_equal(u8.download(np.uint8, (H, W, 3)), E[0])
    t.check(E[1], 1.0, "beside an 8-bit destination")
    t.close()
    u8.close()
    d.close()


def test_round_trip(lm):
    """Export as RGB_F32_PLANAR at 1 / 255 (a network's input), ingest that tensor at 255: the slot's frame again, byte for byte."""
    Wr, Hr = 160, 80
    d = lm.Detector(color_only=True, width=Wr, height=Hr, T=[2, 8], frame_slots=2)
    frame = np.random.default_rng(73).integers(0, 256, (Hr, Wr, 3), dtype=np.uint8)
    frame[1:3].reshape(-1)[:256] = np.arange(256)          # (every byte value is there whatever was drawn)
    d.upload_frame(0, frame)
    buf = lm.DeviceBuffer(3 * Hr * Wr * 4)
    tensor = buf.view(np.float32, (3, Hr, Wr))
    scale = float(np.float32(1.0) / np.float32(255.0))
    d.export_frame(0, tensor, layout="chw", order="rgb", float_scale=scale)
    host = buf.download(np.float32, (3, Hr, Wr))
    assert np.array_equal(host.view(np.uint32), FR.from_u8(np.transpose(frame[..., ::-1], (2, 0, 1)), scale, False))
    assert host.max() == 1.0 and host.min() == 0.0
    d.ingest_frame(1, tensor, layout="chw", order="rgb", float_scale=255.0)
    assert np.array_equal(d.read_frame(1)[0], frame)
    buf.close()
    d.close()


def test_refusals_through_the_library(lm):
    """Grey float formats are source formats; alignment and scale are refused before anything is written."""
    d = lm.Detector(color_only=True, width=W, height=H, T=[2, 8], frame_slots=1)
    d.upload_frame(0, np.zeros((H, W, 3), np.uint8))
    rng = np.random.default_rng(74)
    t = Target(lm, rng, 0x2004, 0, (7, 5))
    who = "destination image of frame 0: "
    good = lm.image_desc(t.view, layout="chw", crop=(7, 5), float_scale=1.0)

    def call(**edit):
        a = (lm.ImageDesc * 1)()
        for name, _ in lm.ImageDesc._fields_:
            setattr(a[0], name, edit.get(name, getattr(good, name)))
        rc = d.lib.lm_export_frames(d.h, 0, 1, a, None, None, 0)
        return rc, (d.lib.lm_last_error().decode() if rc else "")

    for edit, words in ((dict(format=0x2008), "LM_PIX_GRAY_F32 is a source format: not served as a destination"),
                        (dict(format=0x2018), "LM_PIX_GRAY_F16 is a source format: not served as a destination"),
                        (dict(format=0x2006), "unknown pixel format %d" % 0x2006), (dict(format=0x2020), "unknown pixel format %d" % 0x2020),
                        (dict(data=good.data + 2), "data and row_stride of a f32 source must be multiples of 4"),
                        (dict(plane_stride=good.plane_stride + 2), "plane_stride of a f32 source must be a multiple of 4"),
                        (dict(format=0x2014, data=good.data + 1), "data and row_stride of a f16 source must be multiples of 2"),
                        (dict(scale=0.0), "scale must be finite and positive"), (dict(scale=float("nan")), "scale must be finite and positive")):
        assert call(**edit) == (1, who + words)
    assert np.array_equal(t.buf.download(np.uint8, (len(t.s.raw),)), t.s.raw)
    assert call() == (0, "")
    t.close()
    d.close()
