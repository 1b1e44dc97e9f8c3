"""CPU tests of the ingest path (lm_ingest_frames): what the binding makes of a __cuda_array_interface__, the
library's refusal to run without a device, and the numpy reference the GPU tests compare with -- its float rule on the table of special
values and its geometry against an independently written shift."""
import numpy as np
import pytest

import ingest_reference as IR


class Fake:
    """Something that claims to live in device memory: nothing but the interface, with a made-up pointer."""

    def __init__(self, shape, typestr, strides=None, ptr=0x7F0012345600):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "strides": strides, "version": 2}


def fields(d):
    return (d.data, d.row_stride, d.plane_stride, d.width, d.height, d.format, d.crop_x, d.crop_y, d.scale)


def test_exports_and_structures(lm):
    import ctypes as C
    lib = lm.load_library()
    for n in ("lm_ingest_frames", "lm_ingest_release", "lm_read_frame", "lm_device_alloc", "lm_device_free", "lm_device_copy"):
        assert n in lm.EXPORTS and getattr(lib, n).argtypes is not None
    assert C.sizeof(lm.ImageDesc) == 48 and C.sizeof(lm.IngestOpts) == 12
    assert lm.ImageDesc.row_stride.offset == 8 and lm.ImageDesc.width.offset == 24 and lm.ImageDesc.scale.offset == 44
    v = lib.lm_version()
    assert b"0.10" in v and b"lm_ingest_" in v and b"0.9" in v


@pytest.mark.parametrize("order,channels,fmt", [("bgr", 3, "PIX_BGR8"), ("rgb", 3, "PIX_RGB8"), ("bgr", 4, "PIX_BGRA8"), ("rgb", 4, "PIX_RGBA8")])
def test_interleaved_colour_descriptor(lm, order, channels, fmt):
    P = 0x7F0012345600
    # strides=None: C-contiguous
    d = lm.image_desc(Fake((97, 203, channels), "|u1"), order=order, crop=(3, 17))
    assert fields(d) == (P, 203 * channels, 0, 203, 97, getattr(lm, fmt), 3, 17, 1.0)
    # a row pitch that is no multiple of anything, an odd base pointer
    d = lm.image_desc(Fake((97, 203, channels), "|u1", (203 * channels + 3, channels, 1), ptr=P + 1), order=order)
    assert fields(d) == (P + 1, 203 * channels + 3, 0, 203, 97, getattr(lm, fmt), 0, 0, 1.0)
    # pixels that are not adjacent (every second column), channels that are not adjacent (a slice of a planar tensor seen as hwc)
    for strides in ((203 * channels * 2, channels * 2, 1), (203, 1, 203 * 97), (-203 * channels, channels, 1)):
        with pytest.raises(ValueError) as e:
            lm.image_desc(Fake((97, 203, channels), "|u1", strides), order=order)
        assert repr(strides) in str(e.value)


@pytest.mark.parametrize("order,fmt", [("bgr", "PIX_BGR8_PLANAR"), ("rgb", "PIX_RGB8_PLANAR")])
def test_planar_colour_descriptor(lm, order, fmt):
    P = 0x7F0012345600
    d = lm.image_desc(Fake((3, 97, 203), "|u1"), order=order, layout="chw")
    assert fields(d) == (P, 203, 203 * 97, 203, 97, getattr(lm, fmt), 0, 0, 1.0)
    d = lm.image_desc(Fake((3, 97, 203), "|u1", (206 * 97 + 5, 206, 1)), order=order, layout="chw", crop=(43, 0))
    assert fields(d) == (P, 206, 206 * 97 + 5, 203, 97, getattr(lm, fmt), 43, 0, 1.0)
    with pytest.raises(ValueError):
        lm.image_desc(Fake((3, 97, 203), "|u1", (203 * 97, 203 * 2, 2)), order=order, layout="chw")
    with pytest.raises(ValueError):      # four planes
        lm.image_desc(Fake((4, 97, 203), "|u1"), order=order, layout="chw")
    with pytest.raises(ValueError):      # an interleaved image announced as planar
        lm.image_desc(Fake((97, 203, 3), "|u1"), order=order, layout="chw")


def test_depth_descriptor(lm):
    P = 0x7F0012345600
    d = lm.image_desc(Fake((97, 203), "<u2"), depth=True, crop=(1, 2))
    assert fields(d) == (P, 406, 0, 203, 97, lm.PIX_DEPTH_U16, 1, 2, 1.0)
    d = lm.image_desc(Fake((97, 203), "<f4", (203 * 4 + 4, 4)), depth=True, scale=1000.0)
    assert fields(d) == (P, 816, 0, 203, 97, lm.PIX_DEPTH_F32, 0, 0, 1000.0)
    with pytest.raises(ValueError):      # every second pixel
        lm.image_desc(Fake((97, 203), "<u2", (812, 4)), depth=True)


def test_wrong_dtype_rank_and_object(lm):
    for obj, kw, needle in ((Fake((97, 203, 3), "<f4"), {}, "'<f4'"),                # float colour
                            (Fake((97, 203, 3), "<i2"), {}, "'<i2'"),                # a dtype no image has
                            (Fake((97, 203), "|u1"), {}, "(97, 203)"),               # grey image as colour
                            (Fake((97, 203, 2), "|u1"), {}, "(97, 203, 2)"),         # two channels
                            (Fake((97, 203), "|u1"), {"depth": True}, "'|u1'"),      # 8-bit depth
                            (Fake((97, 203, 1), "<u2"), {"depth": True}, "(97, 203, 1)"),
                            (Fake((97, 203), ">u2"), {"depth": True}, "'>u2'"),      # big-endian
                            (Fake((97, 203, 3), "|u1"), {"order": "gbr"}, "'gbr'"),
                            (Fake((97, 203, 3), "|u1"), {"layout": "nhwc"}, "'nhwc'")):
        with pytest.raises(ValueError) as e:
            lm.image_desc(obj, **kw)
        assert needle in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:
        lm.image_desc(np.zeros((97, 203, 3), np.uint8))      # host memory: numpy has no __cuda_array_interface__
    assert "ndarray" in str(e.value)


def test_device_view_carries_the_interface(lm):
    v = lm.DeviceView(0x1000, np.float32, (4, 6), (32, 4))
    assert v.__cuda_array_interface__ == {"shape": (4, 6), "typestr": "<f4", "data": (0x1000, False), "strides": (32, 4), "version": 2}
    assert lm.DeviceView(0x1000, np.uint8, (2, 3, 3)).__cuda_array_interface__["typestr"] == "|u1"
    assert lm.DeviceView(0x1000, np.uint16, (2, 3)).__cuda_array_interface__["typestr"] == "<u2"
    d = lm.image_desc(v, depth=True)
    assert (d.data, d.row_stride, d.format) == (0x1000, 32, lm.PIX_DEPTH_F32)


def _has_gpu(lm):
    d = lm.Detector(color_only=True, width=64, height=64, T=[2, 8])
    try:
        d.stage_pyrdown(np.zeros((8, 8, 3), np.uint8))
        return True
    except lm.LinemodError:
        return False
    finally:
        d.close()


def test_ingest_fails_loudly_without_gpu(lm):
    if _has_gpu(lm):
        pytest.skip("a HIP device is present")
    d = lm.Detector(color_only=False, width=160, height=80)
    col, dep = Fake((97, 203, 3), "|u1"), Fake((97, 203), "<u2")
    calls = (lambda: d.ingest_frame(0, col, dep),
             lambda: d.ingest_frames(0, [dict(colour=col, depth=dep)]),
             lambda: d.ingest_release(0, 1, None),
             lambda: d.read_frame(0),
             lambda: lm.DeviceBuffer(64))
    for call in calls:
        with pytest.raises(lm.LinemodError) as e:
            call()
        assert e.value.code == lm.LM_ERR_NO_DEVICE
        assert "no CPU fallback" in str(e.value)
    # what the binding itself can see is refused before the library is asked
    with pytest.raises(ValueError):
        d.ingest_frame(0, col)                       # RGB-D detector, no depth image
    with pytest.raises(ValueError):
        d.ingest_frames(0, [dict(colour=col, depth=dep, flip=True)])     # (flip_x)
    d.close()


# value, scale 1 -> expected u16.  Halves (ties to even), the saturation edge, large, non-finite, non-positive, ordinary.
SPECIAL = [(0.5, 0), (1.5, 2), (2.5, 2), (65534.5, 65534), (65535.5, 65535), (1e9, 65535), (3e9, 65535), (np.inf, 0), (-np.inf, 0),
           (np.nan, 0), (-0.0, 0), (-1.0, 0), (697.5, 698), (0.49999997, 0)]


def test_reference_float_rule_on_the_special_values():
    v = np.array([a for a, _ in SPECIAL], np.float32)
    exp = np.array([b for _, b in SPECIAL], np.uint16)
    got = IR.to_u16(v, 1.0)
    assert got.dtype == np.uint16 and np.array_equal(got, exp), (got, exp)
    # metres: the same values divided by 1000 in float32 first, then ONE float32 multiply by 1000 -- computed here value by value
    vm = v / np.float32(1000)
    got = IR.to_u16(vm, 1000.0)
    for k in range(len(v)):
        t = np.float32(vm[k]) * np.float32(1000)
        if not np.isfinite(t) or t <= 0:
            e = 0
        elif t >= 65535:
            e = 65535
        else:
            f = np.floor(np.float64(t))
            r = np.float64(t) - f
            e = int(f) + (1 if r > 0.5 or (r == 0.5 and int(f) % 2 == 1) else 0)
        assert got[k] == e, (v[k], vm[k], t, got[k], e)


def shift_with_zeros(img, sx, sy):
    """cv::warpAffine with a pure integer translation, written with slices (independent of ingest_reference's index arithmetic)."""
    H, W = img.shape[:2]
    out = np.zeros_like(img)
    if abs(sx) >= W or abs(sy) >= H:
        return out
    dst_y, src_y = (slice(sy, H), slice(0, H - sy)) if sy >= 0 else (slice(0, H + sy), slice(-sy, H))
    dst_x, src_x = (slice(sx, W), slice(0, W - sx)) if sx >= 0 else (slice(0, W + sx), slice(-sx, W))
    out[dst_y, dst_x] = img[src_y, src_x]
    return out


def test_reference_geometry_equals_an_independent_shift():
    W, H = 160, 80
    rng = np.random.default_rng(7)
    bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    dep = rng.integers(0, 65536, (H, W), dtype=np.uint16)
    for sx, sy in ((0, 0), (7, -3), (-W, 0), (W + 5, 2)):
        assert np.array_equal(IR.colour(bgr, W, H, shift=(sx, sy)), shift_with_zeros(bgr, sx, sy)), (sx, sy)
        assert np.array_equal(IR.depth(dep, W, H, shift=(sx, sy)), shift_with_zeros(dep, sx, sy)), (sx, sy)
    assert np.array_equal(IR.colour(bgr, W, H, shift=(0, 0)), bgr) and IR.colour(bgr, W, H, shift=(-W, 0)).max() == 0
    # mirror, channel order and planar layout against slicing
    assert np.array_equal(IR.colour(bgr, W, H, flip_x=True), bgr[:, ::-1])
    assert np.array_equal(IR.colour(bgr, W, H, order="rgb"), bgr[:, :, ::-1])
    assert np.array_equal(IR.colour(np.ascontiguousarray(bgr.transpose(2, 0, 1)), W, H, layout="chw"), bgr)
    big = rng.integers(0, 256, (97, 203, 4), dtype=np.uint8)
    assert np.array_equal(IR.colour(big, W, H, crop=(43, 17), flip_x=True, shift=(3, -2)),
                          shift_with_zeros(big[17:17 + H, 43:43 + W, :3][:, ::-1], 3, -2))
