"""line-mod-pipeline_amd -- MI355X-native LINE-MOD detector (host-side Python binding).

The product is liblinemod_hip.so (hand-written HIP kernels for gfx950 behind the C ABI of
include/linemod_hip.h).  This package is only the ctypes view of that ABI used by tests, bench.py
and the multi-GPU shard driver; it contains no compute and no fallback: if the library is missing
the import fails, and if no HIP device is present every compute call raises LinemodError.

Import with importlib (the directory name is not a Python identifier):
    lm = importlib.import_module("line-mod-pipeline_amd")
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liblinemod_hip.so")

LM_OK, LM_ERR_INVALID, LM_ERR_NO_DEVICE, LM_ERR_HIP, LM_ERR_OVERFLOW, LM_ERR_IO, LM_ERR_EXTRACT = range(7)

MATCH_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("similarity", "<f4"), ("template_id", "<i4"),
                        ("class_idx", "<i4")])
FEATURE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("label", "<i4")])
DESC_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("pyramid_level", "<i4"), ("num_features", "<i4")])
DEPTH_QUERY_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("slot", "<i4"), ("reserved", "<i4")])   # lm_depth_query
# lm_draw_prim (Detector.export_frames; draw_response / draw_axes / draw_box build arrays of it)
DRAW_PRIM_DTYPE = np.dtype([("kind", "<i4"), ("frame", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("thickness", "<i4"),
                            ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])
DRAW_RING, DRAW_SEGMENT, DRAW_BOX = 0, 1, 2
DEPTH_SELECT_QUERY_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("rank", "<i4"), ("slot", "<i4")])   # lm_depth_select_query


class Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("num_modalities", C.c_int32),
                ("pyramid_levels", C.c_int32), ("T", C.c_int32 * 4), ("weak_threshold", C.c_float),
                ("num_features", C.c_int32), ("strong_threshold", C.c_float), ("distance_threshold", C.c_int32),
                ("difference_threshold", C.c_int32), ("depth_num_features", C.c_int32),
                ("extract_threshold", C.c_int32), ("device", C.c_int32), ("shard_rank", C.c_int32),
                ("shard_size", C.c_int32), ("max_candidates", C.c_int32), ("max_matches", C.c_int32),
                ("frame_slots", C.c_int32), ("flags", C.c_int32)]

FLAG_BYTE_RESPONSES = 1
FLAG_BLOCKING_SYNC = 2
FLAG_KEEP_DEPTH = 4        # LM_FLAG_KEEP_DEPTH: a colour-only detector keeps a depth frame beside the colour frame
TUNE_COPY_STREAMS = 3
TUNE_CBLUR_VARIANT = 4
TUNE_CGRAD_VARIANT = 5
TUNE_PHASE_MAX_SLOTS = 6
TUNE_BATCH_PHASES = 7
TUNE_PYRDOWN_VARIANT = 8
TUNE_BLUR_PYR = 9
TUNE_DMEDIAN_VARIANT = 11
TUNE_BLUR_STRIP = 12
TUNE_WORK_WEIGHT = 13
TUNE_SORT_SPLIT = 14
TUNE_SCAN_LIST_ORDER = 15
TUNE_SCAN_FORM = 16
TUNE_SCAN1_MIN_THRESHOLD = 17
TUNE_CGRAD_LEVELS = 18
TUNE_SURVIVOR_QUEUE = 19
TUNE_RECTIFY_REDUCE_GRID = 20
TUNE_ICP_BATCH_MB = 21


class Rect(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class IcpQuery(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("class_idx", C.c_int32),
                ("first_pose", C.c_int32), ("num_poses", C.c_int32), ("reserved", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class IcpParams(C.Structure):
    _fields_ = [("step", C.c_int32), ("iterations", C.c_int32), ("tolerance", C.c_double), ("rejection_scale", C.c_double),
                ("levels", C.c_int32), ("max_points", C.c_int32)]


class MaskRule(C.Structure):
    """lm_mask_rule: a match-time mask the GPU computes from the resident frame (include/linemod_hip.h; make_mask_rule builds one)."""
    _fields_ = [("modalities", C.c_int32), ("use_depth", C.c_int32), ("keep_invalid", C.c_int32), ("zmin", C.c_int32),
                ("zmax", C.c_int32), ("use_hsv", C.c_int32), ("lower", C.c_double * 3), ("upper", C.c_double * 3),
                ("grow", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("reserved", C.c_int32)]


def make_mask_rule(modalities, depth_range=None, keep_invalid=False, hsv_range=None, grow=0, rect=None):
    """modalities: bit 0 colour, bit 1 depth.  depth_range (zmin, zmax); hsv_range (lower[3], upper[3]); rect (x, y, width, height)."""
    r = MaskRule()
    r.modalities = int(modalities)
    if depth_range is not None:
        r.use_depth, r.zmin, r.zmax = 1, int(depth_range[0]), int(depth_range[1])
    r.keep_invalid = 1 if keep_invalid else 0
    if hsv_range is not None:
        r.use_hsv = 1
        r.lower[:] = [float(v) for v in hsv_range[0]]
        r.upper[:] = [float(v) for v in hsv_range[1]]
    r.grow = int(grow)
    if rect is not None:
        r.x, r.y, r.width, r.height = (int(v) for v in rect)
    return r


class ObjectMask(C.Structure):
    """lm_object_mask: the object mask of one slot of lm_add_templates_slots (Detector.add_templates_slots builds them)."""
    _fields_ = [("data", C.c_void_p), ("row_stride", C.c_int64), ("on_device", C.c_int32), ("rule", C.POINTER(MaskRule))]


# lm_image_desc.format
PIX_BGR8, PIX_RGB8, PIX_BGRA8, PIX_RGBA8, PIX_BGR8_PLANAR, PIX_RGB8_PLANAR, PIX_DEPTH_U16, PIX_DEPTH_F32 = range(8)
PIX_GRAY8, PIX_NV12, PIX_NV21, PIX_YUY2, PIX_UYVY = range(8, 13)          # colour sources, converted by the ingest (0.12)
PIX_BAYER_RGGB8, PIX_BAYER_GRBG8, PIX_BAYER_GBRG8, PIX_BAYER_BGGR8 = range(16, 20)   # raw Bayer colour sources, demosaiced by the ingest (13 .. 15 name no format)
PIX_YUV_BT709, PIX_YUV_FULL = 0x100, 0x200                                 # ORed into PIX_NV12 .. PIX_UYVY: the matrix and the range
# High-bit raw colour sources: PIX_RAW | storage | pattern.  pattern 0 .. 3 = red_x | red_y << 1 as PIX_BAYER_*8 - 16, 4 = mono; storage
# 0x00 / 0x10 / 0x20 / 0x30 = 10 / 12 / 14 / 16 bits in a u16, 0x40 / 0x50 = 10 / 12 bits packed (PFNC "10p" / "12p").
# -> PIX_BAYER_RGGB10 .. PIX_BAYER_BGGR12P, PIX_MONO10 .. PIX_MONO12P
PIX_RAW = 0x1000
_RAW_STORAGE = {(10, False): 0x00, (12, False): 0x10, (14, False): 0x20, (16, False): 0x30, (10, True): 0x40, (12, True): 0x50}
for (_bits, _packed), _st in _RAW_STORAGE.items():
    for _pat, _tile in enumerate(("BAYER_RGGB", "BAYER_GRBG", "BAYER_GBRG", "BAYER_BGGR", "MONO")):
        globals()["PIX_%s%d%s" % (_tile, _bits, "P" if _packed else "")] = PIX_RAW | _st | _pat
del _bits, _packed, _st, _pat, _tile
# Float colour sources and export destinations: PIX_FLOAT | element | layout.  layout = the 8-bit format of the same memory order (0 .. 5,
# 8 = grey: a source only); element 0 = float32, PIX_FLOAT_F16 = float16.  Converted with the descriptor's scale (image_desc: float_scale).
PIX_FLOAT, PIX_FLOAT_F16 = 0x2000, 0x10
for _el, _tag in ((0, "F32"), (PIX_FLOAT_F16, "F16")):
    for _lay, _name in ((0, "BGR_%s"), (1, "RGB_%s"), (2, "BGRA_%s"), (3, "RGBA_%s"), (4, "BGR_%s_PLANAR"), (5, "RGB_%s_PLANAR"), (8, "GRAY_%s")):
        globals()["PIX_" + _name % _tag] = PIX_FLOAT | _el | _lay
del _el, _tag, _lay, _name


class ImageDesc(C.Structure):
    """lm_image_desc: one source image of lm_ingest_frames, in DEVICE memory (include/linemod_hip.h; image_desc builds one)."""
    _fields_ = [("data", C.c_void_p), ("row_stride", C.c_int64), ("plane_stride", C.c_int64), ("width", C.c_int32), ("height", C.c_int32),
                ("format", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32), ("scale", C.c_float)]


class RawProcessing(C.Structure):
    """lm_raw_processing: the raw pipeline (Detector.set_raw_processing builds one)."""
    _fields_ = [("black", C.c_int32), ("gain", C.c_uint32 * 3), ("ccm", C.c_int32 * 9), ("tone", C.c_uint8 * 4096)]


def tone_curve(gamma):
    """A tone table for set_raw_processing: uint8 [4096], entry i = round(255 * (i / 4095) ** (1 / gamma)) -- gamma 1 is (nearly) the
    identity's i >> 4, gamma 2.2 a display curve."""
    if not gamma > 0:
        raise ValueError("gamma %r (a positive number wanted)" % (gamma,))
    return np.rint(255.0 * (np.arange(4096, dtype=np.float64) / 4095.0) ** (1.0 / float(gamma))).astype(np.uint8)


class IngestOpts(C.Structure):
    _fields_ = [("flip_x", C.c_int32), ("shift_x", C.c_int32), ("shift_y", C.c_int32)]


class Camera(C.Structure):
    """lm_camera: a pinhole + Brown-Conrady camera of a registration (camera builds one)."""
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k1", C.c_float), ("k2", C.c_float),
                ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float), ("width", C.c_int32), ("height", C.c_int32)]


class RegistrationDesc(C.Structure):
    """lm_registration_desc (Detector.set_registration builds one)."""
    _fields_ = [("depth", Camera), ("colour", Camera), ("rotation", C.c_float * 9), ("translation", C.c_float * 3),
                ("splat_x", C.c_int32), ("splat_y", C.c_int32), ("rays", C.c_void_p)]


class RectificationDesc(C.Structure):
    """lm_rectification_desc (Detector.set_rectification builds one)."""
    _fields_ = [("source", Camera), ("ideal", Camera), ("map", C.c_void_p)]


RECTIFY_DEPTH_ALIGNED, RECTIFY_DEPTH_REGISTERED = 0, 1


class ReductionDesc(C.Structure):
    """lm_reduction_desc (Detector.set_reduction and reduction_desc build one)."""
    _fields_ = [("num_x", C.c_int32), ("den_x", C.c_int32), ("num_y", C.c_int32), ("den_y", C.c_int32), ("apply", C.c_int32),
                ("depth_rule", C.c_int32)]


REDUCE_COLOUR, REDUCE_DEPTH = 1, 2
REDUCE_DEPTH_NEAREST, REDUCE_DEPTH_MIN_VALID = 0, 1
_REDUCE_DEPTH_RULES = {"nearest": REDUCE_DEPTH_NEAREST, "min_valid": REDUCE_DEPTH_MIN_VALID}


def reduction_desc(ratio, colour=True, depth=True, depth_rule="nearest"):
    """A ReductionDesc: ratio = (num, den), source pixels per reduced pixel, or a pair ((num_x, den_x), (num_y, den_y)); which images of a
    frame it applies to; depth_rule "nearest" / "min_valid" (or the LM_REDUCE_DEPTH_* number).  The library checks the numbers."""
    rx, ry = (ratio, ratio) if not isinstance(ratio[0], (tuple, list)) else ratio
    r = ReductionDesc()
    r.num_x, r.den_x, r.num_y, r.den_y = int(rx[0]), int(rx[1]), int(ry[0]), int(ry[1])
    r.apply = (REDUCE_COLOUR if colour else 0) | (REDUCE_DEPTH if depth else 0)
    if isinstance(depth_rule, str) and depth_rule not in _REDUCE_DEPTH_RULES:
        raise ValueError("depth_rule %r (\"nearest\" or \"min_valid\" wanted)" % (depth_rule,))
    r.depth_rule = _REDUCE_DEPTH_RULES[depth_rule] if isinstance(depth_rule, str) else int(depth_rule)
    return r


def reduced_camera(source, ratio, crop=(0, 0), size=None):
    """lm_reduced_camera: the Camera of a slot's frame -- `source` reduced by `ratio` (as reduction_desc's), the window of `size` =
    (width, height) at `crop` of the reduced geometry (None: the whole reduced geometry of the source's size, crop included)."""
    r = reduction_desc(ratio)
    if size is None:
        size = (int(source.width) * r.den_x // max(r.num_x, 1) - int(crop[0]), int(source.height) * r.den_y // max(r.num_y, 1) - int(crop[1]))
    out = Camera()
    if load_library().lm_reduced_camera(C.byref(source), C.byref(r), int(crop[0]), int(crop[1]), int(size[0]), int(size[1]), C.byref(out)) != 0:
        raise LinemodError(LM_ERR_INVALID, load_library().lm_last_error().decode())
    return out


def camera(width, height, fx, fy, cx, cy, dist=(0.0, 0.0, 0.0, 0.0, 0.0)):
    """A Camera: size in pixels, focal lengths and principal point in pixels, dist = (k1, k2, p1, p2, k3) in OpenCV's order."""
    if len(dist) != 5:
        raise ValueError("dist: %d coefficients ((k1, k2, p1, p2, k3) wanted)" % len(dist))
    k = Camera()
    k.width, k.height, k.fx, k.fy, k.cx, k.cy = int(width), int(height), float(fx), float(fy), float(cx), float(cy)
    k.k1, k.k2, k.p1, k.p2, k.k3 = (float(v) for v in dist)
    return k


def _device_array(obj, what, half=False):
    """(pointer, shape, byte strides, element size, description, is it a float) of an object with __cuda_array_interface__.  half: float16 '<f2' is an
    element too (a float colour image whose scale the caller has named)."""
    cai = getattr(obj, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise ValueError("%s has no __cuda_array_interface__" % type(obj).__name__)
    shape, typestr = tuple(int(v) for v in cai["shape"]), cai["typestr"]
    item = {"|u1": 1, "<u2": 2, "<f4": 4, "<f2": 2 if half else None}.get(typestr)
    found = "typestr %r, shape %r" % (typestr, shape)
    if item is None:
        raise ValueError("%s image: %s (uint8 '|u1', uint16 '<u2' or float32 '<f4' wanted)" % (what, found))
    strides = cai.get("strides")
    if strides is None:
        strides, acc = [], item
        for n in reversed(shape):
            strides.insert(0, acc)
            acc *= n
    strides = tuple(int(v) for v in strides)
    found += ", strides %r" % (strides,)
    ptr = cai["data"][0]
    return (int(ptr) if ptr else None), shape, strides, item, found, typestr in ("<f4", "<f2")


_YUV_LAYOUTS = {"nv12": PIX_NV12, "nv21": PIX_NV21, "yuy2": PIX_YUY2, "uyvy": PIX_UYVY}
_BAYER_LAYOUTS = {"bayer_rggb": PIX_BAYER_RGGB8, "bayer_grbg": PIX_BAYER_GRBG8, "bayer_gbrg": PIX_BAYER_GBRG8, "bayer_bggr": PIX_BAYER_BGGR8}


def image_desc(obj, depth=False, order="bgr", layout="hwc", crop=(0, 0), scale=1.0, matrix="bt601", range="limited", bits=8, packed=False, width=None,
               float_scale=None):
    """The ImageDesc of an object with __cuda_array_interface__ (a torch or cupy tensor, a DeviceBuffer.view).  Colour: uint8, [H, W, 3 | 4]
    with layout "hwc" (interleaved, the channels adjacent) or [3, H, W] with layout "chw" (planar), order "bgr" / "rgb"; [H, W] with layout
    "gray" or, a raw Bayer mosaic named by its top-left 2 x 2 tile, "bayer_rggb" / "bayer_grbg" / "bayer_gbrg" / "bayer_bggr" (H and W
    even; demosaiced by the ingest); [H, W, 2] with layout "yuy2" / "uyvy"; with layout "nv12" / "nv21" ONE [H * 3 / 2, W] object (the chroma rows behind the Y
    rows) or a PAIR (y [H, W], uv [H / 2, W / 2, 2] or [H / 2, W]) of two objects with the same row stride, uv at the higher address.  The YUV
    layouts are converted with matrix "bt601" / "bt709" and range "limited" / "full".  High-bit raw sources: a Bayer layout or "mono" with
    bits = 10 / 12 / 14 / 16 and a uint16 [H, W] object (the sample in the low bits), or with packed=True, bits = 10 / 12, a uint8
    [H, row bytes] object of PFNC-packed rows and width = the pixels of a row; they go through the detector's raw pipeline.  Depth: [H, W] uint16 (millimetres) or float32
    (`scale` millimetres per unit).  Rows and planes may have any positive stride; anything else is a ValueError.
    Float colour: with float_scale given (255 for a 0 .. 1 tensor, 1 for 0 .. 255 floats: a channel becomes rint(v * float_scale) clamped
    to 0 .. 255, NaN 0) a float32 '<f4' or float16 '<f2' object is a colour image too: [H, W, 3 | 4] with layout "hwc", [3, H, W] with
    "chw", [H, W] with "gray"; elements, channels and pixels adjacent.  A torch tensor works as it is, through its
    __cuda_array_interface__ (torch.rand(3, H, W, device="cuda"): layout="chw", order="rgb", float_scale=255).  Without float_scale a
    float colour object stays a ValueError: the caller names the scale, the binding does not guess it."""
    pair = None
    if not depth and layout in ("nv12", "nv21") and isinstance(obj, (tuple, list)):
        if len(obj) != 2:
            raise ValueError("colour image, layout %s: %d objects (one [H * 3 / 2, W] object or a pair (y, uv) wanted)" % (layout, len(obj)))
        obj, pair = obj
    ptr, shape, strides, item, found, is_float = _device_array(obj, "depth" if depth else "colour", half=not depth and float_scale is not None)
    d = ImageDesc()
    d.data, d.crop_x, d.crop_y, d.scale = ptr, int(crop[0]), int(crop[1]), float(scale)
    if depth:
        if item == 1 or len(shape) != 2:
            raise ValueError("depth image: %s ([H, W] uint16 or float32 wanted)" % found)
        if strides[1] != item or strides[0] <= 0:
            raise ValueError("depth image: %s (adjacent pixels and a positive row stride wanted)" % found)
        d.height, d.width, d.row_stride, d.format = shape[0], shape[1], strides[0], PIX_DEPTH_U16 if item == 2 else PIX_DEPTH_F32
        return d
    if order not in ("bgr", "rgb") or layout not in ("hwc", "chw", "gray", "mono") + tuple(_YUV_LAYOUTS) + tuple(_BAYER_LAYOUTS):
        raise ValueError("order %r, layout %r (\"bgr\" / \"rgb\" and \"hwc\" / \"chw\" / \"gray\" / \"nv12\" / \"nv21\" / \"yuy2\" / \"uyvy\" / "
                         "\"bayer_rggb\" / \"bayer_grbg\" / \"bayer_gbrg\" / \"bayer_bggr\" / \"mono\" wanted)" % (order, layout))
    if matrix not in ("bt601", "bt709") or range not in ("limited", "full"):
        raise ValueError("matrix %r, range %r (\"bt601\" / \"bt709\" and \"limited\" / \"full\" wanted)" % (matrix, range))
    rgb = order == "rgb"
    if float_scale is not None and is_float:
        # a float colour source (or export destination): PIX_FLOAT | element | the 8-bit format of the same memory order
        what = "float colour image, layout %s" % layout
        if layout not in ("hwc", "chw", "gray") or bits != 8 or packed or width is not None:
            raise ValueError("%s: %s (a float image is layout \"hwc\" / \"chw\" / \"gray\", without bits, packed or width)" % (what, found))
        d.scale = float(float_scale)
        el = PIX_FLOAT | (PIX_FLOAT_F16 if item == 2 else 0)
        if layout == "gray":
            if len(shape) != 2:
                raise ValueError("%s: %s ([H, W] wanted)" % (what, found))
            if strides[1] != item or strides[0] <= 0:
                raise ValueError("%s: %s (adjacent pixels and a positive row stride wanted)" % (what, found))
            d.height, d.width, d.row_stride, d.format = shape[0], shape[1], strides[0], el | PIX_GRAY8
        elif len(shape) != 3:
            raise ValueError("%s: %s ([H, W, 3 | 4] or [3, H, W] wanted)" % (what, found))
        elif layout == "hwc":
            if shape[2] not in (3, 4):
                raise ValueError("%s: %s (3 or 4 channels wanted)" % (what, found))
            if strides[2] != item or strides[1] != item * shape[2] or strides[0] <= 0:
                raise ValueError("%s: %s (adjacent channels and pixels and a positive row stride wanted)" % (what, found))
            d.height, d.width, d.row_stride = shape[0], shape[1], strides[0]
            d.format = el | ((PIX_RGB8 if rgb else PIX_BGR8) if shape[2] == 3 else (PIX_RGBA8 if rgb else PIX_BGRA8))
        else:
            if shape[0] != 3:
                raise ValueError("%s: %s (3 planes wanted)" % (what, found))
            if strides[2] != item or strides[1] <= 0 or strides[0] <= 0:
                raise ValueError("%s: %s (adjacent pixels and positive row and plane strides wanted)" % (what, found))
            d.height, d.width, d.row_stride, d.plane_stride = shape[1], shape[2], strides[1], strides[0]
            d.format = el | (PIX_RGB8_PLANAR if rgb else PIX_BGR8_PLANAR)
        return d
    if (bits != 8 or packed or layout == "mono") and not isinstance(bits, bool):
        # a high-bit raw source
        what = "colour image, layout %s, bits %r%s" % (layout, bits, ", packed" if packed else "")
        if layout != "mono" and layout not in _BAYER_LAYOUTS:
            raise ValueError("%s (bits and packed belong to the layouts \"bayer_rggb\" / \"bayer_grbg\" / \"bayer_gbrg\" / \"bayer_bggr\" / \"mono\")" % what)
        if (bits, bool(packed)) not in _RAW_STORAGE:
            raise ValueError("%s (bits 10 / 12 / 14 / 16 in uint16, or packed with bits 10 / 12, wanted%s)"
                             % (what, "; an 8-bit mono image is layout \"gray\"" if layout == "mono" and bits == 8 else ""))
        d.format = PIX_RAW | _RAW_STORAGE[bits, bool(packed)] | (4 if layout == "mono" else _BAYER_LAYOUTS[layout] - PIX_BAYER_RGGB8)
        if packed:
            if item != 1 or len(shape) != 2:
                raise ValueError("%s: %s (uint8 [H, row bytes] wanted)" % (what, found))
            if strides[1] != 1 or strides[0] <= 0:
                raise ValueError("%s: %s (adjacent bytes and a positive row stride wanted)" % (what, found))
            if width is None or int(width) < 0 or (int(width) * bits + 7) // 8 > shape[1]:
                raise ValueError("%s: width %r, %s (width = the pixels of a row, within the row's bytes, wanted)" % (what, width, found))
            d.height, d.width, d.row_stride = shape[0], int(width), strides[0]
            return d
        if width is not None:
            raise ValueError("%s: width %r (width belongs to packed=True)" % (what, width))
        if item != 2 or len(shape) != 2 or is_float:
            raise ValueError("%s: %s (uint16 [H, W] wanted)" % (what, found))
        if strides[1] != 2 or strides[0] <= 0:
            raise ValueError("%s: %s (adjacent pixels and a positive row stride wanted)" % (what, found))
        d.height, d.width, d.row_stride = shape[0], shape[1], strides[0]
        return d
    if width is not None:
        raise ValueError("colour image, layout %s: width %r (width belongs to packed=True)" % (layout, width))
    if layout == "gray":
        if item != 1 or len(shape) != 2:
            raise ValueError("colour image, layout gray: %s (uint8 [H, W] wanted)" % found)
        if strides[1] != 1 or strides[0] <= 0:
            raise ValueError("colour image, layout gray: %s (adjacent pixels and a positive row stride wanted)" % found)
        d.height, d.width, d.row_stride, d.format = shape[0], shape[1], strides[0], PIX_GRAY8
        return d
    if layout in _BAYER_LAYOUTS:
        if item != 1 or len(shape) != 2:
            raise ValueError("colour image, layout %s: %s (uint8 [H, W] wanted)" % (layout, found))
        if strides[1] != 1 or strides[0] <= 0:
            raise ValueError("colour image, layout %s: %s (adjacent pixels and a positive row stride wanted)" % (layout, found))
        d.height, d.width, d.row_stride, d.format = shape[0], shape[1], strides[0], _BAYER_LAYOUTS[layout]
        return d
    if layout in _YUV_LAYOUTS:
        d.format = _YUV_LAYOUTS[layout] | (PIX_YUV_BT709 if matrix == "bt709" else 0) | (PIX_YUV_FULL if range == "full" else 0)
        if layout in ("yuy2", "uyvy"):
            if item != 1 or len(shape) != 3 or shape[2] != 2:
                raise ValueError("colour image, layout %s: %s (uint8 [H, W, 2] wanted)" % (layout, found))
            if strides[2] != 1 or strides[1] != 2 or strides[0] <= 0:
                raise ValueError("colour image, layout %s: %s (adjacent bytes and pixels and a positive row stride wanted)" % (layout, found))
            d.height, d.width, d.row_stride = shape[0], shape[1], strides[0]
            return d
        if item != 1 or len(shape) != 2:
            raise ValueError("colour image, layout %s: %s (uint8 [H * 3 / 2, W], or a pair with y uint8 [H, W], wanted)" % (layout, found))
        if strides[1] != 1 or strides[0] <= 0:
            raise ValueError("colour image, layout %s: %s (adjacent pixels and a positive row stride wanted)" % (layout, found))
        if pair is None:
            if shape[0] % 3:
                raise ValueError("colour image, layout %s: %s (H * 3 / 2 rows wanted: a multiple of 3)" % (layout, found))
            d.height, d.width, d.row_stride = shape[0] // 3 * 2, shape[1], strides[0]
            d.plane_stride = d.height * strides[0]
            return d
        uptr, ushape, ustrides, uitem, ufound, _ = _device_array(pair, "colour")
        H, W = shape
        dense = (len(ushape) == 3 and ushape == (H // 2, W // 2, 2) and ustrides[1:] == (2, 1)) or \
                (len(ushape) == 2 and ushape == (H // 2, W) and ustrides[1] == 1)
        if uitem != 1 or H % 2 or W % 2 or not dense:
            raise ValueError("colour image, layout %s: chroma plane %s beside a Y plane %s (uint8 [H / 2, W / 2, 2] or [H / 2, W] with adjacent bytes "
                             "wanted, H and W even)" % (layout, ufound, found))
        if ustrides[0] != strides[0]:
            raise ValueError("colour image, layout %s: chroma plane %s beside a Y plane %s (the same row stride wanted)" % (layout, ufound, found))
        if ptr is None or uptr is None or uptr <= ptr:
            raise ValueError("colour image, layout %s: chroma plane at %s, Y plane at %s (the chroma plane at the higher address wanted)"
                             % (layout, hex(uptr or 0), hex(ptr or 0)))
        d.height, d.width, d.row_stride, d.plane_stride = H, W, strides[0], uptr - ptr
        return d
    if item != 1 or len(shape) != 3:
        raise ValueError("colour image: %s (uint8 [H, W, 3 | 4] or [3, H, W] wanted)" % found)
    if layout == "hwc":
        if shape[2] not in (3, 4):
            raise ValueError("colour image, layout hwc: %s (3 or 4 channels wanted)" % found)
        if strides[2] != 1 or strides[1] != shape[2] or strides[0] <= 0:
            raise ValueError("colour image, layout hwc: %s (adjacent channels and pixels and a positive row stride wanted)" % found)
        d.height, d.width, d.row_stride = shape[0], shape[1], strides[0]
        d.format = (PIX_RGB8 if rgb else PIX_BGR8) if shape[2] == 3 else (PIX_RGBA8 if rgb else PIX_BGRA8)
    else:
        if shape[0] != 3:
            raise ValueError("colour image, layout chw: %s (3 planes wanted)" % found)
        if strides[2] != 1 or strides[1] <= 0 or strides[0] <= 0:
            raise ValueError("colour image, layout chw: %s (adjacent pixels and positive row and plane strides wanted)" % found)
        d.height, d.width, d.row_stride, d.plane_stride = shape[1], shape[2], strides[1], strides[0]
        d.format = PIX_RGB8_PLANAR if rgb else PIX_BGR8_PLANAR
    return d


class VsdQuery(C.Structure):
    _fields_ = [("frame", C.c_int32), ("mesh_idx", C.c_int32), ("view_proj_gt", C.c_float * 16), ("view_proj_est", C.c_float * 16)]


class IcpVerifyQuery(C.Structure):
    _fields_ = [("frame", C.c_int32), ("mesh_idx", C.c_int32), ("view_proj", C.c_float * 16)]


# lm_icp_verify_result: the eroded mask's pixel count, the integer sum of |scene - render| over it and their quotient
ICP_VERIFY_RESULT_DTYPE = np.dtype([("count", np.uint32), ("reserved", np.uint32), ("sum", np.uint64), ("mean", np.float64)])
# lm_vsd_result: the seven pixel counts of calculateVisibilityMasks and the Hodan error
VSD_RESULT_DTYPE = np.dtype([("rendered_gt", np.uint32), ("rendered_est", np.uint32), ("visible_gt", np.uint32), ("visible_est", np.uint32),
                             ("intersection", np.uint32), ("combination", np.uint32), ("within_tau", np.uint32), ("error", np.float32)])
# lm_add_query: R_gt (row-major), t_gt, R_est, t_est
ADD_QUERY_DTYPE = np.dtype([("R_gt", np.float32, (9,)), ("t_gt", np.float32, (3,)), ("R_est", np.float32, (9,)), ("t_est", np.float32, (3,))])


class LinemodError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("liblinemod_hip error %d: %s" % (code, msg))
        self.code = code


# Every symbol include/linemod_hip.h declares (tests check that the library exports all of them).
EXPORTS = [
    "lm_last_error", "lm_version", "lm_default_config", "lm_create", "lm_destroy", "lm_set_similarity_lut",
    "lm_set_normal_lut", "lm_get_similarity_lut", "lm_get_normal_lut", "lm_num_classes", "lm_num_templates",
    "lm_class_num_templates", "lm_class_id", "lm_find_class", "lm_get_T", "lm_num_modalities",
    "lm_pyramid_levels", "lm_add_class", "lm_add_template", "lm_get_template", "lm_match", "lm_upload_frame",
    "lm_match_slot", "lm_match_batch", "lm_merge_matches", "lm_save_bank", "lm_load_bank",
    "lm_stage_color_quantize", "lm_stage_pyrdown", "lm_stage_depth_quantize", "lm_stage_linear_memories",
    "lm_prepare_slot", "lm_debug_read", "lm_stage_scan", "lm_time_scan", "lm_time_stages", "lm_set_scan_variant",
    "lm_last_counts", "lm_set_profiling", "lm_get_profile", "lm_scan_load_bytes",
    "lm_save_yaml", "lm_load_yaml", "lm_yaml_numbers", "lm_yaml_string", "lm_pack_matches", "lm_merge_batch",
    "lm_upload_frame_shifted", "lm_match_begin", "lm_match_end", "lm_synchronize", "lm_merge_frames", "lm_gather_plan", "lm_gather_max_total",
    "lm_upload_frame_pinned", "lm_upload_wait", "lm_host_alloc", "lm_host_free", "lm_set_stage_chunks",
    "lm_set_tuning", "lm_comm_init", "lm_comm_destroy", "lm_comm_info", "lm_match_begin_gathered",
    "lm_match_end_gathered", "lm_comm_barrier", "lm_comm_max", "lm_upload_frames_pinned",
    "lm_rendezvous_broadcast", "lm_normal_lut_is_substitute",
    "lm_set_scan_stats", "lm_get_scan_stats", "lm_color_check_counts",
    "lm_match_batch_classes", "lm_match_prepared", "lm_match_begin_classes", "lm_device_pci_bus_id",
    "lm_get_exchange_profile", "lm_get_stage_counts", "lm_debug_live_resources", "lm_debug_launch_counts", "lm_get_scan_lane_stats", "lm_get_scan_form_stats", "lm_match_classes",
    "lm_time_scan_batch",
    "lm_selftest_float_tail",
    "lm_upload_frame_pinned_shifted", "lm_stage_reserve", "lm_stage_rows", "lm_upload_staged", "lm_match_collect",
    "lm_color_check_counts_slots", "lm_color_check_begin_slots", "lm_color_check_end", "lm_color_mask_prepare",
    "lm_depth_counts_begin", "lm_depth_counts_end",
    "lm_depth_select_begin", "lm_depth_select_end", "lm_time_depth_select",
    "lm_match_masked", "lm_upload_match_mask",
    "lm_set_mask_rule", "lm_get_mask_rule", "lm_stage_mask_rule",
    "lm_icp_set_model", "lm_icp_refine", "lm_stage_icp_scene", "lm_stage_icp_refine_host", "lm_icp_refine_slots", "lm_stage_icp_batch_stats",
    "lm_set_render_mesh", "lm_add_templates_rendered", "lm_stage_render", "lm_stage_rotate",
    "lm_pose_error_vsd", "lm_pose_error_add", "lm_stage_vsd_counts",
    "lm_stage_icp_verify_host", "lm_icp_verify", "lm_stage_icp_verify_counts",
    "lm_ingest_frames", "lm_ingest_release", "lm_read_frame", "lm_device_alloc", "lm_device_free", "lm_device_copy",
    "lm_add_templates_slots", "lm_stage_select",
    "lm_set_registration", "lm_get_registration_rays", "lm_ingest_frames_registered", "lm_stage_register_depth",
    "lm_set_rectification", "lm_get_rectification_map", "lm_ingest_frames_rectified", "lm_stage_rectify",
    "lm_set_raw_processing", "lm_get_raw_processing",
    "lm_set_reduction", "lm_get_reduction", "lm_ingest_frames_reduced", "lm_stage_reduce", "lm_reduced_camera",
    "lm_ingest_frames_rectified_reduced", "lm_stage_rectify_reduce",
    "lm_keeps_depth",
    "lm_export_frames",
]

_lib = None


def load_library(path=None):
    """Loads liblinemod_hip.so; raises OSError if it has not been built (no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OSError("liblinemod_hip.so not built (%s): run `python line-mod-pipeline_amd/build.py` "
                      "or __graft_entry__.build(); there is no CPU fallback" % p)
    lib = C.CDLL(p)
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    lib.lm_last_error.restype = C.c_char_p
    lib.lm_version.restype = C.c_char_p
    lib.lm_default_config.argtypes = [C.POINTER(Config), i, i, i]
    lib.lm_default_config.restype = None
    lib.lm_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.lm_destroy.argtypes = [vp]
    lib.lm_destroy.restype = None
    for name in ("lm_set_similarity_lut", "lm_set_normal_lut", "lm_get_similarity_lut", "lm_get_normal_lut"):
        getattr(lib, name).argtypes = [vp, vp]
    lib.lm_normal_lut_is_substitute.argtypes = [vp]
    lib.lm_num_classes.argtypes = [vp]
    lib.lm_num_templates.argtypes = [vp]
    lib.lm_class_num_templates.argtypes = [vp, i]
    lib.lm_class_id.argtypes = [vp, i]
    lib.lm_class_id.restype = C.c_char_p
    lib.lm_find_class.argtypes = [vp, C.c_char_p]
    lib.lm_get_T.argtypes = [vp, i]
    lib.lm_num_modalities.argtypes = [vp]
    lib.lm_keeps_depth.argtypes = [vp]
    lib.lm_pyramid_levels.argtypes = [vp]
    lib.lm_add_class.argtypes = [vp, C.c_char_p, i, vp, vp, C.POINTER(i)]
    lib.lm_add_template.argtypes = [vp, C.c_char_p, vp, sz, vp, sz, vp, sz, C.POINTER(i), C.POINTER(Rect)]
    lib.lm_get_template.argtypes = [vp, i, i, i, i, C.POINTER(i), C.POINTER(i), vp, C.POINTER(i)]
    lib.lm_match.argtypes = [vp, vp, sz, vp, sz, f, i, vp, sz, C.POINTER(sz)]
    lib.lm_upload_frame.argtypes = [vp, i, vp, sz, vp, sz]
    lib.lm_upload_frame_shifted.argtypes = [vp, i, vp, sz, vp, sz, i, i]
    lib.lm_match_slot.argtypes = [vp, i, f, i, vp, sz, C.POINTER(sz)]
    lib.lm_match_batch.argtypes = [vp, i, f, i, vp, sz, vp]
    lib.lm_match_begin.argtypes = [vp, i, i, i, f, i]
    lib.lm_match_end.argtypes = [vp, i, vp, sz, vp]
    lib.lm_pack_matches.argtypes = [vp, sz, vp, i, vp, sz, C.POINTER(sz)]
    lib.lm_merge_batch.argtypes = [vp, sz, vp, i, i, vp, sz, vp, C.POINTER(sz)]
    lib.lm_merge_frames.argtypes = [vp, sz, vp, i, i, i, i, vp, sz, vp, C.POINTER(sz)]
    lib.lm_gather_plan.argtypes = [vp, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i), vp, vp, vp]
    lib.lm_gather_max_total.argtypes = [vp, i, i, C.POINTER(C.c_uint64)]
    lib.lm_merge_matches.argtypes = [vp, vp, i, sz, vp, sz, C.POINTER(sz)]
    lib.lm_save_bank.argtypes = [vp, C.c_char_p]
    lib.lm_load_bank.argtypes = [vp, C.c_char_p]
    lib.lm_stage_color_quantize.argtypes = [vp, vp, i, i, f, vp, vp]
    lib.lm_stage_pyrdown.argtypes = [vp, vp, i, i, vp]
    lib.lm_stage_depth_quantize.argtypes = [vp, vp, i, i, vp]
    lib.lm_stage_linear_memories.argtypes = [vp, vp, i, i, i, vp]
    lib.lm_prepare_slot.argtypes = [vp, i]
    lib.lm_debug_read.argtypes = [vp, i, i, i, i, vp, sz, C.POINTER(sz)]
    lib.lm_stage_scan.argtypes = [vp, i, f, i, vp, sz, C.POINTER(sz)]
    lib.lm_time_scan.argtypes = [vp, i, f, i, i, i, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.lm_time_stages.argtypes = [vp, i, f, i, i, C.POINTER(C.c_double)]
    lib.lm_time_scan_batch.argtypes = [vp, i, i, f, i, i, i, C.POINTER(C.c_double)]
    lib.lm_selftest_float_tail.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.lm_set_scan_variant.argtypes = [vp, i]
    lib.lm_color_check_counts.argtypes = [vp, i, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, sz, vp, vp]
    lib.lm_set_scan_stats.argtypes = [vp, i]
    lib.lm_get_scan_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.lm_last_counts.argtypes = [vp, i, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.lm_set_profiling.argtypes = [vp, i]
    lib.lm_get_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64)]
    lib.lm_last_error.argtypes = []
    lib.lm_version.argtypes = []
    lib.lm_save_yaml.argtypes = [vp, C.c_char_p]
    lib.lm_load_yaml.argtypes = [vp, C.c_char_p]
    lib.lm_yaml_numbers.argtypes = [C.c_char_p, C.c_char_p, vp, sz, C.POINTER(sz)]
    lib.lm_yaml_string.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, sz]
    lib.lm_scan_load_bytes.argtypes = [vp, i, C.POINTER(C.c_double)]
    lib.lm_synchronize.argtypes = [vp]
    lib.lm_upload_frame_pinned.argtypes = [vp, i, vp, sz, vp, sz]
    lib.lm_upload_wait.argtypes = [vp, i]
    lib.lm_upload_frames_pinned.argtypes = [vp, i, i, vp, sz]
    lib.lm_host_alloc.argtypes = [sz, C.POINTER(vp)]
    lib.lm_host_free.argtypes = [vp]
    lib.lm_host_free.restype = None
    lib.lm_set_stage_chunks.argtypes = [vp, i]
    lib.lm_set_tuning.argtypes = [vp, i, i]
    lib.lm_comm_init.argtypes = [vp, i, i, C.c_char_p, i, i]
    lib.lm_comm_destroy.argtypes = [vp]
    lib.lm_rendezvous_broadcast.argtypes = [i, i, C.c_char_p, i, vp, sz, i]
    lib.lm_comm_info.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    lib.lm_match_begin_gathered.argtypes = [vp, i, i, i, f, i]
    lib.lm_match_end_gathered.argtypes = [vp, i, vp, sz, vp, C.POINTER(i), C.POINTER(i), C.POINTER(sz)]
    lib.lm_comm_barrier.argtypes = [vp]
    lib.lm_comm_max.argtypes = [vp, C.POINTER(C.c_double), i]
    lib.lm_match_classes.argtypes = [vp, vp, sz, vp, sz, f, vp, i, vp, sz, C.POINTER(sz)]
    lib.lm_match_batch_classes.argtypes = [vp, i, i, f, vp, i, vp, sz, vp]
    lib.lm_match_prepared.argtypes = [vp, i, i, f, vp, i, vp, sz, vp]
    lib.lm_match_begin_classes.argtypes = [vp, i, i, i, f, vp, i]
    lib.lm_device_pci_bus_id.argtypes = [vp, C.c_char_p, sz]
    lib.lm_get_exchange_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.lm_get_stage_counts.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.lm_debug_live_resources.argtypes = [C.POINTER(C.c_int64)]
    lib.lm_debug_launch_counts.argtypes = [C.POINTER(C.c_int64)]
    lib.lm_get_scan_form_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.lm_get_scan_lane_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.lm_upload_frame_pinned_shifted.argtypes = [vp, i, vp, sz, vp, sz, i, i]
    lib.lm_stage_reserve.argtypes = [vp, i, i]
    lib.lm_stage_rows.argtypes = [vp, i, vp, sz, vp, sz, i, i, i, i]
    lib.lm_upload_staged.argtypes = [vp, i]
    lib.lm_match_collect.argtypes = [vp, i, i, vp, sz, vp]
    lib.lm_color_check_counts_slots.argtypes = [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, sz, vp, vp]
    lib.lm_color_check_begin_slots.argtypes = [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, sz]
    lib.lm_color_check_end.argtypes = [vp, vp, vp]
    lib.lm_depth_counts_begin.argtypes = [vp, vp, C.c_size_t]
    lib.lm_depth_counts_end.argtypes = [vp, vp, vp]
    lib.lm_depth_select_begin.argtypes = [vp, vp, C.c_size_t]
    lib.lm_depth_select_end.argtypes = [vp, vp]
    lib.lm_time_depth_select.argtypes = [vp, vp, C.c_size_t, i, C.POINTER(C.c_float)]
    lib.lm_color_mask_prepare.argtypes = [vp, i, i, i, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.lm_match_masked.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, sz, f, i, vp, sz, C.POINTER(sz)]
    lib.lm_upload_match_mask.argtypes = [vp, i, i, vp, sz]
    lib.lm_set_mask_rule.argtypes = [vp, i, i, C.POINTER(MaskRule)]
    lib.lm_get_mask_rule.argtypes = [vp, i, C.POINTER(MaskRule), C.POINTER(i)]
    lib.lm_stage_mask_rule.argtypes = [vp, vp, vp, i, i, C.POINTER(MaskRule), vp]
    lib.lm_icp_set_model.argtypes = [vp, i, vp, i, i]
    lib.lm_icp_refine.argtypes = [vp, i, C.POINTER(IcpQuery), i, C.POINTER(IcpParams), vp]
    lib.lm_icp_refine_slots.argtypes = [vp, vp, C.POINTER(IcpQuery), i, C.POINTER(IcpParams), vp, vp]
    lib.lm_stage_icp_batch_stats.argtypes = [vp, vp]
    lib.lm_stage_icp_scene.argtypes = [vp, vp, i, i, vp, vp, i, vp, sz, C.POINTER(i)]
    lib.lm_stage_icp_refine_host.argtypes = [vp, vp, C.POINTER(IcpQuery), i, C.POINTER(IcpParams), vp]
    lib.lm_set_render_mesh.argtypes = [vp, i, vp, i, vp, i]
    lib.lm_add_templates_rendered.argtypes = [vp, C.c_char_p, i, vp, i, vp, i, vp, vp, vp, sz, vp]
    lib.lm_stage_render.argtypes = [vp, i, vp, i, i, vp, vp]
    lib.lm_stage_rotate.argtypes = [vp, vp, vp, i, i, f, vp, vp]
    lib.lm_pose_error_vsd.argtypes = [vp, vp, i, i, i, C.POINTER(VsdQuery), i, i, i, vp]
    lib.lm_pose_error_add.argtypes = [vp, i, i, i, vp, i, vp, vp]
    lib.lm_stage_vsd_counts.argtypes = [vp, vp, vp, vp, i, i, i, i, vp]
    lib.lm_stage_icp_verify_host.argtypes = [vp, vp, i, i, i, C.POINTER(IcpVerifyQuery), i, i, vp]
    lib.lm_icp_verify.argtypes = [vp, C.POINTER(IcpVerifyQuery), i, i, vp]
    lib.lm_stage_icp_verify_counts.argtypes = [vp, vp, vp, i, i, i, vp]
    lib.lm_ingest_frames.argtypes = [vp, i, i, C.POINTER(ImageDesc), C.POINTER(ImageDesc), C.POINTER(IngestOpts), vp]
    lib.lm_ingest_release.argtypes = [vp, i, i, vp]
    lib.lm_read_frame.argtypes = [vp, i, vp, vp]
    lib.lm_export_frames.argtypes = [vp, i, i, C.POINTER(ImageDesc), C.POINTER(IngestOpts), vp, sz]
    lib.lm_device_alloc.argtypes = [sz, C.POINTER(vp)]
    lib.lm_device_free.argtypes = [vp]
    lib.lm_device_free.restype = None
    lib.lm_device_copy.argtypes = [vp, vp, sz, i]
    lib.lm_add_templates_slots.argtypes = [vp, C.c_char_p, i, i, C.POINTER(ObjectMask), vp, vp]
    lib.lm_stage_select.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.lm_set_registration.argtypes = [vp, C.POINTER(RegistrationDesc)]
    lib.lm_get_registration_rays.argtypes = [vp, vp]
    lib.lm_ingest_frames_registered.argtypes = [vp, i, i, C.POINTER(ImageDesc), C.POINTER(ImageDesc), C.POINTER(IngestOpts), vp]
    lib.lm_stage_register_depth.argtypes = [vp, C.POINTER(ImageDesc), vp]
    lib.lm_set_rectification.argtypes = [vp, C.POINTER(RectificationDesc)]
    lib.lm_get_rectification_map.argtypes = [vp, vp]
    lib.lm_ingest_frames_rectified.argtypes = [vp, i, i, C.POINTER(ImageDesc), C.POINTER(ImageDesc), C.POINTER(IngestOpts), i, vp]
    lib.lm_stage_rectify.argtypes = [vp, C.POINTER(ImageDesc), C.POINTER(ImageDesc), vp, vp]
    lib.lm_set_reduction.argtypes = [vp, C.POINTER(ReductionDesc)]
    lib.lm_get_reduction.argtypes = [vp, C.POINTER(ReductionDesc), C.POINTER(C.c_int)]
    lib.lm_ingest_frames_reduced.argtypes = [vp, i, i, C.POINTER(ImageDesc), C.POINTER(ImageDesc), C.POINTER(IngestOpts), vp]
    lib.lm_stage_reduce.argtypes = [vp, C.POINTER(ImageDesc), C.POINTER(ImageDesc), vp, vp]
    lib.lm_ingest_frames_rectified_reduced.argtypes = [vp, i, i, C.POINTER(ImageDesc), C.POINTER(ImageDesc), C.POINTER(IngestOpts), i, vp]
    lib.lm_stage_rectify_reduce.argtypes = [vp, C.POINTER(ImageDesc), C.POINTER(ImageDesc), vp, vp]
    lib.lm_reduced_camera.argtypes = [C.POINTER(Camera), C.POINTER(ReductionDesc), i, i, i, i, C.POINTER(Camera)]
    lib.lm_set_raw_processing.argtypes = [vp, C.POINTER(RawProcessing)]
    lib.lm_get_raw_processing.argtypes = [vp, C.POINTER(RawProcessing)]
    if path is None:
        _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check_out(out, ndim=1):
    """A caller-owned result buffer goes to the library as (pointer, capacity): it must be what the library writes."""
    if not isinstance(out, np.ndarray) or out.dtype != MATCH_DTYPE or not out.flags.c_contiguous or out.ndim != ndim \
            or not out.flags.writeable:
        raise ValueError("out must be a writable C-contiguous %d-d numpy array of MATCH_DTYPE" % ndim)
    return out


def _check_counts(counts, n):
    if not isinstance(counts, np.ndarray) or counts.dtype != np.int32 or not counts.flags.c_contiguous or counts.size < n:
        raise ValueError("counts must be a C-contiguous int32 array with one entry per frame")
    return counts


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def default_config(color_only=False, width=640, height=480, keep_depth=False, **overrides):
    """keep_depth: LM_FLAG_KEEP_DEPTH -- a colour-only detector keeps a depth frame beside the colour frame in every slot (never a
    match source; legal and without effect on an RGB-D detector)."""
    cfg = Config()
    load_library().lm_default_config(C.byref(cfg), 1 if color_only else 0, width, height)
    for k, v in overrides.items():
        if k == "T":
            cfg.pyramid_levels = len(v)
            for i_, t in enumerate(v):
                cfg.T[i_] = t
        else:
            setattr(cfg, k, v)
    if keep_depth:
        cfg.flags |= FLAG_KEEP_DEPTH
    return cfg


def _draw_prims(rows):
    out = np.zeros(len(rows), DRAW_PRIM_DTYPE)
    for k, row in enumerate(rows):
        out[k] = row
    return out


def draw_response(det, match, frame, T=None):
    """HighLevelLineMOD::drawResponse as primitives: one ring of radius T // 2 (T: default the detector's T(0)), thickness 1, per
    level-0 feature of the match's template at (f.x + match.x, f.y + match.y) -- blue (255, 0, 0) for the colour modality, green
    (0, 255, 0) for the depth modality.  match: a MATCH_DTYPE record; frame: the frame of the export call.  Builds the array, draws nothing."""
    radius = (det.get_T(0) if T is None else int(T)) // 2
    colours = ((255, 0, 0), (0, 255, 0))
    rows = []
    for m in range(det.cfg.num_modalities):
        _, _, feats = det.get_template(int(match["class_idx"]), int(match["template_id"]), 0, m)
        b, g, r = colours[m]
        for f in feats:
            rows.append((DRAW_RING, int(frame), int(f["x"]) + int(match["x"]), int(f["y"]) + int(match["y"]), radius, 0, 1, b, g, r, 255))
    return _draw_prims(rows)


def draw_axes(rotation, translation, fx, fy, w, h, length=75.0, frame=0):
    """PoseDetection::drawCoordinateSystem as primitives: the pose's origin and the tips of its three axes (`length` model units along
    x, y, z), projected with (fx, fy, w / 2, h / 2) in float64 and rounded half-to-even, as segments of thickness 2 from the origin -- x red
    (0, 0, 255), y green, z blue.  rotation: 3 x 3 (model -> camera), translation: 3.  An axis with an endpoint at Z <= 0 or outside the
    coordinate bound [-8192, 8191] is left out."""
    R = np.asarray(rotation, np.float64).reshape(3, 3)
    t = np.asarray(translation, np.float64).reshape(3)
    pts = [t] + [float(length) * R[:, k] + t for k in range(3)]      # (one multiply and one add per coordinate: host/Draw.h does the same)
    px = []
    for X, Y, Z in pts:
        if not Z > 0.0:
            px.append(None)
            continue
        u, v = np.rint(float(fx) * X / Z + w / 2.0), np.rint(float(fy) * Y / Z + h / 2.0)
        px.append((int(u), int(v)) if -8192 <= u <= 8191 and -8192 <= v <= 8191 else None)
    rows = []
    for k, (b, g, r) in enumerate(((0, 0, 255), (0, 255, 0), (255, 0, 0))):
        if px[0] is not None and px[k + 1] is not None:
            rows.append((DRAW_SEGMENT, int(frame), px[0][0], px[0][1], px[k + 1][0], px[k + 1][1], 2, b, g, r, 255))
    return _draw_prims(rows)


def draw_box(rect, colour, thickness=1, frame=0):
    """One LM_DRAW_BOX: the outline of rect = (x, y, width, height) in `colour` = (b, g, r) or (b, g, r, a)."""
    x, y, bw, bh = (int(v) for v in rect)
    c = tuple(int(v) for v in colour) + ((255,) if len(colour) == 3 else ())
    return _draw_prims([(DRAW_BOX, int(frame), x, y, x + bw - 1, y + bh - 1, int(thickness), c[0], c[1], c[2], c[3])])


def launch_counts():
    """dict(rgb, yuv, bayer, raw, float: launches of a family's kernel on any ingest route; reduce_conv; export; export_float) in this
    process so far (lm_debug_launch_counts).  A kernel is launched only when the call has a frame for it."""
    lib = load_library()
    v = (C.c_int64 * 8)()
    rc = lib.lm_debug_launch_counts(v)
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    return dict(zip(("rgb", "yuv", "bayer", "raw", "float", "reduce_conv", "export", "export_float"), list(v)))


def live_resources():
    """(device buffers, pinned buffers, streams, events) the library holds in this process right now (lm_debug_live_resources)."""
    lib = load_library()
    v = (C.c_int64 * 4)()
    rc = lib.lm_debug_live_resources(v)
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    return tuple(v)


def yaml_numbers(path, key):
    """fs[key] of a cv::FileStorage YAML file as a float64 array (scalar, flow sequence or !!opencv-matrix data)."""
    lib = load_library()
    n = C.c_size_t()
    rc = lib.lm_yaml_numbers(str(path).encode(), key.encode(), None, 0, C.byref(n))
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    out = np.zeros(n.value, np.float64)
    rc = lib.lm_yaml_numbers(str(path).encode(), key.encode(), _ptr(out), out.size, C.byref(n))
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    return out


def yaml_string(path, key):
    lib = load_library()
    buf = C.create_string_buffer(4096)
    rc = lib.lm_yaml_string(str(path).encode(), key.encode(), buf, 4096)
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    return buf.value.decode()


def rendezvous_broadcast(rank, world, payload, addr="127.0.0.1", port=29511, timeout_s=60):
    """rank 0's `payload` (bytes) to every rank over TCP (what lm_comm_init uses for the ncclUniqueId)."""
    lib = load_library()
    buf = C.create_string_buffer(payload, len(payload))
    rc = lib.lm_rendezvous_broadcast(rank, world, addr.encode(), port, buf, len(payload), timeout_s)
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    return buf.raw


def pack_matches(records, counts):
    """[B, cap] per-frame lists + counts -> one contiguous MATCH_DTYPE array (lm_pack_matches)."""
    lib = load_library()
    records = np.ascontiguousarray(records)
    counts = _c(counts, np.int32)
    out = np.zeros(int(counts.sum()), MATCH_DTYPE)
    n = C.c_size_t()
    rc = lib.lm_pack_matches(_ptr(records), records.shape[1], _ptr(counts), len(counts), _ptr(out), out.size, C.byref(n))
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    return out


def merge_batch(packed, counts, frame_lo=0, frame_hi=None):
    """packed: [R, stride] MATCH_DTYPE (rank r's frames back to back), counts: [R, B] -> (merged packed, counts) of the
    frames [frame_lo, frame_hi) (default: all; lm_merge_frames: per frame R-way merge + adjacent-unique)."""
    lib = load_library()
    packed = np.ascontiguousarray(packed)
    counts = _c(counts, np.int32)
    R, B = counts.shape
    frame_hi = B if frame_hi is None else frame_hi
    out = np.zeros(int(counts[:, frame_lo:frame_hi].sum()), MATCH_DTYPE)
    oc = np.zeros(frame_hi - frame_lo, np.int32)
    n = C.c_size_t()
    rc = lib.lm_merge_frames(_ptr(packed), packed.shape[1], _ptr(counts), R, B, frame_lo, frame_hi, _ptr(out), out.size,
                             _ptr(oc), C.byref(n))
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    return out[:n.value], oc


def gather_plan(all_cnt, n_ranks, n_frames, rank):
    """lm_gather_plan: the host bookkeeping of lm_match_end_gathered on the all-gathered lengths (n_ranks runs of n_frames + 1
    int32: per-frame counts, then the rank's status word).  Returns a dict: status, bad_rank, f0, f1, counts [R, n],
    piece_start [R], piece_len [R], max_total (records of the largest rank's run)."""
    lib = load_library()
    all_cnt = _c(all_cnt, np.int32)
    if all_cnt.size != n_ranks * (n_frames + 1):
        raise ValueError("all_cnt must hold n_ranks * (n_frames + 1) values")
    st, bad, f0, f1 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    counts = np.zeros((n_ranks, n_frames), np.int32)
    ps, pl = np.zeros(n_ranks, np.uint64), np.zeros(n_ranks, np.uint64)
    rc = lib.lm_gather_plan(_ptr(all_cnt), n_ranks, n_frames, rank, C.byref(st), C.byref(bad), C.byref(f0), C.byref(f1), _ptr(counts),
                            _ptr(ps), _ptr(pl))
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    mt = C.c_uint64()
    rc = lib.lm_gather_max_total(_ptr(counts), n_ranks, n_frames, C.byref(mt))
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    return {"status": st.value, "bad_rank": bad.value, "f0": f0.value, "f1": f1.value, "counts": counts,
            "piece_start": ps, "piece_len": pl, "max_total": int(mt.value)}


def merge_matches(lists):
    """R-way merge + adjacent-unique of per-shard sorted match arrays (host side of SURVEY.md 8e)."""
    lib = load_library()
    stride = max([len(l) for l in lists] + [1])
    buf = np.zeros((len(lists), stride), MATCH_DTYPE)
    counts = np.zeros(len(lists), np.int32)
    for k, l in enumerate(lists):
        buf[k, :len(l)] = l
        counts[k] = len(l)
    out = np.zeros(int(counts.sum()) + 1, MATCH_DTYPE)
    n = C.c_size_t()
    rc = lib.lm_merge_matches(_ptr(buf), _ptr(counts), len(lists), stride, _ptr(out), out.size, C.byref(n))
    if rc:
        raise LinemodError(rc, lib.lm_last_error().decode())
    return out[:n.value].copy()


class PinnedBuffer:
    """Pinned host memory from lm_host_alloc, viewed as numpy arrays (sources of Detector.upload_frame_pinned)."""

    def __init__(self, nbytes):
        self.lib = load_library()
        p = C.c_void_p()
        rc = self.lib.lm_host_alloc(nbytes, C.byref(p))
        if rc:
            raise LinemodError(rc, self.lib.lm_last_error().decode())
        self.ptr, self.nbytes = p, nbytes
        self._raw = (C.c_uint8 * nbytes).from_address(p.value)

    def view(self, dtype, shape, offset=0):
        """A numpy view of the block.  Views do NOT own the memory: they dangle after close()."""
        if not self.ptr:
            raise ValueError("PinnedBuffer is closed")
        return np.frombuffer(self._raw, dtype=dtype, count=int(np.prod(shape)), offset=offset).reshape(shape)

    def close(self, detectors=()):
        """Frees the block.  An upload that still reads it must have landed first: pass the detectors that were handed
        views of it (their upload_wait(-1) runs here) or wait yourself."""
        if self.ptr:
            for det in detectors:
                det.upload_wait(-1)
            self._raw = None
            self.lib.lm_host_free(self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceView:
    """An array in device memory: nothing but __cuda_array_interface__ (version 2) for a pointer, a dtype, a shape and byte strides."""

    def __init__(self, ptr, dtype, shape, strides=None, owner=None):
        dt = np.dtype(dtype)
        self.ptr, self.dtype, self.shape, self.owner = int(ptr), dt, tuple(int(v) for v in shape), owner
        self.strides = None if strides is None else tuple(int(v) for v in strides)
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": dt.str if dt.itemsize > 1 else "|" + dt.str[1:], "data": (self.ptr, False),
                                         "strides": self.strides, "version": 2}


class DeviceBuffer:
    """Device memory from lm_device_alloc: the home of camera-format frames on their way to Detector.ingest_frame (tests and small
    callers; a producer on the GPU hands over its own tensors)."""

    def __init__(self, nbytes):
        self.lib = load_library()
        p = C.c_void_p()
        rc = self.lib.lm_device_alloc(nbytes, C.byref(p))
        if rc:
            raise LinemodError(rc, self.lib.lm_last_error().decode())
        self.ptr, self.nbytes = p, int(nbytes)

    def _range(self, offset, nbytes):
        if not self.ptr:
            raise ValueError("DeviceBuffer is closed")
        if offset < 0 or offset + nbytes > self.nbytes:
            raise ValueError("bytes [%d, %d) lie outside the buffer's %d" % (offset, offset + nbytes, self.nbytes))
        return C.c_void_p(self.ptr.value + offset)

    def upload(self, array, offset=0):
        """The array's bytes (C order) to byte `offset` of the buffer; synchronous."""
        a = np.ascontiguousarray(array)
        rc = self.lib.lm_device_copy(self._range(offset, a.nbytes), _ptr(a), a.nbytes, 0)
        if rc:
            raise LinemodError(rc, self.lib.lm_last_error().decode())

    def download(self, dtype, shape, offset=0):
        out = np.zeros(shape, dtype)
        rc = self.lib.lm_device_copy(_ptr(out), self._range(offset, out.nbytes), out.nbytes, 1)
        if rc:
            raise LinemodError(rc, self.lib.lm_last_error().decode())
        return out

    def view(self, dtype, shape, offset=0, strides=None):
        """A DeviceView of the block (byte strides; None = C-contiguous).  Views do NOT own the memory: they dangle after close()."""
        dt = np.dtype(dtype)
        st = strides
        if st is None:
            st, acc = [], dt.itemsize
            for n in reversed(shape):
                st.insert(0, acc)
                acc *= n
        if len(st) != len(shape) or any(int(s) < 0 for s in st):
            raise ValueError("one non-negative byte stride per dimension wanted, found %r" % (st,))
        last = sum((int(n) - 1) * int(s) for n, s in zip(shape, st)) + dt.itemsize if all(int(n) > 0 for n in shape) else 0
        return DeviceView(self._range(offset, last).value, dt, shape, strides, owner=self)

    def close(self):
        """Frees the block.  An ingest that still reads it must have landed first (Detector.upload_wait)."""
        if self.ptr:
            self.lib.lm_device_free(self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Detector:
    """cv::linemod::Detector as the reference uses it, on the GPU (see include/linemod_hip.h)."""

    def __init__(self, cfg=None, **kw):
        self.lib = load_library()
        self.cfg = cfg if cfg is not None else default_config(**kw)
        h = C.c_void_p()
        self._check(self.lib.lm_create(C.byref(self.cfg), C.byref(h)))
        self.h = h

    def _check(self, rc):
        if rc:
            raise LinemodError(rc, self.lib.lm_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.lm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- queries -------------------------------------------------------------------------------
    @property
    def width(self):
        return self.cfg.width

    @property
    def height(self):
        return self.cfg.height

    @property
    def num_modalities(self):
        return self.lib.lm_num_modalities(self.h)

    @property
    def keeps_depth(self):
        """The slots keep a depth frame: an RGB-D detector, or a colour-only one created with keep_depth=True (lm_keeps_depth)."""
        return self.lib.lm_keeps_depth(self.h) == 1

    @property
    def pyramid_levels(self):
        return self.lib.lm_pyramid_levels(self.h)

    def get_T(self, level):
        return self.lib.lm_get_T(self.h, level)

    def num_classes(self):
        return self.lib.lm_num_classes(self.h)

    def num_templates(self):
        return self.lib.lm_num_templates(self.h)

    def class_num_templates(self, ci):
        return self.lib.lm_class_num_templates(self.h, ci)

    def class_ids(self):
        return [self.lib.lm_class_id(self.h, k).decode() for k in range(self.num_classes())]

    def find_class(self, class_id):
        return self.lib.lm_find_class(self.h, class_id.encode())

    # ---- tables --------------------------------------------------------------------------------
    def set_similarity_lut(self, lut):
        lut = _c(lut, np.uint8)
        assert lut.size == 256
        self._check(self.lib.lm_set_similarity_lut(self.h, _ptr(lut)))

    def set_normal_lut(self, lut):
        lut = _c(lut, np.uint8)
        assert lut.size == 8000
        self._check(self.lib.lm_set_normal_lut(self.h, _ptr(lut)))

    def similarity_lut(self):
        out = np.zeros(256, np.uint8)
        self._check(self.lib.lm_get_similarity_lut(self.h, _ptr(out)))
        return out

    def normal_lut_is_substitute(self):
        return bool(self.lib.lm_normal_lut_is_substitute(self.h))

    def normal_lut(self):
        out = np.zeros(8000, np.uint8)
        self._check(self.lib.lm_get_normal_lut(self.h, _ptr(out)))
        return out

    # ---- bank ----------------------------------------------------------------------------------
    def add_class(self, class_id, descs, features):
        descs = _c(descs, DESC_DTYPE)
        features = _c(features, FEATURE_DTYPE)
        per = self.cfg.pyramid_levels * self.cfg.num_modalities
        if descs.size % per or int(descs["num_features"].sum()) != features.size:
            raise ValueError("descs/features do not describe whole template pyramids")
        ci = C.c_int()
        self._check(self.lib.lm_add_class(self.h, class_id.encode(), descs.size // per, _ptr(descs), _ptr(features),
                                          C.byref(ci)))
        return ci.value

    def add_template(self, class_id, bgr, depth=None, mask=None):
        bgr = _c(bgr, np.uint8)
        depth = None if depth is None else _c(depth, np.uint16)
        mask = None if mask is None else _c(mask, np.uint8)
        tid, bb = C.c_int(-1), Rect()
        rc = self.lib.lm_add_template(self.h, class_id.encode(), _ptr(bgr), 0, _ptr(depth), 0, _ptr(mask), 0,
                                      C.byref(tid), C.byref(bb))
        if rc == LM_ERR_EXTRACT:
            return -1, (0, 0, 0, 0)
        self._check(rc)
        return tid.value, (bb.x, bb.y, bb.width, bb.height)

    def get_template(self, ci, tid, level, modality):
        w, h, n = C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.lm_get_template(self.h, ci, tid, level, modality, C.byref(w), C.byref(h), None, C.byref(n)))
        feats = np.zeros(n.value, FEATURE_DTYPE)
        self._check(self.lib.lm_get_template(self.h, ci, tid, level, modality, C.byref(w), C.byref(h), _ptr(feats),
                                             C.byref(n)))
        return w.value, h.value, feats

    def save_bank(self, path):
        self._check(self.lib.lm_save_bank(self.h, str(path).encode()))

    def load_bank(self, path):
        self._check(self.lib.lm_load_bank(self.h, str(path).encode()))

    def save_yaml(self, path):
        """cv::FileStorage layout of the reference's linemod_templates.yml.gz (gzip when path ends in .gz)."""
        self._check(self.lib.lm_save_yaml(self.h, str(path).encode()))

    def load_yaml(self, path):
        self._check(self.lib.lm_load_yaml(self.h, str(path).encode()))

    # ---- matching ------------------------------------------------------------------------------
    def _mask(self, mask):
        if mask is None:
            return None
        m = np.asarray(mask)
        if m.shape != (self.cfg.height, self.cfg.width):
            raise ValueError("a mask is [height, width], one byte per level-0 pixel")
        return _c(m if m.dtype == np.uint8 else (m != 0), np.uint8)      # nonzero keeps the pixel, whatever the dtype

    def _mask_pair(self, masks):
        """masks: one array (every modality) or a per-modality pair (colour, depth), either may be None."""
        if isinstance(masks, (tuple, list)):
            if len(masks) != 2:
                raise ValueError("masks: one array or a (colour, depth) pair")
            cm, dm = masks
        else:
            cm, dm = masks, (masks if self.cfg.num_modalities == 2 else None)
        return self._mask(cm), self._mask(dm)

    def match(self, bgr, depth, threshold, class_idx=-1, cap=1 << 16, out=None, masks=None, rule=None):
        """out: a caller-owned MATCH_DTYPE array to fill (no allocation, the result is a view of it; overflow raises).
        masks: Detector::match's masks -- one [height, width] array for every modality or a (colour, depth) pair, nonzero = search
        there (None: no masks, the plain lm_match).
        rule: a MaskRule (or the keyword arguments of make_mask_rule as a dict) set on slot 0 for this call."""
        if rule is not None:
            self.set_mask_rule(0, 1, rule=rule if isinstance(rule, MaskRule) else make_mask_rule(**rule))
            try:
                return self.match(bgr, depth, threshold, class_idx, cap, out, masks)
            finally:
                self.clear_mask_rule(0, 1)
        if masks is not None:
            return self._match_masked(bgr, depth, threshold, class_idx, cap, out, masks)
        bgr = _c(bgr, np.uint8)
        depth = None if depth is None else _c(depth, np.uint16)
        if bgr.shape != (self.cfg.height, self.cfg.width, 3):
            raise ValueError("frame size does not match the detector")
        if out is not None:
            _check_out(out)
            n = C.c_size_t()
            self._check(self.lib.lm_match(self.h, _ptr(bgr), 0, _ptr(depth), 0, threshold, class_idx, _ptr(out), out.size, C.byref(n)))
            return out[:n.value]
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_size_t()
        rc = self.lib.lm_match(self.h, _ptr(bgr), 0, _ptr(depth), 0, threshold, class_idx, _ptr(out), cap, C.byref(n))
        if rc == LM_ERR_OVERFLOW and n.value > cap:
            return self.match(bgr, depth, threshold, class_idx, cap=n.value)
        self._check(rc)
        return out[:n.value].copy()

    def _match_masked(self, bgr, depth, threshold, class_idx, cap, out, masks):
        bgr = _c(bgr, np.uint8)
        depth = None if depth is None else _c(depth, np.uint16)
        if bgr.shape != (self.cfg.height, self.cfg.width, 3):
            raise ValueError("frame size does not match the detector")
        cm, dm = self._mask_pair(masks)
        own = out is None
        out = np.zeros(cap, MATCH_DTYPE) if own else _check_out(out)
        n = C.c_size_t()
        rc = self.lib.lm_match_masked(self.h, _ptr(bgr), 0, _ptr(depth), 0, _ptr(cm), 0, _ptr(dm), 0, threshold, class_idx,
                                      _ptr(out), out.size, C.byref(n))
        if own and rc == LM_ERR_OVERFLOW and n.value > cap:
            return self._match_masked(bgr, depth, threshold, class_idx, n.value, None, masks)
        self._check(rc)
        return out[:n.value].copy() if own else out[:n.value]

    # ---- template-bank generation on the GPU
    def set_render_mesh(self, mesh_idx, vertices, faces):
        """Keeps a triangle mesh resident: vertices (n, 3) float, faces (m, 3) vertex indices."""
        v = _c(vertices, np.float32)
        t = _c(faces, np.uint32)
        self._check(self.lib.lm_set_render_mesh(self.h, int(mesh_idx), _ptr(v), v.size // 3 if v.ndim else 0, _ptr(t), t.size))
        if not hasattr(self, "_mesh_nv"):
            self._mesh_nv = {}
        self._mesh_nv[int(mesh_idx)] = v.size // 3

    def add_templates_rendered(self, class_id, mesh_idx, view_proj, angles, crop_capacity=None):
        """lm_add_templates_rendered: view_proj (n_views, 16) float32 (SoftRender's projection * view, Mat4 order), angles in degrees.
        Returns (template ids (n_views, n_angles), -1 = dropped; bboxes (n_views, n_angles, 4); crops: a list with the rotated depth
        crop (h, w) of every added template, None for the dropped ones)."""
        vp = _c(view_proj, np.float32).reshape(-1, 16)
        an = _c(angles, np.float32).ravel()
        nv, na = vp.shape[0], an.size
        cap = int(crop_capacity) if crop_capacity is not None else max(nv * na, 1) * self.width * self.height
        ids = np.full(max(nv * na, 1), -1, np.int32)
        bbs = np.zeros((max(nv * na, 1), 4), np.int32)
        crops = np.zeros(max(cap, 1), np.uint16)
        offs = np.zeros(max(nv * na, 1) + 1, np.uint64)
        self._check(self.lib.lm_add_templates_rendered(self.h, class_id.encode(), int(mesh_idx), _ptr(vp), nv, _ptr(an), na, _ptr(ids),
                                                       _ptr(bbs), _ptr(crops), cap, _ptr(offs)))
        out = []
        for k in range(nv * na):
            if ids[k] < 0:
                out.append(None)
                continue
            x, y, w, h = (int(v) for v in bbs[k])
            x0, y0 = max(x, 0), max(y, 0)
            cw, ch = max(min(x + w, self.width) - x0, 0), max(min(y + h, self.height) - y0, 0)
            o = int(offs[k])
            out.append(crops[o:o + cw * ch].reshape(ch, cw).copy())
        return ids[:nv * na].reshape(nv, na), bbs[:nv * na].reshape(nv, na, 4), out

    # ---- learning from resident frames
    def add_templates_slots(self, class_id, first_slot, masks):
        """lm_add_templates_slots: one template per slot first_slot, first_slot + 1, ... from the frames resident there, one per entry of
        `masks`.  An entry is None (unmasked), a [height, width] uint8 numpy array (its row stride is passed on), an object with
        __cuda_array_interface__ (a device mask: a torch or cupy tensor, a DeviceBuffer.view) or a MaskRule (make_mask_rule).
        Returns (template ids int32 [n], -1 = extraction failed; bboxes int32 [n, 4])."""
        masks = list(masks)
        n = len(masks)
        arr = (ObjectMask * max(n, 1))()
        keep = []
        for k, m in enumerate(masks):
            if m is None:
                continue
            if isinstance(m, MaskRule):
                arr[k].rule = C.pointer(m)
                continue
            cai = getattr(m, "__cuda_array_interface__", None)
            if isinstance(cai, dict):
                shape, strides = tuple(int(v) for v in cai["shape"]), cai.get("strides")
                if cai["typestr"] != "|u1" or shape != (self.cfg.height, self.cfg.width):
                    raise ValueError("a device mask is [height, width] uint8: typestr %r, shape %r" % (cai["typestr"], shape))
                strides = (shape[1], 1) if strides is None else tuple(int(v) for v in strides)
                if strides[1] != 1 or strides[0] < shape[1]:
                    raise ValueError("a device mask has adjacent pixels and a row stride of at least the width: strides %r" % (strides,))
                arr[k].data, arr[k].row_stride, arr[k].on_device = int(cai["data"][0]), strides[0], 1
                keep.append(m)
                continue
            a = np.asarray(m)
            if a.dtype != np.uint8 or a.shape != (self.cfg.height, self.cfg.width):
                raise ValueError("a mask is a [height, width] uint8 array, a device array, a MaskRule or None")
            if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
                a = np.ascontiguousarray(a)
            arr[k].data, arr[k].row_stride, arr[k].on_device = a.ctypes.data, a.strides[0], 0
            keep.append(a)
        ids = np.full(max(n, 1), -1, np.int32)
        bbs = np.zeros((max(n, 1), 4), np.int32)
        self._check(self.lib.lm_add_templates_slots(self.h, class_id.encode(), int(first_slot), n, arr, _ptr(ids), _ptr(bbs)))
        del keep
        return ids[:n], bbs[:n]

    def stage_select(self, modality, lists, want, area=None):
        """lm_stage_select: addTemplate's feature selection on host-supplied candidate lists.  lists: a sequence of (xy int16 [n, 2],
        labels int32 [n], scores float32 [n]) in row-major order; want: the features wanted per list; area: the depth interior's pixel
        count per list (modality 1).  Returns a list with FEATURE_DTYPE arrays, None for a list with fewer than `want` candidates."""
        lists = list(lists)
        nl = len(lists)
        offs = np.zeros(nl + 1, np.int32)
        for k, (xy, lab, sc) in enumerate(lists):
            offs[k + 1] = offs[k] + len(lab)
        cat = lambda j, dt, tail: (np.concatenate([_c(l[j], dt).reshape((-1,) + tail) for l in lists]) if nl
                                   else np.zeros((0,) + tail, dt))
        xy, lab, sc = _c(cat(0, np.int16, (2,)), np.int16), _c(cat(1, np.int32, ()), np.int32), _c(cat(2, np.float32, ()), np.float32)
        want = _c(np.broadcast_to(np.asarray(want, np.int32), (nl,)), np.int32)
        ar = None if area is None else _c(np.broadcast_to(np.asarray(area, np.float32), (nl,)), np.float32)
        feats = np.zeros((max(nl, 1), 63), FEATURE_DTYPE)
        nout = np.zeros(max(nl, 1), np.int32)
        self._check(self.lib.lm_stage_select(self.h, int(modality), nl, _ptr(offs), _ptr(xy), _ptr(lab), _ptr(sc), _ptr(want), _ptr(ar),
                                             _ptr(feats), _ptr(nout)))
        return [None if nout[k] < 0 else feats[k, :nout[k]].copy() for k in range(nl)]

    def render(self, mesh_idx, view_proj, width, height):
        """lm_stage_render: (coverage (h, w) uint8 255 / 0, depth (h, w) uint16 mm) of a resident mesh."""
        vp = _c(view_proj, np.float32).ravel()
        if vp.size != 16:
            raise ValueError("view_proj must have 16 entries")
        cov = np.zeros((height, width), np.uint8)
        dep = np.zeros((height, width), np.uint16)
        self._check(self.lib.lm_stage_render(self.h, int(mesh_idx), _ptr(vp), int(width), int(height), _ptr(cov), _ptr(dep)))
        return cov, dep

    def rotate(self, img8, img16, angle):
        """lm_stage_rotate: warp_rotate_u8 (one channel) and warp_rotate_u16 of an image pair by `angle` degrees."""
        a = _c(img8, np.uint8)
        b = _c(img16, np.uint16)
        if a.ndim != 2 or a.shape != b.shape:
            raise ValueError("two 2-d images of one size")
        o8 = np.zeros_like(a)
        o16 = np.zeros_like(b)
        self._check(self.lib.lm_stage_rotate(self.h, _ptr(a), _ptr(b), a.shape[1], a.shape[0], float(angle), _ptr(o8), _ptr(o16)))
        return o8, o16

    # ---- pose-error evaluation (Benchmark.cpp's metrics)
    def pose_error_vsd(self, depth, frames, mesh_idx, view_proj_gt, view_proj_est, delta=15, tau=20):
        """lm_pose_error_vsd: the Hodan error of n queries.  depth: one (h, w) or several (n_frames, h, w) uint16 frames; frames: each query's
        frame index (an int for all); mesh_idx: an int or one per query; view_proj_gt / view_proj_est (n, 16) float32 (projection * view,
        Mat4 order).  Returns a VSD_RESULT_DTYPE array of n results (error NaN when nothing is visible in either render)."""
        d = _c(depth, np.uint16)
        if d.ndim == 2:
            d = d[None]
        if d.ndim != 3:
            raise ValueError("depth must be (h, w) or (n_frames, h, w)")
        g = _c(view_proj_gt, np.float32).reshape(-1, 16)
        e = _c(view_proj_est, np.float32).reshape(-1, 16)
        n = len(g)
        if len(e) != n:
            raise ValueError("one estimate per ground truth")
        fr = np.broadcast_to(np.asarray(frames, np.int64), (n,))
        mi = np.broadcast_to(np.asarray(mesh_idx, np.int64), (n,))
        q = (VsdQuery * max(n, 1))()
        for k in range(n):
            q[k].frame, q[k].mesh_idx = int(fr[k]), int(mi[k])
            q[k].view_proj_gt[:] = [float(v) for v in g[k]]
            q[k].view_proj_est[:] = [float(v) for v in e[k]]
        out = np.zeros(max(n, 1), VSD_RESULT_DTYPE)
        self._check(self.lib.lm_pose_error_vsd(self.h, _ptr(d), d.shape[0], d.shape[2], d.shape[1], q, n, int(delta), int(tau), _ptr(out)))
        return out[:n]

    def pose_error_add(self, mesh_idx, R_gt, t_gt, R_est, t_est, step=1, symmetric=False, n_vertices=None, per_vertex=False):
        """lm_pose_error_add: ADD (symmetric False) or ADD-S over the vertices 0, step, ... of a resident render mesh.  R_* (n, 3, 3) or
        (3, 3), t_* (n, 3) or (3,), float32.  Returns the means (n,) float32 and, with per_vertex (n_vertices = the mesh's vertex count,
        default: the one set_render_mesh recorded), the (n, ceil(n_vertices / step)) distances."""
        parts = [np.asarray(R_gt, np.float32).reshape(-1, 9), np.asarray(t_gt, np.float32).reshape(-1, 3),
                 np.asarray(R_est, np.float32).reshape(-1, 9), np.asarray(t_est, np.float32).reshape(-1, 3)]
        n = max(len(a) for a in parts)
        q = np.zeros(n, ADD_QUERY_DTYPE)
        for name, a in zip(("R_gt", "t_gt", "R_est", "t_est"), parts):
            q[name] = np.broadcast_to(a, (n, a.shape[1]))
        mean = np.zeros(max(n, 1), np.float32)
        pv = None
        if per_vertex:
            nv = n_vertices if n_vertices is not None else getattr(self, "_mesh_nv", {}).get(int(mesh_idx))
            if nv is None:
                raise ValueError("per_vertex needs the mesh's vertex count")
            m = (int(nv) + max(int(step), 1) - 1) // max(int(step), 1)
            pv = np.zeros((max(n, 1), m), np.float32)
        self._check(self.lib.lm_pose_error_add(self.h, int(mesh_idx), int(step), 1 if symmetric else 0, _ptr(q), n, _ptr(mean), _ptr(pv)))
        return (mean[:n], pv[:n]) if per_vertex else mean[:n]

    def vsd_counts(self, gt_depth, est_depth, scene, delta=15, tau=20):
        """lm_stage_vsd_counts: the counting rule of lm_pose_error_vsd on three (h, w) uint16 images; one VSD_RESULT_DTYPE record."""
        g, e, s = _c(gt_depth, np.uint16), _c(est_depth, np.uint16), _c(scene, np.uint16)
        if g.ndim != 2 or g.shape != e.shape or g.shape != s.shape:
            raise ValueError("three 2-d images of one size")
        out = np.zeros(1, VSD_RESULT_DTYPE)
        self._check(self.lib.lm_stage_vsd_counts(self.h, _ptr(g), _ptr(e), _ptr(s), g.shape[1], g.shape[0], int(delta), int(tau), _ptr(out)))
        return out[0]

    # ---- ICP pose refinement (HighLevelLinemodIcp)
    def icp_set_model(self, class_idx, xyzn, step=2):
        """The model cloud of a class: rows 0, step, 2 step, ... of xyzn ((n, 6) float: the PLY's x y z nx ny nz)."""
        a = _c(xyzn, np.float32)
        if a.ndim != 2 or a.shape[1] != 6:
            raise ValueError("xyzn must be an (n, 6) array")
        self._check(self.lib.lm_icp_set_model(self.h, int(class_idx), _ptr(a), len(a), int(step)))

    def icp_scene_cloud(self, depth, bbox, camera, step=2, cap=None):
        """prepareDepthForIcp on the GPU: the (n, 6) float32 scene cloud of bbox (x, y, w, h) of a uint16 depth frame, camera =
        (fx, fy, cx, cy)."""
        d = _c(depth, np.uint16)
        bb = np.asarray(bbox, np.int32).ravel()
        K = np.asarray(camera, np.float64).ravel()
        if bb.size != 4 or K.size != 4 or d.ndim != 2:
            raise ValueError("bbox must be (x, y, w, h), camera (fx, fy, cx, cy), depth 2-d")
        cap = int(max(bb[2], 0) * max(bb[3], 0) // max(int(step), 1)) if cap is None else int(cap)
        out = np.zeros((max(cap, 1), 6), np.float32)
        n = C.c_int(0)
        self._check(self.lib.lm_stage_icp_scene(self.h, _ptr(d), d.shape[1], d.shape[0], _ptr(K), _ptr(bb), int(step), _ptr(out),
                                                cap, C.byref(n)))
        return out[:n.value].copy()

    def icp_refine(self, depth_or_slot, bbox, class_idx, poses, camera, step=2, iterations=6, tolerance=0.1, rejection_scale=2.5,
                   levels=8, counts=None, max_points=0):
        """ICP(iterations, tolerance, rejection_scale, levels)::registerModelToScene of poses ((n, 4, 4), model to camera, mm) against the
        scene cloud of bbox.  depth_or_slot: a frame slot (its resident, principal-point-shifted frame: the intrinsics become (fx, fy,
        w / 2, h / 2)) or a uint16 depth frame of the detector's size (camera used as given).  Several queries in one call: bbox a list
        of (x, y, w, h), class_idx an int or a list, counts the number of poses of each query (consecutive in poses).  Returns the
        refined (n, 4, 4) poses."""
        P = np.array(poses, np.float64).reshape(-1, 4, 4).copy()
        boxes = np.asarray(bbox, np.int64).reshape(-1, 4)
        nq = len(boxes)
        classes = [int(class_idx)] * nq if np.ndim(class_idx) == 0 else [int(c) for c in class_idx]
        counts = [len(P)] if counts is None else [int(c) for c in counts]
        if len(classes) != nq or len(counts) != nq or sum(counts) != len(P):
            raise ValueError("one class and one pose count per bbox, the counts adding up to the poses")
        fx, fy, cx, cy = (float(v) for v in camera)
        q = (IcpQuery * max(nq, 1))()
        first = 0
        for k in range(nq):
            x, y, w, h = (int(v) for v in boxes[k])
            q[k] = IcpQuery(x, y, w, h, classes[k], first, counts[k], 0, fx, fy, cx, cy)
            first += counts[k]
        prm = IcpParams(int(step), int(iterations), float(tolerance), float(rejection_scale), int(levels), int(max_points))
        if isinstance(depth_or_slot, (int, np.integer)):
            rc = self.lib.lm_icp_refine(self.h, int(depth_or_slot), q, nq, C.byref(prm), _ptr(P))
        else:
            d = _c(depth_or_slot, np.uint16)
            if d.shape != (self.cfg.height, self.cfg.width):
                raise ValueError("depth frame size does not match the detector")
            rc = self.lib.lm_stage_icp_refine_host(self.h, _ptr(d), q, nq, C.byref(prm), _ptr(P))
        self._check(rc)
        return P

    def icp_refine_slots(self, slots, bbox, class_idx, poses, camera, counts=None, step=2, iterations=6, tolerance=0.1, rejection_scale=2.5,
                         levels=8, max_points=0, return_status=False):
        """lm_icp_refine_slots: icp_refine over a batch of frames in one call.  slots: the frame slot of each query (an int for all);
        bbox a list of (x, y, w, h), class_idx an int or one per query, counts the poses of each query (consecutive in poses; None: one
        query takes them all), camera (fx, fy, cx, cy) or one per query.  Every query reads its slot's resident, principal-point-shifted
        frame with (fx, fy, w / 2, h / 2).  Returns the refined (n, 4, 4) poses; with return_status (poses, status (n_queries,) int32, rc)
        and no exception for a query that was not refined (a cloud of fewer than 6 points, or one over the capacity: its poses stay);
        without it the first such query raises.  A refused call always raises."""
        P = np.array(poses, np.float64).reshape(-1, 4, 4).copy()
        boxes = np.asarray(bbox, np.int64).reshape(-1, 4)
        nq = len(boxes)
        sl = np.ascontiguousarray(np.broadcast_to(np.asarray(slots, np.int32), (nq,)))
        classes = [int(class_idx)] * nq if np.ndim(class_idx) == 0 else [int(c) for c in class_idx]
        counts = [len(P)] if counts is None else [int(c) for c in counts]
        cams = np.broadcast_to(np.asarray(camera, np.float64), (nq, 4))
        if len(classes) != nq or len(counts) != nq or sum(counts) != len(P):
            raise ValueError("one class and one pose count per bbox, the counts adding up to the poses")
        q = (IcpQuery * max(nq, 1))()
        first = 0
        for k in range(nq):
            x, y, w, h = (int(v) for v in boxes[k])
            q[k] = IcpQuery(x, y, w, h, classes[k], first, counts[k], 0, *(float(v) for v in cams[k]))
            first += counts[k]
        prm = IcpParams(int(step), int(iterations), float(tolerance), float(rejection_scale), int(levels), int(max_points))
        status = np.full(max(nq, 1), -1, np.int32)
        rc = self.lib.lm_icp_refine_slots(self.h, _ptr(sl) if nq else None, q, nq, C.byref(prm), _ptr(P), _ptr(status))
        status = status[:nq]
        refused = rc != LM_OK and (nq == 0 or (status == -1).all())      # (a refused call leaves the statuses as they were)
        if rc != LM_OK and (refused or not return_status):
            self._check(rc)
        return (P, status, rc) if return_status else P

    def icp_batch_stats(self):
        """(chunks, kernel launches, host synchronisations) of the detector's last ICP refinement."""
        out = np.zeros(3, np.int32)
        self._check(self.lib.lm_stage_icp_batch_stats(self.h, _ptr(out)))
        return tuple(int(v) for v in out)

    def icp_verify(self, depth_or_slots, frames, mesh_idx, view_proj, scene_min=600):
        """The best-pose check of n poses (estimateBestMatch's mean depth difference): the resident render mesh under view_proj (n, 16)
        float32 (projection * view, Mat4 order) against a depth frame.  depth_or_slots: one (h, w) or several (n_frames, h, w) uint16
        frames, `frames` then being each query's frame index (an int for all; lm_stage_icp_verify_host); or a frame slot or a sequence
        of one slot per query, whose resident frames are read (lm_icp_verify; `frames` is not used and may be None).  mesh_idx: an int
        or one per query.  Returns (count (n,) uint32, sum (n,) uint64, mean (n,) float64)."""
        v = _c(view_proj, np.float32).reshape(-1, 16)
        n = len(v)
        mi = np.broadcast_to(np.asarray(mesh_idx, np.int64), (n,))
        is_slots = isinstance(depth_or_slots, (int, np.integer)) or (
            isinstance(depth_or_slots, (list, tuple)) and all(isinstance(x, (int, np.integer)) for x in depth_or_slots)) or (
            isinstance(depth_or_slots, np.ndarray) and depth_or_slots.ndim <= 1 and depth_or_slots.dtype.kind in "iu")
        if is_slots:
            fr = np.broadcast_to(np.asarray(depth_or_slots, np.int64), (n,))
        else:
            d = _c(depth_or_slots, np.uint16)
            if d.ndim == 2:
                d = d[None]
            if d.ndim != 3:
                raise ValueError("depth must be (h, w) or (n_frames, h, w)")
            fr = np.broadcast_to(np.asarray(frames, np.int64), (n,))
        q = (IcpVerifyQuery * max(n, 1))()
        for k in range(n):
            q[k].frame, q[k].mesh_idx = int(fr[k]), int(mi[k])
            q[k].view_proj[:] = [float(x) for x in v[k]]
        out = np.zeros(max(n, 1), ICP_VERIFY_RESULT_DTYPE)
        if is_slots:
            self._check(self.lib.lm_icp_verify(self.h, q, n, int(scene_min), _ptr(out)))
        else:
            self._check(self.lib.lm_stage_icp_verify_host(self.h, _ptr(d), d.shape[0], d.shape[2], d.shape[1], q, n, int(scene_min), _ptr(out)))
        out = out[:n]
        return out["count"].copy(), out["sum"].copy(), out["mean"].copy()

    def icp_verify_counts(self, render, scene, scene_min=600):
        """lm_stage_icp_verify_counts: the counting rule of icp_verify on two (h, w) uint16 images; returns (count, sum, mean)."""
        r, s = np.asarray(render, np.uint16), np.asarray(scene, np.uint16)
        if r.ndim != 2 or r.shape != s.shape:
            raise ValueError("two 2-d images of one size")
        r, s = np.ascontiguousarray(r), np.ascontiguousarray(s)
        out = np.zeros(1, ICP_VERIFY_RESULT_DTYPE)
        self._check(self.lib.lm_stage_icp_verify_counts(self.h, _ptr(r), _ptr(s), r.shape[1], r.shape[0], int(scene_min), _ptr(out)))
        return int(out[0]["count"]), int(out[0]["sum"]), float(out[0]["mean"])

    def upload_match_mask(self, slot, mask, modality=-1):
        """Detector::match's mask for the frame resident in `slot` (upload the frame first: a frame upload clears the slot's masks).
        modality 0 = colour, 1 = depth, -1 = every modality; mask None clears it."""
        m = self._mask(mask)
        self._check(self.lib.lm_upload_match_mask(self.h, slot, modality, _ptr(m), 0))

    def set_mask_rule(self, first_slot, n_slots, *, modalities=None, depth_range=None, keep_invalid=False, hsv_range=None, grow=0,
                      rect=None, rule=None):
        """A sticky mask rule on slots [first_slot, first_slot + n_slots): every pre-processing of such a slot computes the mask from
        the frame it then holds (lm_set_mask_rule).  Either the fields (see make_mask_rule) or a ready MaskRule as `rule`."""
        if rule is None:
            rule = make_mask_rule(modalities, depth_range, keep_invalid, hsv_range, grow, rect)
        self._check(self.lib.lm_set_mask_rule(self.h, int(first_slot), int(n_slots), C.byref(rule)))

    def clear_mask_rule(self, first_slot=0, n_slots=None):
        n = self.cfg.frame_slots - int(first_slot) if n_slots is None else int(n_slots)
        self._check(self.lib.lm_set_mask_rule(self.h, int(first_slot), n, None))

    def mask_rule(self, slot):
        """The slot's MaskRule, or None."""
        r, on = MaskRule(), C.c_int()
        self._check(self.lib.lm_get_mask_rule(self.h, int(slot), C.byref(r), C.byref(on)))
        return r if on.value else None

    def stage_mask_rule(self, bgr, depth, rule):
        """lm_stage_mask_rule: the [height, width] level-0 mask (0 / 255) of `rule` for host images of the detector's size."""
        b = None if bgr is None else _c(bgr, np.uint8)
        d = None if depth is None else _c(depth, np.uint16)
        h, w = self.cfg.height, self.cfg.width
        if (b is not None and b.shape != (h, w, 3)) or (d is not None and d.shape != (h, w)):
            raise ValueError("frame size does not match the detector")
        out = np.zeros((h, w), np.uint8)
        self._check(self.lib.lm_stage_mask_rule(self.h, _ptr(b), _ptr(d), w, h, C.byref(rule), _ptr(out)))
        return out

    def upload_frame(self, slot, bgr, depth=None):
        bgr = _c(bgr, np.uint8)
        depth = None if depth is None else _c(depth, np.uint16)
        if bgr.shape != (self.cfg.height, self.cfg.width, 3):
            raise ValueError("frame size does not match the detector")
        self._check(self.lib.lm_upload_frame(self.h, slot, _ptr(bgr), 0, _ptr(depth), 0))

    def upload_frame_shifted(self, slot, bgr, depth, shift_x, shift_y):
        """upload_frame of the frame translated by (shift_x, shift_y) pixels, zeros shifted in (the reference's principal-point shift)."""
        bgr = _c(bgr, np.uint8)
        depth = None if depth is None else _c(depth, np.uint16)
        if bgr.shape != (self.cfg.height, self.cfg.width, 3):
            raise ValueError("frame size does not match the detector")
        self._check(self.lib.lm_upload_frame_shifted(self.h, slot, _ptr(bgr), 0, _ptr(depth), 0, int(shift_x), int(shift_y)))

    def upload_frame_pinned(self, slot, bgr, depth=None):
        """Source arrays must live in pinned host memory (PinnedBuffer) and stay untouched until upload_wait(slot)
        or until a match that covers the slot has been collected."""
        if bgr.dtype != np.uint8 or not bgr.flags.c_contiguous or bgr.shape != (self.cfg.height, self.cfg.width, 3):
            raise ValueError("pinned colour frame must be a C-contiguous uint8 [h, w, 3] array of the detector's size")
        if depth is not None and (depth.dtype != np.uint16 or not depth.flags.c_contiguous):
            raise ValueError("pinned depth frame must be a C-contiguous uint16 array")
        self._check(self.lib.lm_upload_frame_pinned(self.h, slot, _ptr(bgr), 0, _ptr(depth), 0))

    def upload_frames_pinned(self, first_slot, n_slots, frames_ptr, frame_stride=0):
        """frames_ptr: address (int / c_void_p) of n_slots pinned host frames, each [colour | depth] dense."""
        self._check(self.lib.lm_upload_frames_pinned(self.h, first_slot, n_slots, C.c_void_p(frames_ptr), frame_stride))

    def upload_wait(self, slot=-1):
        self._check(self.lib.lm_upload_wait(self.h, slot))

    def set_registration(self, depth_cam, colour_cam, rotation, translation, splat=(0, 0), rays=None):
        """lm_set_registration: the rig's depth and colour cameras (Camera, see camera()), P_colour = rotation (3 x 3) * P_depth +
        translation (millimetres), the splat's half widths (0 .. 3 each) and optionally the depth camera's own ray table, a float32
        [height, width, 2] host array (rx, ry per pixel) for a camera that is no pinhole.  depth_cam = None clears the registration."""
        if depth_cam is None:
            self._check(self.lib.lm_set_registration(self.h, None))
            self._reg_sizes = None
            return
        r = RegistrationDesc()
        r.depth, r.colour = depth_cam, colour_cam
        R, t = _c(rotation, np.float32).reshape(-1), _c(translation, np.float32).reshape(-1)
        if R.size != 9 or t.size != 3:
            raise ValueError("rotation with %d and translation with %d numbers (3 x 3 and 3 wanted)" % (R.size, t.size))
        r.rotation[:], r.translation[:] = R.tolist(), t.tolist()
        r.splat_x, r.splat_y = int(splat[0]), int(splat[1])
        if rays is not None:
            rays = _c(rays, np.float32)
            if rays.size != 2 * int(depth_cam.width) * int(depth_cam.height):
                raise ValueError("ray table with %d floats (2 x %d x %d wanted)" % (rays.size, depth_cam.width, depth_cam.height))
            r.rays = rays.ctypes.data
        self._check(self.lib.lm_set_registration(self.h, C.byref(r)))
        self._reg_sizes = (int(depth_cam.width), int(depth_cam.height), int(colour_cam.width), int(colour_cam.height))

    def registration_rays(self):
        """lm_get_registration_rays: the depth camera's ray table as the device uses it, float32 [height, width, 2]."""
        sizes = getattr(self, "_reg_sizes", None)
        if sizes is None:
            self._check(self.lib.lm_get_registration_rays(self.h, None))      # (the library's refusal, in its words)
        out = np.zeros((sizes[1], sizes[0], 2), np.float32)
        self._check(self.lib.lm_get_registration_rays(self.h, _ptr(out)))
        return out

    def stage_register_depth(self, depth, scale=1.0):
        """lm_stage_register_depth: the whole registered image, uint16 [colour height, colour width], of a raw depth image (a host
        uint16 or float32 [height, width] array of the depth camera's size, float times `scale` = millimetres)."""
        sizes = getattr(self, "_reg_sizes", None)
        depth = np.ascontiguousarray(depth)
        if depth.dtype not in (np.uint16, np.float32) or depth.ndim != 2:
            raise ValueError("raw depth image: %s %r ([H, W] uint16 or float32 wanted)" % (depth.dtype, depth.shape))
        with DeviceBuffer(max(depth.nbytes, 1)) as buf:
            buf.upload(depth)
            desc = image_desc(buf.view(depth.dtype.type, depth.shape), True, scale=scale)
            out = np.zeros((sizes[3], sizes[2]) if sizes else (1, 1), np.uint16)
            self._check(self.lib.lm_stage_register_depth(self.h, C.byref(desc), _ptr(out)))
        return out

    def set_rectification(self, source, ideal=None, map=None):
        """lm_set_rectification: the source camera (Camera, see camera(): pinhole + Brown-Conrady, the size of the source images) and the
        ideal camera (zero coefficients; its size is the rectified geometry; None = the source's pinhole with zero coefficients), and
        optionally the caller's own map, a float32 [ideal height, ideal width, 2] host array ((sx, sy) per ideal pixel, anything allowed)
        for a lens that is no Brown-Conrady one.  source = None clears the rectification."""
        if source is None:
            self._check(self.lib.lm_set_rectification(self.h, None))
            self._rect_sizes = None
            return
        if ideal is None:
            ideal = camera(source.width, source.height, source.fx, source.fy, source.cx, source.cy)
        r = RectificationDesc()
        r.source, r.ideal = source, ideal
        if map is not None:
            map = _c(map, np.float32)
            if map.size != 2 * int(ideal.width) * int(ideal.height):
                raise ValueError("map with %d floats (2 x %d x %d wanted)" % (map.size, ideal.width, ideal.height))
            r.map = map.ctypes.data
        self._check(self.lib.lm_set_rectification(self.h, C.byref(r)))
        self._rect_sizes = (int(source.width), int(source.height), int(ideal.width), int(ideal.height))

    def rectification_map(self):
        """lm_get_rectification_map: the fixed-point map as the device uses it, int32 [ideal height, ideal width, 2] = (qx, qy)."""
        sizes = getattr(self, "_rect_sizes", None)
        if sizes is None:
            self._check(self.lib.lm_get_rectification_map(self.h, None))      # (the library's refusal, in its words)
        out = np.zeros((sizes[3], sizes[2], 2), np.int32)
        self._check(self.lib.lm_get_rectification_map(self.h, _ptr(out)))
        return out

    def set_raw_processing(self, black=0, gains=(1.0, 1.0, 1.0), ccm=None, tone=None):
        """lm_set_raw_processing: the raw pipeline of the raw colour layouts (high-bit Bayer and mono, and 8-bit Bayer while one is set):
        black level in source sample units, white-balance gains (R, G, B) and the 3 x 3 colour matrix (rows = output R, G, B; None = the
        identity) as floats, taken to Q10 with numpy.rint, and the tone table (uint8 [4096], indexed by the 16-bit result >> 4; None =
        i >> 4; tone_curve(gamma) makes one).  set_raw_processing(None) resets to "nothing set"."""
        if black is None:
            self._check(self.lib.lm_set_raw_processing(self.h, None))
            return
        g = np.rint(np.asarray(gains, np.float64) * 1024.0)
        m = np.rint(np.asarray(np.eye(3) if ccm is None else ccm, np.float64) * 1024.0)
        t = np.arange(4096, dtype=np.int64) >> 4 if tone is None else np.asarray(tone)
        if g.shape != (3,) or m.shape != (3, 3) or t.shape != (4096,):
            raise ValueError("gains %r, ccm %r, tone %r (3 gains, a 3 x 3 matrix and 4096 table entries wanted)" % (g.shape, m.shape, t.shape))
        if not (np.isfinite(g).all() and np.isfinite(m).all()) or g.min() < 0 or g.max() > 0xFFFFFFFF or np.abs(m).max() > 0x7FFFFFFF:
            raise ValueError("gains %r, ccm %r (finite numbers, gains not negative, wanted)" % (g.tolist(), m.tolist()))
        if t.dtype.kind not in "iu" or t.min() < 0 or t.max() > 255:
            raise ValueError("tone: dtype %s, %d .. %d (integers 0 .. 255 wanted)" % (t.dtype, int(t.min()), int(t.max())))
        p = RawProcessing()
        p.black = int(min(max(int(black), -0x80000000), 0x7FFFFFFF))
        p.gain[:] = [int(v) for v in g]
        p.ccm[:] = [int(v) for v in m.reshape(9)]
        t8 = np.ascontiguousarray(t, np.uint8)
        C.memmove(p.tone, t8.ctypes.data, 4096)
        self._check(self.lib.lm_set_raw_processing(self.h, C.byref(p)))

    def raw_processing(self):
        """lm_get_raw_processing: dict(black, gain uint32 [3], ccm int32 [3, 3], tone uint8 [4096]) as the device uses them, Q10; with
        nothing set, the identity."""
        p = RawProcessing()
        self._check(self.lib.lm_get_raw_processing(self.h, C.byref(p)))
        return dict(black=int(p.black), gain=np.array(p.gain[:], np.uint32), ccm=np.array(p.ccm[:], np.int32).reshape(3, 3),
                    tone=np.frombuffer(bytes(p.tone), np.uint8).copy())

    def set_reduction(self, ratio, colour=True, depth=True, depth_rule="nearest"):
        """lm_set_reduction: the area-averaged reduction of the reduced ingest.  ratio = (num, den), source pixels per reduced pixel
        (1 <= den <= 16, den <= num <= 8 den), or a pair of them for x and y; colour / depth: which images of a frame are reduced (an
        image that is not takes the plain ingest's rule); depth_rule "nearest" or "min_valid".  ratio = None clears the reduction."""
        if ratio is None:
            self._check(self.lib.lm_set_reduction(self.h, None))
            return
        r = reduction_desc(ratio, colour, depth, depth_rule)
        self._check(self.lib.lm_set_reduction(self.h, C.byref(r)))

    def reduction(self):
        """lm_get_reduction: None, or dict(ratio=((num_x, den_x), (num_y, den_y)) in lowest terms, colour, depth, depth_rule)."""
        r, on = ReductionDesc(), C.c_int(0)
        self._check(self.lib.lm_get_reduction(self.h, C.byref(r), C.byref(on)))
        if not on.value:
            return None
        return dict(ratio=((r.num_x, r.den_x), (r.num_y, r.den_y)), colour=bool(r.apply & REDUCE_COLOUR), depth=bool(r.apply & REDUCE_DEPTH),
                    depth_rule={v: k for k, v in _REDUCE_DEPTH_RULES.items()}[r.depth_rule])

    def stage_reduce(self, colour=None, depth=None, *, order="bgr", layout="hwc", matrix="bt601", range="limited", depth_scale=1.0, bits=8, packed=False,
                     width=None, float_scale=None):
        """lm_stage_reduce: the whole reduced images (bgr uint8 [Ry, Rx, 3] or None, depth uint16 [Ry, Rx] or None, each of its own
        image's reduced size) of one source pair in DEVICE memory (objects with __cuda_array_interface__, see image_desc)."""
        cd = image_desc(colour, False, order, layout, matrix=matrix, range=range, bits=bits, packed=packed, width=width, float_scale=float_scale) if colour is not None else None
        dd = image_desc(depth, True, scale=depth_scale) if depth is not None else None
        red = self.reduction()

        def shape(desc, on):
            if red is None:
                return (1, 1)
            (nx, dx), (ny, dy) = red["ratio"] if on else ((1, 1), (1, 1))
            return (max(int(desc.height), 0) * dy // ny, max(int(desc.width), 0) * dx // nx)
        bgr = np.zeros(shape(cd, red and red["colour"]) + (3,), np.uint8) if cd is not None else None
        dep = np.zeros(shape(dd, red and red["depth"]), np.uint16) if dd is not None else None
        self._check(self.lib.lm_stage_reduce(self.h, None if cd is None else C.byref(cd), None if dd is None else C.byref(dd), _ptr(bgr), _ptr(dep)))
        return bgr, dep

    def stage_rectify_reduce(self, colour=None, depth=None, *, order="bgr", layout="hwc", matrix="bt601", range="limited", depth_scale=1.0, bits=8,
                             packed=False, width=None, float_scale=None):
        """lm_stage_rectify_reduce: the whole rectified and reduced images (bgr uint8 [Ry, Rx, 3] or None, depth uint16 [Ry, Rx] or None,
        each the reduced IDEAL geometry of its own ratio; an image the reduction does not apply to: the whole rectified image) of one
        source pair in DEVICE memory (objects with __cuda_array_interface__, see image_desc)."""
        cd = image_desc(colour, False, order, layout, matrix=matrix, range=range, bits=bits, packed=packed, width=width, float_scale=float_scale) if colour is not None else None
        dd = image_desc(depth, True, scale=depth_scale) if depth is not None else None
        red, sizes = self.reduction(), getattr(self, "_rect_sizes", None)

        def shape(on):
            if red is None or sizes is None:
                return (1, 1)
            (nx, dx), (ny, dy) = red["ratio"] if on else ((1, 1), (1, 1))
            return (sizes[3] * dy // ny, sizes[2] * dx // nx)
        bgr = np.zeros(shape(red and red["colour"]) + (3,), np.uint8) if cd is not None else None
        dep = np.zeros(shape(red and red["depth"]), np.uint16) if dd is not None else None
        self._check(self.lib.lm_stage_rectify_reduce(self.h, None if cd is None else C.byref(cd), None if dd is None else C.byref(dd), _ptr(bgr), _ptr(dep)))
        return bgr, dep

    def stage_rectify(self, colour=None, depth=None, *, order="bgr", layout="hwc", matrix="bt601", range="limited", depth_scale=1.0, bits=8, packed=False,
                      width=None, float_scale=None):
        """lm_stage_rectify: the whole rectified images (bgr uint8 [ideal height, ideal width, 3] or None, depth uint16 [ideal height,
        ideal width] or None) of one source pair in DEVICE memory (objects with __cuda_array_interface__, see image_desc)."""
        sizes = getattr(self, "_rect_sizes", None)
        shape = (sizes[3], sizes[2]) if sizes else (1, 1)
        cd = image_desc(colour, False, order, layout, matrix=matrix, range=range, bits=bits, packed=packed, width=width, float_scale=float_scale) if colour is not None else None
        dd = image_desc(depth, True, scale=depth_scale) if depth is not None else None
        bgr = np.zeros(shape + (3,), np.uint8) if cd is not None else None
        dep = np.zeros(shape, np.uint16) if dd is not None else None
        self._check(self.lib.lm_stage_rectify(self.h, None if cd is None else C.byref(cd), None if dd is None else C.byref(dd), _ptr(bgr), _ptr(dep)))
        return bgr, dep

    def ingest_frame(self, slot, colour, depth=None, *, order="bgr", layout="hwc", crop=(0, 0), depth_crop=None, depth_scale=1.0,
                     flip_x=False, shift=(0, 0), stream=None, matrix="bt601", range="limited", register_depth=False, rectified=False,
                     registered=False, bits=8, packed=False, width=None, reduced=False, rectify_reduce=False, float_scale=None):
        """A frame that lies in DEVICE memory in its producer's format -> slot (lm_ingest_frames): the detector-size window at `crop`
        (depth_crop: the depth image's own, default the same), channels to BGR (grey and YUV layouts: converted with `matrix` and
        `range`; raw layouts with `bits`, `packed`, `width`: image_desc; a float32 / float16 colour object with `float_scale`: every channel
        rint(v * float_scale) clamped to 0 .. 255), float depth times depth_scale to uint16 millimetres, mirrored (flip_x), translated by `shift` with zeros shifted in.  colour, depth: objects with __cuda_array_interface__ (see
        image_desc).  Asynchronous: the sources stay untouched until upload_wait(slot) or until work behind ingest_release runs.
        register_depth: `depth` is the RAW image of the depth camera, registered onto the colour camera first (set_registration,
        lm_ingest_frames_registered); depth_crop (default: crop) then places the window in the colour camera's geometry.
        rectified: the images are the source camera's and go through the lens rectification first (set_rectification,
        lm_ingest_frames_rectified); crop and depth_crop then place the window in the IDEAL geometry.  With registered=True `depth` is the
        RAW image of the depth camera and takes the registration's route, and only the colour image is rectified.
        reduced: the images are at the camera's resolution and go through the area-averaged reduction first (set_reduction,
        lm_ingest_frames_reduced); crop and depth_crop then place the window in each image's REDUCED geometry.  Not together with
        rectified / register_depth: a lens map in front of the reduction is rectify_reduce's.
        rectify_reduce: the images are the source camera's, at its resolution, and go through the lens rectification AND the reduction in
        one pass (set_rectification and set_reduction, lm_ingest_frames_rectified_reduced): what cv::remap followed by
        cv::resize(INTER_AREA) gives; crop and depth_crop then place the window in the REDUCED IDEAL geometry.  With registered=True
        `depth` is the RAW image of the depth camera and takes the registration's route onto the slot's camera.  A keyword of its own,
        not together with rectified, reduced or register_depth."""
        self.ingest_frames(slot, [dict(colour=colour, depth=depth, order=order, layout=layout, crop=crop, depth_crop=depth_crop,
                                       depth_scale=depth_scale, flip_x=flip_x, shift=shift, matrix=matrix, range=range,
                                       register_depth=register_depth, rectified=rectified, registered=registered, bits=bits, packed=packed,
                                       width=width, reduced=reduced, rectify_reduce=rectify_reduce, float_scale=float_scale)], stream=stream)

    def ingest_frames(self, first_slot, frames, stream=None):
        """frames[i] (a dict of ingest_frame's arguments; `colour` is required) -> slot first_slot + i, all in ONE kernel launch under one
        upload ticket.  stream: the integer handle of the HIP stream that produces the sources (the ingest waits for the work enqueued
        on it so far), or None = they are complete.  register_depth, rectified, registered, reduced and rectify_reduce are the call's:
        every frame of a call has the same."""
        n = len(frames)
        rgbd = self.keeps_depth
        if rgbd and self.cfg.num_modalities < 2:
            # the depth image is optional beside a colour-only detector, for the call as a whole
            given = {f.get("depth") is not None for f in frames}
            if len(given) > 1:
                raise ValueError("some frames of the call bring a depth image and some do not")
            rgbd = True in given
        col, dep, opts = (ImageDesc * max(n, 1))(), (ImageDesc * max(n, 1))(), (IngestOpts * max(n, 1))()
        registered = {bool(f.get("register_depth", False)) for f in frames}
        if len(registered) > 1:
            raise ValueError("register_depth differs between the frames of one call")
        registered = True in registered
        routes = {(bool(f.get("rectified", False)), bool(f.get("registered", False))) for f in frames}
        if len(routes) > 1:
            raise ValueError("rectified / registered differ between the frames of one call")
        rectified, rect_registered = routes.pop() if routes else (False, False)
        both = {bool(f.get("rectify_reduce", False)) for f in frames}
        if len(both) > 1:
            raise ValueError("rectify_reduce differs between the frames of one call")
        both = True in both
        if both and (rectified or registered or True in {bool(f.get("reduced", False)) for f in frames}):
            raise ValueError("rectify_reduce=True does not go together with rectified, reduced or register_depth: it is both routes in one "
                             "(registered=True is the raw depth image beside it)")
        if rect_registered and not (rectified or both):
            raise ValueError("registered=True belongs to rectified=True (without rectification: register_depth=True)")
        reduced = {bool(f.get("reduced", False)) for f in frames}
        if len(reduced) > 1:
            raise ValueError("reduced differs between the frames of one call")
        reduced = True in reduced
        if reduced and (rectified or registered or rect_registered):
            raise ValueError("reduced=True does not go together with rectified / register_depth: a reduction behind a lens map or a registration is not served")
        for k, f in enumerate(frames):
            unknown = set(f) - {"colour", "depth", "order", "layout", "crop", "depth_crop", "depth_scale", "flip_x", "shift", "matrix", "range",
                                "register_depth", "rectified", "registered", "bits", "packed", "width", "reduced", "rectify_reduce", "float_scale"}
            if unknown or "colour" not in f:
                raise ValueError("frame %d: %s" % (k, "unknown keys %s" % sorted(unknown) if unknown else "no colour image"))
            crop = f.get("crop", (0, 0))
            col[k] = image_desc(f["colour"], False, f.get("order", "bgr"), f.get("layout", "hwc"), crop, matrix=f.get("matrix", "bt601"),
                                range=f.get("range", "limited"), bits=f.get("bits", 8), packed=f.get("packed", False), width=f.get("width"),
                                float_scale=f.get("float_scale"))
            if rgbd:
                if f.get("depth") is None:
                    raise ValueError("frame %d: an RGB-D detector needs a depth image" % k)
                dcrop = f.get("depth_crop")
                dep[k] = image_desc(f["depth"], True, crop=crop if dcrop is None else dcrop, scale=f.get("depth_scale", 1.0))
            sh = f.get("shift", (0, 0))
            opts[k].flip_x, opts[k].shift_x, opts[k].shift_y = (1 if f.get("flip_x", False) else 0), int(sh[0]), int(sh[1])
        if rectified or both:
            route = RECTIFY_DEPTH_REGISTERED if rect_registered or registered else RECTIFY_DEPTH_ALIGNED
            call = self.lib.lm_ingest_frames_rectified_reduced if both else self.lib.lm_ingest_frames_rectified
            self._check(call(self.h, int(first_slot), n, col, dep if rgbd else None, opts, route,
                                                            None if stream is None else C.c_void_p(int(stream))))
            return
        call = self.lib.lm_ingest_frames_reduced if reduced else self.lib.lm_ingest_frames_registered if registered else self.lib.lm_ingest_frames
        self._check(call(self.h, int(first_slot), n, col, dep if rgbd else None, opts, None if stream is None else C.c_void_p(int(stream))))

    def ingest_release(self, first_slot, n_slots, stream):
        """Makes `stream` (an integer HIP stream handle) wait for the pending uploads of the slots: work enqueued on it afterwards may
        overwrite the sources of their ingest."""
        self._check(self.lib.lm_ingest_release(self.h, int(first_slot), int(n_slots), None if stream is None else C.c_void_p(int(stream))))

    def read_frame(self, slot, depth=None):
        """(bgr [H, W, 3] uint8, depth [H, W] uint16 or None): the slot's resident frame as it lies in device memory.  depth: read the
        depth frame too (default: where the detector keeps one; a slot whose frame came without depth then raises)."""
        h, w = self.cfg.height, self.cfg.width
        bgr = np.zeros((h, w, 3), np.uint8)
        depth = np.zeros((h, w), np.uint16) if (self.keeps_depth if depth is None else depth) else None
        self._check(self.lib.lm_read_frame(self.h, int(slot), _ptr(bgr), _ptr(depth)))
        return bgr, depth

    def export_frame(self, slot, target, prims=None, undo=None, *, order="bgr", layout="hwc", window=(0, 0), matrix="bt601", range="limited",
                     float_scale=None):
        """The slot's colour frame, with `prims` drawn, into `target` in DEVICE memory (lm_export_frames): the one-frame case of
        export_frames.  undo: an IngestOpts, a dict(flip_x=, shift=) or None."""
        self.export_frames(slot, [dict(target=target, order=order, layout=layout, window=window, matrix=matrix, range=range, float_scale=float_scale)], prims,
                           None if undo is None else [undo])

    def export_frames(self, first_slot, targets, prims=None, undo=None):
        """The colour frames of slots first_slot + i, with the primitives of `prims` (a DRAW_PRIM_DTYPE array: draw_response, draw_axes,
        draw_box; `frame` = i) composited in list order, into targets[i] in DEVICE memory, all in ONE kernel launch (lm_export_frames;
        the rule: include/linemod_hip.h).  A target is a writable object with __cuda_array_interface__ (a torch or cupy tensor, a
        DeviceBuffer.view), or a dict(target=, order=, layout=, window=, matrix=, range=, float_scale=) of image_desc's keywords: layout "hwc" ([H, W, 3 | 4],
        alpha written as 255), "chw" ([3, H, W]) or "nv12" (one [H * 3 / 2, W] object or a pair (y, uv)), order "bgr" / "rgb", matrix and
        range for NV12, window = (x, y): the top-left of the frame's window inside the target's surface.  With float_scale a float32 / float16
        target ("hwc" or "chw": what a network behind the detector takes) receives every channel as (float)c * float_scale, rounded once to
        float16 where the target is one (1 / 255 for a 0 .. 1 tensor; alpha = 255 * float_scale).  undo: per frame an IngestOpts, a
        dict(flip_x=, shift=(sx, sy)) or None -- the ingest's mirror and shift, undone in the exported image (primitives stay in frame
        coordinates).  Synchronous."""
        n = len(targets)
        dst, opts = (ImageDesc * max(n, 1))(), (IngestOpts * max(n, 1))()
        for k, t in enumerate(targets):
            t = t if isinstance(t, dict) else dict(target=t)
            unknown = set(t) - {"target", "order", "layout", "window", "matrix", "range", "float_scale"}
            if unknown or "target" not in t:
                raise ValueError("target %d: %s" % (k, "unknown keys %s" % sorted(unknown) if unknown else "no target"))
            layout = t.get("layout", "hwc")
            if layout not in ("hwc", "chw", "nv12"):
                raise ValueError("target %d: layout %r (\"hwc\" / \"chw\" / \"nv12\" wanted)" % (k, layout))
            objs = t["target"] if isinstance(t["target"], (tuple, list)) else (t["target"],)
            for o in objs:
                cai = getattr(o, "__cuda_array_interface__", None)
                if isinstance(cai, dict) and cai["data"][1]:
                    raise ValueError("target %d is read-only" % k)
            dst[k] = image_desc(t["target"], False, t.get("order", "bgr"), layout, t.get("window", (0, 0)), matrix=t.get("matrix", "bt601"),
                                range=t.get("range", "limited"), float_scale=t.get("float_scale"))
        if undo is not None:
            if len(undo) != n:
                raise ValueError("undo: %d entries for %d targets" % (len(undo), n))
            for k, o in enumerate(undo):
                if o is None:
                    continue
                if isinstance(o, IngestOpts):
                    opts[k] = o
                    continue
                unknown = set(o) - {"flip_x", "shift"}
                if unknown:
                    raise ValueError("undo %d: unknown keys %s" % (k, sorted(unknown)))
                sh = o.get("shift", (0, 0))
                opts[k].flip_x, opts[k].shift_x, opts[k].shift_y = (1 if o.get("flip_x", False) else 0), int(sh[0]), int(sh[1])
        if prims is not None:
            prims = np.ascontiguousarray(prims)
            if prims.dtype != DRAW_PRIM_DTYPE or prims.ndim != 1:
                raise ValueError("prims: a one-dimensional DRAW_PRIM_DTYPE array wanted")
        npr = 0 if prims is None else len(prims)
        self._check(self.lib.lm_export_frames(self.h, int(first_slot), n, dst, None if undo is None else opts, _ptr(prims) if npr else None, npr))

    def set_stage_chunks(self, chunks):
        self._check(self.lib.lm_set_stage_chunks(self.h, chunks))

    def set_tuning(self, key, value):
        self._check(self.lib.lm_set_tuning(self.h, key, value))

    def match_slot(self, slot, threshold, class_idx=-1, cap=1 << 16, out=None):
        """out: a caller-owned MATCH_DTYPE array to fill (no allocation, the result is a view of it; overflow raises)."""
        if out is not None:
            _check_out(out)
            n = C.c_size_t()
            self._check(self.lib.lm_match_slot(self.h, slot, threshold, class_idx, _ptr(out), out.size, C.byref(n)))
            return out[:n.value]
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_size_t()
        rc = self.lib.lm_match_slot(self.h, slot, threshold, class_idx, _ptr(out), cap, C.byref(n))
        if rc == LM_ERR_OVERFLOW and n.value > cap:
            return self.match_slot(slot, threshold, class_idx, cap=n.value)
        self._check(rc)
        return out[:n.value].copy()

    def match_batch(self, n_slots, threshold, class_idx=-1, cap_per_frame=4096, out=None, counts=None):
        if out is None:
            out = np.zeros((n_slots, cap_per_frame), MATCH_DTYPE)
        if counts is None:
            counts = np.zeros(n_slots, np.int32)
        _check_out(out, 2)
        _check_counts(counts, n_slots)
        if out.shape[0] < n_slots or out.shape[1] != cap_per_frame:
            raise ValueError("out must be [n_slots, cap_per_frame]")
        self._check(self.lib.lm_match_batch(self.h, n_slots, threshold, class_idx, _ptr(out), cap_per_frame, _ptr(counts)))
        return out, counts

    def _class_list(self, classes):
        c = _c([] if classes is None else classes, np.int32).reshape(-1)
        return c, _ptr(c) if c.size else None

    def match_classes(self, bgr, depth, threshold, classes=None, cap=1 << 16):
        """Detector::match(sources, threshold, matches, class_ids) on a host frame with a class list."""
        bgr = _c(bgr, np.uint8)
        depth = None if depth is None else _c(depth, np.uint16)
        if bgr.shape != (self.cfg.height, self.cfg.width, 3):
            raise ValueError("frame size does not match the detector")
        c, cp = self._class_list(classes)
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_size_t()
        rc = self.lib.lm_match_classes(self.h, _ptr(bgr), 0, _ptr(depth), 0, threshold, cp, c.size, _ptr(out), cap, C.byref(n))
        if rc == LM_ERR_OVERFLOW and n.value > cap:
            return self.match_classes(bgr, depth, threshold, classes, cap=n.value)
        self._check(rc)
        return out[:n.value].copy()

    def match_batch_classes(self, first_slot, n_slots, threshold, classes=None, cap_per_frame=4096):
        """Detector::match with upstream's class list: one pre-processing per frame for all the named classes."""
        out = np.zeros((n_slots, cap_per_frame), MATCH_DTYPE)
        counts = np.zeros(n_slots, np.int32)
        c, cp = self._class_list(classes)
        self._check(self.lib.lm_match_batch_classes(self.h, first_slot, n_slots, threshold, cp, c.size, _ptr(out),
                                                    cap_per_frame, _ptr(counts)))
        return out, counts

    def match_prepared(self, first_slot, n_slots, threshold, classes=None, cap_per_frame=4096):
        """a11-a15 only on slots whose a3-a10 results are current (raises LinemodError otherwise)."""
        out = np.zeros((n_slots, cap_per_frame), MATCH_DTYPE)
        counts = np.zeros(n_slots, np.int32)
        c, cp = self._class_list(classes)
        self._check(self.lib.lm_match_prepared(self.h, first_slot, n_slots, threshold, cp, c.size, _ptr(out),
                                               cap_per_frame, _ptr(counts)))
        return out, counts

    def match_begin_classes(self, lane, first_slot, n_slots, threshold, classes=None):
        c, cp = self._class_list(classes)
        self._check(self.lib.lm_match_begin_classes(self.h, lane, first_slot, n_slots, threshold, cp, c.size))

    def pci_bus_id(self):
        buf = C.create_string_buffer(64)
        self._check(self.lib.lm_device_pci_bus_id(self.h, buf, 64))
        return buf.value.decode()

    def comm_info(self):
        r, w = C.c_int(), C.c_int()
        self._check(self.lib.lm_comm_info(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def get_exchange_profile(self):
        """(accumulated HIP-event microseconds of the gathered path's exchange, number of exchanges, lane-steps that needed
        the sized second exchange)."""
        us, n, fb = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self.lib.lm_get_exchange_profile(self.h, C.byref(us), C.byref(n), C.byref(fb)))
        return us.value, n.value, fb.value

    def get_stage_counts(self):
        """dict(preprocess_frames, scan_launches, refine_launches, sort_launches) since set_profiling()."""
        v = (C.c_int64 * 4)()
        self._check(self.lib.lm_get_stage_counts(self.h, v))
        return dict(zip(("preprocess_frames", "scan_launches", "refine_launches", "sort_launches"), list(v)))

    def synchronize(self):
        """hipDeviceSynchronize on the detector's device."""
        self._check(self.lib.lm_synchronize(self.h))

    def match_begin(self, lane, first_slot, n_slots, threshold, class_idx=-1):
        """Enqueue the match of the resident frames in slots [first_slot, first_slot + n_slots) on `lane` (0 or 1)."""
        self._check(self.lib.lm_match_begin(self.h, lane, first_slot, n_slots, threshold, class_idx))

    # ---- multi-GPU exchange (RCCL, include/linemod_hip.h "multi-GPU") ---------------------------
    def comm_init(self, rank, world, addr="127.0.0.1", port=29511, recs_per_frame_cap=0):
        self._check(self.lib.lm_comm_init(self.h, rank, world, addr.encode(), port, recs_per_frame_cap))

    def comm_destroy(self):
        self._check(self.lib.lm_comm_destroy(self.h))

    def comm_barrier(self):
        self._check(self.lib.lm_comm_barrier(self.h))

    def comm_max(self, values):
        v = (C.c_double * len(values))(*values)
        self._check(self.lib.lm_comm_max(self.h, v, len(values)))
        return list(v)

    def match_begin_gathered(self, lane, first_slot, n_slots, threshold, class_idx=-1):
        self._check(self.lib.lm_match_begin_gathered(self.h, lane, first_slot, n_slots, threshold, class_idx))

    def match_end_gathered(self, lane, out, counts):
        """-> (first owned frame, n owned frames, total records): merged lists of the frames this rank owns, back to
        back in `out`, lengths in counts[:n]."""
        _check_out(out)
        _check_counts(counts, 0)
        f0, nf, n = C.c_int(), C.c_int(), C.c_size_t()
        self._check(self.lib.lm_match_end_gathered(self.h, lane, _ptr(out), out.size, _ptr(counts), C.byref(f0),
                                                   C.byref(nf), C.byref(n)))
        return f0.value, nf.value, n.value

    def match_end(self, lane, cap_per_frame=4096, out=None, counts=None, n_slots=None):
        """Wait for `lane` and fetch its lists (same layout as match_batch)."""
        if out is None:
            out = np.zeros((n_slots, cap_per_frame), MATCH_DTYPE)
        if counts is None:
            counts = np.zeros(len(out), np.int32)
        _check_out(out, 2)
        _check_counts(counts, 0)
        if out.shape[1] != cap_per_frame:
            raise ValueError("out must be [n_slots, cap_per_frame]")
        self._check(self.lib.lm_match_end(self.h, lane, _ptr(out), cap_per_frame, _ptr(counts)))
        return out, counts

    # ---- stage hooks ---------------------------------------------------------------------------
    def stage_color_quantize(self, bgr, weak_threshold=10.0, want_magnitude=False):
        bgr = _c(bgr, np.uint8)
        h, w, _ = bgr.shape
        q = np.empty((h, w), np.uint8)
        mag = np.empty((h, w), np.float32) if want_magnitude else None
        self._check(self.lib.lm_stage_color_quantize(self.h, _ptr(bgr), w, h, weak_threshold, _ptr(q), _ptr(mag)))
        return (q, mag) if want_magnitude else q

    def stage_pyrdown(self, bgr):
        bgr = _c(bgr, np.uint8)
        h, w, _ = bgr.shape
        out = np.empty((h // 2, w // 2, 3), np.uint8)
        self._check(self.lib.lm_stage_pyrdown(self.h, _ptr(bgr), w, h, _ptr(out)))
        return out

    def stage_depth_quantize(self, depth):
        depth = _c(depth, np.uint16)
        h, w = depth.shape
        out = np.empty((h, w), np.uint8)
        self._check(self.lib.lm_stage_depth_quantize(self.h, _ptr(depth), w, h, _ptr(out)))
        return out

    def stage_linear_memories(self, quantized, T):
        q = _c(quantized, np.uint8)
        h, w = q.shape
        out = np.empty((8, T * T, (h // T) * (w // T)), np.uint8)
        self._check(self.lib.lm_stage_linear_memories(self.h, _ptr(q), w, h, T, _ptr(out)))
        return out

    def prepare_slot(self, slot):
        self._check(self.lib.lm_prepare_slot(self.h, slot))

    def debug_read(self, slot, what, level, modality):
        n = C.c_size_t()
        self._check(self.lib.lm_debug_read(self.h, slot, what, level, modality, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint8)
        self._check(self.lib.lm_debug_read(self.h, slot, what, level, modality, _ptr(out), out.size, C.byref(n)))
        return out

    def stage_scan(self, slot, threshold, class_idx=-1, cap=1 << 20):
        out = np.zeros((cap, 4), np.int32)
        n = C.c_size_t()
        self._check(self.lib.lm_stage_scan(self.h, slot, threshold, class_idx, _ptr(out), cap, C.byref(n)))
        if n.value > cap:
            return self.stage_scan(slot, threshold, class_idx, cap=n.value)
        return out[:n.value].copy()

    # ---- measurement ---------------------------------------------------------------------------
    def time_scan(self, slot, threshold, class_idx=-1, iters=50, variant=0):
        us, by = C.c_double(), C.c_double()
        self._check(self.lib.lm_time_scan(self.h, slot, threshold, class_idx, iters, variant, C.byref(us), C.byref(by)))
        return us.value, by.value

    def time_scan_batch(self, first_slot, n_slots, threshold, class_idx=-1, iters=20, variant=0):
        """Average microseconds of one scan launch over n_slots prepared slots (candidates counted, not stored)."""
        us = C.c_double()
        self._check(self.lib.lm_time_scan_batch(self.h, first_slot, n_slots, threshold, class_idx, iters, variant, C.byref(us)))
        return us.value

    def selftest_float_tail(self):
        """(reciprocals, square roots) of the depth-normal tail's float domain that differ from the correctly rounded forms.
        `self.last_bare_sqrt_mismatches` = floats on which the bare v_sqrt_f32 differs from the correctly rounded root."""
        out = (C.c_uint64 * 8)()
        self._check(self.lib.lm_selftest_float_tail(self.h, out))
        self.last_bare_sqrt_mismatches = int(out[2])
        self.last_candidate_mismatches = {"v_rcp + six steps (r03)": int(out[3]), "v_sqrt + fix-up": int(out[4]), "v_sqrt + v_rsq step": int(out[5]), "1 / root from the root's own v_rsq + one step": int(out[6])}
        return int(out[0]), int(out[1])

    def time_stages(self, slot, threshold, class_idx=-1, iters=20):
        out = (C.c_double * 4)()
        self._check(self.lib.lm_time_stages(self.h, slot, threshold, class_idx, iters, out))
        return list(out)

    def last_counts(self, slot=0):
        """(scan candidates, refined matches before sort+unique) of the last match on `slot`."""
        a, b = C.c_uint32(), C.c_uint32()
        self._check(self.lib.lm_last_counts(self.h, slot, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_profiling(self, enable=True):
        self._check(self.lib.lm_set_profiling(self.h, 1 if enable else 0))

    def get_profile(self):
        """dict(stage_us=[preprocess, scan, refine, sort], scan_bytes, launches, frames) accumulated by
        the match calls since set_profiling()."""
        st = (C.c_double * 4)()
        by, la, fr = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self.lib.lm_get_profile(self.h, st, C.byref(by), C.byref(la), C.byref(fr)))
        return dict(stage_us=list(st), scan_bytes=by.value, launches=la.value, frames=fr.value)

    def scan_load_bytes(self, class_idx=-1):
        """Bytes the scan's vector loads request per frame (L2 -> L1 traffic of the hot kernel)."""
        v = C.c_double()
        self._check(self.lib.lm_scan_load_bytes(self.h, class_idx, C.byref(v)))
        return v.value

    def color_check_counts(self, slot, lower_hsv, upper_hsv, matches):
        """(in_hull, in_both) int64 arrays: the two countNonZero of the reference's colorCheck for every match."""
        m = _c(matches, MATCH_DTYPE)
        a, b = np.zeros(len(m), np.int64), np.zeros(len(m), np.int64)
        lo, hi = (C.c_double * 3)(*lower_hsv), (C.c_double * 3)(*upper_hsv)
        self._check(self.lib.lm_color_check_counts(self.h, slot, lo, hi, _ptr(m), len(m), _ptr(a), _ptr(b)))
        return a, b

    def color_check_counts_slots(self, slot_of_match, lower_hsv, upper_hsv, matches):
        """The same for a list whose matches lie in several resident frames: ONE mask launch, one hull launch, one wait."""
        m = _c(matches, MATCH_DTYPE)
        sl = _c(slot_of_match, np.int32)
        if sl.size != len(m):
            raise ValueError("one slot per match")
        a, b = np.zeros(len(m), np.int64), np.zeros(len(m), np.int64)
        lo, hi = (C.c_double * 3)(*lower_hsv), (C.c_double * 3)(*upper_hsv)
        self._check(self.lib.lm_color_check_counts_slots(self.h, _ptr(sl), lo, hi, _ptr(m), len(m), _ptr(a), _ptr(b)))
        return a, b

    def depth_counts(self, queries):
        """r06: per query (DEPTH_QUERY_DTYPE: crop x0, y0, x1, y1 of the frame resident in `slot`, window lo..hi) the number of crop values below lo and
        inside [lo, hi], depths <= 1 counted as 65535 -- the depth check's early verdicts (lm_depth_counts_begin / _end)."""
        q = np.ascontiguousarray(queries, DEPTH_QUERY_DTYPE)
        below = np.zeros(len(q), np.uint32); inside = np.zeros(len(q), np.uint32)
        self._check(self.lib.lm_depth_counts_begin(self.h, _ptr(q) if len(q) else None, len(q)))
        self._check(self.lib.lm_depth_counts_end(self.h, _ptr(below) if len(q) else None, _ptr(inside) if len(q) else None))
        return below, inside

    def depth_select_begin(self, queries):
        """Enqueues the selection of a query list (DEPTH_SELECT_QUERY_DTYPE) on the colour-check stream and returns: lm_depth_select_begin."""
        q = np.ascontiguousarray(queries, DEPTH_SELECT_QUERY_DTYPE)
        self._check(self.lib.lm_depth_select_begin(self.h, _ptr(q) if len(q) else None, len(q)))
        self._depth_select_n = len(q)

    def depth_select_end(self):
        """Waits for the list begun and returns its values (uint16, the queries' order): lm_depth_select_end."""
        n = getattr(self, "_depth_select_n", 0)
        self._depth_select_n = 0
        value = np.zeros(n, np.uint16)
        self._check(self.lib.lm_depth_select_end(self.h, _ptr(value) if n else None))
        return value

    def depth_select(self, queries):
        """The depth check's sorted order statistic: per query (crop x0, y0, x1, y1 of the frame resident in `slot`, 0-based `rank`) the element at
        index rank of the ascending sort of the crop's depths, depths <= 1 taken as 65535; an empty crop gives 65535."""
        self.depth_select_begin(queries)
        return self.depth_select_end()

    def time_depth_select(self, queries, what=0):
        """Milliseconds of ONE kernel launch for the queries between two HIP events on the colour-check stream (lm_time_depth_select): what = 0
        k_depth_select, 1 the same with the naive shared histogram, 2 k_depth_counts for the same crops."""
        q = np.ascontiguousarray(queries, DEPTH_SELECT_QUERY_DTYPE)
        ms = C.c_float(0)
        self._check(self.lib.lm_time_depth_select(self.h, _ptr(q) if len(q) else None, len(q), what, C.byref(ms)))
        return ms.value

    def color_mask_prepare(self, lane, first_slot, n_slots, lower_hsv, upper_hsv):
        """The slots' colour masks for one HSV range on `lane`'s stream, ahead of the match begun on that lane next."""
        lo, hi = (C.c_double * 3)(*lower_hsv), (C.c_double * 3)(*upper_hsv)
        self._check(self.lib.lm_color_mask_prepare(self.h, lane, first_slot, n_slots, lo, hi))

    def upload_frame_pinned_shifted(self, slot, bgr, depth, shift_x, shift_y):
        """upload_frame_shifted from pinned memory: the DMA engine's row-offset copy, no staging pass."""
        if bgr.dtype != np.uint8 or not bgr.flags.c_contiguous or bgr.shape != (self.cfg.height, self.cfg.width, 3):
            raise ValueError("pinned colour frame must be a C-contiguous uint8 [h, w, 3] array of the detector's size")
        if depth is not None and (depth.dtype != np.uint16 or not depth.flags.c_contiguous):
            raise ValueError("pinned depth frame must be a C-contiguous uint16 array")
        self._check(self.lib.lm_upload_frame_pinned_shifted(self.h, slot, _ptr(bgr), 0, _ptr(depth), 0, int(shift_x), int(shift_y)))

    def stage_reserve(self, first_slot, n_slots):
        self._check(self.lib.lm_stage_reserve(self.h, first_slot, n_slots))

    def stage_rows(self, slot, bgr, depth, shift_x, shift_y, row0, row1):
        """Rows [row0, row1) of both images into the slot's pinned staging buffers (host memory only; any thread)."""
        bgr = _c(bgr, np.uint8)
        depth = None if depth is None else _c(depth, np.uint16)
        self._check(self.lib.lm_stage_rows(self.h, slot, _ptr(bgr), 0, _ptr(depth), 0, int(shift_x), int(shift_y), int(row0), int(row1)))

    def upload_staged(self, slot):
        self._check(self.lib.lm_upload_staged(self.h, slot))

    def match_collect(self, first_slot, n_slots, cap_per_frame=4096):
        """The lists of the last completed match on the slots once more (after LM_ERR_OVERFLOW: with the capacity counts[] named)."""
        out = np.zeros((n_slots, cap_per_frame), MATCH_DTYPE)
        counts = np.zeros(n_slots, np.int32)
        rc = self.lib.lm_match_collect(self.h, first_slot, n_slots, _ptr(out), cap_per_frame, _ptr(counts))
        if rc == LM_ERR_OVERFLOW:
            return None, counts
        self._check(rc)
        return out, counts

    def set_scan_stats(self, enable=True):
        self._check(self.lib.lm_set_scan_stats(self.h, 1 if enable else 0))

    def get_scan_stats(self):
        """(feature loads made, feature loads of an exhaustive scan) since set_scan_stats()."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.lib.lm_get_scan_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def get_scan_lane_stats(self):
        """(16-byte lane-loads issued, lane-loads of an exhaustive scan) since set_scan_stats()."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.lib.lm_get_scan_lane_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def get_scan_form_stats(self):
        """(scan launches that took the bit-plane kernel, all scan launches, survivors of its miss bound since set_scan_stats(),
        lanes per frame of the last scan launch -- 0: the nibble kernel)."""
        v = (C.c_int64 * 4)()
        self._check(self.lib.lm_get_scan_form_stats(self.h, v))
        return tuple(int(x) for x in v)

    def set_scan_variant(self, variant):
        self._check(self.lib.lm_set_scan_variant(self.h, variant))
