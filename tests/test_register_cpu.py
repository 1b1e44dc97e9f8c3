"""CPU tests of the depth registration (ABI 0.13): csrc/lm_register.h -- the per-pixel rule k_register_scatter calls --
as a stand-alone host program (tests/cpp/register_host.cpp, g++ -ffp-contract=off, plain and under ASan / UBSan) against the independent
numpy reference tests/register_reference.py over the scenes of the GPU tests and a value sweep; the ray table; lm_set_registration's
refusals, which need no device; the version string and the refusal to run without a device."""
import os
import subprocess

import numpy as np
import pytest

import register_reference as RR
import register_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "line-mod-pipeline_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
F = np.float32


@pytest.fixture(scope="module", params=[["-O2"], ["-O1", "-g"] + SAN], ids=["plain", "asan_ubsan"])
def host_program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("register_host") / "register_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + request.param +
                          ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "register_host.cpp")])
    return exe


def run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return int(r.stdout.split()[1])


def host_project(exe, tmp_path, colour, R, tr, rx, ry, t):
    head = np.concatenate([np.asarray(R, F).reshape(9), np.asarray(tr, F).reshape(3),
                           np.array([colour["fx"], colour["fy"], colour["cx"], colour["cy"]] + list(colour["dist"]), F)])
    rec = np.stack([np.asarray(a, F).reshape(-1) for a in (rx, ry, t)], axis=1)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(head.tobytes() + rec.tobytes())
    assert run(exe, ["project", fin, fout]) == len(rec)
    out = np.fromfile(fout, np.dtype([("dropped", np.int32), ("u", F), ("v", F), ("m", np.uint32)]))
    assert len(out) == len(rec)
    return out


def assert_same(out, ref, what):
    dropped, u, v, m = (np.asarray(a).reshape(-1) for a in ref)
    assert np.array_equal(out["dropped"] != 0, dropped), "%s: dropped differs at %d records" % (what, int(((out["dropped"] != 0) != dropped).sum()))
    k = ~dropped
    assert np.array_equal(out["u"][k], u[k]) and np.array_equal(out["v"][k], v[k]), "%s: (u, v) differs" % what
    assert np.array_equal(out["m"][k], m[k]), "%s: m differs" % what
    return int(k.sum())


def host_rays(exe, tmp_path, c):
    fout = str(tmp_path / "rays.bin")
    # the library holds the camera as floats: the program gets the doubles those floats are
    args = [repr(float(F(v))) for v in (c["fx"], c["fy"], c["cx"], c["cy"]) + tuple(c["dist"])]
    assert run(exe, ["rays", fout, c["width"], c["height"]] + args) == 2 * c["width"] * c["height"]
    return np.fromfile(fout, F).reshape(c["height"], c["width"], 2)


@pytest.mark.parametrize("dist", [S.ZERO, S.DIST], ids=["pinhole", "brown"])
def test_host_program_equals_reference_on_the_scenes(host_program, tmp_path, dist):
    """(dropped, u, v, m) of every pixel of scene A (both distances) and scene B, through the ray table the program itself builds."""
    cc = S.colour_cam(dist)
    rays = host_rays(host_program, tmp_path, S.depth_cam_a(dist))
    kept = 0
    for far in (0.0, 700.0):
        t = RR.to_t(S.scene_a(far=far), 1.0)
        out = host_project(host_program, tmp_path, cc, S.ROT, S.TRANS, rays[:, :, 0], rays[:, :, 1], t)
        kept += assert_same(out, RR.hits(t, rays[:, :, 0], rays[:, :, 1], cc, S.ROT, S.TRANS), "scene A + %g" % far)
    rays_b = host_rays(host_program, tmp_path, S.depth_cam_b())
    assert np.array_equal(rays_b, RR.pinhole_rays(S.depth_cam_b()))
    t = RR.to_t(S.scene_b())
    out = host_project(host_program, tmp_path, cc, S.ROT, S.TRANS, rays_b[:, :, 0], rays_b[:, :, 1], t)
    kept += assert_same(out, RR.hits(t, rays_b[:, :, 0], rays_b[:, :, 1], cc, S.ROT, S.TRANS), "scene B")
    assert kept > 2 * 5000 + 70000


def test_host_program_equals_reference_on_the_value_sweep(host_program, tmp_path):
    """t in {0, NaN, +-inf, negative, 1e9, ...} x rays x rigs: the identity, scene A's, a rotation of 180 degrees about y (every point
    behind the colour camera), translations that bring Z' to 0.4, 0.5, 0.6, 1.5 and beyond 65535, and focal lengths that throw the
    projection far outside the int range (and to infinity)."""
    ts = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -5.0, 1e9, 1e-30, 0.4, 0.5, 0.6, 1.0, 1.5, 2.5, 499.5, 500.5, 65534.4, 65534.5, 65535.0, 65536.0, 1e5,
                   3e38], F)
    r = np.array([-3.0, -0.8, -0.01, 0.0, 1e-20, 0.013, 0.5, 0.77, 40.0], F)
    rx, ry, t = (a.reshape(-1) for a in np.meshgrid(r, r, ts, indexing="ij"))
    eye = np.eye(3, dtype=F)
    back = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], F)
    huge = RR.cam(S.CW, S.CH, 3e30, 1e38, 103.5, 59.5, S.DIST)
    rigs = [(S.colour_cam(), eye, np.zeros(3, F)), (S.colour_cam(S.DIST), S.ROT, S.TRANS), (S.colour_cam(S.DIST), back, np.array([52, -4, 0], F)),
            (S.colour_cam(), back, np.array([0, 0, 1000.25], F)), (S.colour_cam(), eye, np.array([7, -7, -0.5], F)),
            (S.colour_cam(), eye, np.array([0, 0, -499.0], F)), (S.colour_cam(), eye, np.array([1e6, -1e6, 65000.0], F)),
            (huge, eye, np.zeros(3, F)), (huge, S.ROT, np.array([3e38, -3e38, 0], F))]
    seen = set()
    for k, (cc, R, tr) in enumerate(rigs):
        ref = RR.hits(t, rx, ry, cc, R, tr)
        out = host_project(host_program, tmp_path, cc, R, tr, rx, ry, t)
        kept = assert_same(out, ref, "rig %d" % k)
        dropped, u, v, m = ref
        if kept:
            seen |= {"kept"}
            seen |= {"m=1"} if (m[~dropped] == 1).any() else set()
            seen |= {"m=65535"} if (m[~dropped] == 65535).any() else set()
            seen |= {"beyond int"} if (np.abs(u[~dropped]) > F(2.0 ** 40)).any() else set()
        if k == 2:
            assert dropped.all(), "a point behind the colour camera was kept"
        with np.errstate(all="ignore"):
            # Z' that rounds to 0 (identity rotation: Z' = t + tz exactly for these values)
            if k in (4, 5):
                z = t + tr[2]
                assert ((z > 0) & (z <= F(0.5)) & dropped).any()
    assert seen == {"kept", "m=1", "m=65535", "beyond int"}


def test_ray_table(lm):
    """Through the library (lm_set_registration builds the table on the host: no device): zero coefficients give the rounded quotient
    exactly; with scene A's coefficients the ray, pushed forward through the Brown model in double, returns to the pixel centre within
    1e-3 pixel; a caller's table is returned as it was handed over."""
    d = lm.Detector(color_only=False, width=S.W, height=S.H)
    kc = lm.camera(S.CW, S.CH, 130.0, 130.0, 103.5, 59.5)
    for c in (S.depth_cam_a(), S.depth_cam_b(), RR.cam(33, 17, 61.7, 59.3, 15.25, 8.125)):
        d.set_registration(lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"]), kc, S.ROT, S.TRANS)
        assert np.array_equal(d.registration_rays(), RR.pinhole_rays(c))
    c = S.depth_cam_a(S.DIST)
    d.set_registration(lm.camera(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], S.DIST), kc, S.ROT, S.TRANS, splat=(2, 1))
    rays = d.registration_rays()
    assert rays.shape == (64, 96, 2) and rays.dtype == F
    xd, yd = RR.brown_forward(rays[:, :, 0], rays[:, :, 1], [float(F(v)) for v in S.DIST])
    i, j = np.meshgrid(np.arange(96.0), np.arange(64.0))
    err = np.maximum(np.abs(xd * c["fx"] + c["cx"] - i), np.abs(yd * c["fy"] + c["cy"] - j)).max()
    print("largest distance of a ray's forward projection from its pixel centre: %.3g pixel" % err)
    assert err <= 1e-3
    assert np.abs(rays - RR.pinhole_rays(c)).max() > 1e-3          # (the coefficients did something)
    own = np.random.default_rng(5).uniform(-1, 1, (64, 96, 2)).astype(F)
    d.set_registration(lm.camera(96, 64, 60.0, 60.0, 47.5, 31.5), kc, S.ROT, S.TRANS, rays=own)
    assert np.array_equal(d.registration_rays(), own)
    d.set_registration(None, None, None, None)
    with pytest.raises(lm.LinemodError) as e:
        d.registration_rays()
    assert e.value.code == lm.LM_ERR_INVALID and "no registration set: lm_set_registration first" in str(e.value)
    d.close()


def test_setter_refusals(lm):
    d = lm.Detector(color_only=False, width=S.W, height=S.H)
    good = dict(width=96, height=64, fx=60.0, fy=60.0, cx=47.5, cy=31.5)
    kc = lm.camera(S.CW, S.CH, 130.0, 130.0, 103.5, 59.5)

    def refused(words, depth=None, colour=None, R=S.ROT, t=S.TRANS, **kw):
        with pytest.raises(lm.LinemodError) as e:
            d.set_registration(lm.camera(**dict(good, **(depth or {}))), lm.camera(**dict(good, **(colour or {}))), R, t, **kw)
        assert e.value.code == lm.LM_ERR_INVALID and words in str(e.value), str(e.value)

    d.set_registration(lm.camera(**good), kc, S.ROT, S.TRANS, splat=(3, 3))
    before = d.registration_rays()
    finite = "registration: every number must be finite"
    for bad in (np.nan, np.inf, -np.inf):
        for key in ("fx", "fy", "cx", "cy"):
            refused(finite, depth={key: bad})
            refused(finite, colour={key: bad})
        for k in range(5):
            dist = [0.0] * 5
            dist[k] = bad
            refused(finite, depth={"dist": dist})
            refused(finite, colour={"dist": dist})
        R = S.ROT.copy()
        R[1, 2] = bad
        refused(finite, R=R)
        refused(finite, t=[0.0, bad, 0.0])
    for key in ("fx", "fy"):
        for bad in (0.0, -60.0):
            refused("registration: fx and fy of both cameras must be positive", depth={key: bad})
            refused("registration: fx and fy of both cameras must be positive", colour={key: bad})
    for key in ("width", "height"):
        for bad in (0, -1, 16385):
            refused("registration: width and height of both cameras must lie in 1 .. 16384", colour={key: bad})
        refused("registration: width and height of both cameras must lie in 1 .. 16384", depth={key: 0})
    for splat in ((-1, 0), (0, -1), (4, 0), (0, 4)):
        refused("registration: splat_x and splat_y must lie in 0 .. 3", splat=splat)
    rays = np.zeros((64, 96, 2), F)
    rays[63, 95, 1] = np.nan
    refused("registration: every ray must be finite", rays=rays)
    with pytest.raises(ValueError):
        d.set_registration(lm.camera(**good), kc, S.ROT, S.TRANS, rays=np.zeros((64, 95, 2), F))
    with pytest.raises(ValueError):
        d.set_registration(lm.camera(**good), kc, np.eye(4), S.TRANS)
    # a refusal leaves the registration as it was
    assert np.array_equal(d.registration_rays(), before)
    d.close()


def test_version_and_constants(lm):
    v = lm.load_library().lm_version()
    assert v.startswith(b"linemod_hip 0.13 ") and b"0.13 = the 0.12 ABI plus the depth registration" in v
    for earlier in (b"0.12 = the 0.11 ABI", b"0.10", b"gfx950", b"lm_ingest_frames_registered"):
        assert earlier in v
    import ctypes as C
    assert C.sizeof(lm.Camera) == 44 and C.sizeof(lm.RegistrationDesc) == 2 * 44 + 36 + 12 + 8 + 8


def _has_gpu(lm):
    d = lm.Detector(color_only=True, width=64, height=64, T=[2, 8])
    try:
        d.stage_pyrdown(np.zeros((8, 8, 3), np.uint8))
        return True
    except lm.LinemodError:
        return False
    finally:
        d.close()


class Fake:
    def __init__(self, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (0x7F0012345600, False), "strides": None, "version": 2}


def test_registered_ingest_fails_loudly_without_gpu(lm):
    if _has_gpu(lm):
        pytest.skip("a HIP device is present")
    d = lm.Detector(color_only=False, width=S.W, height=S.H)
    d.set_registration(lm.camera(96, 64, 60.0, 60.0, 47.5, 31.5), lm.camera(S.CW, S.CH, 130.0, 130.0, 103.5, 59.5), S.ROT, S.TRANS)
    with pytest.raises(lm.LinemodError) as e:
        d.ingest_frame(0, Fake((S.CH, S.CW, 3), "|u1"), Fake((64, 96), "<f4"), crop=S.CROP, register_depth=True)
    assert e.value.code == lm.LM_ERR_NO_DEVICE and "no CPU fallback" in str(e.value)
    with pytest.raises(ValueError):
        d.ingest_frames(0, [dict(colour=Fake((S.CH, S.CW, 3), "|u1"), depth=Fake((64, 96), "<f4"), register_depth=True),
                            dict(colour=Fake((S.CH, S.CW, 3), "|u1"), depth=Fake((S.CH, S.CW), "<u2"))])
    d.close()
