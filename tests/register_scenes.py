"""The scenes of the registration tests (tests/test_register_cpu.py, tests/test_gpu_register.py): cameras, extrinsics and raw depth images,
built once and left unchanged."""
import numpy as np

import register_reference as RR

W, H = 160, 80                      # the detector
CW, CH = 208, 120                   # the colour camera's geometry
CROP = (24, 20)                     # where scene A's window lies in it
DIST = (0.08, -0.02, 0.001, -0.002, 0.003)
ZERO = (0.0,) * 5
ANGLE = np.deg2rad(3.0)
ROT = np.array([[np.cos(ANGLE), 0.0, np.sin(ANGLE)], [0.0, 1.0, 0.0], [-np.sin(ANGLE), 0.0, np.cos(ANGLE)]], np.float32)     # 3 degrees about y
TRANS = np.array([52.0, -4.0, 3.0], np.float32)
SPECIAL = np.array([0.0, np.nan, np.inf, -5.0, 1e9, -np.inf], np.float32)


def colour_cam(dist=ZERO):
    return RR.cam(CW, CH, 130.0, 130.0, 103.5, 59.5, dist)


def depth_cam_a(dist=ZERO):
    return RR.cam(96, 64, 60.0, 60.0, 47.5, 31.5, dist)


def depth_cam_b():
    return RR.cam(400, 200, 250.0, 250.0, 199.5, 99.5)


def scene_a(seed=7, far=0.0):
    """96 x 64 float32 millimetres: a background near 1000 (+ far) with +-3 mm noise, a 36 x 24 block near 500 (+ far) in the middle, and
    the first two rows strewn with 0, NaN, +inf, -5, 1e9 and -inf."""
    rng = np.random.default_rng(seed)
    d = (1000.0 + far + rng.uniform(-3.0, 3.0, (64, 96))).astype(np.float32)
    d[20:44, 30:66] = (500.0 + far + rng.uniform(-3.0, 3.0, (24, 36))).astype(np.float32)
    d[0, :] = SPECIAL[np.arange(96) % len(SPECIAL)]
    d[1, ::3] = SPECIAL[(np.arange(32) + 2) % len(SPECIAL)]
    d.setflags(write=False)
    return d


def scene_b(seed=11):
    """400 x 200 uint16 millimetres, four raw pixels per colour pixel: a noisy background, a nearer block, some zeros."""
    rng = np.random.default_rng(seed)
    d = rng.integers(960, 1040, (200, 400)).astype(np.uint16)
    d[60:140, 150:260] = rng.integers(480, 520, (80, 110)).astype(np.uint16)
    d[rng.random((200, 400)) < 0.01] = 0
    d.setflags(write=False)
    return d


def window(Rg, crop=CROP):
    return Rg[crop[1]:crop[1] + H, crop[0]:crop[0] + W]
