"""Every HIP resource the library creates is released: lm_debug_live_resources (device buffers, pinned buffers, streams, events live in the
process, counted by the owners of csrc/lm_own.h) before a detector exists, after every subsystem that allocates lazily has run once, and
after close() -- twice in one process, so that state only a first call initialises shows too.  128 x 96 RGB-D, T = [2, 8], two pyramid
levels, 4 frame slots (two lanes with two slots each).  No timing and no free-memory comparison: other tenants of the device would
make either flaky.

The ICP runs through its model, scene cloud, refinement (host frame and slot) and best-pose check, the generator through a rendered
template, the evaluation through ADD and VSD -- all on a square pyramid of five vertices, so no entry point is left out."""
import numpy as np
import pytest

import pose_error_reference as R

pytestmark = pytest.mark.gpu

W, H, T, SLOTS, THR = 128, 96, [2, 8], 4, 80.0
K = (200.0, 200.0, W / 2, H / 2)
HSV_LO, HSV_HI = [0, 40, 40], [100, 255, 255]


def _pyramid():
    """A square pyramid, 60 mm wide, apex towards the camera, and its view-projection 400 mm in front of a 128 x 96 camera."""
    v = np.array([[-30, -30, 0], [30, -30, 0], [30, 30, 0], [-30, 30, 0], [0, 0, 40]], np.float32)
    f = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]], np.uint32)
    V = np.eye(4, dtype=np.float32)
    V[2, 3] = -400
    return v, f, R.view_proj_mat4(R.projection(fy=K[1], w=W, h=H), V)


def _work(lm, synth):
    """Creates a detector, drives everything that allocates on first use once, returns (detector, the test's own blocks, the counts)."""
    d = lm.Detector(lm.default_config(color_only=False, width=W, height=H, T=T, frame_slots=SLOTS, num_features=24, depth_num_features=24))
    frames = [synth.make_frame(W, H, seed=5100 + k, n_shapes=12) for k in range(2)]
    bgr, depth = frames[0]
    # a template from an image (slot 0's quantisers, the bank), a staged upload of every slot, a pinned upload
    tid, _ = d.add_template("image", bgr, depth)
    assert tid >= 0
    for k in range(SLOTS):
        d.upload_frame(k, *frames[k % 2])
    pin = lm.PinnedBuffer(W * H * 5)
    pb, pd = pin.view(np.uint8, (H, W, 3)), pin.view(np.uint16, (H, W), offset=W * H * 3)
    pb[:], pd[:] = bgr, depth
    d.upload_frame_pinned(1, pb, pd)
    d.upload_wait(-1)
    # a match mask and a mask rule, then the batch: nibble scan first ...
    m = np.zeros((H, W), np.uint8)
    m[8:80, 8:120] = 255
    d.upload_match_mask(0, m)
    d.set_mask_rule(2, 2, modalities=3, depth_range=(400, 1500), hsv_range=(HSV_LO, HSV_HI), grow=2)
    d.match_batch(SLOTS, THR)
    # ... then lanes 0 and 1 with the bit-plane scan, so that each lane's survivor queue exists; the queue's size changed: freed, re-made
    d.set_tuning(lm.TUNE_SCAN_FORM, 2)
    for size in (1 << 16, 1 << 12):
        d.set_tuning(lm.TUNE_SURVIVOR_QUEUE, size)
        for lane in (0, 1):
            d.match_begin(lane, 2 * lane, 2, THR)
        for lane in (0, 1):
            d.match_end(lane, n_slots=2)
    assert d.get_scan_form_stats()[0] > 0, "no bit-plane scan ran: the survivor queue was never needed"
    d.set_tuning(lm.TUNE_SCAN_FORM, 0)
    # colour check (its stream, the hulls, the HSV tables), the prepared masks on a lane, depth counts
    mt = np.zeros(3, lm.MATCH_DTYPE)
    mt["x"], mt["y"] = [10, 20, 30], [10, 12, 14]
    d.color_check_counts(0, HSV_LO, HSV_HI, mt)
    d.color_mask_prepare(1, 2, 2, HSV_LO, HSV_HI)
    d.color_check_counts_slots(np.array([2, 3, 2], np.int32), HSV_LO, HSV_HI, mt)
    q = np.zeros(2, lm.DEPTH_QUERY_DTYPE)
    q["x1"], q["y1"], q["lo"], q["hi"], q["slot"] = 40, 30, 500, 1000, [0, 3]
    d.depth_counts(q)
    # an ingest from lm_device_alloc memory
    dev = lm.DeviceBuffer(W * H * 5)
    dev.upload(bgr)
    dev.upload(depth, offset=W * H * 3)
    d.ingest_frame(3, dev.view(np.uint8, (H, W, 3)), dev.view(np.uint16, (H, W), offset=W * H * 3))
    d.upload_wait(3)
    # stage hooks on the detector's scratch, the self-test's temporary
    d.stage_color_quantize(bgr)
    d.stage_depth_quantize(depth)
    d.selftest_float_tail()
    # a second class: the device bank and the hull tables are rebuilt
    descs, feats, _ = synth.make_bank(6, 2, 2, seed=5200, frame_size=(W, H), T0=T[0], num_features=24, size_range=(16, 32))
    d.add_class("listed", descs, feats)
    d.match_batch(SLOTS, THR)
    d.color_check_counts(0, HSV_LO, HSV_HI, mt)
    # generator, evaluation and ICP on the pyramid
    v, f, vp = _pyramid()
    d.set_render_mesh(0, v, f)
    d.add_templates_rendered("rendered", 0, vp[None], [0.0])
    _, rd = d.render(0, vp, W, H)
    assert (rd > 0).sum() > 100
    d.pose_error_add(0, np.eye(3), [0, 0, 400], np.eye(3), [1, 0, 400])
    d.pose_error_vsd(rd, 0, 0, vp[None], vp[None])
    bbox = (34, 18, 60, 60)
    cloud = d.icp_scene_cloud(rd, bbox, K, step=1)
    assert len(cloud) > 50
    d.icp_set_model(0, cloud, step=1)
    d.icp_refine(rd, bbox, 0, np.eye(4), K, step=1)
    d.upload_frame(0, bgr, rd)
    d.icp_refine(0, bbox, 0, np.eye(4), K, step=1)
    d.icp_verify(rd, 0, 0, vp[None])
    d.match_batch(SLOTS, THR)        # (the rendered class: the bank once more)
    steady = lm.live_resources()
    d.match_batch(SLOTS, THR)
    assert lm.live_resources() == steady, "a match in the steady state created or released a resource"
    return d, (pin, dev), steady


def test_every_resource_is_released(lm, synth):
    start = lm.live_resources()
    for cycle in range(2):
        d, blocks, live = _work(lm, synth)
        assert all(a > b for a, b in zip(live, start)), (cycle, live, start)
        d.close()
        for b in blocks:
            b.close()
        assert lm.live_resources() == start, (cycle, lm.live_resources(), start)
