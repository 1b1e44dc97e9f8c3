"""Which call the library refuses, with which words: every entry point that writes a slot's frame, staging, masks or rule (and
lm_match_collect, which reads its lists) against a slot that a lane's match in flight holds, that lies inside the range of a colour
check or of depth counts begun and not ended, and against calls that are wrong in two ways at once -- the FIRST check of the entry
point decides the message.  The same calls succeed on a slot outside the held range and on the held slots once the match / the check
has ended.  Every refusal happens on the host before any HIP call of the refused entry point.

Slots (one 320 x 240 RGB-D detector, 4 slots, the same frame in each): the lane holds slot 1, the checks name slots 0 and 2 (their
range [0, 2] covers slot 1 too), slot 3 stays free."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, THR = 320, 240, 75.0
LANE_SLOT, CHECK_SLOTS, FREE_SLOT = 1, (0, 2), 3
INVALID = 1     # LM_ERR_INVALID

NO_COLOUR = "sources.size() != modalities.size(): colour image missing"
SHORT_ROW = "stride smaller than a row"
BUSY = "slot belongs to a match in flight"
COLOUR_CHECK = "slot is read by a colour check in flight: call lm_color_check_end first"
DEPTH_COUNTS = "slot is read by depth counts in flight: call lm_depth_counts_end first"


class Rig:
    def __init__(self, lm, orc, synth):
        self.lm = lm
        self.d = d = lm.Detector(color_only=False, width=W, height=H, frame_slots=4)
        self.lib, self.h = d.lib, d.h
        self.bgr, self.depth = synth.make_frame(W, H, seed=500)
        o = orc.Detector(color_only=False)
        o.prepare(self.bgr, self.depth)
        q = {(l, m): o.stage(0, l, m).reshape(H >> l, W >> l) for l in range(2) for m in range(2)}
        descs, feats, _ = synth.make_bank(40, 2, 2, seed=99, size_range=(48, 120), quantized=q, crop_fraction=0.3, frame_size=(W, H),
                                          T0=d.get_T(0))
        d.add_class("c", descs, feats)
        self.fb = W * H * 5
        self.pb = lm.PinnedBuffer(self.fb)
        self.pbgr = self.pb.view(np.uint8, (H, W, 3))
        self.pdepth = self.pb.view(np.uint16, (H, W), offset=W * H * 3)
        self.pbgr[...] = self.bgr
        self.pdepth[...] = self.depth
        self.mask = np.full((H, W), 255, np.uint8)
        self.rule = lm.make_mask_rule(1, depth_range=(400, 1500))
        self.bad_rule = lm.make_mask_rule(1, depth_range=(400, 1500))
        self.bad_rule.grow = 99
        self.matches = None
        self.entry_points = self._entry_points()

    def close(self):
        self.pb.close([self.d])
        self.d.close()

    def _entry_points(self):
        """name -> (call(first, n, null, short) -> rc, the defects it can be given, its words for them).  In ORDER: the successes run
        in this order, so that what needs the slot's earlier state (its lists, its open staging) comes before the uploads."""
        lib, h = self.lib, self.h
        vp = lambda a: a.ctypes.data_as(C.c_void_p)

        def frame_call(fn, src_bgr, src_depth, *shift):
            def call(first, n, null, short):
                return fn(h, first, None if null else vp(src_bgr), W * 3 - 1 if short else 0, vp(src_depth), 0, *shift)
            return call

        def collect(first, n, null, short):
            out, counts = np.zeros((n, 4096), self.lm.MATCH_DTYPE), np.zeros(n, np.int32)
            return lib.lm_match_collect(h, first, n, vp(out), 4096, vp(counts))

        frame_words = {"null": NO_COLOUR, "short": SHORT_ROW}
        return [
            ("match_collect", collect, (), {}),
            ("upload_staged", lambda first, n, null, short: lib.lm_upload_staged(h, first), (), {}),
            ("stage_reserve", lambda first, n, null, short: lib.lm_stage_reserve(h, first, n), (), {}),
            ("upload_frame", frame_call(lib.lm_upload_frame, self.bgr, self.depth), ("null", "short"), frame_words),
            ("upload_frame_shifted", frame_call(lib.lm_upload_frame_shifted, self.bgr, self.depth, 5, -3), ("null", "short"), frame_words),
            ("upload_frame_pinned", frame_call(lib.lm_upload_frame_pinned, self.pbgr, self.pdepth), ("null", "short"), frame_words),
            ("upload_frame_pinned_shifted", frame_call(lib.lm_upload_frame_pinned_shifted, self.pbgr, self.pdepth, 5, -3), ("null", "short"), frame_words),
            ("upload_frames_pinned", lambda first, n, null, short: lib.lm_upload_frames_pinned(h, first, n, None if null else vp(self.pbgr), self.fb - 1 if short else 0),
             ("null", "short"), {"null": "bad argument", "short": "frame stride smaller than a frame"}),
            ("upload_match_mask", lambda first, n, null, short: lib.lm_upload_match_mask(h, first, -1, vp(self.mask), W - 1 if short else 0),
             ("short",), {"short": "mask stride smaller than a row"}),
            ("set_mask_rule", lambda first, n, null, short: lib.lm_set_mask_rule(h, first, n, C.byref(self.rule)), (), {}),
        ]

    def reset(self):
        """Every slot holds the frame, a completed match (lm_match_collect has lists to hand out) and open, filled staging buffers
        (lm_upload_staged gets as far as its claim); no masks, no rules."""
        d = self.d
        d.upload_wait(-1)        # (the pinned source is shared: its last upload has landed)
        d.clear_mask_rule()
        for s in range(4):
            d.upload_frame(s, self.bgr, self.depth)
        out, cnt = d.match_batch(4, THR, 0)
        assert cnt.min() > 0
        self.matches = [out[s, :cnt[s]].copy() for s in range(4)]
        d.stage_reserve(0, 4)
        for s in range(4):
            d.stage_rows(s, self.bgr, self.depth, 0, 0, 0, H)

    def status(self, rc):
        return rc, (self.lib.lm_last_error().decode() if rc else "")

    def refused(self, name, call, first, n, words, null=False, short=False):
        got = self.status(call(first, n, null, short))
        assert got == (INVALID, words), "%s(first %d, n %d, null %s, short %s): %r, expected %r" % (name, first, n, null, short, got, words)

    def succeeds(self, first):
        for name, call, _, _ in self.entry_points:
            self.d.upload_wait(-1)       # (the uploads share one pinned source)
            got = self.status(call(first, 1, False, False))
            assert got == (0, ""), "%s(slot %d): %r" % (name, first, got)
        self.d.clear_mask_rule(first, 1)

    def begin_lane(self):
        self.d.match_begin(1, LANE_SLOT, 1, THR, 0)

    def end_lane(self):
        self.d.match_end(1, n_slots=1)

    def begin_colour_check(self):
        m = np.concatenate([self.matches[s][:3] for s in CHECK_SLOTS])
        sl = np.repeat(np.array(CHECK_SLOTS, np.int32), [len(self.matches[s][:3]) for s in CHECK_SLOTS])
        lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(180, 255, 255)
        self.n_checked = len(m)
        self.d._check(self.lib.lm_color_check_begin_slots(self.h, sl.ctypes.data_as(C.c_void_p), lo, hi, m.ctypes.data_as(C.c_void_p), len(m)))

    def end_colour_check(self):
        a, b = np.zeros(self.n_checked, np.int64), np.zeros(self.n_checked, np.int64)
        self.d._check(self.lib.lm_color_check_end(self.h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))

    def begin_depth_counts(self):
        q = np.zeros(2, self.lm.DEPTH_QUERY_DTYPE)
        for k, s in enumerate(CHECK_SLOTS):
            q[k] = (10, 10, 60, 50, 500, 900, s, 0)
        self.d._check(self.lib.lm_depth_counts_begin(self.h, q.ctypes.data_as(C.c_void_p), len(q)))

    def end_depth_counts(self):
        below, inside = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
        self.d._check(self.lib.lm_depth_counts_end(self.h, below.ctypes.data_as(C.c_void_p), inside.ctypes.data_as(C.c_void_p)))


@pytest.fixture(scope="module")
def rig(lm, orc, synth):
    r = Rig(lm, orc, synth)
    yield r
    r.close()


def test_slot_of_a_lane_in_flight(rig):
    rig.reset()
    rig.begin_lane()
    try:
        for name, call, _, _ in rig.entry_points:
            rig.refused(name, call, LANE_SLOT, 1, BUSY)
        # the range forms: a range that only touches the lane's slot
        for name in ("match_collect", "stage_reserve", "upload_frames_pinned", "set_mask_rule"):
            call = dict((e[0], e[1]) for e in rig.entry_points)[name]
            rig.refused(name, call, 0, 2, BUSY)
            rig.refused(name, call, 1, 3, BUSY)
        rig.succeeds(FREE_SLOT)
        rig.succeeds(0)
    finally:
        rig.end_lane()
    rig.succeeds(LANE_SLOT)


@pytest.mark.parametrize("check", ["colour_check", "depth_counts"])
def test_slot_inside_the_range_of_a_check_in_flight(rig, check):
    words = COLOUR_CHECK if check == "colour_check" else DEPTH_COUNTS
    rig.reset()
    getattr(rig, "begin_" + check)()
    try:
        for name, call, _, _ in rig.entry_points:
            for slot in (0, 1, 2):      # (slot 1: not named by the check, inside its range)
                if name == "match_collect":     # reads the lists, not the frame: no check in flight is in its way
                    assert rig.status(call(slot, 1, False, False)) == (0, "")
                else:
                    rig.refused(name, call, slot, 1, words)
        for name in ("stage_reserve", "upload_frames_pinned", "set_mask_rule"):
            call = dict((e[0], e[1]) for e in rig.entry_points)[name]
            rig.refused(name, call, 2, 2, words)
        rig.succeeds(FREE_SLOT)
    finally:
        getattr(rig, "end_" + check)()
    for slot in (0, 1, 2):
        rig.succeeds(slot)


@pytest.mark.parametrize("check", ["colour_check", "depth_counts"])
def test_first_check_wins(rig, check):
    """Null colour image, a stride one byte too small, a busy lane's slot (1), a check's slot (0, 1, 2): every pair an entry point can
    be given.  The order of every entry point: its arguments, then the lane, then the checks."""
    words = COLOUR_CHECK if check == "colour_check" else DEPTH_COUNTS
    rig.reset()
    getattr(rig, "begin_" + check)()      # (before the lane: a colour check may have to build the bank's hulls, which no busy lane allows)
    rig.begin_lane()
    try:
        for name, call, defects, own in rig.entry_points:
            if "null" in defects and "short" in defects:
                rig.refused(name, call, FREE_SLOT, 1, own["null"], null=True, short=True)
            for k in defects:
                kw = {k: True}
                rig.refused(name, call, FREE_SLOT, 1, own[k], **kw)      # (alone)
                rig.refused(name, call, LANE_SLOT, 1, own[k], **kw)      # + lane (+ check)
                rig.refused(name, call, 0, 1, own[k], **kw)              # + check
            rig.refused(name, call, LANE_SLOT, 1, BUSY)                  # lane + check
            if name != "match_collect":
                rig.refused(name, call, 0, 1, words)
        # lm_stage_rows shares the frame uploads' source checks (host memory only: it asks neither the lanes nor the checks)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        for null, short, w in ((True, True, NO_COLOUR), (True, False, NO_COLOUR), (False, True, SHORT_ROW)):
            rc = rig.lib.lm_stage_rows(rig.h, FREE_SLOT, None if null else vp(rig.bgr), W * 3 - 1 if short else 0, vp(rig.depth), 0, 0, 0, 0, H)
            assert rig.status(rc) == (INVALID, w)
        # lm_set_mask_rule looks at the rule before it looks at the slots
        rc = rig.lib.lm_set_mask_rule(rig.h, LANE_SLOT, 1, C.byref(rig.bad_rule))
        assert rig.status(rc) == (INVALID, "mask rule: grow out of range (0 .. 16)")
        rig.succeeds(FREE_SLOT)
    finally:
        rig.end_lane()
        getattr(rig, "end_" + check)()
    for slot in (0, 1, 2):
        rig.succeeds(slot)
