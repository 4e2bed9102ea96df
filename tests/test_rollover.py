"""Every forward-only 32-bit counter behind a tagged granule, carried across its roll-over (DESIGN.md "Forward-only counters").

The library hands work between workgroups, and between device and host, in 8-byte granules {tag, payload}; the tags are epochs and
sequence numbers that only move forward, and 2^32 of them is weeks to years of uptime.  itm_debug_counter (include/itm_debug.h) places
a handle's counter a few steps before the roll-over; every test then makes the same calls it would make anywhere else and compares bit
for bit -- with the CPU oracle where there is one, and with the same call made far from the roll-over.  No tolerance anywhere.

  * visible list (listEpoch, frameParity): the turning-camera scenarios of test_hip_parity.py whose blocks live in the excess region,
    with the last epoch and the launch after it on frames 2-3; with a fresh scene's very first launch being the one after the wrap
    (every stamp cell still zero); with a ResetScene between the two; with a FindVisibleBlocks on a second render state between the
    two.  Counters, visible ids and types every frame, the whole state at the end, statusFlags 0; fused sweep and separate sweep.
  * trackers (GHChannel::seq of all four, the ICP tracker's session number): one evaluation at the last number, the first number of the
    next round and an ordinary one; TrackCamera calls that straddle the wrap, through the resident session, host-memory commands and one
    launch per evaluation, large (gathering workgroups) and small (per-workgroup records) evaluations in turn; the session number.
  * image maps (LimitSlot::epoch): valid image at the last epoch, all-invalid image at the first of the next round, valid image.
  * the pose-quality handle shares the trackers' channel and gets the same treatment.

Without the fixes of this change, on an MI355X: a fresh scene whose first launch carries epoch 0 lists 0 visible blocks where the oracle
lists 692 (both scenarios, both sweeps), no status flag raised; a wrap in mid-run (frames 2-3, also behind a ResetScene) still produced
the oracle's list in that run -- every stamp cell it read held a recent epoch or had been overtaken by its producer -- and fails only
the check that 0 is never handed out.  Session number 0 changed no pose and replaced no session in that run: every reader compares
it for equality with a number the host wraps alike, and the one alias -- the exit word of a handle that has never had a session is 0 too --
only acts when an answer takes longer than 1 024 polls; test_session_number_crosses_its_wrap fails there on the numbering alone
([1, 1, 2] for [2, 2, 3]).  The sequence-number and image-map cases pass with and without the fixes: their wrap code was right, and had
never run."""
import ctypes as C

import numpy as np
import pytest

import colour_cases as CC
import image_map_cases as IC
import image_map_terms as IT
import itm_testlib as T
import ren_cases as RC
import wicp_cases as WC
from infinitam_amd import capi, synth
from infinitam_amd.capi import ColourEval, RenEval, TrackerConfig, TrackerGH
from itm_testlib import Scenario

pytestmark = pytest.mark.gpu

M32 = 0xffffffff
LAST_EPOCH = M32            # the visible list, the session number and the image maps use every value but 0
LAST_SEQ = M32 - 1          # the sequence numbers skip 0 and ~0 (gh_reduce.h, next_seq)


def next_seq(s):
    s = (s + 1) & M32
    return 1 if s in (0, M32) else s


def steps_between(a, b, limit=1000):
    """evaluations that took a channel from sequence number a to b"""
    n = 0
    while a != b:
        a, n = next_seq(a), n + 1
        assert n <= limit
    return n


def debug_key(hip, key, value):
    hip.check(hip.fn["debug_set"](key, value), "debug_set")


# ---- visible list ------------------------------------------------------------------------------------------------------------------
TURNING = {sc.name: sc for sc in (
    Scenario(name="turning_away_tiny_table", frames=7, bucketNum=0x1000, excessNum=0x2000, w=320, h=240, voxelSize=0.01, trajectory="yaw", yaw_rate=0.12),
    Scenario(name="turning_away_ragged_excess", frames=6, bucketNum=0x1000, excessNum=0x1238, w=320, h=240, voxelSize=0.01, trajectory="yaw", yaw_rate=0.15))}
SIDE_POSE = synth.pose_matrix_yaw((0.1, 0.0, 0.0), 0.2)          # FindVisibleBlocks on the second render state
_oracle_runs = {}


def frame_record(ses):
    c = ses.scene.counters(ses.rs)
    n = c["noVisibleEntries"]
    return c, ses.scene.download(T.BUF_VISIBLE_IDS, ses.rs)[:n].copy(), ses.scene.download(T.BUF_VISIBLE_TYPE, ses.rs).copy()


def side_list(ses, rs2):
    """FindVisibleBlocks from SIDE_POSE on a second render state: (count, ids)"""
    ses.scene.vis.FindVisibleBlocks(SIDE_POSE, ses.sc.intr(), rs2)
    n = ses.scene.counters(rs2)["noVisibleEntries"]
    return n, ses.scene.download(T.BUF_VISIBLE_IDS, rs2)[:n].copy()


def oracle_run(oracle, sc):
    """The oracle's run of `sc`, once per module: per-frame records, the side list after frame 2, the state at the end."""
    if sc.name not in _oracle_runs:
        ses = T.Session(oracle, sc)
        rs2 = ses.scene.vis.CreateRenderState((sc.w, sc.h))
        frames, side = [], None
        for k in range(sc.frames):
            ses.frame(k)
            frames.append(frame_record(ses))
            if k == 2:
                side = side_list(ses, rs2)
        end = ses.snapshot()
        end.counters = [f[0] for f in frames]
        rs2.close()
        ses.close()
        # the scenario does what it is here for: most blocks in the excess region, hundreds of them leaving the list
        vis = [f[0]["noVisibleEntries"] for f in frames]
        free = [f[0]["lastFreeBlockId"] for f in frames]
        assert sum((free[k - 1] - free[k]) - (vis[k] - vis[k - 1]) for k in range(1, len(vis))) > 300
        assert (end.hash["ptr"][sc.bucketNum:] >= 0).sum() > 300
        _oracle_runs[sc.name] = (frames, side, end)
    return _oracle_runs[sc.name]


def assert_frame(k, got, want, what):
    (ca, ia, ta), (cb, ib, tb) = got, want
    tag = f"[{what}, frame {k}] "
    assert ca["statusFlags"] == 0, tag + f"statusFlags {ca['statusFlags']}"
    for key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries"):
        assert ca[key] == cb[key], f"{tag}counter {key}: {ca[key]} vs {cb[key]}"
    assert np.array_equal(ia, ib), tag + "visible ids"
    assert np.array_equal(ta, tb), tag + f"visible types: {(ta != tb).sum()} differ"


def place(hip, ses, steps_to_last):
    """The scene's next `steps_to_last` visible-list launches end on the last epoch; the frame count wraps with it."""
    hip.debug_counter(capi.COUNTER_LIST_EPOCH, ses.scene, LAST_EPOCH - steps_to_last)
    parity = hip.debug_counter(capi.COUNTER_FRAME_PARITY, ses.scene) & 1
    near = (M32 - steps_to_last) & M32
    hip.debug_counter(capi.COUNTER_FRAME_PARITY, ses.scene, near if (near & 1) == parity else (near - 1) & M32)


def run_across_the_wrap(hip, oracle, sc, how, what):
    frames, side, end = oracle_run(oracle, sc)
    ses = T.Session(hip, sc)
    rs2 = None
    try:
        if how == "frames_2_3":
            place(hip, ses, 3)                        # frames 0, 1, 2 take the last three epochs
        elif how == "first_launch":
            place(hip, ses, 0)                        # nothing launched yet: every stamp cell is as scene creation left it
        elif how == "reset_between":
            place(hip, ses, 2)
            for k in range(2):
                ses.frame(k, fused=True)
            assert hip.debug_counter(capi.COUNTER_LIST_EPOCH, ses.scene) == LAST_EPOCH
            ses.scene.reco.ResetScene()
            ses.rs.close()
            ses.rs = ses.scene.vis.CreateRenderState((sc.w, sc.h))
        elif how == "find_visible_between":
            place(hip, ses, 3)
            rs2 = ses.scene.vis.CreateRenderState((sc.w, sc.h))
        for k in range(sc.frames):
            before = hip.debug_counter(capi.COUNTER_LIST_EPOCH, ses.scene)
            ses.frame(k, fused=True)
            after = hip.debug_counter(capi.COUNTER_LIST_EPOCH, ses.scene)
            assert_frame(k, frame_record(ses), frames[k], what)
            assert after == (1 if before == LAST_EPOCH else before + 1), (k, before, after)       # one launch a frame; 0 is never an epoch
            if rs2 is not None and k == 2:
                # between the last epoch and the first of the next round.  FindVisibleBlocks lists through the two-pass compaction,
                # which carries no epoch: the counter stays where it is
                assert after == LAST_EPOCH
                n, ids = side_list(ses, rs2)
                assert hip.debug_counter(capi.COUNTER_LIST_EPOCH, ses.scene) == LAST_EPOCH
                assert n == side[0] and np.array_equal(ids, side[1]), f"[{what}] FindVisibleBlocks on the second render state"
        a = ses.snapshot()
        a.counters = [ses.scene.counters(ses.rs)]
        b = T.RunResult(**{**end.__dict__, "counters": end.counters[-1:]})
        T.compare_results(a, b, sc, what=what)
        assert a.counters[-1]["statusFlags"] == 0
    finally:
        if rs2 is not None:
            rs2.close()
        ses.close()


@pytest.mark.parametrize("sweep", ["fused_sweep", "separate_sweep"])
@pytest.mark.parametrize("how", ["frames_2_3", "first_launch", "reset_between", "find_visible_between"])
@pytest.mark.parametrize("name", list(TURNING))
def test_visible_list_epoch_crosses_its_wrap(hip, oracle, name, how, sweep):
    """listEpoch (and frameParity with it) across 2^32: the look-back, the wait for the excess sweeps and the shared re-test verdicts
    all accept a granule by its epoch, and a cell that no launch has stamped holds 0."""
    sc = TURNING[name]
    debug_key(hip, 13, 1 if sweep == "separate_sweep" else 0)
    try:
        run_across_the_wrap(hip, oracle, sc, how, f"{name}/{how}/{sweep}")
    finally:
        debug_key(hip, 13, 0)


def test_first_launch_of_a_fresh_scene_is_the_one_after_the_wrap(hip, oracle):
    """The worst case for stale zeros by itself (it is also a case of the test above): a scene whose stamp cells have never been
    written makes its first launch right after epoch 0xffffffff."""
    sc = TURNING["turning_away_tiny_table"]
    run_across_the_wrap(hip, oracle, sc, "first_launch", sc.name + "/first launch after the wrap")


def test_table_epoch_crosses_its_wrap(hip, oracle):
    """tableEpoch is compared for equality between a frame issued ahead and the allocation that consumes it; a reset that takes it
    from 0xffffffff to 0 is a change like any other."""
    sc = Scenario(name="table_epoch", w=160, h=120, voxelSize=0.01, frames=3)
    want = T.run_scenario(oracle, sc)
    ses = T.Session(hip, sc)
    try:
        hip.debug_counter(capi.COUNTER_TABLE_EPOCH, ses.scene, M32)
        ses.frame(0, fused=True)
        ses.scene.reco.ResetScene()
        assert hip.debug_counter(capi.COUNTER_TABLE_EPOCH, ses.scene) == 0
        ses.rs.close()
        ses.rs = ses.scene.vis.CreateRenderState((sc.w, sc.h))
        counters = []
        for k in range(sc.frames):
            ses.frame(k, fused=True)
            counters.append(ses.scene.counters(ses.rs))
        a = ses.snapshot()
        a.counters = counters
        T.compare_results(a, want, sc, what="table epoch")
    finally:
        ses.close()


# ---- trackers ----------------------------------------------------------------------------------------------------------------------
SC_SMALL = WC.SCENES["offaxis"]                                                                        # 160 x 120: 80 workgroups at most
SC_LARGE = Scenario(name="roll_qvga", w=320, h=240, voxelSize=0.01, frames=3, stream=3, trajectory="yaw")   # 320 x 240: 150 on level 0
_inputs = {}


def fptr(a):
    return np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))


class IcpInputs:
    """ICP maps of a fused scene, the next depth frame and its sigmaZ in device memory (computed on the product, once per module)."""

    def __init__(self, hip, sc):
        points, normals, self.M_d, depth, sigma = WC.build(hip, sc)
        self.sc = sc
        self.points, self.normals = hip.to_backend(points), hip.to_backend(normals)
        self.depth, self.sigma = hip.to_backend(depth), hip.to_backend(sigma)
        self.inv = WC.eval_inv_poses(self.M_d)["off"]


def icp_inputs(hip, sc):
    if sc.name not in _inputs:
        _inputs[sc.name] = IcpInputs(hip, sc)
    return _inputs[sc.name]


def icp_config(sc):
    cfg = TrackerConfig.default()
    levels = 4 if sc.w >= 320 else 3
    cfg.noHierarchyLevels = levels
    cfg.trackingRegime[:levels] = [3, 3, 1, 1][:levels]
    return cfg


class IcpHandle:
    def __init__(self, hip):
        self.hip, self.h = hip, C.c_void_p()
        hip.check(hip.fn["tracker_create"](C.byref(self.h)), "tracker_create")

    def close(self):
        self.hip.check(self.hip.fn["tracker_destroy"](self.h), "tracker_destroy")

    def counter(self, which, value=None):
        return self.hip.debug_counter(which, self.h, value)

    def evaluate(self, inp, mode, weighted=False):
        out, sc = TrackerGH(), inp.sc
        common = (sc.w, sc.h, fptr(sc.intr()), inp.points.ptr, inp.normals.ptr, sc.w, sc.h, fptr(sc.intr()), fptr(inp.inv), fptr(inp.M_d),
                  WC.DIST_THRESH, mode, C.byref(out), None)
        if weighted:
            self.hip.check(self.hip.fn["tracker_weighted_g_and_h"](self.h, inp.depth.ptr, inp.sigma.ptr, *common), "tracker_weighted_g_and_h")
        else:
            self.hip.check(self.hip.fn["tracker_g_and_h"](self.h, inp.depth.ptr, *common), "tracker_g_and_h")
        return out.noValidPoints, np.float32(out.f).tobytes(), np.array(out.nabla[:], np.float32).tobytes(), np.array(out.hessian[:], np.float32).tobytes()

    def track(self, inp, weighted=False):
        """-> (pose, evaluations): one TrackCamera call; the evaluations are the sequence numbers it took"""
        sc = inp.sc
        view = capi.View(inp.depth, sc.w, sc.h, M_d=inp.M_d, intr_d=sc.intr()).struct()
        out = (C.c_float * 16)()
        before = self.counter(capi.COUNTER_TRACKER_SEQ)
        if weighted:
            cfg = icp_config(sc)
            cfg.noICPRunTillLevel = 0
            cfg.distThresh, cfg.terminationThreshold = WC.DIST_THRESH, WC.TERMINATION
            self.hip.check(self.hip.fn["tracker_weighted_track_camera"](self.h, C.byref(cfg), C.byref(view), inp.sigma.ptr, inp.points.ptr, inp.normals.ptr,
                                                                        fptr(inp.M_d), out, None), "tracker_weighted_track_camera")
        else:
            cfg = icp_config(sc)
            self.hip.check(self.hip.fn["tracker_track_camera"](self.h, C.byref(cfg), C.byref(view), inp.points.ptr, inp.normals.ptr, fptr(inp.M_d), out, None),
                           "tracker_track_camera")
        return np.array(out[:], np.float32), steps_between(before, self.counter(capi.COUNTER_TRACKER_SEQ))


def at_three_numbers(evaluate, set_seq, get_seq):
    """One evaluation at the last sequence number, at the first of the next round and at an ordinary one: identical bits."""
    set_seq(LAST_SEQ - 1)
    last = evaluate()
    assert get_seq() == LAST_SEQ
    first = evaluate()
    assert get_seq() == 1
    set_seq(1000)
    ordinary = evaluate()
    assert get_seq() == 1001
    assert last == first == ordinary
    return ordinary


@pytest.mark.parametrize("weighted", [False, True], ids=["icp", "wicp"])
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("size", ["small", "large"])
def test_icp_evaluation_at_the_last_number_the_first_and_an_ordinary_one(hip, weighted, mode, size):
    inp = icp_inputs(hip, SC_SMALL if size == "small" else SC_LARGE)
    trk = IcpHandle(hip)
    try:
        n, *_ = at_three_numbers(lambda: trk.evaluate(inp, mode, weighted), lambda v: trk.counter(capi.COUNTER_TRACKER_SEQ, v),
                                 lambda: trk.counter(capi.COUNTER_TRACKER_SEQ))
        assert n > 1000
    finally:
        trk.close()


PATHS = {"session": None, "host_command": 11, "launch_per_evaluation": 10}


@pytest.mark.parametrize("path", list(PATHS))
def test_icp_track_camera_straddles_the_sequence_wrap(hip, path):
    """A large call (150 workgroups on level 0: the gathering workgroups and their device records), a small one (80: per-workgroup records
    in pinned memory), a large one again -- the first straddling the wrap, the others behind it, where the records that only the large
    evaluations write still carry the tags of the calls made before.  Every call equals the same call on a fresh handle: pose,
    number of evaluations, no session given up or replaced."""
    large, small = icp_inputs(hip, SC_LARGE), icp_inputs(hip, SC_SMALL)
    key = PATHS[path]
    if key:
        debug_key(hip, key, 1)
    fresh, used = None, None
    try:
        fresh, used = IcpHandle(hip), IcpHandle(hip)           # (created under key 11: its command granules lie in host memory)
        order = [large, small, large]
        want = [fresh.track(inp) for inp in order]
        assert all(n >= 4 for _, n in want), want
        # ordinary numbers first, so that every record carries a small tag the next round will hand out again; then the wrap in the
        # middle of the first call
        for inp in (large, small):
            used.track(inp)
        used.counter(capi.COUNTER_TRACKER_SEQ, LAST_SEQ - want[0][1] // 2)
        got = [used.track(inp) for inp in order]
        assert used.counter(capi.COUNTER_TRACKER_SEQ) == sum(n for _, n in want) - want[0][1] // 2
        for (pa, na), (pb, nb) in zip(got, want):
            assert na == nb and np.array_equal(pa, pb), (na, nb, np.abs(pa - pb).max())
        for h in (fresh, used):
            assert h.counter(capi.COUNTER_TRACKER_FALLBACKS) == 0 and h.counter(capi.COUNTER_TRACKER_RELAUNCHES) == 0
    finally:
        if key:
            debug_key(hip, key, 0)
        for h in (fresh, used):
            if h:
                h.close()


def test_icp_sessions_after_a_wrap_that_a_single_evaluation_crossed(hip):
    """The numbers start over in an evaluation that goes through a launch of its own (itm_tracker_g_and_h), on a handle whose sessions
    have left tagged records in device memory and in the pinned segment sums: the sessions that follow equal a fresh handle's."""
    large, small = icp_inputs(hip, SC_LARGE), icp_inputs(hip, SC_SMALL)
    fresh, used = IcpHandle(hip), IcpHandle(hip)
    try:
        order = [large, small, large]
        want = [fresh.track(inp) for inp in order]
        used.track(large)
        used.counter(capi.COUNTER_TRACKER_SEQ, LAST_SEQ - 1)
        assert used.evaluate(small, 3) == used.evaluate(small, 3)           # the last number, the first of the next round
        assert used.counter(capi.COUNTER_TRACKER_SEQ) == 1
        for inp, (pb, nb) in zip(order, want):
            pa, na = used.track(inp)
            assert na == nb and np.array_equal(pa, pb), (na, nb, np.abs(pa - pb).max())
        assert used.counter(capi.COUNTER_TRACKER_FALLBACKS) == 0 and used.counter(capi.COUNTER_TRACKER_RELAUNCHES) == 0
    finally:
        fresh.close()
        used.close()


def test_wicp_track_camera_straddles_the_sequence_wrap(hip):
    """The weighted tracker: one launch per evaluation on the same channel."""
    large, small = icp_inputs(hip, SC_LARGE), icp_inputs(hip, SC_SMALL)
    fresh, used = IcpHandle(hip), IcpHandle(hip)
    try:
        order = [large, small, large]
        want = [fresh.track(inp, weighted=True) for inp in order]
        assert all(n >= 3 for _, n in want), want
        for inp in (large, small):
            used.track(inp, weighted=True)
        used.counter(capi.COUNTER_TRACKER_SEQ, LAST_SEQ - want[0][1] // 2)
        got = [used.track(inp, weighted=True) for inp in order]
        for (pa, na), (pb, nb) in zip(got, want):
            assert na == nb and np.array_equal(pa, pb), (na, nb, np.abs(pa - pb).max())
    finally:
        fresh.close()
        used.close()


@pytest.mark.parametrize("path", ["session", "host_command"])
def test_session_number_crosses_its_wrap(hip, path):
    """Two TrackCamera calls on a handle whose session number is one step before the wrap: 0 means "no session yet" and is what the
    pinned exit word holds before any session has left, so it is never a session.  Same poses as a fresh handle, no session given up,
    none replaced, no "session did not end" (an error of the call)."""
    inp = icp_inputs(hip, SC_SMALL)
    if path == "host_command":
        debug_key(hip, 11, 1)
    handles = []
    try:
        fresh, used = IcpHandle(hip), IcpHandle(hip)
        handles += [fresh, used]
        want = [fresh.track(inp) for _ in range(3)]
        # placed before the handle's first session (nothing pinned yet, the exit word will be created 0) ...
        used.counter(capi.COUNTER_TRACKER_SESSION, M32 - 1)
        got = [used.track(inp) for _ in range(3)]
        numbers = [used.counter(capi.COUNTER_TRACKER_SESSION)]              # 0xffffffff, 1, 2
        # ... and on a handle that has had sessions
        used.counter(capi.COUNTER_TRACKER_SESSION, M32 - 1)
        got += [used.track(inp) for _ in range(3)]
        numbers.append(used.counter(capi.COUNTER_TRACKER_SESSION))
        # ... and a handle whose very first session is the one after the wrap: its exit word still holds the 0 it was created with
        first = IcpHandle(hip)
        handles.append(first)
        first.counter(capi.COUNTER_TRACKER_SESSION, M32)
        got += [first.track(inp) for _ in range(3)]
        numbers.append(first.counter(capi.COUNTER_TRACKER_SESSION))         # 1, 2, 3
        for (pa, na), (pb, nb) in zip(got, want * 3):
            assert na == nb and np.array_equal(pa, pb), (na, nb, np.abs(pa - pb).max())
        for h in (used, first):
            assert h.counter(capi.COUNTER_TRACKER_FALLBACKS) == 0
            assert h.counter(capi.COUNTER_TRACKER_RELAUNCHES) == 0, "a session was replaced although it was there and answering"
        assert numbers == [2, 2, 3], numbers                                # 0 is never a session
    finally:
        if path == "host_command":
            debug_key(hip, 11, 0)
        for h in handles:
            if h:
                h.close()


# ---- colour tracker ------------------------------------------------------------------------------------------------------------------
COLOUR_INTR = tuple(float(v) for v in synth.intrinsics_for(CC.ODD_W, CC.ODD_H))       # the 161 x 121 frame of colour_cases


class ColourHandle:
    def __init__(self, hip):
        self.hip, self.h = hip, C.c_void_p()
        hip.check(hip.fn["colour_tracker_create"](C.byref(self.h)), "colour_tracker_create")

    def close(self):
        self.hip.check(self.hip.fn["colour_tracker_destroy"](self.h), "colour_tracker_destroy")

    def counter(self, value=None):
        return self.hip.debug_counter(capi.COUNTER_COLOUR_SEQ, self.h, value)


def colour_inputs(hip):
    if "colour" not in _inputs:
        img = CC.odd_frame()
        loc, col = synth.textured_point_cloud(CC.ODD_W, CC.ODD_H, CC.IDENTITY, COLOUR_INTR, step=1)
        rgb = hip.to_backend(np.ascontiguousarray(img))
        dummy = hip.to_backend(np.zeros(img.shape[:2], np.float32))
        view = capi.View(dummy, CC.ODD_W, CC.ODD_H, M_d=CC.IDENTITY, intr_d=COLOUR_INTR, rgb=rgb, w_rgb=CC.ODD_W, h_rgb=CC.ODD_H, intr_rgb=COLOUR_INTR,
                         rgb_to_depth=CC.IDENTITY, rgb_to_depth_inv=CC.IDENTITY)
        _inputs["colour"] = (view, hip.to_backend(loc), hip.to_backend(col), loc.shape[0], (rgb, dummy))
    return _inputs["colour"]


COLOUR_LEVELS = 3


def colour_track(hip, trk, inputs):
    view, loc, col, n, _ = inputs
    cfg = TrackerConfig.default()
    cfg.noHierarchyLevels = COLOUR_LEVELS
    cfg.trackingRegime[:COLOUR_LEVELS] = [3, 3, 1]
    out = (C.c_float * 16)()
    before = trk.counter()
    hip.check(hip.fn["colour_tracker_track_camera"](trk.h, C.byref(cfg), C.byref(view.struct()), None, loc.ptr, col.ptr, n, out, None), "colour_tracker_track_camera")
    return np.array(out[:], np.float32), steps_between(before, trk.counter())


def test_colour_tracker_crosses_the_sequence_wrap(hip):
    inputs = colour_inputs(hip)
    view, loc, col, n, _ = inputs
    fresh, used = ColourHandle(hip), ColourHandle(hip)
    try:
        hip.check(hip.fn["colour_tracker_prepare"](used.h, C.byref(view.struct()), COLOUR_LEVELS, None), "colour_tracker_prepare")

        def evaluate(level, mode):
            out = ColourEval()
            hip.check(hip.fn["colour_tracker_evaluate"](used.h, level, loc.ptr, col.ptr, n, fptr(CC.eval_poses()["perturbed"]), mode, 1, C.byref(out), None),
                      "colour_tracker_evaluate")
            k = out.numPara
            return out.noValidPoints, np.float32(out.f).tobytes(), np.array(out.nabla[:k], np.float32).tobytes(), np.array(out.hessian[:k * k], np.float32).tobytes()

        for level in range(COLOUR_LEVELS):
            for mode in (1, 2, 3):
                count, *_ = at_three_numbers(lambda: evaluate(level, mode), used.counter, used.counter)
                assert count > 100, (level, mode, count)
        want, evals = colour_track(hip, fresh, inputs)
        assert evals >= 4
        used.counter(LAST_SEQ - evals // 2)
        got, n2 = colour_track(hip, used, inputs)
        assert used.counter() == evals - evals // 2
        assert n2 == evals and np.array_equal(got, want), (n2, evals, np.abs(got - want).max())
    finally:
        fresh.close()
        used.close()


# ---- Ren tracker ---------------------------------------------------------------------------------------------------------------------
class RenHandle:
    def __init__(self, hip):
        self.hip, self.h = hip, C.c_void_p()
        hip.check(hip.fn["ren_tracker_create"](C.byref(self.h)), "ren_tracker_create")

    def close(self):
        self.hip.check(self.hip.fn["ren_tracker_destroy"](self.h), "ren_tracker_destroy")

    def counter(self, value=None):
        return self.hip.debug_counter(capi.COUNTER_REN_SEQ, self.h, value)


def test_ren_tracker_crosses_the_sequence_wrap(hip):
    sc = RC.SCENES["hash_s"]
    ses = T.Session(hip, sc)
    fresh, used = RenHandle(hip), RenHandle(hip)
    try:
        for k in range(sc.frames):
            ses.frame(k)
        depth = hip.to_backend(RC.depth(sc))
        inv = RC.eval_inv_poses(sc)["yaw"]
        start = np.asarray(RC.starts()["both"], np.float32)

        def view(M_d):
            return capi.View(depth, sc.w, sc.h, M_d=np.asarray(M_d, np.float32), intr_d=sc.intr())

        def evaluate():
            out = RenEval()
            hip.check(hip.fn["ren_tracker_evaluate"](used.h, C.c_void_p(ses.scene.h), fptr(inv), 1, C.byref(out), None), "ren_tracker_evaluate")
            return out.noValidPoints, np.float32(out.f).tobytes(), np.array(out.nabla[:], np.float32).tobytes(), np.array(out.hessian[:], np.float32).tobytes()

        def track(trk):
            out, n = (C.c_float * 16)(), C.c_int()
            before = trk.counter()
            hip.check(hip.fn["ren_tracker_track_camera"](trk.h, C.c_void_p(ses.scene.h), C.byref(view(start).struct()), out, C.byref(n), None), "ren_tracker_track_camera")
            assert steps_between(before, trk.counter()) >= n.value >= 2
            return np.array(out[:], np.float32), n.value, steps_between(before, trk.counter())

        hip.check(hip.fn["ren_tracker_prepare"](used.h, C.byref(view(RC.true_pose(sc)).struct()), None, None), "ren_tracker_prepare")
        count, *_ = at_three_numbers(evaluate, used.counter, used.counter)
        assert count > 100
        want = track(fresh)
        used.counter(LAST_SEQ - want[2] // 2)
        got = track(used)
        assert used.counter() == want[2] - want[2] // 2
        assert got[1:] == want[1:] and np.array_equal(got[0], want[0]), (got[1:], want[1:])
    finally:
        fresh.close()
        used.close()
        ses.close()


# ---- pose quality (the trackers' channel behind another handle) ---------------------------------------------------------------------
def test_pose_quality_crosses_the_sequence_wrap(hip):
    sc = SC_SMALL
    ses = T.Session(hip, sc)
    q = capi.PoseQuality(hip)
    try:
        for k in range(sc.frames):
            ses.frame(k)
        depth = hip.to_backend(sc.depth(sc.frames))
        view = capi.View(depth, sc.w, sc.h, M_d=sc.pose(sc.frames), intr_d=sc.intr())

        def evaluate():
            stats, img = q.evaluate(ses.scene, view, residuals=True)
            return tuple(sorted(stats.as_dict().items())), img.tobytes()

        def counter(value=None):
            return hip.debug_counter(capi.COUNTER_POSE_QUALITY_SEQ, q.h, value)

        stats, _ = at_three_numbers(evaluate, counter, counter)
        assert dict(stats)["noInliers"] > 1000
    finally:
        q.close()
        ses.close()


# ---- image maps ----------------------------------------------------------------------------------------------------------------------
def new_stream(hip):
    p = C.c_void_p()
    hip.check(hip.fn["stream_create"](C.byref(p)), "stream_create")
    return p


@pytest.mark.parametrize("kind", ["depth", "weight"])
def test_image_map_epoch_crosses_its_wrap(hip, kind):
    """A stream's limit slot: max-reductions of {epoch, bits} words, read back by epoch.  A valid image at the last epoch, an image
    without a valid pixel at the first epoch of the next round (it must not see the limits stamped 0xffffffff, nor may they survive
    as the maximum), a valid image again -- each equal to the restatement and to the same call on a stream whose slot is new."""
    w, h = 160, 120
    make = IC.depth_image if kind == "depth" else IC.uncertainty_image
    fn, restate = ("depth_to_uchar4", IT.depth_to_uchar4) if kind == "depth" else ("weight_to_uchar4", IT.weight_to_uchar4)
    a, c = make(w, h, 31), make(w, h, 32)
    c = np.where(c > 0, c * np.float32(0.5), c).astype(np.float32)          # other limits than a's, and a smaller maximum
    images = [a, np.full((h, w), -1, np.float32), c]
    want = [restate(x) for x in images]
    assert want[0].any() and not want[1].any() and want[2].any() and IT.depth_limits(a) != IT.depth_limits(c)
    near, far = new_stream(hip), new_stream(hip)
    try:
        src = [hip.to_backend(x) for x in images]
        hip.debug_counter(capi.COUNTER_IMAGE_MAP_EPOCH, near, LAST_EPOCH - 1)
        base = hip.debug_counter(capi.COUNTER_IMAGE_MAP_EPOCH, far)       # 0 unless the runtime hands out a stream it has handed out before
        assert base < 1 << 31
        for st, epochs in ((near, [LAST_EPOCH, 1, 2]), (far, [base + 1, base + 2, base + 3])):
            for i, s in enumerate(src):
                dst = hip.to_backend(np.full((h, w, 4), 0xCD, np.uint8))
                hip.check(hip.fn[fn](s.ptr, dst.ptr, w, h, st), fn)
                assert hip.debug_counter(capi.COUNTER_IMAGE_MAP_EPOCH, st) == epochs[i]
                got = dst.numpy(st.value)
                assert np.array_equal(got, want[i]), (kind, "near the wrap" if st is near else "new slot", i, int((got != want[i]).sum()))
    finally:
        for st in (near, far):
            hip.sync(st.value)
            hip.fn["stream_destroy"](st)
