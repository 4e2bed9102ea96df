"""ICP depth tracker: depth pyramid, per-level gradient/Hessian reduction and the
Levenberg-Marquardt pose update.

  * oracle vs the reference's ITMDepthTracker_CPU / ITMLowLevelEngine_CPU: bit-exact (same sequential sums);
  * HIP vs oracle: the pyramid and the valid-point count are exact; the sums come from a fixed-order
    double-precision tree instead of the reference's sequential float sum, tolerance 2e-4 relative to the
    largest Hessian entry (float accumulation error of ~2e4 terms);
  * the host side of the product's tracker (own damped Gauss-Newton over SE(3) in double precision,
    infinitam_amd/csrc/icp_solver.h + se3.h) against ITMDepthTracker::TrackCamera: driven by the SAME evaluator (the
    oracle's cost / gradient / Hessian) through the host-only hook itm_debug_icp_track, the pose agrees to 2e-5 in every
    element on well-conditioned inputs; runs on CPU;
  * end to end on the GPU the tracked pose agrees with the oracle's to 2e-5 in translation and in the observable
    rotations.  The roll about the optical axis is (nearly) unobservable in the sphere + frontal wall scene: its value is
    set by rounding noise in the sums (the reference itself returns 9e-3 rad of roll for a pure 1 cm translation), so it
    is compared at 2e-4 there and at 2e-5 only on the off-axis / rotated configuration where it is constrained.
"""
import ctypes as C

import numpy as np
import pytest

import itm_testlib as T
from infinitam_amd import capi, synth
from infinitam_amd.capi import DevBuffer, TrackerConfig, TrackerGH
from itm_testlib import Scenario

W, H = 160, 120
SC = Scenario(name="trk", w=W, h=H, voxelSize=0.01, frames=3)


def fp(a):
    a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def build_maps(be):
    """Three frames of fusion -> ICP maps of the last pose (on `be`), plus the next depth frame."""
    ses = T.Session(be, SC)
    for k in range(SC.frames):
        v = ses.frame(k)
    nxt = SC.depth(SC.frames)
    return ses, v, nxt


def subsample(be, img):
    h, w = img.shape
    src = be.to_backend(img)
    dst = DevBuffer(be, (w // 2) * (h // 2) * 4, np.float32, (h // 2, w // 2))
    be.check(be.fn["filter_subsample_with_holes"](src.ptr, w, h, dst.ptr, None), "subsample")
    return dst.numpy()


def g_and_h(be, depth_dev, w, h, intr, ses, inv_pose, scene_pose, dist, it):
    out = TrackerGH()
    _, vi = fp(intr); _, si = fp(SC.intr()); _, ip = fp(inv_pose); _, sp = fp(scene_pose)
    be.check(be.fn["tracker_compute_g_and_h"](depth_dev.ptr, w, h, vi, ses.points.ptr, ses.normals.ptr, W, H, si, ip, sp,
                                              dist, it, C.byref(out), None), "g_and_h")
    return out.noValidPoints, out.f, np.array(out.nabla[:]), np.array(out.hessian[:]).reshape(6, 6)


SC_VGA = Scenario(name="trk_vga", voxelSize=0.01, frames=3)      # 640x480: the 5-level default hierarchy needs it


def build_maps_vga(be):
    ses = T.Session(be, SC_VGA)
    for k in range(SC_VGA.frames):
        v = ses.frame(k)
    return ses, v, SC_VGA.depth(SC_VGA.frames)


def track(be, ses, v, depth_next, cfg=None):
    cfg = cfg or TrackerConfig.default()
    d = be.to_backend(depth_next)
    view = capi.View(d, ses.sc.w, ses.sc.h, M_d=v.M_d, intr_d=ses.sc.intr()).struct()
    out = (C.c_float * 16)()
    _, sp = fp(v.M_d)
    be.check(be.fn["track_camera"](C.byref(cfg), C.byref(view), ses.points.ptr, ses.normals.ptr, sp, out, None), "track_camera")
    return np.array(out[:], np.float32)


def holes_image():
    img = SC.depth(1).copy()
    img[::5, ::3] = -1.0
    img[7:20, 30:60] = 0.0
    return img


def test_subsample_oracle_vs_reference(oracle, ref):
    img = holes_image()
    a = subsample(oracle, img)
    if ref.backend is not None:
        assert np.array_equal(a, subsample(ref.backend, img))
    ref.check("subsample", a)


@pytest.mark.parametrize("it", [1, 2, 3])
def test_g_and_h_oracle_vs_reference(oracle, ref, it):
    res = []
    for be in (oracle, ref.backend) if ref.backend is not None else (oracle,):
        ses, v, nxt = build_maps(be)
        inv = np.linalg.inv(np.asarray(v.M_d, np.float64).reshape(4, 4).T).T.astype(np.float32).reshape(16)   # any fixed matrix works: both get the same
        res.append(g_and_h(be, be.to_backend(nxt), W, H, SC.intr(), ses, inv, v.M_d, 0.01, it))
        ses.close()
    n0, f0, g0, h0 = res[0]
    assert n0 > 5000
    np_ = 3 if it != 3 else 6
    if len(res) > 1:
        n1, f1, g1, h1 = res[1]
        assert n0 == n1
        assert f0 == f1 and np.array_equal(g0[:np_], g1[:np_]) and np.array_equal(h0[:np_, :np_], h1[:np_, :np_])
    ref.check("g_and_h", (n0, f0, g0[:np_], h0[:np_, :np_]))


def test_track_camera_oracle_vs_reference(oracle, ref):
    poses = []
    for be in (oracle, ref.backend) if ref.backend is not None else (oracle,):
        ses, v, nxt = build_maps_vga(be)
        poses.append(track(be, ses, v, nxt))
        ses.close()
    if len(poses) > 1:
        assert np.array_equal(poses[0], poses[1])
    ref.check("pose", poses[0])
    # and it actually tracks: the camera moved 1 cm along x between the two frames
    # (translation only: a sphere on the optical axis in front of a frontal wall leaves the roll unconstrained)
    truth = synth.pose_matrix(SC_VGA.position(SC_VGA.frames))
    assert abs(poses[0][12] - truth[12]) < 1e-3 and abs(poses[0][13]) < 1e-3 and abs(poses[0][14]) < 1e-3


@pytest.mark.gpu
def test_subsample_hip_vs_oracle(hip, oracle):
    img = holes_image()
    assert np.array_equal(subsample(hip, img), subsample(oracle, img))


@pytest.mark.gpu
@pytest.mark.parametrize("it", [1, 2, 3])
def test_g_and_h_hip_vs_oracle(hip, oracle, it):
    res = []
    for be in (hip, oracle):
        ses, v, nxt = build_maps(be)
        inv = np.linalg.inv(np.asarray(v.M_d, np.float64).reshape(4, 4).T).T.astype(np.float32).reshape(16)
        res.append(g_and_h(be, be.to_backend(nxt), W, H, SC.intr(), ses, inv, v.M_d, 0.01, it))
        ses.close()
    (n0, f0, g0, h0), (n1, f1, g1, h1) = res
    assert n0 == n1 and n0 > 5000                        # validity is decided by identical float operations
    scale = np.abs(h1).max()
    assert np.abs(h0 - h1).max() <= 2e-4 * scale
    assert np.abs(g0 - g1).max() <= 2e-4 * max(np.abs(g1).max(), 1e-6) + 1e-7 * n1
    assert abs(f0 - f1) <= 2e-4 * abs(f1)


ROLL = [1, 4]          # elements of the column-major model-view matrix that carry the rotation about the optical axis


def assert_pose_close(a, b, roll_tol):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    rest = [i for i in range(16) if i not in ROLL]
    assert d[rest].max() <= 2e-5, d
    assert d[ROLL].max() <= roll_tol, d


@pytest.mark.gpu
def test_track_camera_hip_vs_oracle(hip, oracle):
    poses = []
    for be in (hip, oracle):
        ses, v, nxt = build_maps_vga(be)
        poses.append(track(be, ses, v, nxt))
        ses.close()
    assert_pose_close(poses[0], poses[1], roll_tol=2e-4)     # on-axis sphere + frontal wall: roll unobservable


SC_OFFAXIS = Scenario(name="trk_offaxis", voxelSize=0.01, frames=3, stream=3, trajectory="yaw")   # camera 15 cm off the sphere's axis, rotating


def build_maps_offaxis(be):
    ses = T.Session(be, SC_OFFAXIS)
    for k in range(SC_OFFAXIS.frames):
        v = ses.frame(k)
    return ses, v, SC_OFFAXIS.depth(SC_OFFAXIS.frames)


@pytest.mark.gpu
def test_track_camera_hip_vs_oracle_well_conditioned(hip, oracle):
    poses = []
    for be in (hip, oracle):
        ses, v, nxt = build_maps_offaxis(be)
        poses.append(track(be, ses, v, nxt))
        ses.close()
    assert_pose_close(poses[0], poses[1], roll_tol=2e-5)


@pytest.mark.gpu
def test_session_kernel_and_launch_per_evaluation_give_the_same_pose_bit_for_bit(hip):
    """TrackCamera through the resident evaluation kernel (one launch per call) and through one launch per evaluation (debug key
    10): the partial sums are formed over the same tiles and added in the same order, so the tracked poses are identical; and a
    tracker handle survives many sessions back to back, also after its resident kernel has hit the idle limit."""
    import time
    ses, v, nxt = build_maps_offaxis(hip)
    try:
        a = track(hip, ses, v, nxt)
        hip.check(hip.fn["debug_set"](10, 1), "debug_set")
        try:
            b = track(hip, ses, v, nxt)
        finally:
            hip.check(hip.fn["debug_set"](10, 0), "debug_set")
        assert np.array_equal(a, b), np.abs(a - b).max()
        for i in range(20):
            assert np.array_equal(track(hip, ses, v, nxt), a), i
        time.sleep(0.05)                                   # far beyond the 2 ms idle limit of a session
        assert np.array_equal(track(hip, ses, v, nxt), a)
    finally:
        ses.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nth", [1, 3, 7])
def test_unusable_session_falls_back_to_one_launch_per_evaluation(hip, nth):
    """A resident evaluation kernel that cannot serve (its workgroups not co-resident: masked compute units, another process's
    session, a smaller device) ends the session; the call -- and the handle's later calls -- finish through one launch per
    evaluation with the same pose, instead of failing with ITM_ERR_DEVICE (debug key 18 makes the n-th evaluation report it)."""
    ses, v, nxt = build_maps_offaxis(hip)
    h = C.c_void_p()
    hip.check(hip.fn["tracker_create"](C.byref(h)), "tracker_create")
    try:
        want = track(hip, ses, v, nxt)
        hip.check(hip.fn["debug_set"](18, nth), "debug_set")
        try:
            got = track_with_handle(hip, h, ses, v, nxt)          # the session gives up at evaluation `nth` of this call
        finally:
            hip.check(hip.fn["debug_set"](18, 0), "debug_set")
        assert np.array_equal(got, want), np.abs(got - want).max()
        for _ in range(3):                                         # and the handle keeps working (launch per evaluation from now on)
            assert np.array_equal(track_with_handle(hip, h, ses, v, nxt), want)
    finally:
        hip.fn["tracker_destroy"](h)
        ses.close()


def track_with_handle(be, handle, ses, v, depth_next, cfg=None):
    cfg = cfg or TrackerConfig.default()
    d = be.to_backend(depth_next)
    view = capi.View(d, ses.sc.w, ses.sc.h, M_d=v.M_d, intr_d=ses.sc.intr()).struct()
    out = (C.c_float * 16)()
    _, sp = fp(v.M_d)
    be.check(be.fn["tracker_track_camera"](handle, C.byref(cfg), C.byref(view), ses.points.ptr, ses.normals.ptr, sp, out, None), "tracker_track_camera")
    return np.array(out[:], np.float32)


@pytest.mark.gpu
def test_session_commands_through_host_memory_give_the_same_pose(hip):
    """Debug key 11: the command granules lie in pinned host memory, workgroup 0 fetches them over PCIe and republishes them in
    device memory for the others (the path of devices without a large BAR).  A tracker handle created under the key uses that
    path for its whole life; poses are identical to the default path's, call after call and after an idle session has left."""
    import time
    ses, v, nxt = build_maps_offaxis(hip)
    handle = C.c_void_p()
    try:
        a = track(hip, ses, v, nxt)
        hip.check(hip.fn["debug_set"](11, 1), "debug_set")
        try:
            hip.check(hip.fn["tracker_create"](C.byref(handle)), "tracker_create")
            b = track_with_handle(hip, handle, ses, v, nxt)          # the handle's buffers are chosen at its first session
        finally:
            hip.check(hip.fn["debug_set"](11, 0), "debug_set")
        assert np.array_equal(a, b), np.abs(a - b).max()
        for i in range(10):
            assert np.array_equal(track_with_handle(hip, handle, ses, v, nxt), a), i
        time.sleep(0.05)
        assert np.array_equal(track_with_handle(hip, handle, ses, v, nxt), a)
    finally:
        if handle:
            hip.check(hip.fn["tracker_destroy"](handle), "tracker_destroy")
        ses.close()


@pytest.mark.gpu
def test_four_trackers_on_four_streams_at_once(hip):
    """Four host threads, each with its own tracker handle and HIP stream, call TrackCamera at the same time: four resident
    evaluation kernels share the GPU, every call returns the pose a lone call returns."""
    import threading
    # streams from the library's own runtime (itm_stream_create): a process that also holds a framework's bundled copy of the HIP
    # runtime would otherwise hand the library streams of the wrong one
    ses, v, nxt = build_maps_offaxis(hip)
    handles, streams = [], []
    try:
        want = track(hip, ses, v, nxt)
        hip.sync()
        d = hip.to_backend(nxt)
        view = capi.View(d, ses.sc.w, ses.sc.h, M_d=v.M_d, intr_d=ses.sc.intr()).struct()
        _, sp = fp(v.M_d)
        cfg = TrackerConfig.default()
        for _ in range(4):
            h = C.c_void_p()
            hip.check(hip.fn["tracker_create"](C.byref(h)), "tracker_create")
            handles.append(h)
            st = C.c_void_p()
            hip.check(hip.fn["stream_create"](C.byref(st)), "stream_create")
            streams.append(st)
        results, errors = [[] for _ in range(4)], []
        gate = threading.Barrier(4)

        def work(i):
            try:
                gate.wait()
                for _ in range(8):
                    out = (C.c_float * 16)()
                    hip.check(hip.fn["tracker_track_camera"](handles[i], C.byref(cfg), C.byref(view), ses.points.ptr, ses.normals.ptr, sp, out,
                                                             streams[i]), "tracker_track_camera")
                    results[i].append(np.array(out[:], np.float32))
            except Exception as e:      # noqa: BLE001 -- reported below, in the main thread
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for i in range(4):
            assert len(results[i]) == 8
            for r in results[i]:
                assert np.array_equal(r, want), (i, np.abs(r - want).max())
    finally:
        hip.sync()
        for h in handles:
            hip.check(hip.fn["tracker_destroy"](h), "tracker_destroy")
        for st in streams:
            hip.fn["stream_destroy"](st)
        ses.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(632, 472), (336, 248), (200, 152)], ids=lambda s: "%dx%d" % s)
def test_evaluation_on_ragged_levels_session_vs_launch_vs_oracle(hip, oracle, size):
    """Image sizes that are no multiple of the 16-pixel tiles, of the one-wave-high coarse tiles or of the 32-workgroup segments:
    TrackCamera through the session kernel == one launch per evaluation (bit for bit), and both follow the oracle."""
    w, h = size
    sc = Scenario(name="trk_ragged_%dx%d" % size, voxelSize=0.01, frames=3, stream=3, trajectory="yaw", w=w, h=h)
    cfg = TrackerConfig.default()
    cfg.noHierarchyLevels = 4
    cfg.trackingRegime[:4] = [3, 3, 1, 1]
    poses = []
    for be in (hip, oracle):
        ses = T.Session(be, sc)
        try:
            for k in range(sc.frames):
                v = ses.frame(k)
            nxt = sc.depth(sc.frames)
            poses.append(track(be, ses, v, nxt, cfg))
            if be is hip:
                hip.check(hip.fn["debug_set"](10, 1), "debug_set")
                try:
                    per_launch = track(be, ses, v, nxt, cfg)
                finally:
                    hip.check(hip.fn["debug_set"](10, 0), "debug_set")
                assert np.array_equal(poses[0], per_launch), np.abs(poses[0] - per_launch).max()
        finally:
            ses.close()
    assert np.abs(poses[0] - poses[1]).max() < 2e-4, np.abs(poses[0] - poses[1]).max()


# ---- the product's host-side solver against the reference's TrackCamera with the same evaluator (CPU) ------------------
EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, C.POINTER(TrackerGH))


def solve_with_oracle_evaluator(host, oracle, sc, ses, v, depth_next, cfg):
    """itm_debug_icp_track (product library, host code only) with cost / gradient / Hessian from the oracle."""
    d = oracle.to_backend(depth_next)
    levels = [(d, sc.w, sc.h, np.array(sc.intr(), np.float32))]
    for _ in range(1, cfg.noHierarchyLevels):
        pd, pw, ph, pi = levels[-1]
        nd = DevBuffer(oracle, (pw // 2) * (ph // 2) * 4, np.float32, (ph // 2, pw // 2))
        oracle.check(oracle.fn["filter_subsample_with_holes"](pd.ptr, pw, ph, nd.ptr, None), "subsample")
        levels.append((nd, pw // 2, ph // 2, pi * np.float32(0.5)))
    _, si = fp(sc.intr()); _, sp = fp(v.M_d)
    calls = []

    def evaluate(user, level, mode, inv_pose, dist, out):
        ld, lw, lh, li = levels[level]
        _, vi = fp(li)
        calls.append(level)
        return oracle.fn["tracker_compute_g_and_h"](ld.ptr, lw, lh, vi, ses.points.ptr, ses.normals.ptr, sc.w, sc.h, si, inv_pose, sp,
                                                    dist, mode, out, None)

    cb = EVAL_FN(evaluate)
    out = (C.c_float * 16)(); _, mp = fp(v.M_d)
    host.check(host.fn["debug_icp_track"](C.byref(cfg), mp, C.cast(cb, C.c_void_p), None, out), "debug_icp_track")
    return np.array(out[:], np.float32), calls


@pytest.mark.parametrize("sc", [SC_VGA, Scenario(name="trk_off", voxelSize=0.01, frames=3, stream=3), SC_OFFAXIS], ids=lambda s: s.name)
def test_host_solver_matches_track_camera_with_the_same_evaluator(hip_host, oracle, sc):
    ses = T.Session(oracle, sc)
    for k in range(sc.frames):
        v = ses.frame(k)
    nxt = sc.depth(sc.frames)
    cfg = TrackerConfig.default()
    want = track(oracle, ses, v, nxt, cfg)                      # == the reference's ITMDepthTracker_CPU, bit for bit (test above)
    got, calls = solve_with_oracle_evaluator(hip_host, oracle, sc, ses, v, nxt, cfg)
    assert np.abs(got - want).max() <= 2e-5, (got, want)
    assert calls[0] == cfg.noHierarchyLevels - 1 and calls[-1] == 0 and calls == sorted(calls, reverse=True)   # coarse to fine
    ses.close()


def test_host_solver_schedule_and_rejection(hip_host):
    """The iteration scheme itself, on a synthetic quadratic: at most 2 (l + 1) evaluations on level l, a rising cost is
    rejected (the evaluator then sees the last accepted pose again), and a tiny step ends a level early."""
    cfg = TrackerConfig.default()
    cfg.noHierarchyLevels = 3
    cfg.trackingRegime[:3] = [3, 2, 1]
    seen = []

    def evaluate(user, level, mode, inv_pose, dist, out):
        inv = np.array([inv_pose[i] for i in range(16)], np.float32)
        seen.append((level, mode, inv.copy(), float(dist)))
        gh = out.contents
        gh.noValidPoints = 1000
        n = 6 if mode == 3 else 3
        for i in range(36):
            gh.hessian[i] = 0.0
        for i in range(n):
            gh.hessian[i + 6 * i] = 1000.0
            gh.nabla[i] = 0.0
        # cost rises on the second evaluation of level 1 -> must be rejected
        gh.f = 2.0 if (level == 1 and sum(1 for s in seen if s[0] == 1) == 2) else 1.0
        if level == 2:
            gh.nabla[0] = 10.0          # a rotation step of 1e-2 / (1 + damping) per evaluation
        return 0

    cb = EVAL_FN(evaluate)
    M = np.eye(4, dtype=np.float32).reshape(16)
    out = (C.c_float * 16)(); _, mp = fp(M)
    hip_host.check(hip_host.fn["debug_icp_track"](C.byref(cfg), mp, C.cast(cb, C.c_void_p), None, out), "debug_icp_track")
    per_level = {l: [s for s in seen if s[0] == l] for l in (2, 1, 0)}
    assert len(per_level[2]) == 6                       # 2 (l + 1) evaluations: the steps never fall below the threshold
    assert [s[1] for s in per_level[2]] == [1] * 6 and per_level[1][0][1] == 2 and per_level[0][0][1] == 3
    # distance threshold: linear from distThresh (coarsest) down in steps of distThresh / levels
    assert abs(per_level[2][0][3] - 0.01) < 1e-9 and abs(per_level[1][0][3] - (0.01 - 0.01 / 3)) < 1e-8
    # zero gradient on levels 1 and 0 -> zero step -> the level ends after its first evaluation ...
    assert len(per_level[0]) == 1
    # ... except that level 1's first step is zero as well, so it also stops at once
    assert len(per_level[1]) == 1
    res = np.array(out[:], np.float32).reshape(4, 4).T
    assert np.abs(res[:3, :3] @ res[:3, :3].T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(res[:3, :3]) - 1) < 1e-6   # stays on SE(3)
    assert res[1, 2] != 0.0                              # rotated about x


def closed_loop(be, frames=5, handle=None, stream=None, depths=None, start=None):
    """ITMMainEngine::ProcessFrame with the ICP tracker instead of external poses: Track -> fuse -> Prepare.  With `handle` /
    `stream` the loop runs on a tracker handle and a HIP stream of its own; `start` is a threading.Barrier to leave together."""
    sc = Scenario(name="loop", voxelSize=0.01, frames=frames)
    ses = T.Session(be, sc)
    pose = synth.pose_matrix(sc.position(0))
    traj = [pose.copy()]
    cfg = TrackerConfig.default()
    if start is not None:
        start.wait()
    for k in range(frames):
        d = depths[k] if depths is not None else be.to_backend(sc.depth(k))
        if k > 0:   # age_pointCloud != -1: track against the maps rendered from the previous pose
            view = capi.View(d, sc.w, sc.h, M_d=pose, intr_d=sc.intr()).struct()
            out = (C.c_float * 16)()
            _, sp = fp(pose)
            if handle is None:
                be.check(be.fn["track_camera"](C.byref(cfg), C.byref(view), ses.points.ptr, ses.normals.ptr, sp, out, stream), "track")
            else:
                be.check(be.fn["tracker_track_camera"](handle, C.byref(cfg), C.byref(view), ses.points.ptr, ses.normals.ptr, sp, out, stream), "track")
            pose = np.array(out[:], np.float32)
            traj.append(pose.copy())
        v = capi.View(d, sc.w, sc.h, M_d=pose, intr_d=sc.intr())
        ses.scene.process_frame(v, ses.rs, ses.points, ses.normals, stream=stream.value if stream is not None else None)
    be.sync(stream.value if stream is not None else None)
    ses.close()
    return sc, np.array(traj)


def test_closed_loop_oracle_follows_the_trajectory(oracle):
    sc, traj = closed_loop(oracle, frames=4)
    for k in range(1, 4):
        assert abs(traj[k][12] - (-0.01 * k)) < 1.5e-3, (k, traj[k][12])   # world->camera translation = -camera position


@pytest.mark.gpu
def test_closed_loop_hip_follows_the_trajectory_and_the_oracle(hip, oracle):
    sc, a = closed_loop(hip, frames=6)
    for k in range(1, 6):
        assert abs(a[k][12] - (-0.01 * k)) < 1.5e-3, (k, a[k][12])
    _, b = closed_loop(oracle, frames=6)
    # Tiny differences in the summed Hessians are amplified by the feedback through the map.  The constrained
    # part (translation) stays far below the voxel size (1 cm); the roll about the optical axis is unobservable
    # in this scene (sphere on the axis + frontal wall), drifts in both runs and is not compared.
    assert np.abs(a[:, 12:15] - b[:, 12:15]).max() < 2e-4


@pytest.mark.gpu
def test_four_closed_loops_on_four_streams_keep_trajectory_and_pace(hip):
    """Four tracking + mapping loops on four streams from four host threads.  While one loop's evaluation kernel is resident the
    others' fusion and ray-cast kernels share its compute units; workgroups of the evaluation kernel that have no tiles on a coarse
    level then look at a command late -- they must join at the command they find, and a replaced session's stragglers must leave at
    once (before: records missing on the next fine level, idle limits, 10 frames/s).  Every loop ends on the lone loop's trajectory,
    bit for bit, and the four together take about as long as their tracking calls one after the other."""
    import threading
    import time
    frames, loops = 30, 4
    sc0 = Scenario(name="loop", voxelSize=0.01, frames=frames)
    depths = [hip.to_backend(sc0.depth(k)) for k in range(frames)]
    _, want = closed_loop(hip, frames=frames, depths=depths)
    handles, streams = [], []
    try:
        for _ in range(loops):
            h = C.c_void_p(); hip.check(hip.fn["tracker_create"](C.byref(h)), "tracker_create"); handles.append(h)
            st = C.c_void_p(); hip.check(hip.fn["stream_create"](C.byref(st)), "stream_create"); streams.append(st)
        results, errors = [None] * loops, []
        start = threading.Barrier(loops + 1)

        def work(i):
            try:
                results[i] = closed_loop(hip, frames=frames, handle=handles[i], stream=streams[i], depths=depths, start=start)[1]
            except Exception as e:      # noqa: BLE001 -- reported below, in the main thread
                errors.append(e)
                try:
                    start.abort()
                except Exception:       # noqa: BLE001
                    pass

        threads = [threading.Thread(target=work, args=(i,)) for i in range(loops)]
        for t in threads:
            t.start()
        start.wait()
        t0 = time.perf_counter()
        for t in threads:
            t.join()
        elapsed = time.perf_counter() - t0
        assert not errors, errors
        for i in range(loops):
            assert np.array_equal(results[i], want), (i, np.abs(results[i] - want).max())
        assert elapsed < 1.5, f"{loops} loops x {frames} frames took {elapsed:.2f} s (about 0.05 s when the sessions hand over cleanly)"
    finally:
        hip.sync()
        for h in handles:
            hip.check(hip.fn["tracker_destroy"](h), "tracker_destroy")
        for st in streams:
            hip.fn["stream_destroy"](st)
