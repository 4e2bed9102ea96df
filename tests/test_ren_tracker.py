"""Ren SDF tracker: unprojection, per-point energy / Jacobian reduction and the Levenberg-Marquardt pose loop
(infinitam_amd/csrc/ren_tracker.hip + ren_solver.h) against the reference's ITMRenTracker_CPU.

Inputs are regenerated from infinitam_amd.synth (tests/ren_cases.py: scenes fused from the first frames of the parity trajectory,
the depth frame one step further); tests/golden/g_ren_tracker.{json,npz} hold their digests and the reference's outputs
(tests/golden/make_golden_ren_tracker.py).  Every GPU test first checks that the library fused the very voxels the reference fused.

  * unprojection: HIP, a numpy restatement and the reference agree bit for bit;
  * evaluation: the valid count of G is exact; F, the gradient and the Hessian come from a fixed-order double-precision tree
    instead of the reference's sequential float sums, so they agree to float accumulation error, relative to the largest entry of
    the same quantity: GH_TOL for the gradient and Hessian, whose terms have mixed signs, and F_TOL for F, whose terms are all
    positive -- at 640 x 480 the reference's running float sum of ~300 000 terms grows to ~1e5, where every addition rounds by up
    to 4e-3, and drifts by ~1e-3 relative (measured on an MI355X: F 1.5e-3, gradient / Hessian 7e-5 at 640 x 480; 4e-6 at
    160 x 120);
  * TrackCamera on the 160 x 120 scenes: every element of the tracked pose within POSE_TOL of the reference's.  The accept test
    (energy below the last) and the 1e-4 relative-decrease test act on the energies and take another branch where a comparison
    is within the energies' error of a tie.  At 160 x 120 that error is 8e-5 relative at most (4e-6 dense), and the nine tracked
    poses show no branch taken differently: on ITMVoxel_s (hash and dense) they agree to 1.3e-7, the float rounding of the final
    pose.  On ITMVoxel_f_rgb two cases end 1.8e-5 and 9.9e-5 apart -- a different branch would move the pose by a whole step,
    millimetres here -- because the 6 x 6 solve near this scene's sideways-move / yaw degeneracy amplifies the rounding of the
    reference's float Cholesky (the solve here is in double); POSE_TOL = 2e-4 covers it.  At 640 x 480 the reference's own energy
    error (1.5e-3) is larger than the threshold, so where it stops is decided by its rounding (its ITMVoxel_s and ITMVoxel_f_rgb
    scenes, whose sdf values differ by quantisation only, stop 2.5 mm apart from the same start); the VGA scene is compared
    evaluation by evaluation.  The sums here are deterministic, so no outcome varies from run to run.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import itm_testlib as T
import ren_cases as RC
from infinitam_amd import capi, synth
from infinitam_amd.capi import RenEval

GOLDEN = os.path.join(T.ROOT, "tests", "golden", "g_ren_tracker")
F_TOL = 3e-3
GH_TOL = 2e-4
POSE_TOL = 2e-4


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN + ".json") as f:
        meta = json.load(f)
    z = np.load(GOLDEN + ".npz")
    return meta, {k: z[k] for k in z.files}


def voxel_digest(vox):
    return {n: synth.sha256(np.ascontiguousarray(vox[n])) for n in vox.dtype.names}


# ---- CPU: inputs and the numpy restatements against the reference -----------------------------------------------------------
def test_depth_inputs_match_the_golden_digests(golden):
    meta, _ = golden
    for name, sc in RC.SCENES.items():
        assert synth.sha256(RC.depth(sc)) == meta["scenes"][name]["depth_sha256"], name
        assert np.array_equal(np.stack(list(RC.eval_inv_poses(sc).values())), np.array(meta["scenes"][name]["eval_inv"], np.float32))
        for s, M in RC.starts().items():
            assert np.array_equal(np.asarray(M, np.float32), np.array(meta["scenes"][name]["tracks"][s]["M_in"], np.float32))


def test_numpy_unprojection_matches_the_reference(golden):
    meta, _ = golden
    for name, sc in RC.SCENES.items():
        pts = RC.unproject(RC.depth(sc), sc.intr())
        assert synth.sha256(pts) == meta["scenes"][name]["points_sha256"], name
        assert (pts[..., 3] == 1).all()                 # the synth frames have no holes: test_unprojection_of_holes covers them


def test_numpy_mrp_step_matches_the_reference(golden):
    meta, _ = golden
    for case in meta["mrp"]:
        got = RC.mrp_matrix(case["step"])
        want = np.array(case["M"], np.float32)
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-7)
        R = RC.mat(got)[:3, :3]
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-5)        # a rotation


def test_ren_tracker_is_declared_and_bound():
    names = capi.declared_functions()
    for n in ("ren_tracker_create", "ren_tracker_destroy", "ren_tracker_prepare", "ren_tracker_evaluate", "ren_tracker_track_camera"):
        assert n in names and n in capi._HOST_IO_SIGS


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    return T.hip_backend()


class Tracker:
    def __init__(self, be):
        self.be = be
        self.h = C.c_void_p()
        be.check(be.fn["ren_tracker_create"](C.byref(self.h)), "ren_tracker_create")

    def close(self):
        if self.h:
            self.be.fn["ren_tracker_destroy"](self.h)
            self.h = C.c_void_p()

    def prepare(self, sc, M_d=None):
        """-> (points read back, the view and the buffers it points into)"""
        d = self.be.to_backend(RC.depth(sc))
        v = capi.View(d, sc.w, sc.h, M_d=np.asarray(M_d if M_d is not None else RC.true_pose(sc), np.float32), intr_d=sc.intr())
        pts = np.zeros((sc.h, sc.w, 4), np.float32)
        self.be.check(self.be.fn["ren_tracker_prepare"](self.h, C.byref(v.struct()), pts.ctypes.data_as(C.c_void_p), None), "prepare")
        return pts, (v, d)

    def evaluate(self, scene, invM, g=True):
        out = RenEval()
        m = np.ascontiguousarray(invM, np.float32)
        self.be.check(self.be.fn["ren_tracker_evaluate"](self.h, C.c_void_p(scene.h), m.ctypes.data_as(C.POINTER(C.c_float)), int(g),
                                                         C.byref(out), None), "evaluate")
        return out.f, out.noValidPoints, np.array(out.nabla[:]), np.array(out.hessian[:])

    def track(self, scene, sc, M_d):
        d = self.be.to_backend(RC.depth(sc))
        v = capi.View(d, sc.w, sc.h, M_d=np.asarray(M_d, np.float32), intr_d=sc.intr())
        out = (C.c_float * 16)()
        n = C.c_int()
        self.be.check(self.be.fn["ren_tracker_track_camera"](self.h, C.c_void_p(scene.h), C.byref(v.struct()), out, C.byref(n), None),
                      "track_camera")
        return np.array(out[:], np.float32), n.value


def fuse(be, sc, last_recorded=False):
    """A session holding the scene of `sc`.  last_recorded: the last frame's allocation and integration are RECORDED by the library
    (deferred fusion) and not launched yet when this returns."""
    ses = T.Session(be, sc)
    for k in range(sc.frames):
        if last_recorded and k == sc.frames - 1:
            v = ses.view(k)
            ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
            ses.scene.reco.IntegrateIntoScene(v, ses.rs)
            ses._keep = v
        else:
            ses.frame(k)
    return ses


def rel(a, b):
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RC.SCENES))
def test_against_the_reference(hip, golden, name):
    """Voxels fused bit-equal to the reference's; points bit-equal; at every evaluation pose the count exact and F / gradient /
    Hessian within F_TOL / GH_TOL; TrackCamera from every starting pose within POSE_TOL."""
    meta, g = golden
    sc = RC.SCENES[name]
    m = meta["scenes"][name]
    ses = fuse(hip, sc)
    trk = Tracker(hip)
    worst, worst_f, worst_pose = 0.0, 0.0, 0.0
    try:
        assert voxel_digest(ses.scene.download(T.BUF_VOXEL_BLOCKS)) == m["voxel_sha256"]
        pts, keep = trk.prepare(sc)
        np.testing.assert_array_equal(pts, RC.unproject(RC.depth(sc), sc.intr()))
        assert synth.sha256(pts) == m["points_sha256"]
        for k, invM in enumerate(np.array(m["eval_inv"], np.float32)):
            f, n, nab, hes = trk.evaluate(ses.scene, invM)
            assert n == g[name + "_count"][k], (k, n)
            rf, rn, rh = rel(f, g[name + "_f"][k]), rel(nab, g[name + "_nabla"][k]), rel(hes, g[name + "_hessian"][k])
            worst = max(worst, rn, rh)
            worst_f = max(worst_f, rf)
            assert rf < F_TOL and max(rn, rh) < GH_TOL, (k, rf, rn, rh)
            f2, n2, nab2, _ = trk.evaluate(ses.scene, invM, g=False)
            assert f2 == f and n2 == 0 and not nab2.any()      # the energy-only pass returns the same energy
        bad = []
        for s, t in (m["tracks"].items() if name not in RC.VGA_SCENES else ()):
            got, evals = trk.track(ses.scene, sc, np.array(t["M_in"], np.float32))
            d = float(np.abs(got - np.array(t["M_out"], np.float32)).max())
            worst_pose = max(worst_pose, d)
            print(f"Ren {name} {s}: {evals} evaluations, pose difference {d:.3g}, translation {got[12:15]}")
            assert evals >= 2
            if d >= POSE_TOL:
                bad.append((s, d, got[12:15], t["M_out"][12:15]))
        assert not bad, bad
    finally:
        trk.close()
        ses.close()
    print(f"Ren {name}: worst relative difference F {worst_f:.3g}, gradient / Hessian {worst:.3g}, worst pose element difference {worst_pose:.3g}")


COMBOS = [(vt, it) for it in (T.INDEX_HASH, T.INDEX_DENSE) for vt in (T.VOXEL_S, T.VOXEL_F, T.VOXEL_S_RGB, T.VOXEL_F_RGB)]


@pytest.mark.gpu
def test_all_voxel_and_index_types_agree(hip):
    """All 8 combinations on the same frames.  Voxel types that store the same sdf (s / s_rgb, f / f_rgb) give identical F / G and
    counts; short and float sdf agree to their quantisation; hash and dense fuse different sets of voxels and are only required to
    track (a non-empty Jacobian set, a finite energy)."""
    import dataclasses
    base = RC.SCENES["dense_s"]
    res = {}
    for vt, it in COMBOS:
        sc = dataclasses.replace(base, voxelType=vt, indexType=it, colour=vt in (T.VOXEL_S_RGB, T.VOXEL_F_RGB))
        if it == T.INDEX_HASH:
            sc = dataclasses.replace(sc, denseSize=(0, 0, 0), denseOffset=None)
        ses = fuse(hip, sc)
        trk = Tracker(hip)
        try:
            trk.prepare(sc)
            res[(vt, it)] = [trk.evaluate(ses.scene, invM) for invM in RC.eval_inv_poses(sc).values()]
        finally:
            trk.close()
            ses.close()
    for it in (T.INDEX_HASH, T.INDEX_DENSE):
        for a, b in ((T.VOXEL_S, T.VOXEL_S_RGB), (T.VOXEL_F, T.VOXEL_F_RGB)):
            for x, y in zip(res[(a, it)], res[(b, it)]):
                assert x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3]), (a, b, it)
        for x, y in zip(res[(T.VOXEL_S, it)], res[(T.VOXEL_F, it)]):
            assert rel(x[0], y[0]) < 1e-3 and abs(x[1] - y[1]) <= max(10, 0.01 * y[1]), (it, x[:2], y[:2])
    for r in res.values():
        for f, n, _, _ in r:
            assert np.isfinite(f) and f < 0 and n > 100


@pytest.mark.gpu
def test_mirror_directory_and_table_walk_agree(hip):
    """The hash scene read through the sdf mirror / block directory (default) and through the table walk alone: same bits."""
    sc = RC.SCENES["hash_s"]
    ses = fuse(hip, sc)
    trk = Tracker(hip)
    try:
        trk.prepare(sc)
        poses = list(RC.eval_inv_poses(sc).values())
        a = [trk.evaluate(ses.scene, p) for p in poses]
        hip.check(hip.fn["debug_set"](5, 1), "debug_set")          # ITM_DEBUG_NO_DIRECTORY: no directory, no mirror
        try:
            b = [trk.evaluate(ses.scene, p) for p in poses]
        finally:
            hip.check(hip.fn["debug_set"](5, 0), "debug_set")
        for x, y in zip(a, b):
            assert x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])
    finally:
        trk.close()
        ses.close()


@pytest.mark.gpu
def test_recorded_fusion_is_launched_before_the_tracker_reads(hip):
    """With the last frame's allocation and integration recorded but not launched, evaluate and TrackCamera see the scene as if
    they had run: the same results as on a scene fused call by call."""
    sc = RC.SCENES["hash_s"]
    inv = RC.eval_inv_poses(sc)["previous"]
    start = RC.starts()["previous"]
    want = []
    for recorded in (False, True):
        ses = fuse(hip, sc, last_recorded=recorded)
        trk = Tracker(hip)
        try:
            trk.prepare(sc)
            e = trk.evaluate(ses.scene, inv)
            want.append((e, trk.track(ses.scene, sc, start)[0]))
        finally:
            trk.close()
            ses.close()
    (a, pa), (b, pb) = want
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    np.testing.assert_array_equal(pa, pb)


@pytest.mark.gpu
def test_unprojection_of_holes(hip):
    """A depth image with zero, negative and NaN pixels at an odd size: HIP and the numpy restatement agree bit for bit."""
    w, h = 161, 121
    rng = np.random.default_rng(7)
    dep = rng.uniform(0.3, 4.0, (h, w)).astype(np.float32)
    dep[rng.random((h, w)) < 0.2] = 0.0
    dep[rng.random((h, w)) < 0.1] = -1.0
    dep[rng.random((h, w)) < 0.05] = np.nan
    intr = synth.intrinsics_for(w, h)
    d = hip.to_backend(dep)
    v = capi.View(d, w, h, intr_d=intr)
    pts = np.zeros((h, w, 4), np.float32)
    trk = Tracker(hip)
    try:
        hip.check(hip.fn["ren_tracker_prepare"](trk.h, C.byref(v.struct()), pts.ctypes.data_as(C.c_void_p), None), "prepare")
    finally:
        trk.close()
    want = RC.unproject(dep, intr)
    assert (want[..., 3] == -1).sum() > 0.3 * w * h * 0.5
    np.testing.assert_array_equal(pts, want)


@pytest.mark.gpu
def test_errors(hip):
    sc = RC.SCENES["hash_s"]
    ses = T.Session(hip, sc)
    trk = Tracker(hip)
    try:
        out = RenEval()
        m = np.eye(4, dtype=np.float32).reshape(16)
        rc = hip.fn["ren_tracker_evaluate"](trk.h, C.c_void_p(ses.scene.h), m.ctypes.data_as(C.POINTER(C.c_float)), 1, C.byref(out), None)
        assert rc != 0                      # nothing prepared
        rc = hip.fn["ren_tracker_evaluate"](trk.h, None, m.ctypes.data_as(C.POINTER(C.c_float)), 1, C.byref(out), None)
        assert rc != 0
    finally:
        trk.close()
        ses.close()
