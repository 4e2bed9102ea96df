"""Colour (photometric) tracker: rgb pyramid and gradients, per-level cost / gradient / Hessian, the Levenberg-Marquardt pose
loop (infinitam_amd/csrc/colour_tracker.hip + colour_solver.h) against the reference's ITMColorTracker_CPU.

Inputs are regenerated from infinitam_amd.synth (tests/colour_cases.py: a textured sphere + wall, a 320 x 240 point cloud seen from
the identity pose, rgb frames at the true poses); tests/golden/g_colour_tracker.{json,npz} hold their digests and the reference's
outputs (tests/golden/make_golden_colour_tracker.py).

  * pyramid and gradients: HIP, a numpy restatement and the reference agree bit for bit;
  * evaluation: the valid count is exact; f, the gradient and the Hessian come from a fixed-order double-precision tree instead of
    the reference's sequential float sums over ~75 000 points, so they agree to float accumulation error: EVAL_TOL = 2e-4
    relative to the largest entry of the same quantity (measured on an MI355X: 1.3e-4 at worst);
  * TrackCamera: every element of the tracked pose within POSE_TOL = 5e-6 of the reference's (measured: 3e-7 on all five cases,
    the float rounding of the final pose).  The accept test f2 < f - |f| 1e-5 and the gain-ratio thresholds act on those sums and
    could take another branch where a comparison is within ~1e-4 relative of a tie; none of the five cases comes close (the
    sums are deterministic, so the result does not vary from run to run), and no case here needs a looser bound.
"""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import colour_cases as CC
import itm_testlib as T
from infinitam_amd import capi, synth
from infinitam_amd.capi import ColourEval, TrackerConfig

GOLDEN = os.path.join(T.ROOT, "tests", "golden", "g_colour_tracker")
EVAL_TOL = 2e-4
POSE_TOL = 5e-6


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN + ".json") as f:
        meta = json.load(f)
    z = np.load(GOLDEN + ".npz")
    return meta, {k: z[k] for k in z.files}


def fp(a):
    a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def config(regime=None):
    cfg = TrackerConfig.default()
    cfg.noHierarchyLevels = CC.LEVELS
    cfg.trackingRegime[:CC.LEVELS] = regime or CC.REGIME
    return cfg


# ---- CPU: inputs and the numpy restatement of PrepareForEvaluation against the reference ---------------------------------------
def test_inputs_match_the_golden_digests(golden):
    meta, _ = golden
    loc, col = CC.cloud()
    assert [synth.sha256(loc), synth.sha256(col)] == meta["cloud_sha256"]
    assert synth.sha256(CC.frame(CC.motions()["both"][0])) == meta["vga_frame_sha256"]
    assert synth.sha256(CC.odd_frame()) == meta["odd_frame_sha256"]
    for name, (M, calib, _) in CC.motions().items():
        assert synth.sha256(CC.frame(M, calib)) == meta["tracks"][name]["frame_sha256"], name


@pytest.mark.parametrize("which", ["vga", "odd"])
def test_numpy_pyramid_matches_the_reference(golden, which):
    meta, _ = golden
    img = CC.frame(CC.motions()["both"][0]) if which == "vga" else CC.odd_frame()
    pyr = CC.numpy_pyramid(img, CC.LEVELS)
    for lv, (rgb, gx, gy) in enumerate(pyr):
        assert [synth.sha256(rgb), synth.sha256(gx), synth.sha256(gy)] == meta[which + "_pyramid_sha256"][lv], (which, lv)
        for g in (gx, gy):
            assert not g[0].any() and not g[-1].any() and not g[:, 0].any() and not g[:, -1].any()
    assert (pyr[1][1][..., :3] < 0).any()          # negative gradients occur: truncation toward zero matters


def test_colour_tracker_is_declared_and_bound():
    names = capi.declared_functions()
    for n in ("colour_tracker_create", "colour_tracker_prepare", "colour_tracker_evaluate", "colour_tracker_track_camera"):
        assert n in names and n in capi._HOST_IO_SIGS


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    return T.hip_backend()


class Tracker:
    def __init__(self, be):
        self.be = be
        self.h = C.c_void_p()
        be.check(be.fn["colour_tracker_create"](C.byref(self.h)), "colour_tracker_create")

    def close(self):
        if self.h:
            self.be.fn["colour_tracker_destroy"](self.h)
            self.h = C.c_void_p()


@pytest.fixture(scope="module")
def cloud(hip):
    loc, col = CC.cloud()
    return hip.to_backend(loc), hip.to_backend(col), loc.shape[0]


def view_of(be, img, M_d=None, calib=None, intr=CC.INTR):
    h, w = img.shape[:2]
    rgb = be.to_backend(np.ascontiguousarray(img))
    dummy = be.to_backend(np.zeros((h, w), np.float32))
    calib = np.asarray(calib if calib is not None else CC.IDENTITY, np.float32)
    v = capi.View(dummy, w, h, M_d=np.asarray(M_d if M_d is not None else CC.IDENTITY, np.float32), intr_d=intr, rgb=rgb,
                  w_rgb=w, h_rgb=h, intr_rgb=intr, rgb_to_depth=calib,
                  rgb_to_depth_inv=np.linalg.inv(CC.mat(calib)).T.reshape(16).astype(np.float32))
    return v, (rgb, dummy)


def read_level(be, trk, lv):
    w, h = C.c_int(), C.c_int()
    be.check(be.fn["colour_tracker_read_level"](trk.h, lv, None, None, None, C.byref(w), C.byref(h), None), "read_level")
    rgb = np.zeros((h.value, w.value, 4), np.uint8); gx = np.zeros((h.value, w.value, 4), np.int16); gy = np.zeros_like(gx)
    be.check(be.fn["colour_tracker_read_level"](trk.h, lv, rgb.ctypes.data_as(C.c_void_p), gx.ctypes.data_as(C.c_void_p),
                                                gy.ctypes.data_as(C.c_void_p), C.byref(w), C.byref(h), None), "read_level")
    return rgb, gx, gy


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["vga", "odd"])
def test_pyramid_and_gradients_hip_vs_numpy_and_reference(hip, golden, which):
    meta, _ = golden
    if which == "vga":
        img, intr = CC.frame(CC.motions()["both"][0]), CC.INTR
    else:
        img, intr = CC.odd_frame(), synth.intrinsics_for(CC.ODD_W, CC.ODD_H)
    v, keep = view_of(hip, img, intr=intr)
    trk = Tracker(hip)
    try:
        hip.check(hip.fn["colour_tracker_prepare"](trk.h, C.byref(v.struct()), CC.LEVELS, None), "prepare")
        ref = CC.numpy_pyramid(img, CC.LEVELS)
        for lv in range(CC.LEVELS):
            got = read_level(hip, trk, lv)
            for a, b in zip(got, ref[lv]):
                np.testing.assert_array_equal(a, b)
            assert [synth.sha256(x) for x in got] == meta[which + "_pyramid_sha256"][lv]
    finally:
        trk.close()


def evaluate(be, trk, cloud, level, pose, it, gh=True, stream=None):
    out = ColourEval()
    _, p = fp(pose)
    be.check(be.fn["colour_tracker_evaluate"](trk.h, level, cloud[0].ptr, cloud[1].ptr, cloud[2], p, it, int(gh), C.byref(out), stream),
             "evaluate")
    n = out.numPara
    return out.f, out.noValidPoints, np.array(out.nabla[:n]), np.array(out.hessian[:n * n])


@pytest.mark.gpu
def test_evaluation_vs_reference(hip, golden, cloud):
    """Per level x type (ROTATION, TRANSLATION, BOTH) at two poses: the count exact, f / gradient / Hessian within EVAL_TOL of
    the largest entry (sequential float sums of ~75 000 terms in the reference)."""
    _, g = golden
    v, keep = view_of(hip, CC.frame(CC.motions()["both"][0]))
    trk = Tracker(hip)
    worst = 0.0
    try:
        hip.check(hip.fn["colour_tracker_prepare"](trk.h, C.byref(v.struct()), CC.LEVELS, None), "prepare")
        k = 0
        for pose in CC.eval_poses().values():
            for lv in range(CC.LEVELS):
                for it in (1, 2, 3):
                    f, n, nab, hes = evaluate(hip, trk, cloud, lv, pose, it)
                    np_ = 3 if it == 1 else 6
                    assert n == g["eval_count"][k], (lv, it)
                    rf = abs(f - g["eval_f"][k]) / abs(g["eval_f"][k])
                    gn = g["eval_nabla"][k][:np_]; gh_ = g["eval_hessian"][k][:np_ * np_]
                    rn = np.abs(nab - gn).max() / np.abs(gn).max()
                    rh = np.abs(hes - gh_).max() / np.abs(gh_).max()
                    worst = max(worst, rf, rn, rh)
                    assert max(rf, rn, rh) < EVAL_TOL, (lv, it, rf, rn, rh)
                    f2, n2, _, _ = evaluate(hip, trk, cloud, lv, pose, it, gh=False)
                    assert (f2, n2) == (f, n)            # the fused pass returns the same cost as the cost-only pass
                    k += 1
    finally:
        trk.close()
    print("colour evaluation: worst relative difference", worst)


def track(be, trk, cloud, img, M_d, calib=None, regime=None, n=None, stream=None):
    v, keep = view_of(be, img, M_d=M_d, calib=calib)
    out = (C.c_float * 16)()
    cfg = config(regime)
    be.check(be.fn["colour_tracker_track_camera"](trk.h, C.byref(cfg), C.byref(v.struct()), None, cloud[0].ptr, cloud[1].ptr,
                                                  cloud[2] if n is None else n, out, stream), "track_camera")
    return np.array(out[:], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["t1cm", "yaw1", "both", "extrinsic", "translation_only"])
def test_track_camera_vs_reference(hip, golden, cloud, name):
    meta, _ = golden
    M_true, calib, regime = CC.motions()[name]
    trk = Tracker(hip)
    try:
        got = track(hip, trk, cloud, CC.frame(M_true, calib), CC.IDENTITY, calib=calib, regime=regime)
    finally:
        trk.close()
    want = np.array(meta["tracks"][name]["M_out"], np.float32)
    d = np.abs(got - want).max()
    print(f"colour track {name}: max |pose - reference| = {d:.2e}")
    assert d < POSE_TOL, (name, d)


@pytest.mark.gpu
def test_track_camera_recovers_the_motion(hip, cloud):
    """Independent of the reference: the rotation of a 1 degree yaw and the translation of a 1 cm move (translation-only
    regime) are recovered to well under 20 % of the motion.  (With rotation-only coarse levels, a sideways move on this
    distant, nearly planar scene is largely explained as a rotation -- the reference does the same -- so the translation is
    judged on the translation-only regime.)"""
    trk = Tracker(hip)
    try:
        M_true = CC.motions()["yaw1"][0]
        got = track(hip, trk, cloud, CC.frame(M_true), CC.IDENTITY)
        err = np.abs(CC.mat(got)[:3, :3] - CC.mat(M_true)[:3, :3]).max()
        assert err < 0.2 * np.deg2rad(1.0), err
        M_true = CC.motions()["translation_only"][0]
        got = track(hip, trk, cloud, CC.frame(M_true), CC.IDENTITY, regime=[2] * CC.LEVELS)
        err = np.abs(CC.mat(got)[:3, 3] - CC.mat(M_true)[:3, 3]).max()
        assert err < 0.2 * 0.01, err
    finally:
        trk.close()


@pytest.mark.gpu
def test_empty_point_cloud_returns_the_reference_pose(hip, golden, cloud):
    meta, _ = golden
    rec = meta["tracks"]["empty"]
    trk = Tracker(hip)
    try:
        got = track(hip, trk, cloud, CC.frame(CC.motions()["t1cm"][0]), np.array(rec["M_in"], np.float32), n=0)
        f, n, nab, hes = evaluate(hip, trk, (cloud[0], cloud[1], 0), 0, CC.IDENTITY, 3)
    finally:
        trk.close()
    assert n == 0 and f == np.float32(0x7f800000) and not nab.any()
    assert np.abs(got - np.array(rec["M_out"], np.float32)).max() < 1e-6


@pytest.mark.gpu
def test_bad_arguments_are_rejected(hip, cloud):
    trk = Tracker(hip)
    try:
        img = CC.frame(CC.motions()["t1cm"][0])
        v, keep = view_of(hip, img)
        out = (C.c_float * 16)()
        cfg = config([3, 3, 1, 1, 4])                     # NONE on the coarsest level
        assert hip.fn["colour_tracker_track_camera"](trk.h, C.byref(cfg), C.byref(v.struct()), None, cloud[0].ptr, cloud[1].ptr,
                                                     cloud[2], out, None) == capi.ERR_INVALID
        s = v.struct()
        s.rgb = None
        assert hip.fn["colour_tracker_track_camera"](trk.h, C.byref(config()), C.byref(s), None, cloud[0].ptr, cloud[1].ptr,
                                                     cloud[2], out, None) == capi.ERR_INVALID
        ev = ColourEval()
        _, p = fp(CC.IDENTITY)
        assert hip.fn["colour_tracker_evaluate"](trk.h, 0, cloud[0].ptr, cloud[1].ptr, cloud[2], p, 4, 1, C.byref(ev), None) == capi.ERR_INVALID
    finally:
        trk.close()


@pytest.mark.gpu
def test_two_handles_on_two_streams_match_sequential_runs(hip, cloud):
    names = ["both", "yaw1"]
    imgs = [CC.frame(CC.motions()[n][0]) for n in names]
    trks = [Tracker(hip), Tracker(hip)]
    streams = [C.c_void_p(), C.c_void_p()]
    try:
        seq = [track(hip, trks[0], cloud, im, CC.IDENTITY) for im in imgs]
        for s in streams:
            hip.check(hip.fn["stream_create"](C.byref(s)), "stream_create")
        res = [None, None]
        start = threading.Barrier(2)

        def run(i):
            start.wait()
            res[i] = track(hip, trks[i], cloud, imgs[i], CC.IDENTITY, stream=streams[i])
        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for a, b in zip(seq, res):
            np.testing.assert_array_equal(a, b)
    finally:
        for t in trks:
            t.close()
        for s in streams:
            if s:
                hip.fn["stream_destroy"](s)
