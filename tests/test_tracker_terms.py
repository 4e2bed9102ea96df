"""The four tracker evaluation kernels -- ICP, weighted ICP, colour and Ren -- against a float64 restatement of the same
per-residual float terms (tests/tracker_terms.py).

The kernels form every residual's terms in float with the reference's operations and add each term
in double (gh_reduce.h: per lane, DPP row shifts, waves, workgroups, segments -- a fixed order).  Their target is therefore not
the reference's sequential float sum but the exact sum of the same float terms, `sum64`, and each element is held to its own
scale -- never to a fraction of the largest entry:

  * CPU: the restatement is pinned to the reference first.  Its sequential float32 sum `seq32` equals, bit for bit, the oracle's
    tracker_compute_g_and_h (itself bit-exact with the reference) on the fused 160 x 120 scene, a ragged fused scene and synthetic
    maps with holes, in all three modes; the reference's recorded weighted ICP evaluations (tests/golden/g_wicp_tracker.npz, all
    42); the reference's recorded colour evaluations (tests/golden/g_colour_tracker.npz, all 30); and the reference's recorded Ren
    evaluations (tests/golden/g_ren_tracker.npz, all 16, on the oracle's fused voxels, whose digests match the golden's), with the
    host libm's expf -- numpy's float32 exp differs from it by an ulp on many arguments.
  * GPU: the count is exact, and every gradient / Hessian element k satisfies

        |got[k] - sum64[k]| <= ulp32(sum64[k]) + n 2^-52 A[k],        A[k] = sum_i |t[i, k]|

    -- the rounding of the final double -> float conversion (half an ulp, one allowed) plus a bound of the error of any order of n
    double additions of float terms (each addition errs by at most 2^-53 of the running magnitude, which never exceeds A[k]).
    ICP f = sqrt((float)S0) / n goes through a square root and a division: 2 ulp of the restated f.  The colour outputs are
    (float)S times the occlusion scale sc = total / valid (one more float rounding): the bound is sc times the one above plus
    ulp32(sc sum64[k]).  Elements outside the active block (the gradient beyond the mode's parameters, the Hessian outside its
    np x np block) are exactly 0.
    Ren: the device's expf is not the host libm's (it may differ by about an ulp), and an ulp in exp(-6 dt) moves a term by a
    few ulp of the largest intermediate of its formula (the Jacobian prefix is a difference of two such quantities), so the
    reordering term gives way to REN_C 2^-24 A[k] with REN_C = 16; f = -(float)S0.

    Measured worst ratio |got - sum64| / bound on an MI355X (each GPU test prints its own): 0.500 on every tiling (ICP and
    weighted ICP), 0.495 for the counts and edges, 0.499 on the fused scenes, 0.468 for the colour evaluations -- the kernels
    round their double sums to the nearest float, and their reordering error stays far below the rounding of the result.
    Ren (bound with REN_C = 16): 0.843 on hash_s, dense_s and the paged mirror, 0.389 on hash_f_rgb.
"""
import ctypes as C

import numpy as np
import pytest

import colour_cases as CC
import itm_testlib as T
import tracker_terms as TT
import wicp_cases as WC
from infinitam_amd import capi, synth
from infinitam_amd.capi import ColourEval, TrackerGH
from itm_testlib import Scenario

F = np.float32
EPS52 = 2.0 ** -52


def fptr(a):
    return np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64).astype(F))).astype(np.float64)


# ---- synthetic ICP scenes: a tilted plane and a sphere, ray cast analytically, with holes -------------------------------------
SPHERE_C, SPHERE_R = np.array([0.06, -0.03, 1.0]), 0.22
PLANE_N = np.array([0.25, 0.15, -1.0]) / np.linalg.norm([0.25, 0.15, -1.0])
PLANE_D = -1.5                                                         # n . X = d


def rigid(yaw, pitch, t):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M


def col(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).T.reshape(16), np.float32)


def intr_for(w, h, fov_scale=1.0):
    f = 0.9 * max(w, h) * fov_scale
    return np.array([f, f, (w - 1) / 2.0, (h - 1) / 2.0], np.float32)


def ray_cast(cam_to_world, intr, w, h):
    """world points, world normals and camera depth of the plane + sphere seen by a pinhole camera (float64)"""
    fx, fy, cx, cy = [float(v) for v in intr]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    d_cam = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1)
    R, o = cam_to_world[:3, :3], cam_to_world[:3, 3]
    dw = d_cam @ R.T
    tp = (PLANE_D - o @ PLANE_N) / (dw @ PLANE_N)
    oc = o - SPHERE_C
    b = dw @ oc
    a = (dw * dw).sum(-1)
    disc = b * b - a * (oc @ oc - SPHERE_R ** 2)
    ts = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
    use_s = (ts > 0) & (ts < np.where(tp > 0, tp, np.inf))
    t = np.where(use_s, ts, np.where(tp > 0, tp, np.nan))
    X = o + dw * t[..., None]
    N = np.where(use_s[..., None], (X - SPHERE_C) / SPHERE_R, np.broadcast_to(-PLANE_N, X.shape))
    return X, N, t


class Synth:
    """A scene map (points, normals in world coordinates, w = 1 / holes w = -1) of sceneW x sceneH at scene pose `scene_pose`
    (world -> camera), and depth images of other sizes from a nearby camera."""

    def __init__(self, scene_w, scene_h, seed=0, holes=0.03):
        rng = np.random.default_rng(seed)
        self.sw, self.sh = scene_w, scene_h
        self.s_intr = intr_for(scene_w, scene_h, 0.6)                  # wider field of view than the views
        self.cam = rigid(0.03, -0.02, (0.01, 0.005, -0.02))            # scene camera -> world
        X, N, t = ray_cast(self.cam, self.s_intr, scene_w, scene_h)
        ok = np.isfinite(t)
        pts = np.zeros((scene_h, scene_w, 4), F)
        nrm = np.zeros((scene_h, scene_w, 4), F)
        pts[..., :3] = np.where(ok[..., None], X, 0)
        pts[..., 3] = np.where(ok, 1.0, -1.0)
        nrm[..., :3] = np.where(ok[..., None], N, 0)
        nrm[..., 3] = np.where(ok, 1.0, -1.0)
        pts[rng.random((scene_h, scene_w)) < holes, 3] = -1.0
        nrm[rng.random((scene_h, scene_w)) < holes, 3] = -1.0          # a normal hole without a point hole: zero normal, counts
        self.points, self.normals = pts, nrm
        self.scene_pose = col(np.linalg.inv(self.cam))

    def view(self, w, h, seed=1, holes=0.04, outliers=0.02):
        """(depth, view intrinsics, approxInvPose) of a camera near the scene camera; depth with 0 / negative holes and outliers"""
        rng = np.random.default_rng(seed)
        cam = rigid(0.02, -0.01, (0.02, 0.0, -0.01))
        intr = intr_for(w, h)
        _, _, t = ray_cast(cam, intr, w, h)
        depth = np.where(np.isfinite(t), t, 0.0) * (1.0 + 0.002 * rng.standard_normal((h, w)))
        r = rng.random((h, w))
        depth[r < holes / 2] = 0.0
        depth[(r >= holes / 2) & (r < holes)] = -1.0
        depth[(r >= holes) & (r < holes + outliers)] *= 1.3
        approx = rigid(0.023, -0.012, (0.021, -0.002, -0.012))          # a slightly wrong estimate of `cam`
        return np.ascontiguousarray(depth, F), intr, col(approx)


def sigma_image(shape, seed=2):
    """sigmaZ-like weights: mostly positive, with 0 (border), -1 (no normal), tiny and huge sigma"""
    rng = np.random.default_rng(seed)
    s = (0.001 + 0.004 * rng.random(shape)).astype(F)
    r = rng.random(shape)
    s[r < 0.05] = 0.0
    s[(r >= 0.05) & (r < 0.1)] = -1.0
    s[(r >= 0.1) & (r < 0.12)] = 1e-6
    s[(r >= 0.12) & (r < 0.14)] = 1e30
    return s


# ---- checks ---------------------------------------------------------------------------------------------------------------------
def icp_bound_check(got, terms, what):
    """got = (n, f, nabla[6], hessian[36]) of an ICP / weighted ICP evaluation; returns the worst ratio to the bound"""
    n, f, nabla, hessian = got
    assert n == terms.n, (what, n, terms.n)
    np_ = terms.np_
    s64, A = terms.sum64, terms.A
    if n > 100:
        f_ref = TT.icp_f(s64[0], n)
        assert abs(float(f) - float(f_ref)) <= 2 * ulp32(f_ref), (what, f, f_ref)
    else:
        assert f == F(1e5), (what, f)
    H = np.asarray(hessian, F).reshape(6, 6)                      # hessian[r + c * 6]: H[c, r]
    outside = np.ones((6, 6), bool)
    outside[:np_, :np_] = False
    assert not np.asarray(nabla, F)[np_:].any() and not H[outside].any(), what
    assert np.array_equal(H, H.T), what
    vals = TT.pack(nabla, hessian, np_)
    worst = 0.0
    for k in TT.active(np_)[1:]:
        g = vals[k - 1]
        bound = ulp32(s64[k]) + n * EPS52 * A[k]
        err = abs(g - s64[k])
        assert err <= bound, (what, k, g, s64[k], err, bound)
        worst = max(worst, err / bound)
    return worst


class Icp:
    """the product's ICP / weighted ICP evaluation: through a tracker handle or the handle-less entry point"""

    def __init__(self, hip):
        self.hip = hip
        self.h = C.c_void_p()
        hip.check(hip.fn["tracker_create"](C.byref(self.h)), "tracker_create")

    def close(self):
        self.hip.check(self.hip.fn["tracker_destroy"](self.h), "tracker_destroy")

    def __call__(self, depth, w, h, v_intr, points, normals, sw, sh, s_intr, inv, scene_pose, dist, mode, weight=None, handle=True):
        out = TrackerGH()
        if weight is not None:
            self.hip.check(self.hip.fn["tracker_weighted_g_and_h"](self.h, depth.ptr, weight.ptr, w, h, fptr(v_intr), points.ptr, normals.ptr,
                                                                   sw, sh, fptr(s_intr), fptr(inv), fptr(scene_pose), dist, mode,
                                                                   C.byref(out), None), "tracker_weighted_g_and_h")
        elif handle:
            self.hip.check(self.hip.fn["tracker_g_and_h"](self.h, depth.ptr, w, h, fptr(v_intr), points.ptr, normals.ptr, sw, sh,
                                                          fptr(s_intr), fptr(inv), fptr(scene_pose), dist, mode, C.byref(out), None),
                           "tracker_g_and_h")
        else:
            self.hip.check(self.hip.fn["tracker_compute_g_and_h"](depth.ptr, w, h, fptr(v_intr), points.ptr, normals.ptr, sw, sh,
                                                                  fptr(s_intr), fptr(inv), fptr(scene_pose), dist, mode, C.byref(out), None),
                           "tracker_compute_g_and_h")
        return out.noValidPoints, out.f, np.array(out.nabla[:], F), np.array(out.hessian[:], F)


def gh_tiling(w, h, limit=96):
    """tracker.hip gh_tiling with the per-launch limit: (tileH, tiles, workgroups)"""
    tiles_x = (w + 15) // 16
    tile_h = 4
    while tile_h < 16 and tiles_x * ((h + tile_h - 1) // tile_h) > limit:
        tile_h *= 2
    tiles = tiles_x * ((h + tile_h - 1) // tile_h)
    rounds = (tiles + 255) // 256
    return tile_h, tiles, (tiles + rounds - 1) // rounds


def oracle_g_and_h(oracle, depth, v_intr, points, normals, s_intr, inv, scene_pose, dist, mode):
    h, w = depth.shape
    sh, sw = points.shape[:2]
    d, p, nm = oracle.to_backend(depth), oracle.to_backend(points), oracle.to_backend(normals)
    out = TrackerGH()
    oracle.check(oracle.fn["tracker_compute_g_and_h"](d.ptr, w, h, fptr(v_intr), p.ptr, nm.ptr, sw, sh, fptr(s_intr), fptr(inv),
                                                      fptr(scene_pose), dist, mode, C.byref(out), None), "tracker_compute_g_and_h")
    return out.noValidPoints, F(out.f), np.array(out.nabla[:], F), np.array(out.hessian[:], F).reshape(6, 6)


def assert_seq32_equal(got, terms, what):
    n, f, g, H = TT.icp_seq32(terms)
    assert got[0] == n, (what, got[0], n)
    assert got[1] == f, (what, got[1], f)
    assert np.array_equal(got[2], g), what
    assert np.array_equal(got[3].reshape(6, 6), H), what


# ---- CPU: the restatements against the oracle and the reference's recordings ----------------------------------------------------
@pytest.fixture(scope="module")
def fused_icp():
    """the fused 160 x 120 scene of tests/test_tracker.py and a ragged one: (points, normals, M_d, next depth, intrinsics)"""
    oracle = T.oracle_backend()
    out = {}
    for sc in (Scenario(name="trk", w=160, h=120, voxelSize=0.01, frames=3),
               Scenario(name="trk_ragged_200x152", voxelSize=0.01, frames=3, stream=3, trajectory="yaw", w=200, h=152)):
        ses = T.Session(oracle, sc)
        try:
            for k in range(sc.frames):
                v = ses.frame(k)
            out[sc.name] = (ses.points.numpy().reshape(sc.h, sc.w, 4), ses.normals.numpy().reshape(sc.h, sc.w, 4),
                            np.asarray(v.M_d, F), np.ascontiguousarray(sc.depth(sc.frames), F), np.asarray(sc.intr(), F))
        finally:
            ses.close()
    return out


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_icp_restatement_equals_the_oracle_bit_for_bit(fused_icp, mode):
    oracle = T.oracle_backend()
    for name, (pts, nrm, M_d, depth, intr) in fused_icp.items():
        inv = col(np.linalg.inv(np.asarray(M_d, np.float64).reshape(4, 4).T))
        for dist in (0.01, 0.0005):
            terms = TT.icp_terms(depth, pts, nrm, intr, intr, inv, M_d, dist, mode)
            assert terms.n > 100
            assert_seq32_equal(oracle_g_and_h(oracle, depth, intr, pts, nrm, intr, inv, M_d, dist, mode), terms, (name, dist))
    # synthetic maps with point holes, normal holes, depth holes and outliers, scene and view of different sizes
    s = Synth(97, 71)
    for (w, h) in ((33, 65), (161, 121)):
        depth, v_intr, inv = s.view(w, h)
        for dist in (0.01, 0.0002):
            terms = TT.icp_terms(depth, s.points, s.normals, v_intr, s.s_intr, inv, s.scene_pose, dist, mode)
            got = oracle_g_and_h(oracle, depth, v_intr, s.points, s.normals, s.s_intr, inv, s.scene_pose, dist, mode)
            assert_seq32_equal(got, terms, ("synth", w, h, dist))


@pytest.fixture(scope="module")
def wicp_inputs():
    oracle = T.oracle_backend()
    return {name: WC.build(oracle, sc) for name, sc in list(WC.SCENES.items()) + [("vga", WC.SCENE_VGA)]}


@pytest.fixture(scope="module")
def wicp_golden():
    import json
    import os
    path = os.path.join(T.ROOT, "tests", "golden", "g_wicp_tracker")
    with open(path + ".json") as f:
        meta = json.load(f)
    z = np.load(path + ".npz")
    return meta, {k: z[k] for k in z.files}


def wicp_cases_of(meta, g, inputs):
    """every recorded weighted ICP evaluation: (name, i, level depth, level sigma, level intrinsics, scene, inputs, inv, dist, mode)"""
    for name, inp in inputs.items():
        sc = WC.SCENE_VGA if name == "vga" else WC.SCENES[name]
        levels = 1 if name == "vga" else WC.LEVELS
        m = meta["scenes"][name]
        dp, wp = WC.numpy_pyramid(inp[3], levels), WC.numpy_pyramid(inp[4], levels)
        for i in range(len(g[f"{name}_eval_level"])):
            l, mode = int(g[f"{name}_eval_level"][i]), int(g[f"{name}_eval_mode"][i])
            intr = np.array(sc.intr(), F) * F(0.5 ** l)
            yield name, i, dp[l], wp[l], intr, sc, inp, g[f"{name}_eval_inv"][i], m["eval_dist"][i], mode


def test_wicp_restatement_equals_the_reference_recordings(wicp_golden, wicp_inputs):
    meta, g = wicp_golden
    for name, inp in wicp_inputs.items():
        assert WC.digests(inp) == meta["scenes"][name]["inputs_sha256"], name
    count = 0
    for name, i, depth, sigma, intr, sc, inp, inv, dist, mode in wicp_cases_of(meta, g, wicp_inputs):
        points, normals, M_d = inp[0].reshape(sc.h, sc.w, 4), inp[1].reshape(sc.h, sc.w, 4), inp[2]
        terms = TT.icp_terms(depth, points, normals, intr, sc.intr(), inv, M_d, dist, mode, weight=sigma)
        want = (g[f"{name}_eval_count"][i], g[f"{name}_eval_f"][i], g[f"{name}_eval_nabla"][i], g[f"{name}_eval_hessian"][i])
        assert_seq32_equal(want, terms, (name, i))
        count += 1
    assert count == 42


def test_colour_restatement_equals_the_reference_recordings():
    import json
    import os
    path = os.path.join(T.ROOT, "tests", "golden", "g_colour_tracker")
    with open(path + ".json") as f:
        meta = json.load(f)
    z = np.load(path + ".npz")
    loc, colours = CC.cloud()
    img = CC.frame(CC.motions()["both"][0])
    assert [synth.sha256(loc), synth.sha256(colours)] == meta["cloud_sha256"]
    assert synth.sha256(img) == meta["vga_frame_sha256"]
    pyr = CC.numpy_pyramid(img, CC.LEVELS)
    k = 0
    for pose in CC.eval_poses().values():
        for lv in range(CC.LEVELS):
            for it in (1, 2, 3):
                terms = TT.colour_terms(loc, colours, *pyr[lv], level_intr(CC.INTR, lv), pose, it)
                f, n, nab, hes = TT.colour_seq32(terms, loc.shape[0])
                np_ = terms.np_
                assert n == z["eval_count"][k] and f == z["eval_f"][k], (lv, it)
                assert np.array_equal(nab, z["eval_nabla"][k][:np_]) and np.array_equal(hes, z["eval_hessian"][k][:np_ * np_]), (lv, it)
                k += 1
    assert k == 30


def level_intr(intr, lv):
    """the level's intrinsics as the colour tracker forms them: intr / (float)(1 << level)"""
    return [F(v) / F(1 << lv) for v in intr]


def test_restatement_edges_on_the_cpu():
    """the hole rules of the ICP restatement on constructed pixels (identity poses, unit view intrinsics: u = -vcx exactly)"""
    sw, sh = 9, 7
    pts, nrm = edge_maps(sw, sh)
    for vcx, vcy, want in edge_cases(sw, sh):
        terms = TT.icp_terms(np.ones((1, 1), F), pts, nrm, (1, 1, vcx, vcy), (1, 1, 0, 0), EYE, EYE, 10.0, 3)
        assert terms.n == want, (vcx, vcy)


# ---- constructed edges ----------------------------------------------------------------------------------------------------------
EYE = np.eye(4, dtype=F).reshape(16)


def edge_maps(sw, sh, seed=5):
    """a scene map in the 'unit' camera (identity pose, fx = fy = 1, cx = cy = 0): point (x, y, 1) + noise at pixel (x, y)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:sh, 0:sw].astype(F)
    pts = np.stack([xs, ys, np.ones_like(xs), np.ones_like(xs)], -1).astype(F)
    pts[..., :3] += (0.01 * rng.standard_normal((sh, sw, 3))).astype(F)
    nrm = np.zeros_like(pts)
    nrm[..., :3] = rng.standard_normal((sh, sw, 3)).astype(F)
    nrm[..., 3] = 1.0
    return pts, nrm


def edge_cases(sw, sh):
    """(vcx, vcy, expected count) of a 1 x 1 depth image of depth 1 at pixel (0, 0): u = -vcx, v = -vcy exactly"""
    up = lambda a: F(np.nextafter(F(a), F(np.inf)))
    mid = F(-(sh // 2) - 0.25)
    return [(F(-(sw - 2)), mid, 1), (-up(sw - 2), mid, 0),             # u = sceneW - 2 (inclusive) and one float step beyond
            (F(-2.5), F(-(sh - 2)), 1), (F(-2.5), -up(sh - 2), 0),     # v = sceneH - 2 and beyond
            (F(0), F(0), 1), (F(np.nextafter(F(0), F(1))), mid, 0),    # u = 0 exactly and just below
            (F(-1.5), F(np.nextafter(F(0), F(1))), 0)]                 # v just below 0


# ---- GPU: ICP and weighted ICP --------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 2), (15, 3), (16, 4), (17, 5), (33, 65), (79, 59), (161, 61), (161, 121), (319, 239), (640, 480), (1280, 960)]


def test_shapes_cover_the_tilings():
    """every tile height of gh_tiling, the B-tile tail (tiles not a multiple of twice the workgroups) and grids above 96"""
    t = [gh_tiling(w, h) for w, h in SHAPES]
    assert {th for th, _, _ in t} == {4, 8, 16}
    assert any(tiles % (2 * g) for _, tiles, g in t)
    assert any(g > 96 for _, _, g in t)


@pytest.fixture(scope="module")
def synth_scene():
    return Synth(211, 157)            # scene map of its own ragged size


def device_maps(hip, s):
    return hip.to_backend(s.points), hip.to_backend(s.normals)


@pytest.mark.gpu
def test_icp_and_wicp_on_every_tiling(hip, synth_scene):
    s = synth_scene
    pts, nrm = device_maps(hip, s)
    icp = Icp(hip)
    worst = 0.0
    try:
        for (w, h) in SHAPES:
            depth, v_intr, inv = s.view(w, h, seed=w * 1000 + h)
            sigma = sigma_image((h, w), seed=w + h)
            d_dev, s_dev = hip.to_backend(depth), hip.to_backend(sigma)
            big = w * h > 400_000
            for mode in ((3,) if big else (1, 2, 3)):
                for dist in (0.01,) if big else (0.01, 0.0003):
                    terms = TT.icp_terms(depth, s.points, s.normals, v_intr, s.s_intr, inv, s.scene_pose, dist, mode)
                    for handle in (True, False):
                        got = icp(d_dev, w, h, v_intr, pts, nrm, s.sw, s.sh, s.s_intr, inv, s.scene_pose, dist, mode, handle=handle)
                        worst = max(worst, icp_bound_check(got, terms, ("icp", w, h, mode, dist, handle)))
                    wt = TT.icp_terms(depth, s.points, s.normals, v_intr, s.s_intr, inv, s.scene_pose, dist, mode, weight=sigma)
                    got = icp(d_dev, w, h, v_intr, pts, nrm, s.sw, s.sh, s.s_intr, inv, s.scene_pose, dist, mode, weight=s_dev)
                    worst = max(worst, icp_bound_check(got, wt, ("wicp", w, h, mode, dist)))
            if w * h >= 1000:
                assert terms.n > 0.5 * w * h, (w, h, terms.n)          # the scene is mostly valid, holes and outliers included
    finally:
        icp.close()
    print(f"icp / wicp on every tiling: worst ratio {worst:.3f}")


@pytest.mark.gpu
def test_one_valid_pixel_at_a_time(hip):
    """33 x 17 (15 tiles of 16 x 4): every pixel alone; and the corners and the first / last pixel of the last tile of two large
    shapes: count 1, f = 1e5, nabla and Hessian exactly that pixel's float terms -- a dropped or doubled tile cannot hide."""
    s = Synth(211, 157, holes=0.0)
    pts, nrm = device_maps(hip, s)
    icp = Icp(hip)
    try:
        cases = []
        full, v_intr, inv = s.view(33, 17, seed=7, holes=0.0, outliers=0.0)
        cases += [(full, v_intr, inv, (x, y)) for y in range(17) for x in range(33)]
        for (w, h) in ((319, 239), (1280, 960)):
            full_b, vi, ib = s.view(w, h, seed=8, holes=0.0, outliers=0.0)
            th, _, _ = gh_tiling(w, h)
            tx0, ty0 = ((w + 15) // 16 - 1) * 16, ((h + th - 1) // th - 1) * th
            pix = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (tx0, ty0), (tx0 + 3, h - 1)}
            cases += [(full_b, vi, ib, p) for p in sorted(pix)]
        checked = 0
        for full, v_intr, inv, (x, y) in cases:
            h, w = full.shape
            depth = np.zeros_like(full)
            depth[y, x] = full[y, x]
            sigma = np.full_like(full, 0.002)
            for mode, weight in ((3, None), (1, sigma), (2, None)):
                terms = TT.icp_terms(depth, s.points, s.normals, v_intr, s.s_intr, inv, s.scene_pose, 0.01, mode, weight=weight)
                got = icp(hip.to_backend(depth), w, h, v_intr, pts, nrm, s.sw, s.sh, s.s_intr, inv, s.scene_pose, 0.01, mode,
                          weight=None if weight is None else hip.to_backend(weight))
                if terms.n == 0 and w == 33:                      # a residual beyond distThresh: rejected, nothing added
                    assert got[0] == 0 and got[1] == F(1e5) and not got[2].any() and not got[3].any(), (x, y)
                    continue
                assert terms.n == 1, (x, y, w, h)
                assert got[0] == 1 and got[1] == F(1e5), (x, y, w, h, got[:2])
                want = TT.unpack_hessian(terms.t[0], terms.np_)
                assert np.array_equal(got[2], TT.unpack_nabla(terms.t[0], terms.np_)), (x, y, w, h, mode)
                assert np.array_equal(got[3].reshape(6, 6), want), (x, y, w, h, mode)
                checked += 1
        assert checked >= 0.95 * 3 * len(cases), checked         # (nearly) every pixel of the view sees the scene
    finally:
        icp.close()


@pytest.mark.gpu
def test_counts_100_and_101_and_the_edges(hip, synth_scene):
    s = synth_scene
    pts, nrm = device_maps(hip, s)
    icp = Icp(hip)
    worst = 0.0
    try:
        full, v_intr, inv = s.view(79, 59, seed=9, holes=0.0, outliers=0.0)
        terms = TT.icp_terms(full, s.points, s.normals, v_intr, s.s_intr, inv, s.scene_pose, 0.01, 3)
        order = np.flatnonzero(terms.valid)
        for keep in (100, 101):
            depth = np.zeros(full.size, F)
            depth[order[:keep]] = full.reshape(-1)[order[:keep]]
            depth = depth.reshape(full.shape)
            t = TT.icp_terms(depth, s.points, s.normals, v_intr, s.s_intr, inv, s.scene_pose, 0.01, 3)
            assert t.n == keep
            got = icp(hip.to_backend(depth), 79, 59, v_intr, pts, nrm, s.sw, s.sh, s.s_intr, inv, s.scene_pose, 0.01, 3)
            worst = max(worst, icp_bound_check(got, t, ("count", keep)))
            assert (got[1] == F(1e5)) == (keep == 100)
        # dist == distThresh counts, one float step less does not
        one = np.zeros_like(full)
        i = order[len(order) // 2]
        one.reshape(-1)[i] = full.reshape(-1)[i]
        t = TT.icp_terms(one, s.points, s.normals, v_intr, s.s_intr, inv, s.scene_pose, 0.01, 3)
        dist = F(t.extra["dist"][0])
        d_dev = hip.to_backend(one)
        for thr, want in ((dist, 1), (F(np.nextafter(dist, F(0))), 0)):
            t = TT.icp_terms(one, s.points, s.normals, v_intr, s.s_intr, inv, s.scene_pose, float(thr), 3)
            assert t.n == want
            got = icp(d_dev, 79, 59, v_intr, pts, nrm, s.sw, s.sh, s.s_intr, inv, s.scene_pose, float(thr), 3)
            assert got[0] == want, (thr, got[0])
        # u = sceneW - 2 / v = sceneH - 2 inclusive, one float step beyond, u = 0 and just below
        sw, sh = 9, 7
        e_pts, e_nrm = edge_maps(sw, sh)
        ep, en = hip.to_backend(e_pts), hip.to_backend(e_nrm)
        d1 = hip.to_backend(np.ones((1, 1), F))
        for vcx, vcy, want in edge_cases(sw, sh):
            for mode in (1, 2, 3):
                t = TT.icp_terms(np.ones((1, 1), F), e_pts, e_nrm, (1, 1, vcx, vcy), (1, 1, 0, 0), EYE, EYE, 10.0, mode)
                assert t.n == want
                got = icp(d1, 1, 1, np.array([1, 1, vcx, vcy], F), ep, en, sw, sh, np.array([1, 1, 0, 0], F), EYE, EYE, 10.0, mode)
                worst = max(worst, icp_bound_check(got, t, ("edge", vcx, vcy, mode)))
    finally:
        icp.close()
    print(f"counts and edges: worst ratio {worst:.3f}")


@pytest.mark.gpu
def test_fused_scenes_at_the_recorded_poses(hip, wicp_golden, wicp_inputs):
    """every recorded weighted ICP evaluation (frontal, off axis, 640 x 480) weighted and unweighted, and the 640 x 480 ICP scene of
    tests/test_tracker.py at its last pose"""
    meta, g = wicp_golden
    icp = Icp(hip)
    worst = 0.0
    dev = {}
    try:
        for name, i, depth, sigma, intr, sc, inp, inv, dist, mode in wicp_cases_of(meta, g, wicp_inputs):
            if name not in dev:
                dev[name] = (hip.to_backend(inp[0]), hip.to_backend(inp[1]))
            h, w = depth.shape
            d_dev, s_dev = hip.to_backend(depth), hip.to_backend(sigma)
            points, normals, M_d = inp[0].reshape(sc.h, sc.w, 4), inp[1].reshape(sc.h, sc.w, 4), inp[2]
            for weight in (sigma, None):
                terms = TT.icp_terms(depth, points, normals, intr, sc.intr(), inv, M_d, dist, mode, weight=weight)
                got = icp(d_dev, w, h, intr, *dev[name], sc.w, sc.h, sc.intr(), inv, M_d, dist, mode,
                          weight=None if weight is None else s_dev)
                worst = max(worst, icp_bound_check(got, terms, (name, i, weight is None)))
        oracle = T.oracle_backend()
        sc = Scenario(name="trk_vga", voxelSize=0.01, frames=3)
        ses = T.Session(oracle, sc)
        try:
            for k in range(sc.frames):
                v = ses.frame(k)
            points, normals = ses.points.numpy().reshape(sc.h, sc.w, 4), ses.normals.numpy().reshape(sc.h, sc.w, 4)
        finally:
            ses.close()
        depth = np.ascontiguousarray(sc.depth(sc.frames), F)
        M_d = np.asarray(v.M_d, F)
        inv = col(np.linalg.inv(np.asarray(M_d, np.float64).reshape(4, 4).T))
        p_dev, n_dev, d_dev = hip.to_backend(points), hip.to_backend(normals), hip.to_backend(depth)
        for mode in (1, 2, 3):
            terms = TT.icp_terms(depth, points, normals, sc.intr(), sc.intr(), inv, M_d, 0.01, mode)
            got = icp(d_dev, sc.w, sc.h, np.asarray(sc.intr(), F), p_dev, n_dev, sc.w, sc.h, np.asarray(sc.intr(), F), inv, M_d, 0.01, mode)
            worst = max(worst, icp_bound_check(got, terms, ("vga", mode)))
    finally:
        icp.close()
    print(f"fused scenes: worst ratio {worst:.3f}")


# ---- GPU: colour ----------------------------------------------------------------------------------------------------------------
class Colour:
    def __init__(self, hip):
        self.hip = hip
        self.h = C.c_void_p()
        hip.check(hip.fn["colour_tracker_create"](C.byref(self.h)), "colour_tracker_create")

    def close(self):
        self.hip.check(self.hip.fn["colour_tracker_destroy"](self.h), "colour_tracker_destroy")

    def prepare(self, img, levels, intr):
        h, w = img.shape[:2]
        intr = tuple(float(v) for v in intr)
        self.keep = (self.hip.to_backend(np.ascontiguousarray(img)), self.hip.to_backend(np.zeros((h, w), F)))
        v = capi.View(self.keep[1], w, h, M_d=EYE, intr_d=intr, rgb=self.keep[0], w_rgb=w, h_rgb=h, intr_rgb=intr,
                      rgb_to_depth=EYE, rgb_to_depth_inv=EYE)
        self.hip.check(self.hip.fn["colour_tracker_prepare"](self.h, C.byref(v.struct()), levels, None), "colour_tracker_prepare")

    def read_level(self, lv):
        w, h = C.c_int(), C.c_int()
        self.hip.check(self.hip.fn["colour_tracker_read_level"](self.h, lv, None, None, None, C.byref(w), C.byref(h), None), "read_level")
        rgb = np.zeros((h.value, w.value, 4), np.uint8)
        gx = np.zeros((h.value, w.value, 4), np.int16)
        gy = np.zeros_like(gx)
        self.hip.check(self.hip.fn["colour_tracker_read_level"](self.h, lv, rgb.ctypes.data_as(C.c_void_p), gx.ctypes.data_as(C.c_void_p),
                                                                gy.ctypes.data_as(C.c_void_p), C.byref(w), C.byref(h), None), "read_level")
        return rgb, gx, gy

    def evaluate(self, lv, loc, colours, n, pose, mode, gh=True):
        out = ColourEval()
        self.hip.check(self.hip.fn["colour_tracker_evaluate"](self.h, lv, loc.ptr, colours.ptr, n, fptr(pose), mode, int(gh), C.byref(out),
                                                              None), "colour_tracker_evaluate")
        np_ = out.numPara
        return F(out.f), out.noValidPoints, np_, np.array(out.nabla[:], F), np.array(out.hessian[:], F)


def colour_bound_check(got, terms, total, what, gh=True):
    f, n, np_, nabla, hessian = got
    assert n == terms.n, (what, n, terms.n)
    assert np_ == terms.np_, what
    s64, A = terms.sum64, terms.A
    if n == 0:
        assert f == TT.MY_INF and not nabla.any() and not hessian.any(), what
        return 0.0
    sc = float(TT.colour_scale(total, n))
    vals = np.zeros(TT.KV)
    vals[0] = f
    if gh:
        vals[1:] = TT.pack(nabla, hessian, np_, ld=np_)
        assert not nabla[np_:].any() and not hessian[np_ * np_:].any(), what
        Hm = hessian[:np_ * np_].reshape(np_, np_)
        assert np.array_equal(Hm, Hm.T), what
    worst = 0.0
    for k in (TT.active(np_) if gh else [0]):
        target = s64[k] * sc
        bound = (ulp32(s64[k]) + n * EPS52 * A[k]) * sc + ulp32(target)
        err = abs(vals[k] - target)
        assert err <= bound, (what, k, vals[k], target, err, bound)
        worst = max(worst, err / bound)
    return worst


def random_image(w, h, seed):
    """a smooth random colour image (gradients of every size) with alpha 255, a block of alpha 200 and scattered 253"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 4), np.uint8)
    for c in range(3):
        a, b, p = rng.uniform(0.01, 0.2, 2).tolist() + [rng.uniform(0, 6)]
        v = 127 + 90 * np.sin(a * xs + p) * np.cos(b * ys) + rng.integers(-20, 20, (h, w))
        img[..., c] = np.clip(v, 0, 255).astype(np.uint8)
    img[..., 3] = 255
    img[h // 3:h // 2, w // 4:w // 3, 3] = 200
    img[rng.random((h, w)) < 0.01, 3] = 253
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("size,levels", [((1021, 767), 6), ((1021, 767), 7), ((1021, 767), 8), ((161, 121), 6), ((161, 121), 7)],
                         ids=lambda v: str(v))
def test_colour_pyramid_deep_levels_bit_exact(hip, size, levels):
    """six to eight levels: the second pyramid launch (levels 6-8, first = 4) included"""
    w, h = size
    img = random_image(w, h, seed=w + levels)
    trk = Colour(hip)
    try:
        trk.prepare(img, levels, intr_for(w, h))
        want = CC.numpy_pyramid(img, levels)
        for lv in range(levels):
            got = trk.read_level(lv)
            for a, b in zip(got, want[lv]):
                np.testing.assert_array_equal(a, b, err_msg=f"level {lv}")
    finally:
        trk.close()


def colour_cloud(n, w, h, intr, seed):
    """n points that the identity rgb pose projects mostly inside a w x h image (some outside, some behind: cz <= 0)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = [float(v) for v in intr]
    u = rng.uniform(-0.05 * w, 1.05 * w, n)
    v = rng.uniform(-0.05 * h, 1.05 * h, n)
    z = rng.uniform(0.5, 2.0, n)
    z[rng.random(n) < 0.02] *= -1.0
    loc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z, np.ones(n)], -1).astype(F)
    colours = np.concatenate([rng.random((n, 3)), np.ones((n, 1))], -1).astype(F)
    return loc, colours


def edge_points(w, h, intr):
    """(points, expected valid) that the identity pose projects (cz = 1) exactly onto u = 0, u = W-1, v = H-1 (valid), onto the
    first reachable float position outside each of these edges (invalid), and points with cz <= 0 (invalid)"""
    fx, fy, cx, cy = [F(v) for v in intr]

    def proj(x, f, c):
        return f * x / F(1) + c

    def solve(target, f, c):             # x with fl(fl(f x) / 1 + c) == target, if one exists near (target - c) / f
        x = F((float(target) - float(c)) / float(f))
        for _ in range(64):
            u = proj(x, f, c)
            if u == target:
                return x
            x = F(np.nextafter(x, F(np.inf) if u < target else F(-np.inf)))
        return None

    def beyond(x, f, c, up):             # the first x past the edge position whose projection leaves it
        u0 = proj(x, f, c)
        while proj(x, f, c) == u0:
            x = F(np.nextafter(x, F(np.inf) if up else F(-np.inf)))
        return x

    pts = []
    mx, my = solve(F(w // 2 + 0.25), fx, cx), solve(F(h // 2 + 0.5), fy, cy)
    for tu, up in ((F(0), False), (F(w - 1), True)):
        x = solve(tu, fx, cx)
        if x is not None:
            pts += [((x, my, 1.0, 1.0), True), ((beyond(x, fx, cx, up), my, 1.0, 1.0), False)]
    for tv, up in ((F(0), False), (F(h - 1), True)):
        y = solve(tv, fy, cy)
        if y is not None:
            pts += [((mx, y, 1.0, 1.0), True), ((mx, beyond(y, fy, cy, up), 1.0, 1.0), False)]
    pts += [((0.0, 0.0, 0.0, 1.0), False), ((0.1, 0.1, -1.0, 1.0), False)]
    return np.array([p for p, _ in pts], F), np.array([v for _, v in pts])


@pytest.mark.gpu
def test_colour_evaluation_against_the_restatement(hip):
    """clouds of 0 .. ~200 000 points (a partial wave, one full grid pass of 256 x 256 lanes, more than one grid-stride round),
    edge points, alpha below 254, all three modes on levels 0 and 6"""
    w, h, levels = 640, 480, 7
    intr = CC.INTR
    img = random_image(w, h, seed=11)
    pyr = CC.numpy_pyramid(img, levels)
    trk = Colour(hip)
    worst = 0.0
    try:
        trk.prepare(img, levels, intr)
        edge, edge_valid = edge_points(w, h, intr)
        assert edge_valid.sum() >= 3 and len(edge) >= 8
        for n in (0, 1, 255, 256, 257, 65535, 65536, 65537, 200_003):
            loc, colours = colour_cloud(n, w, h, intr, seed=n)
            if n >= 256:
                loc[:len(edge)] = edge
            loc_d, col_d = hip.to_backend(loc if n else np.zeros((1, 4), F)), hip.to_backend(colours if n else np.zeros((1, 4), F))
            for lv in (0, 6):
                if n > 70_000 and lv == 0:
                    modes = (3,)
                else:
                    modes = (1, 2, 3)
                for mode in modes:
                    terms = TT.colour_terms(loc, colours, *pyr[lv], level_intr(intr, lv), EYE, mode)
                    got = trk.evaluate(lv, loc_d, col_d, n, EYE, mode)
                    worst = max(worst, colour_bound_check(got, terms, n, (n, lv, mode)))
                    got2 = trk.evaluate(lv, loc_d, col_d, n, EYE, mode, gh=False)
                    assert (got2[0], got2[1]) == (got[0], got[1])
            if n >= 256:                         # the inclusive edges count (alpha is 255 there), the positions outside do not
                t0 = TT.colour_terms(edge, colours[:len(edge)], *pyr[0], level_intr(intr, 0), EYE, 3)
                assert np.array_equal(t0.valid, edge_valid), t0.valid
        # a perturbed pose on level 6 and level 0 (a real rotation and translation)
        pose = synth.pose_matrix_yaw((0.004, 0.002, 0.001), np.deg2rad(0.4))
        loc, colours = colour_cloud(30_000, w, h, intr, seed=3)
        loc_d, col_d = hip.to_backend(loc), hip.to_backend(colours)
        for lv in (0, 6):
            for mode in (1, 2, 3):
                terms = TT.colour_terms(loc, colours, *pyr[lv], level_intr(intr, lv), pose, mode)
                worst = max(worst, colour_bound_check(trk.evaluate(lv, loc_d, col_d, 30_000, pose, mode), terms, 30_000, ("pose", lv, mode)))
    finally:
        trk.close()
    print(f"colour: worst ratio {worst:.3f}")


# ---- Ren ------------------------------------------------------------------------------------------------------------------------
REN_C = 16


def ren_reader(be, scene, sc):
    """the restatement's voxel access, built from the scene's downloaded buffers"""
    vox = scene.download(T.BUF_VOXEL_BLOCKS)
    if sc.indexType == T.INDEX_DENSE:
        return TT.VoxelReader(vox, dense=(sc.denseSize, sc.denseOffset)), vox
    return TT.VoxelReader(vox, entries=scene.download(T.BUF_HASH_ENTRIES)), vox


def fused_session(be, sc):
    ses = T.Session(be, sc)
    for k in range(sc.frames):
        ses.frame(k)
    return ses


def test_ren_restatement_equals_the_reference_recordings():
    import json
    import os
    import ren_cases as RC
    path = os.path.join(T.ROOT, "tests", "golden", "g_ren_tracker")
    with open(path + ".json") as f:
        meta = json.load(f)
    z = np.load(path + ".npz")
    oracle = T.oracle_backend()
    count = 0
    for name, sc in RC.SCENES.items():
        ses = fused_session(oracle, sc)
        try:
            reader, vox = ren_reader(oracle, ses.scene, sc)
        finally:
            ses.close()
        assert {n: synth.sha256(np.ascontiguousarray(vox[n])) for n in vox.dtype.names} == meta["scenes"][name]["voxel_sha256"], name
        pts = RC.unproject(RC.depth(sc), sc.intr())
        for k, inv in enumerate(np.array(meta["scenes"][name]["eval_inv"], F)):
            f, n, nab, hes = TT.ren_seq32(TT.ren_terms(pts, inv, sc.voxelSize, reader))
            assert n == z[name + "_count"][k] and f == z[name + "_f"][k], (name, k, n, f)
            assert np.array_equal(nab, z[name + "_nabla"][k]) and np.array_equal(hes, z[name + "_hessian"][k]), (name, k)
            count += 1
    assert count == 16


class Ren:
    def __init__(self, hip):
        self.hip = hip
        self.h = C.c_void_p()
        hip.check(hip.fn["ren_tracker_create"](C.byref(self.h)), "ren_tracker_create")

    def close(self):
        self.hip.check(self.hip.fn["ren_tracker_destroy"](self.h), "ren_tracker_destroy")

    def prepare(self, depth, intr):
        """-> the unprojected points the kernel reads"""
        h, w = depth.shape
        self.keep = self.hip.to_backend(np.ascontiguousarray(depth, F))
        v = capi.View(self.keep, w, h, intr_d=tuple(float(x) for x in intr))
        pts = np.zeros((h, w, 4), F)
        self.hip.check(self.hip.fn["ren_tracker_prepare"](self.h, C.byref(v.struct()), pts.ctypes.data_as(C.c_void_p), None), "prepare")
        return pts

    def evaluate(self, scene, invM, g=True):
        out = capi.RenEval()
        self.hip.check(self.hip.fn["ren_tracker_evaluate"](self.h, C.c_void_p(scene.h), fptr(invM), int(g), C.byref(out), None), "evaluate")
        return F(out.f), out.noValidPoints, np.array(out.nabla[:], F), np.array(out.hessian[:], F)


def ren_bound_check(got, terms, what):
    f, n, nabla, hessian = got
    assert n == terms.n, (what, n, terms.n)
    s64, A = terms.sum64, terms.A
    H = hessian.reshape(6, 6)
    assert np.array_equal(H, H.T), what
    vals = np.concatenate([[-float(f)], TT.pack(nabla, hessian, 6)])
    worst = 0.0
    for k in range(TT.KV):
        bound = ulp32(s64[k]) + REN_C * 2.0 ** -24 * A[k]
        err = abs(vals[k] - s64[k])
        assert err <= bound, (what, k, vals[k], s64[k], err, bound)
        worst = max(worst, err / bound)
    return worst


def ren_poses(sc):
    """the recorded evaluation poses and the true pose moved so that points straddle blocks (8 voxels), cross into negative block
    coordinates, fall into unallocated blocks and leave the fused region (and any mirrored cube) entirely"""
    import ren_cases as RC
    poses = dict(RC.eval_inv_poses(sc))
    base = poses["truth"]
    for shift in ((0.04, 0.0, 0.0), (0.0, -0.045, 0.035), (-0.25, -0.2, 0.0), (0.0, 0.0, 0.6), (0.15, 0.1, -0.1), (5.0, 5.0, 5.0)):
        m = base.copy()
        m[12:15] += np.asarray(shift, F)
        poses[shift] = m
    return poses


def ren_depths(sc):
    """depth images of the tracked frame at 1 x 1, 37 x 29, 161 x 121 and 640 x 480 (more than 65 536 points)"""
    import dataclasses
    import ren_cases as RC
    out = {}
    for w, h in ((37, 29), (161, 121), (640, 480)):
        s = dataclasses.replace(sc, w=w, h=h)
        out[(w, h)] = (np.ascontiguousarray(s.depth(RC.TRACKED_FRAME), F), np.asarray(s.intr(), F))
    d, intr = out[(161, 121)]              # 1 x 1: pixel (80, 60) of 161 x 121, the principal point moved with it
    out[(1, 1)] = (np.ascontiguousarray(d[60:61, 80:81]), intr - np.array([0, 0, 80, 60], F))
    return out


def ren_compare(hip, trk, scene, sc, reader, depths, poses, what, cache=None, table_walk=False):
    import ren_cases as RC
    worst, seen = 0.0, 0
    for size, (depth, intr) in depths.items():
        pts = trk.prepare(depth, intr)
        np.testing.assert_array_equal(pts, RC.unproject(depth, intr))
        for key, inv in poses.items():
            ck = (size, key)
            if cache is None or ck not in cache:
                terms = TT.ren_terms(pts, inv, sc.voxelSize, reader)
                if cache is not None:
                    cache[ck] = terms
            else:
                terms = cache[ck]
            if table_walk:
                hip.check(hip.fn["debug_set"](5, 1), "debug_set")
            try:
                got = trk.evaluate(scene, inv)
                f2, n2, nab2, _ = trk.evaluate(scene, inv, g=False)
            finally:
                if table_walk:
                    hip.check(hip.fn["debug_set"](5, 0), "debug_set")
            worst = max(worst, ren_bound_check(got, terms, (what, size, key)))
            assert f2 == got[0] and n2 == 0 and not nab2.any(), (what, size, key)
            seen += terms.n > 0
    assert seen >= (len(depths) - 1) * (len(poses) - 2)           # the 1 x 1 image and the far poses may see nothing
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hash_s", "hash_f_rgb", "dense_s"])
def test_ren_against_the_restatement(hip, name):
    """the default read path (sdf mirror / block directory, or the dense array) and, for the hash scenes, the table walk alone
    (debug key 5): every depth size and pose against the restatement built from the downloaded scene"""
    import ren_cases as RC
    sc = RC.SCENES[name]
    depths = ren_depths(sc)
    if name != "hash_s":
        depths.pop((640, 480))
    ses = fused_session(hip, sc)
    trk = Ren(hip)
    try:
        reader, _ = ren_reader(hip, ses.scene, sc)
        cache = {}
        poses = ren_poses(sc)
        worst = ren_compare(hip, trk, ses.scene, sc, reader, depths, poses, (name, "default"), cache)
        if sc.indexType != T.INDEX_DENSE:
            worst = max(worst, ren_compare(hip, trk, ses.scene, sc, reader, depths, poses, (name, "table walk"), cache, table_walk=True))
    finally:
        trk.close()
        ses.close()
    print(f"Ren {name}: worst ratio {worst:.3f}")


@pytest.mark.gpu
def test_ren_through_a_paged_mirror_with_unmapped_pages(hip, monkeypatch):
    """ITM_MIRROR=paged with a one-page pool (read when the scene is created): most of the scene's pages stay unmapped and their
    voxels are read through the directory; the values are the restatement's all the same"""
    import ren_cases as RC
    monkeypatch.setenv("ITM_MIRROR", "paged")
    monkeypatch.setenv("ITM_MIRROR_PAGES", "1")
    sc = RC.SCENES["hash_s"]
    depths = ren_depths(sc)
    depths.pop((640, 480))
    ses = fused_session(hip, sc)
    trk = Ren(hip)
    try:
        reader, _ = ren_reader(hip, ses.scene, sc)
        worst = ren_compare(hip, trk, ses.scene, sc, reader, depths, ren_poses(sc), "paged")
    finally:
        trk.close()
        ses.close()
    print(f"Ren paged: worst ratio {worst:.3f}")
