"""A colour camera of its own size, intrinsics and pose next to the depth camera (tests/colour_camera_cases.py), through every path
that reads the colour image or the render state of the colour size: the colour part of IntegrateIntoScene (row stride, bounds and
intrinsics of the RGB image, calib_inv * M_d), AllocateSceneFromDepth through a render state of the tracked (= colour) size as
ITMMainEngine does for TRACKER_COLOR (Engine/ITMMainEngine.cpp:50-52), the TRACKER_COLOR branch of Prepare (CreateExpectedDepths
through the colour camera + CreatePointCloud) and the colour tracker's pyramid.

  CPU   oracle == reference (bit for bit; records where the reference build is absent), oracle against the float64 restatement of
        one integration step (tests/colour_camera_terms.py), the conditions every case must meet
  gpu   HIP == oracle (bit for bit) in all three call forms and frame-ahead, HIP against the restatement, the colour branch of Prepare
        with deferred fusion on and off and with swapping, the colour tracker with 213 x 171 next to 160 x 120"""
import ctypes as C

import numpy as np
import pytest

import colour_camera_cases as CCC
import colour_camera_terms as CT
import colour_cases as CC
import itm_testlib as T
import tracker_terms as TT
from infinitam_amd import capi, synth

CAMS = CCC.CAMERA_NAMES
HASH, DENSE = capi.INDEX_HASH, capi.INDEX_DENSE
KINDS = {"hash_s_rgb": (capi.VOXEL_S_RGB, HASH), "hash_f_rgb": (capi.VOXEL_F_RGB, HASH),
         "dense_s_rgb": (capi.VOXEL_S_RGB, DENSE), "dense_f_rgb": (capi.VOXEL_F_RGB, DENSE)}


def run_sequence(be, kind, cam, rs_size, small_pool=True, form="separate", deferred=True, prepare=True):
    """Frames of allocate + integrate (in the call form `form`), each followed by the colour branch of Prepare.  Returns everything a
    comparison needs: counters, table, the blocks the table points to (or the volume), per-frame outputs of Prepare."""
    vt, it = KINDS[kind]
    sc = CCC.scenario(vt, it, small_pool=small_pool)
    ses = CCC.ColourSession(be, sc, cam, rs_size=rs_size, deferred_fusion=deferred)
    s, rs = ses.scene, ses.rs
    out = {"frames": []}
    for k in range(sc.frames):
        if form == "separate":
            v = ses.view(k)
            s.reco.AllocateSceneFromDepth(v, rs)
            s.flush(rs)
            s.reco.IntegrateIntoScene(v, rs)
            s.flush(rs)
        elif form == "recorded":                       # the mapper's two calls back to back, nothing in between
            v = ses.view(k)
            s.reco.AllocateSceneFromDepth(v, rs)
            s.reco.IntegrateIntoScene(v, rs)
        else:
            v = ses.frame(k, fused={"four": "four", "fused": True}[form])
        fr = {"counters": {key: val for key, val in s.counters(rs).items() if key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries")}}
        if prepare:
            fr.update(ses.prepare_colour(k, v))
        out["frames"].append(fr)
    st = ses.state()
    if s.is_hash:
        out["hash"] = st["hash"]
        out["blocks"] = st["voxels"] if small_pool else CCC.used_blocks(st)
    else:
        out["blocks"] = st["voxels"]
    ses.close()
    return out


def assert_same(a, b, what):
    for k, (fa, fb) in enumerate(zip(a["frames"], b["frames"])):
        assert fa["counters"] == fb["counters"], f"{what}: frame {k}: {fa['counters']} vs {fb['counters']}"
        for key in fa:
            if key != "counters":
                assert np.array_equal(fa[key], fb[key]), f"{what}: frame {k}: {key}"
    if "hash" in a:
        T.assert_fields_equal(a["hash"], b["hash"], what + ": table")
    T.assert_fields_equal(a["blocks"].reshape(-1), b["blocks"].reshape(-1), what + ": voxels")


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rs_size", ["depth", "colour"])
@pytest.mark.parametrize("kind", ["hash_s_rgb", "hash_f_rgb", "dense_s_rgb"])
@pytest.mark.parametrize("cam", CAMS)
def test_oracle_matches_the_reference(oracle, ref, cam, kind, rs_size):
    a = run_sequence(oracle, kind, cam, rs_size, small_pool=False)
    assert a["frames"][-1]["count_0"] > 500 and a["frames"][-1]["count_1"] > 100
    if ref.backend is not None:
        assert_same(a, run_sequence(ref.backend, kind, cam, rs_size, small_pool=False), f"{cam}/{kind}/{rs_size}")
    ref.check("run", a)


def stepwise(be, kind, cam, rs_size="depth", deferred=True):
    """Yields (frame, state before the integration, view as the restatement reads it, scene parameters, voxels after it)."""
    vt, it = KINDS[kind]
    sc = CCC.scenario(vt, it)
    ses = CCC.ColourSession(be, sc, cam, rs_size=rs_size, deferred_fusion=deferred)
    s, rs = ses.scene, ses.rs
    cfg = {"voxelSize": sc.voxelSize, "mu": sc.mu, "maxW": sc.maxW, "denseSize": sc.denseSize, "denseOffset": sc.denseOffset}
    rgb = synth.rgb_frame(ses.wc, ses.hc)
    for k in range(sc.frames):
        v = ses.view(k)
        s.reco.AllocateSceneFromDepth(v, rs)
        before = ses.state()
        s.reco.IntegrateIntoScene(v, rs)
        after = s.download(capi.BUF_VOXEL_BLOCKS)
        view = {"M_d": v.M_d, "intr_d": v.intr_d, "depth": CCC.depth(k), "rgb": rgb, "intr_rgb": v.intr_rgb, "rgb_to_depth_inv": v.rgb_to_depth_inv}
        yield k, before, view, cfg, after
    ses.close()


def check_against_restatement(be, kind, cam, what, conditions=False):
    figs = []
    for k, before, view, cfg, after in stepwise(be, kind, cam):
        terms = CT.integrate(before, view, cfg)
        fig = CT.compare(terms, before["voxels"], after, what=f"{what}/{cam}/{kind}/frame{k}")
        if conditions:
            # the conditions of tests/colour_camera_cases.py, on every frame: the backend's own count of voxels that received a colour ...
            got_coloured = int((after["w_color"] != before["voxels"]["w_color"]).sum())
            outside = {e: int(terms["out_" + e].sum()) for e in ("left", "right", "top", "bottom")}
            total = int((terms["out_left"] | terms["out_right"] | terms["out_top"] | terms["out_bottom"]).sum())
            print(f"{cam}/frame{k}: coloured {got_coloured}, in the band but outside the colour image {total}: {outside}")
            assert got_coloured >= 1000
            assert total >= 1000                       # ... and the band voxels that the colour image's bounds must turn away,
            assert min(outside.values()) > 0, outside  # beyond each of its four edges
        figs.append(fig)
    return figs


@pytest.mark.parametrize("cam", CAMS)
def test_case_conditions(oracle, cam):
    check_against_restatement(oracle, "hash_s_rgb", cam, "oracle", conditions=True)


@pytest.mark.parametrize("kind", ["hash_f_rgb", "hash_s_rgb", "dense_f_rgb"])
@pytest.mark.parametrize("cam", CAMS)
def test_oracle_matches_the_restatement(oracle, cam, kind):
    check_against_restatement(oracle, kind, cam, "oracle")


def test_allocation_through_a_render_state_of_another_size(oracle):
    """The visible list and the table do not depend on the render state's size (only the view's size enters the allocation)."""
    a = run_sequence(oracle, "hash_s_rgb", CAMS[0], "depth", prepare=False)
    for cam in CAMS:
        b = run_sequence(oracle, "hash_s_rgb", cam, "colour", prepare=False)
        T.assert_fields_equal(a["hash"], b["hash"], cam + ": table")
        assert [f["counters"] for f in a["frames"]] == [f["counters"] for f in b["frames"]]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
_oracle_runs = {}


def oracle_run(oracle, kind, cam, rs_size):
    """the oracle's sequence, computed once per case and shared (never modified) by the tests that compare with it"""
    key = (kind, cam, rs_size)
    if key not in _oracle_runs:
        _oracle_runs[key] = run_sequence(oracle, kind, cam, rs_size)
    return _oracle_runs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cam", CAMS)
def test_hip_matches_the_oracle_in_every_call_form(hip, oracle, cam, kind):
    """separate calls with flushes and the mapper's calls recorded, through render states of both sizes; the four calls recorded and
    itm_process_frame with the render state at the depth size (the fused frame's rule)"""
    for rs_size, form, deferred in (("colour", "separate", True), ("colour", "recorded", True), ("colour", "recorded", False),
                                    ("depth", "separate", True), ("depth", "recorded", True), ("depth", "four", True), ("depth", "fused", True)):
        a = run_sequence(hip, kind, cam, rs_size, form=form, deferred=deferred)
        assert_same(a, oracle_run(oracle, kind, cam, rs_size), f"{cam}/{kind}/{rs_size}/{form}/deferred={deferred}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["hash_s_rgb", "hash_f_rgb"])
def test_frames_issued_ahead_with_a_colour_camera(hip, oracle, kind):
    cam = CAMS[0]
    vt, it = KINDS[kind]
    sc = CCC.scenario(vt, it)
    ses = CCC.ColourSession(hip, sc, cam)
    depths = [hip.to_backend(CCC.depth(k)) for k in range(sc.frames)]
    views = []
    for k in range(sc.frames):
        v = ses.view(k)
        v.depth = depths[k]
        views.append(v)
    frames = []
    for k in range(sc.frames):
        nxt = views[k + 1] if k + 1 < sc.frames else None
        ses.scene.process_frame_ahead(views[k], nxt, ses.rs, ses.points, ses.normals)
        fr = {"counters": {key: val for key, val in ses.scene.counters(ses.rs).items() if key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries")}}
        frames.append(fr)
    st = ses.state()
    a = {"frames": frames, "hash": st["hash"], "blocks": st["voxels"]}
    b = oracle_run(oracle, kind, cam, "depth")
    b = {"frames": [{"counters": f["counters"]} for f in b["frames"]], "hash": b["hash"], "blocks": b["blocks"]}
    ses.close()
    # (the oracle's sequence ran Prepare's colour branch between the frames: it reads the scene only)
    assert_same(a, b, f"ahead/{kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["hash_f_rgb", "hash_s_rgb", "dense_f_rgb", "dense_s_rgb"])
@pytest.mark.parametrize("cam", CAMS)
def test_hip_matches_the_restatement(hip, cam, kind):
    check_against_restatement(hip, kind, cam, "hip")


@pytest.mark.gpu
@pytest.mark.parametrize("cam", CAMS)
def test_prepare_colour_branch_with_swapping(hip, oracle, cam):
    """A hash scene with a global cache, render state of the colour size, the two swapping calls between mapping and Prepare
    (Engine/ITMDenseMapper.cpp:59-64)."""
    def run(be):
        vt, it = KINDS["hash_s_rgb"]
        sc = CCC.scenario(vt, it)
        ses = CCC.ColourSession(be, sc, cam, rs_size="colour", useSwapping=True)
        frames = []
        for k in range(sc.frames):
            v = ses.view(k)
            ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
            ses.scene.reco.IntegrateIntoScene(v, ses.rs)
            ses.scene.swap_integrate_global_into_local(ses.rs)
            ses.scene.swap_save_to_global_memory(ses.rs)
            fr = {"counters": {key: val for key, val in ses.scene.counters(ses.rs).items() if key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries")}}
            fr.update(ses.prepare_colour(k, v))
            frames.append(fr)
        st = ses.state()
        ses.close()
        return {"frames": frames, "hash": st["hash"], "blocks": st["voxels"]}
    assert_same(run(hip), run(oracle), f"swapping/{cam}")


class ColourTracker:
    """the colour tracker's evaluation object with a view whose RGB image has its own size"""

    def __init__(self, hip):
        self.hip, self.h = hip, C.c_void_p()
        hip.check(hip.fn["colour_tracker_create"](C.byref(self.h)), "colour_tracker_create")

    def close(self):
        self.hip.check(self.hip.fn["colour_tracker_destroy"](self.h), "colour_tracker_destroy")

    def prepare(self, view, levels):
        self.hip.check(self.hip.fn["colour_tracker_prepare"](self.h, C.byref(view.struct()), levels, None), "colour_tracker_prepare")

    def read_level(self, lv):
        w, h = C.c_int(), C.c_int()
        self.hip.check(self.hip.fn["colour_tracker_read_level"](self.h, lv, None, None, None, C.byref(w), C.byref(h), None), "read_level")
        rgb = np.zeros((h.value, w.value, 4), np.uint8)
        gx = np.zeros((h.value, w.value, 4), np.int16)
        gy = np.zeros_like(gx)
        self.hip.check(self.hip.fn["colour_tracker_read_level"](self.h, lv, rgb.ctypes.data_as(C.c_void_p), gx.ctypes.data_as(C.c_void_p),
                                                                gy.ctypes.data_as(C.c_void_p), C.byref(w), C.byref(h), None), "read_level")
        return rgb, gx, gy

    def evaluate(self, lv, loc, colours, n, pose, mode):
        out = capi.ColourEval()
        M = np.ascontiguousarray(pose, np.float32)
        self.hip.check(self.hip.fn["colour_tracker_evaluate"](self.h, lv, loc.ptr, colours.ptr, n, M.ctypes.data_as(C.POINTER(C.c_float)), mode, 1,
                                                              C.byref(out), None), "colour_tracker_evaluate")
        return np.float32(out.f), out.noValidPoints, out.numPara, np.array(out.nabla[:], np.float32), np.array(out.hessian[:], np.float32)


@pytest.mark.gpu
def test_colour_tracker_with_an_rgb_image_of_its_own_size(hip):
    """213 x 171 next to 160 x 120 depth: every pyramid level's size and contents against the numpy pyramid, one evaluation per level
    against the float64 restatement of the evaluation kernel (tolerances of tests/test_tracker_terms.py)."""
    import test_tracker_terms as TTT
    cam = "larger_213x171"
    wc, hc = CCC.size(cam)
    levels = 4
    intr = CCC.intr_rgb(cam)
    img = synth.textured_rgb_frame(wc, hc, CCC.pose_rgb(0), intr)
    calib, calib_inv = CCC.extrinsic()
    keep = (hip.to_backend(CCC.depth(0)), hip.to_backend(np.ascontiguousarray(img)))
    view = capi.View(keep[0], CCC.W, CCC.H, M_d=CCC.pose(0), intr_d=CCC.INTR_D, rgb=keep[1], w_rgb=wc, h_rgb=hc, intr_rgb=intr,
                     rgb_to_depth=calib, rgb_to_depth_inv=calib_inv)
    want = CC.numpy_pyramid(img, levels)
    loc, colours = TTT.colour_cloud(20_000, wc, hc, intr, seed=5)
    loc_d, col_d = hip.to_backend(loc), hip.to_backend(colours)
    pose = synth.pose_matrix_yaw((0.004, 0.002, 0.001), np.deg2rad(0.4))
    trk = ColourTracker(hip)
    try:
        trk.prepare(view, levels)
        for lv in range(levels):
            got = trk.read_level(lv)
            assert got[0].shape[:2] == (hc >> lv, wc >> lv), (lv, got[0].shape)
            for a, b in zip(got, want[lv]):
                np.testing.assert_array_equal(a, b, err_msg=f"level {lv}")
            mode = (3, 1, 2, 3)[lv]
            terms = TT.colour_terms(loc, colours, *want[lv], TTT.level_intr(intr, lv), pose, mode)
            assert terms.n > 1000
            TTT.colour_bound_check(trk.evaluate(lv, loc_d, col_d, len(loc), pose, mode), terms, len(loc), (lv, mode))
    finally:
        trk.close()
