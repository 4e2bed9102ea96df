"""Distance field (include/itm_hip.h: itm_scene_esdf / itm_esdf_transform): the Euclidean distance transform of a box of the volume.
Everything is compared bit for bit with the restatement (tests/esdf_terms.py, pinned to the literal definition by
tests/test_esdf_terms.py), no tolerances:

  * CPU: the boxes of the scenes hold what they are for, shown on the restatement with the CPU oracle's scenes.
  * GPU: the transform alone on masks at every line length that takes another route through the kernels (shorter and longer than a
    wave, a workgroup, a panel), every window, the empty and the full mask and the tie masks, with and without `nearest`; scenes of
    every voxel type and both indexes, three boxes each, both site rules, two weights; one scene under every access path; a sub-box
    is a crop; recorded frames are launched first; the scene is left as it was; the limits; the C++ adapter."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import esdf_cases as EC
import esdf_terms as E
import itm_testlib as T
from infinitam_amd import capi
from infinitam_amd.capi import BUF_HASH_ENTRIES, BUF_VOXEL_BLOCKS
from esdf_cases import random_mask, tie_masks

F = np.float32
DEBUG_NO_DIRECTORY = 5          # include/itm_debug.h
ALL = ("dist2", "nearest", "distance", "state")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what):
    for k in got:
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {k}: {len(bad)} of {g.size} cells differ, first at (z, y, x) {bad[:4].tolist()}: "
                                 f"{[got[k][tuple(b)] for b in bad[:4]]} vs {[want[k][tuple(b)] for b in bad[:4]]}")


_built = {}


def built(be, name, form="default", moved_away=False):
    key = (id(be), name, form, moved_away)
    if key not in _built:
        _built[key] = EC.Built(be, EC.SCENES[name], form, moved_away)
    return _built[key]


@pytest.fixture(scope="module", autouse=True)
def close_scenes():
    yield
    for b in _built.values():
        b.close()
    _built.clear()


# ---- CPU: the boxes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(EC.SCENES))
def test_boxes_hold_a_surface_unobserved_cells_and_cells_out_of_reach(oracle, name):
    EC.assert_boxes_are_not_vacuous(built(oracle, name))


def test_boxes_of_the_moved_scene_lie_on_its_first_place(oracle):
    b = built(oracle, "mesh_micro", moved_away=True)
    EC.assert_boxes_are_not_vacuous(b)
    assert np.all(np.abs(np.array(b.boxes()["surface"][0])) > 1000)


# ---- GPU: the transform alone -----------------------------------------------------------------------------------------------------------

RADII = [0, 1, 3, 40, 1023]
TRANSFORM_SIZES = [(1, 1, 1), (65, 1, 1), (1, 129, 1), (1, 1, 257), (70, 37, 19), (1024, 2, 2), (2, 1024, 2), (2, 2, 1024)]      # (nx, ny, nz)


def check_transform(hip, mask, R, what):
    want_d, want_n = E.transform_separable(mask, R)
    want = {"dist2": want_d, "nearest": want_n, "distance": E.distance(want_d, mask, 0.0125)}
    # the variant with `nearest` and the lean one are different kernels; `distance` is a branch of the last pass
    for names in (("dist2", "nearest", "distance"), ("dist2",), ("dist2", "distance"), ("nearest",)):
        got = hip.esdf_transform(mask, R, 0.0125, names)
        assert set(got) == set(names)
        assert_same(got, want, f"{what}, R = {R}, {names}")


@pytest.mark.gpu
@pytest.mark.parametrize("size", TRANSFORM_SIZES)
def test_transform_of_random_masks_equals_the_restatement(hip, size):
    n = size[0] * size[1] * size[2]
    for density, seed in ((0.02, 1), (0.3, 2)):
        mask = random_mask(size, density, seed + n)
        mask.reshape(-1)[n // 2] |= E.SITE
        for R in RADII:
            check_transform(hip, mask, R, f"{size}, density {density}")
    # a single site at the far end of the longest line: the whole line is walked
    lone = np.zeros(size[::-1], np.uint8)
    lone.reshape(-1)[n - 1] = E.SITE | E.INSIDE
    for R in (0, 1023):
        check_transform(hip, lone, R, f"{size}, one site")


@pytest.mark.gpu
def test_transform_of_the_empty_the_full_and_the_tie_masks(hip):
    for size in ((70, 37, 19), (1, 1, 1), (5, 1, 300)):
        for fill in (0, E.SITE, E.SITE | E.INSIDE):
            mask = np.full(size[::-1], fill, np.uint8)
            for R in (0, 3):
                check_transform(hip, mask, R, f"{size}, every cell {fill}")
        none = hip.esdf_transform(np.zeros(size[::-1], np.uint8), 0, 1.0, ("dist2", "nearest", "distance"))
        assert np.all(none["dist2"] == capi.ESDF_NONE) and np.all(none["nearest"] == -1) and np.all(none["distance"] == np.inf)
    for k, mask in enumerate(tie_masks()):
        for R in (0, 1, 2, 5):
            check_transform(hip, mask, R, f"tie mask {k}")


# ---- GPU: scenes ------------------------------------------------------------------------------------------------------------------------

def check_scene(b, what, sites=tuple(EC.SITE_MASKS), weights=(1, 2), radii=(0, EC.R_NEAR)):
    results = {}
    for box_name, (origin, size) in b.boxes().items():
        for s in sites:
            for mw in weights:
                for R in radii:
                    want = b.restated((origin, size), s, mw, R)
                    names = ALL if R else ("dist2", "distance", "state")          # the lean kernels at R = 0
                    got = b.scene.distance_field(origin, size, {"both": ("surface", "unknown")}.get(s, (s,)), mw, R, names)
                    assert_same(got, want, f"{what}, box {box_name} {origin}, sites {s}, min_weight {mw}, R = {R}")
                    results[(box_name, s, mw, R)] = got
    return results


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EC.SCENES))
def test_scenes_equal_the_restatement(hip, name):
    b = built(hip, name)
    EC.assert_boxes_are_not_vacuous(b)
    check_scene(b, name)


def all_blocks_outside_the_cubes(b):
    probe = b.scene.accel_probe(b.old_blocks)
    return not probe["dir_covered"].any() and not probe["mirror_covered"].any()


@pytest.mark.gpu
def test_one_scene_under_every_access_path(hip):
    name = "mesh_micro"
    first = check_scene(built(hip, name), f"{name}, default", weights=(1,))
    for form in ("paged", "mirror_off"):
        b = built(hip, name, form=form)
        info = b.scene.accel_info()
        assert (info["mirror_pages"] > 0) if form == "paged" else (info["mirror_bytes"] == 0 and info["directory_bytes"] > 0), info
        again = check_scene(b, f"{name}, {form}", weights=(1,))
        for key in first:
            assert_same(again[key], first[key], f"{name}, {form} against default, {key}")
    hip.check(hip.fn["debug_set"](DEBUG_NO_DIRECTORY, 1), "debug_set")
    try:
        again = check_scene(built(hip, name), f"{name}, no directory", weights=(1,))
    finally:
        hip.check(hip.fn["debug_set"](DEBUG_NO_DIRECTORY, 0), "debug_set")
    for key in first:
        assert_same(again[key], first[key], f"{name}, no directory against default, {key}")
    # fused 40 m away, then moved: the boxes' blocks lie outside both cubes and are found by walking the table
    b = built(hip, name, moved_away=True)
    assert b.scene.accel_info()["moves"] >= 1 and all_blocks_outside_the_cubes(b)
    EC.assert_boxes_are_not_vacuous(b)
    check_scene(b, f"{name}, table walk", weights=(1,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mesh_f_rgb", "dense"])
def test_state_of_a_sub_box_is_the_crop_of_the_enclosing_box(hip, name):
    b = built(hip, name)
    origin, size = b.boxes()["surface"]
    whole = b.scene.distance_field(origin, size, ("surface", "unknown"), 1, 0, ("state",))["state"]
    for lo, n in (((0, 0, 0), (1, 1, 1)), ((5, 7, 3), (9, 8, 7)), ((31, 1, 2), (9, 30, 15)), ((39, 32, 16), (1, 1, 1))):
        part = b.scene.distance_field(tuple(o + d for o, d in zip(origin, lo)), n, ("surface", "unknown"), 1, 0, ("state",))["state"]
        assert np.array_equal(part, whole[lo[2]:lo[2] + n[2], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[0]]), (lo, n)
    assert np.any(whole & E.SITE) and not np.all(whole & E.SITE)


@pytest.mark.gpu
def test_recorded_frames_are_launched_first(hip):
    sc = EC.SCENES["mesh_f_rgb"]
    origin, size = built(hip, "mesh_f_rgb").boxes()["surface"]
    results = []
    for deferred in (True, False):
        ses = T.Session(hip, sc, deferred_fusion=deferred)
        ses.frame(0, fused="four" if deferred else False)
        view = ses.view(1)
        ses.scene.reco.AllocateSceneFromDepth(view, ses.rs)          # deferred: recorded, not launched
        ses.scene.reco.IntegrateIntoScene(view, ses.rs)
        ses.scene.vis.CreateExpectedDepths(view.M_d, view.intr_d, ses.rs)
        results.append(ses.scene.distance_field(origin, size, ("surface", "unknown"), 2, 4, ALL))
        ses.close()
    assert_same(results[0], results[1], "recorded frame")
    # ... and the second frame is in what they saw: at min_weight 2 a scene of one frame has nothing observed
    assert np.any(results[1]["state"] & E.OBSERVED)
    one = T.Session(hip, sc, deferred_fusion=False)
    one.frame(0)
    assert not np.any(one.scene.distance_field(origin, size, ("surface",), 2, 4, ("state",))["state"] & E.OBSERVED)
    one.close()


def scene_digest(scene):
    which = (BUF_HASH_ENTRIES, BUF_VOXEL_BLOCKS) if scene.is_hash else (BUF_VOXEL_BLOCKS,)
    return [hashlib.sha256(scene.download(w).tobytes()).hexdigest() for w in which]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mesh_micro", "dense"])
def test_the_scene_is_left_as_it_was(hip, name):
    b = built(hip, name)
    before = scene_digest(b.scene)
    for origin, size in b.boxes().values():
        b.scene.distance_field(origin, size, ("surface", "unknown"), 1, 0, ALL)
        b.scene.distance_field(origin, size, ("surface",), 2, 5, ("dist2",))
    assert scene_digest(b.scene) == before


@pytest.mark.gpu
def test_limits_are_refused(hip):
    b = built(hip, "mesh_micro")
    s = b.scene
    ok = s.distance_field((0, 0, 0), (1, 1, 1), ("unknown",), 1, 0, ALL)          # the smallest call there is
    assert ok["dist2"].shape == (1, 1, 1)
    refused = [dict(size=(0, 4, 4)), dict(size=(4, 1025, 4)), dict(size=(4, 4, -1)), dict(size=(1024, 1024, 129)), dict(max_distance=-1),
               dict(max_distance=1024), dict(origin=(262136 - 4, 0, 0)), dict(origin=(0, -262135, 0)), dict(origin=(0, 0, 2 ** 31 - 3)),
               dict(sites=0), dict(sites=4), dict(sites=7), dict(min_weight=0)]
    for kw in refused:
        args = dict(origin=(0, 0, 0), size=(4, 4, 4), sites=("surface",), min_weight=1, max_distance=0, want=("dist2",))
        args.update(kw)
        with pytest.raises(capi.ItmError, match=r"\(-1\)"):
            s.distance_field(**args)
    # the last valid box at either end of the coordinate range
    s.distance_field((262136 - 5, 0, 0), (4, 4, 4), ("surface",), 1, 0, ("dist2",))
    s.distance_field((0, -262134, 0), (4, 4, 4), ("surface",), 1, 0, ("dist2",))
    # a null dist2, a null box
    box = capi.EsdfBox()
    box.size[:] = [2, 2, 2]
    for out in (capi.EsdfOut(), None):
        with pytest.raises(capi.ItmError, match=r"\(-1\)"):
            hip.check(hip.fn["scene_esdf"](capi._P(s.h), capi.C.byref(box), 1, 1, 0, capi.C.byref(out) if out is not None else None, None), "scene_esdf")
    # the transform alone: the same limits on its own arguments
    for shape, R in (((1, 1, 1025), 0), ((2, 2, 2), 1024), ((2, 2, 2), -1), ((0, 2, 2), 0)):
        with pytest.raises(capi.ItmError, match=r"\(-1\)"):
            hip.esdf_transform(np.zeros(shape, np.uint8), R)
    state = hip.to_backend(np.zeros(8, np.uint8))
    size = (capi.C.c_int32 * 3)(2, 2, 2)
    empty = capi.EsdfOut()
    with pytest.raises(capi.ItmError, match=r"\(-1\)"):
        hip.check(hip.fn["esdf_transform"](capi._P(state.ptr), size, 0, 1.0, capi.C.byref(empty), None), "esdf_transform")
    state.close()


# ---- GPU: the C++ adapter ---------------------------------------------------------------------------------------------------------------

DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "distance_field_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "distance_field_demo")


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_demo_compiles():
    assert os.path.exists(build_demo())


def fnv(a):
    h = 1469598103934665603
    for byte in np.ascontiguousarray(a).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


@pytest.mark.gpu
def test_cpp_demo_equals_the_python_binding(hip, tmp_path):
    out = subprocess.run([build_demo(), str(tmp_path)], check=True, capture_output=True, text=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    s = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.01))
    s.reco.ResetScene()
    s.load(str(tmp_path))
    origin, size = (-21, -13, 143), (40, 33, 17)
    res = s.distance_field(origin, size, ("surface",), 1, 6, ALL)
    assert got["cells"] == res["state"].size
    assert got["sites"] == int(np.count_nonzero(res["state"] & E.SITE)) > 1000
    assert got["observed"] == int(np.count_nonzero(res["state"] & E.OBSERVED)) > 1000
    assert got["none"] == int(np.count_nonzero(res["dist2"] == capi.ESDF_NONE)) > 0
    for name in ALL:
        assert got[name] == fnv(res[name]), name
    # ... and both are the restatement's
    import scene_query_terms as Q
    assert_same(res, E.esdf(Q.reader_of(s), (origin, size), E.SITE_SURFACE, 1, 6, 0.01), "demo scene")
    s.close()
