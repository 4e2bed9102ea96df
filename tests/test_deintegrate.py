"""itm_deintegrate_from_scene on the GPU against its numpy restatement (tests/defusion_terms.py), bit for bit and without a tolerance
anywhere: from the prepared voxel states of tests/prepared_state_cases.py (every weight 0 .. 255, every stored sdf edge, colour weights
decorrelated from the depth weights) in hash and dense scenes and for both keepSaturated values; in every form of the sdf mirror and
without the directories, with an audit and a ray cast afterwards; behind a frame recorded for the fused launch; through the C++
adapters (ITMMainEngine_HIP::ReintegrateFrame / RemoveFrame) against the same calls made by hand; and every refusal.

Coverage.  Which (voxel, shot) pairs pass the gates is geometry alone -- the integration's gates -- so the conditions of
prepared_state_cases.assert_coverage are asserted here on the restatement of each case: a pair counts when a voxel passes the depth gate
while it still holds its prepared state (weight 0 then counts among `unobserved`, weights at or above maxW with keepSaturated among
`saturated`), a colour weight when a voxel reaches the cases on w_color.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import accel_terms as A
import defusion_terms as DT
import esdf_cases as EC
import fusion_terms as FT
import itm_testlib as T
import prepared_state_cases as P
from infinitam_amd import capi, synth

F = np.float32
_P = capi._P
CASES = [("hash", k, 100) for k in P.TYPES] + [("dense", k, 100) for k in P.TYPES] + [("hash", "s_rgb", 255), ("dense", "f_rgb", 255)]
case_id = lambda c: "%s-%s-maxW%d" % c


def scenario(index, kind, maxW):
    return (P.hash_scenario if index == "hash" else P.dense_scenario)(kind, maxW)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def assert_pool(got, want, before, what):
    same = all(np.array_equal(bits(want[n]), bits(got[n])) for n in want.dtype.names)
    assert same, "%s: %s" % (what, FT.describe(before, want, got))


def scene_state(ses):
    """Everything of the scene and its render state that a de-integration must leave alone."""
    s, rs = ses.scene, ses.rs
    out = {"alloc_list": s.download(capi.BUF_ALLOCATION_LIST), "counters": s.counters(rs)}
    if s.is_hash:
        out.update(hash=s.download(capi.BUF_HASH_ENTRIES), excess=s.download(capi.BUF_EXCESS_LIST), visible_ids=s.download(capi.BUF_VISIBLE_IDS, rs),
                   visible_type=s.download(capi.BUF_VISIBLE_TYPE, rs))
    return out


def assert_state_unchanged(a, b, what):
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])
    for k in a:
        if k != "counters":
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


def visited(ses, p, k):
    """(pool indices, coordinates) of the voxels shot k visits: the blocks of the render state's list as it is now, or the whole volume."""
    sc = p.sc
    if sc.indexType == capi.INDEX_DENSE:
        return (np.arange(len(p.voxels)),) + tuple(FT.dense_coordinates(sc.denseSize, sc.denseOffset))
    n = ses.scene.counters(ses.rs)["noVisibleEntries"]
    return FT.hash_coordinates(p.hash, ses.scene.download(capi.BUF_VISIBLE_IDS, ses.rs)[:n])


def deintegrate_shots(hip, p, keep, after_shot=None):
    """The case's shots de-integrated in turn from the running state on a fresh scene holding the placement; every shot compared with
    the restatement.  Hash scenes: the placement's visible list for shot 0, FindVisibleBlocks under the shot's pose afterwards.  Returns
    (session -- the caller closes it --, the restated pool, the coverage, the summed counts)."""
    sc = p.sc
    ses = T.Session(hip, sc)
    try:
        P.upload(ses, p)
        vox = p.voxels.copy()
        prepared = p.pair_of >= 0
        cov = P.Coverage(blocks=p.blocks, pairs=np.zeros(P.N_PAIRS, bool), w_color=np.zeros(256, bool))
        total = dict.fromkeys(DT.STATS, 0)
        initial = P.sentinel_free_initial(sc.voxelType)
        unvisited = np.ones(len(vox), bool)
        for k in range(sc.frames):
            v = ses.view(k)
            if ses.scene.is_hash and k > 0:
                ses.scene.vis.FindVisibleBlocks(v.M_d, v.intr_d, ses.rs)
            idx, ix, iy, iz = visited(ses, p, k)
            state = scene_state(ses)
            got_stats = ses.scene.deintegrate(v, ses.rs, keep_saturated=keep, stats=True)
            assert_state_unchanged(state, scene_state(ses), "%s shot %d" % (sc.name, k))
            old = vox[idx]
            new, facts = DT.deintegrate(sc.voxelType, old, ix, iy, iz, sc.frame_inputs(k), keep)
            before = vox.copy()
            vox[idx] = new
            got = ses.scene.download(capi.BUF_VOXEL_BLOCKS)
            assert_pool(got, vox, before, "%s keep=%s shot %d" % (sc.name, keep, k))
            unvisited[idx] = False
            want_stats = dict(DT.counts(facts), blocks=(len(idx) // 512 if ses.scene.is_hash else 0), visited=len(idx))
            print("%s keep=%s shot %d: %s" % (sc.name, keep, k, got_stats))
            assert got_stats == want_stats, (sc.name, k, got_stats, want_stats)
            for n in total:
                total[n] += want_stats[n]
            # coverage, as prepared_state_cases.restate gathers it
            held, w = prepared[idx], facts["would"]
            cov.pairs[p.pair_of[idx[w & held]]] = True
            if sc.colour:
                cov.w_color[old["w_color"][facts["colour_gate"] & held]] = True
            obs1 = w & (facts["eta"] >= F(sc.mu))
            cov.clamped_initial += int(np.count_nonzero(obs1 & (old["sdf"] == initial)))
            cov.clamped_other += int(np.count_nonzero(obs1 & (old["sdf"] != initial)))
            cov.above_maxW += int(np.count_nonzero(w & (old["w_depth"] > sc.maxW)))
            assert not (facts["touched"] & (old["w_depth"] == 0)).any() and (facts["unobserved"] == (w & (old["w_depth"] == 0))).all()
            prepared[idx[facts["touched"] | facts["coloured"]]] = False
            if after_shot:
                after_shot(ses, k, vox)
        # every byte of every voxel no shot visited is as it was uploaded
        raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
        assert unvisited.any() or not ses.scene.is_hash
        assert np.array_equal(raw(got)[unvisited], raw(p.voxels)[unvisited])
        cov.pairs = cov.pairs.reshape(P.N_W, P.N_SDF)
        return ses, vox, cov, total
    except BaseException:
        ses.close()
        raise


# ---- prepared states ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("keep", [False, True], ids=["all", "keep_saturated"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_prepared_states_equal_the_restatement(hip, oracle, case, keep):
    sc = scenario(*case)
    p = P.placement(oracle, sc)
    ses, _, cov, total = deintegrate_shots(hip, p, keep)
    ses.close()
    P.assert_coverage(cov, sc)
    assert cov.pairs[0].any() and total["unobserved"] > 0, "weight 0 is not covered among the unobserved voxels"
    assert total["reset"] > 0 and total["clamped"] > 0 and (total["saturated"] > 0) == keep, total
    if sc.colour:
        assert total["colourReset"] > 0 and total["coloured"] > total["colourReset"], total
    else:
        assert total["coloured"] == 0 and total["colourReset"] == 0


@pytest.mark.gpu
def test_default_config_follows_the_scene(hip, oracle):
    """cfg == NULL: keepSaturated = stopIntegratingAtMaxW of the scene."""
    for stop in (False, True):
        sc = P.dense_scenario("s", 100, stop)
        p = P.placement(oracle, sc)
        ses = T.Session(hip, sc)
        try:
            P.upload(ses, p)
            st = ses.scene.deintegrate(ses.view(0), ses.rs, stats=True)
            ix, iy, iz = FT.dense_coordinates(sc.denseSize, sc.denseOffset)
            new, facts = DT.deintegrate(sc.voxelType, p.voxels, ix, iy, iz, sc.frame_inputs(0), stop)
            assert_pool(ses.scene.download(capi.BUF_VOXEL_BLOCKS), new, p.voxels, sc.name)
            assert (st["saturated"] > 0) == stop and st["saturated"] == DT.counts(facts)["saturated"]
        finally:
            ses.close()


@pytest.mark.gpu
def test_without_stats_nothing_differs(hip, oracle):
    """stats == NULL selects the kernels without the tallies: the same voxels."""
    for sc in (P.hash_scenario("f_rgb"), P.dense_scenario("s_rgb")):
        p = P.placement(oracle, sc)
        pools = []
        for stats in (True, False):
            ses = T.Session(hip, sc)
            try:
                P.upload(ses, p)
                assert (ses.scene.deintegrate(ses.view(0), ses.rs, keep_saturated=False, stats=stats) is not None) == stats
                pools.append(ses.scene.download(capi.BUF_VOXEL_BLOCKS))
            finally:
                ses.close()
        assert pools[0].tobytes() == pools[1].tobytes() and pools[0].tobytes() != p.voxels.tobytes(), sc.name


# ---- the sdf mirror and the directories ------------------------------------------------------------------------------------------------
def icp_maps(ses):
    v = ses.view(0)
    ses.scene.vis.CreateExpectedDepths(v.M_d, v.intr_d, ses.rs)
    ses.scene.vis.CreateICPMaps(v, ses.rs, ses.points, ses.normals)
    return {"raycast": ses.scene.download(capi.BUF_RAYCAST_RESULT, ses.rs), "points": ses.points.numpy(), "normals": ses.normals.numpy(),
            "image": ses.scene.download(capi.BUF_RAYCAST_IMAGE, ses.rs)}


def mirror_case(hip, oracle, expect_form):
    sc = P.hash_scenario("s")
    p = P.placement(oracle, sc)
    ses, vox, _, total = deintegrate_shots(hip, p, False)
    try:
        facts = A.audit(ses.scene, ses.rs, what=sc.name + " after the de-integration")
        if expect_form:
            assert facts["form"] == expect_form, facts["form"]
        # the placement's list again: both scenes cast through the same blocks
        ses.scene.upload(capi.BUF_VISIBLE_IDS, p.visible_ids, ses.rs)
        ses.scene.upload(capi.BUF_VISIBLE_TYPE, p.visible_type, ses.rs)
        ses.scene.set_counters(ses.rs, p.counters["lastFreeBlockId"], p.counters["lastFreeExcessListId"], p.counters["noVisibleEntries"])
        got = icp_maps(ses)
    finally:
        ses.close()
    fresh = T.Session(hip, sc)
    try:
        P.upload(fresh, p, voxels=vox)
        want = icp_maps(fresh)
    finally:
        fresh.close()
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), (sc.name, k)
    assert np.isfinite(want["points"][..., 3]).any() and (want["points"][..., 3] > 0).sum() > 1000, "the ray cast found no surface: the case is empty"
    assert total["touched"] > 100000


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(EC.FORMS))
def test_mirror_forms_stay_in_step(hip, oracle, form):
    with EC.environment(EC.FORMS[form]):
        mirror_case(hip, oracle, {"default": None, "paged": "paged", "mirror_off": "none"}[form])


@pytest.mark.gpu
def test_without_the_directories(hip, oracle):
    hip.check(hip.fn["debug_set"](5, 1), "debug_set")
    try:
        mirror_case(hip, oracle, None)
    finally:
        hip.check(hip.fn["debug_set"](5, 0), "debug_set")


# ---- a recorded frame goes first ---------------------------------------------------------------------------------------------------------
SMALL = T.Scenario(name="deintegrate_hash_s_160", w=160, h=120, frames=3, localBlockNum=0x4000)


@pytest.mark.gpu
def test_recorded_frame_is_launched_before_the_deintegration(hip):
    """Allocation and integration recorded under deferred fusion and not yet launched: the de-integration of the same frame finds it
    fused (an empty scene would give it nothing to visit)."""
    out = []
    for deferred in (True, False):
        ses = T.Session(hip, SMALL, deferred_fusion=deferred)
        try:
            ses.frame(0, fused=True)
            v = ses.view(1)
            ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
            ses.scene.reco.IntegrateIntoScene(v, ses.rs)          # deferred: recorded, nothing launched
            st = ses.scene.deintegrate(v, ses.rs, stats=True)
            out.append((st, ses.scene.download(capi.BUF_VOXEL_BLOCKS), ses.scene.download(capi.BUF_HASH_ENTRIES), ses.scene.counters(ses.rs)))
        finally:
            ses.close()
    (a, va, ha, ca), (b, vb, hb, cb) = out
    assert a == b and a["blocks"] > 500 and a["touched"] > 100000 and a["reset"] > 0, (a, b)
    assert va.tobytes() == vb.tobytes() and ha.tobytes() == hb.tobytes() and ca == cb


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def sha_of(ses):
    h = hashlib.sha256()
    st = scene_state(ses)
    st["voxels"] = ses.scene.download(capi.BUF_VOXEL_BLOCKS)
    for k in sorted(st):
        h.update(json.dumps(st[k], sort_keys=True).encode() if isinstance(st[k], dict) else st[k].tobytes())
    return h.hexdigest()


@pytest.mark.gpu
def test_every_refusal_leaves_the_scene_as_it_was(hip):
    colour = T.Scenario(name="deintegrate_hash_s_rgb_160", w=160, h=120, frames=1, localBlockNum=0x4000, voxelType=capi.VOXEL_S_RGB, colour=True)
    ses, other = T.Session(hip, colour), T.Session(hip, SMALL)
    try:
        ses.frame(0, fused=True)
        v = ses.view(0)
        before = sha_of(ses)
        vs = v.struct()
        fn = hip.fn["deintegrate_from_scene"]
        cfg = lambda k: C.byref(capi.DeintegrateConfig(k))
        no_depth, no_rgb = v.struct(), v.struct()
        no_depth.depth, no_rgb.rgb = None, None
        calls = {"null scene": lambda: fn(None, C.byref(vs), _P(ses.rs.h), None, None, None),
                 "null view": lambda: fn(_P(ses.scene.h), None, _P(ses.rs.h), None, None, None),
                 "null render state": lambda: fn(_P(ses.scene.h), C.byref(vs), None, None, None, None),
                 "null depth": lambda: fn(_P(ses.scene.h), C.byref(no_depth), _P(ses.rs.h), None, None, None),
                 "another scene's render state": lambda: fn(_P(ses.scene.h), C.byref(vs), _P(other.rs.h), None, None, None),
                 "colour voxels without rgb": lambda: fn(_P(ses.scene.h), C.byref(no_rgb), _P(ses.rs.h), None, None, None),
                 "keepSaturated 2": lambda: fn(_P(ses.scene.h), C.byref(vs), _P(ses.rs.h), cfg(2), None, None),
                 "keepSaturated -1": lambda: fn(_P(ses.scene.h), C.byref(vs), _P(ses.rs.h), cfg(-1), None, None)}
        for what, call in calls.items():
            assert call() == -1, what          # ITM_ERR_INVALID
            assert hip.fn["last_error"](), what
            assert sha_of(ses) == before, what
        with pytest.raises(capi.ItmError):
            ses.scene.deintegrate(v, ses.rs, keep_saturated=2)
        assert ses.scene.deintegrate(v, ses.rs, keep_saturated=True, stats=True)["touched"] > 0 and sha_of(ses) != before
    finally:
        ses.close()
        other.close()


# ---- the C++ adapters -----------------------------------------------------------------------------------------------------------------------
DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "deintegrate_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "deintegrate_demo")
N_FRAMES = 4


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_deintegrate_adapters_compile_and_link():
    assert os.path.exists(build_demo())


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "itm_hip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(itm_deintegrate_config),'
                   'sizeof(itm_deintegrate_stats), offsetof(itm_deintegrate_stats, colourReset), offsetof(itm_deintegrate_stats, saturated)); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(capi.DeintegrateConfig), C.sizeof(capi.DeintegrateStats), capi.DeintegrateStats.colourReset.offset,
                   capi.DeintegrateStats.saturated.offset] == [16, 64, 32, 20]


def word_digest(arr):
    w = np.frombuffer(np.ascontiguousarray(arr).tobytes(), np.uint32).astype(np.uint64)
    return "%016x" % int((w * (2 * np.arange(len(w), dtype=np.uint64) + 1)).sum(dtype=np.uint64))


def standard_frames():
    """The sphere in front of the wall from the parity trajectory, 160 x 120: raw frames, their poses, and a corrected pose (2 mm and
    half a degree off) for the frame that is moved."""
    w, h = 160, 120
    intr = synth.intrinsics_for(w, h)
    raw = np.stack([synth.raw_depth_mm(w, h, synth.parity_position(k), intr) for k in range(N_FRAMES)])
    poses = [synth.pose_matrix(synth.parity_position(k)) for k in range(N_FRAMES)]
    t = synth.parity_position(1)
    corrected = synth.pose_matrix_yaw((t[0] + F(0.002), t[1] - F(0.001), t[2] + F(0.0015)), 0.009)
    return raw, np.stack(poses + [corrected]).astype(F)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,j", [("reintegrate", 1), ("same", N_FRAMES - 1), ("remove", 1)])
def test_cpp_reintegrate_frame_equals_the_calls_made_by_hand(hip, tmp_path, mode, j):
    """ITMMainEngine_HIP::ReintegrateFrame / RemoveFrame against FindVisibleBlocks + deintegrate (+ AllocateSceneFromDepth +
    IntegrateIntoScene) through the binding, in every buffer.  `same`: the LAST frame taken out and fused again under its own pose --
    every block it sees existed when it was fused and was on its list, so no voxel loses an observation it never got (include/itm_hip.h
    says what happens otherwise) -- returns every weight exactly (none is saturated after four frames)."""
    raw, poses = standard_frames()
    raw.tofile(str(tmp_path / "frames.bin"))
    poses.tofile(str(tmp_path / "poses.bin"))
    got = json.loads(subprocess.run([build_demo(), str(tmp_path), mode, str(j)], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
    w, h, n = 160, 120, 160 * 120
    intr = synth.intrinsics_for(w, h)
    s = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.005), localBlockNum=0x4000)
    s.reco.ResetScene()
    s.set_deferred_fusion(True)
    rs, rs2 = s.vis.CreateRenderState((w, h)), s.vis.CreateRenderState((w, h))
    depth = capi.DevBuffer(hip, n * 4, np.float32, (h, w))
    pts = capi.DevBuffer(hip, n * 16, np.float32, (n, 4)); nrm = capi.DevBuffer(hip, n * 16, np.float32, (n, 4))

    def load(k):
        dev = hip.to_backend(raw[k])
        hip.check(hip.fn["convert_depth_affine"](_P(dev.ptr), _P(depth.ptr), w, h, 0.001, 0.0, None), "convert_depth_affine")
        hip.sync()
        dev.close()
    try:
        for k in range(N_FRAMES):
            load(k)
            s.process_frame(capi.View(depth, w, h, M_d=poses[k], intr_d=intr), rs, pts, nrm)
        load(j)
        weights = s.download(capi.BUF_VOXEL_BLOCKS)["w_depth"].copy()
        old, new = capi.View(depth, w, h, M_d=poses[j], intr_d=intr), capi.View(depth, w, h, M_d=poses[N_FRAMES if mode == "reintegrate" else j], intr_d=intr)
        s.vis.FindVisibleBlocks(old.M_d, intr, rs2)
        st = s.deintegrate(old, rs2, stats=True)
        if mode != "remove":
            s.reco.AllocateSceneFromDepth(new, rs2)
            s.reco.IntegrateIntoScene(new, rs2)
            s.flush(rs2)
        c = s.counters(rs)
        vox = s.download(capi.BUF_VOXEL_BLOCKS)
        want = dict(st, lastFreeBlockId=c["lastFreeBlockId"], lastFreeExcessListId=c["lastFreeExcessListId"], noVisibleEntries=c["noVisibleEntries"],
                    table=word_digest(s.download(capi.BUF_HASH_ENTRIES)), voxels=word_digest(vox), excess=word_digest(s.download(capi.BUF_EXCESS_LIST)),
                    allocList=word_digest(s.download(capi.BUF_ALLOCATION_LIST)), visibleIds=word_digest(s.download(capi.BUF_VISIBLE_IDS, rs)),
                    visibleType=word_digest(s.download(capi.BUF_VISIBLE_TYPE, rs)))
        print(got)
        assert got == want
        assert st["blocks"] > 500 and st["touched"] > 100000 and st["reset"] > 0 and st["saturated"] == 0, st
        if mode == "same":
            assert weights.max() < 100 and np.array_equal(vox["w_depth"], weights)
        else:
            assert not np.array_equal(vox["w_depth"], weights)
    finally:
        rs.close(); rs2.close(); s.close()
