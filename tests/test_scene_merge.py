"""itm_scene_merge (include/itm_hip.h): one TSDF scene fused into another on the GPU.

The product is compared, as whole arrays and bit for bit, with the restatement in tests/scene_merge_terms.py applied to the downloads
taken before the call.  The restatement itself is anchored without a GPU: its combine against the oracle's IntegrateGlobalIntoLocal
(the reference's CombineVoxelInformation), its allocation against hand-written tables, and its invariants on oracle scenes."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import scene_merge_terms as M
import swapped_cases
import test_swapping
from infinitam_amd import capi, synth
from swapped_cases import swapping_scene       # (test_scene_resample builds on it through this module)

W, H = 320, 240
POOL = 0x4000              # voxel blocks per scene: the scenes below hold a few thousand (whole pools are downloaded and compared)
_P = C.c_void_p


def scenario(name, **kw):
    kw.setdefault("localBlockNum", POOL)
    return T.Scenario(name=name, w=W, h=H, voxelSize=0.01, **kw)


def scenario_a(**kw):
    return scenario("merge_A", frames=3, **kw)


def scenario_b(**kw):
    """Overlaps A: the same wall and sphere from a camera that turns and stands a little aside."""
    kw.setdefault("origin", (0.05, 0.02, -0.1))
    return scenario("merge_B", frames=3, trajectory="yaw", yaw_rate=0.1, **kw)


def build(be, sc, frames=None, deferred=True):
    ses = T.Session(be, sc, deferred_fusion=deferred)
    for k in range(sc.frames if frames is None else frames):
        ses.frame(k, fused=True)
    return ses


def snapshot(scene):
    st = M.state_of(scene)
    if scene.cfg.useSwapping:
        st["swap"] = scene.download(capi.BUF_SWAP_STATES)
    return st


def merge_and_compare(dst, src, slots=None, what="merge"):
    """dst.merge_from(src) against the restatement on the downloads taken before the call; src must come out untouched."""
    d0, s0 = snapshot(dst), snapshot(src)
    want, wstats, _ = M.merge(d0, s0, slots)
    stats = dst.merge_from(src, slots)
    got, s1 = snapshot(dst), snapshot(src)
    print(what, "stats", stats, "restatement", wstats)
    assert stats == wstats, "%s: stats %s vs restatement %s" % (what, stats, wstats)
    M.assert_state_equal(got, want, what, T.assert_fields_equal)
    M.assert_state_equal(s1, s0, what + " (src untouched)", T.assert_fields_equal)
    assert np.array_equal(s1["alloc"], s0["alloc"]) and np.array_equal(s1["excess"], s0["excess"])
    if "swap" in d0:
        assert np.array_equal(got["swap"], d0["swap"]), what + ": swap states of dst changed"
    return stats, got


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("voxel,colour", [(capi.VOXEL_S, False), (capi.VOXEL_F_RGB, True)])
def test_restated_combine_is_the_reference_combine(oracle, voxel, colour):
    """The oracle's IntegrateGlobalIntoLocal (CombineVoxelInformation, pinned to the reference by test_swapping) on the frames where the
    camera turns back: restated combine of (cached block, block before) == block after, bit for bit, for every combined block."""
    be = oracle
    intr, seq = test_swapping.poses_and_depths()
    s = be.create_scene(voxel, capi.INDEX_HASH, capi.default_params(voxelSize=0.005), useSwapping=True)
    s.reco.ResetScene()
    rs = s.vis.CreateRenderState((W, H))
    rgb = be.to_backend(synth.rgb_frame(W, H)) if colour else None
    cap, combined = 0x1000, 0
    for k, (Mk, depth) in enumerate(seq[:9]):
        v = capi.View(be.to_backend(depth), W, H, M_d=Mk, intr_d=intr, rgb=rgb, w_rgb=W, h_rgb=H, intr_rgb=intr)
        s.reco.AllocateSceneFromDepth(v, rs)
        s.reco.IntegrateIntoScene(v, rs)
        if k >= 7:
            hsh, swap, flags = s.download(capi.BUF_HASH_ENTRIES), s.download(capi.BUF_SWAP_STATES), s.global_cache_flags()
            ids = np.nonzero(swap == 1)[0][:cap]                  # LoadFromGlobalMemory: the first entries in state 1, table order
            ids = ids[(flags[ids] != 0) & (hsh["ptr"][ids] >= 0)]
            before = s.download(capi.BUF_VOXEL_BLOCKS).reshape(-1, 512)
            cached = np.stack([s.global_cache_block(int(e)) for e in ids]) if len(ids) else None
        s.swap_integrate_global_into_local(rs)
        if k >= 7 and len(ids):
            after = s.download(capi.BUF_VOXEL_BLOCKS).reshape(-1, 512)
            ptr = hsh["ptr"][ids]
            want = M.combine_voxels(cached, before[ptr], voxel, int(s.params.maxW))
            T.assert_fields_equal(want.reshape(-1), after[ptr].reshape(-1), "frame %d: combined blocks" % k)
            assert int(np.count_nonzero(cached["w_depth"])) > 0
            combined += len(ids)
        s.swap_save_to_global_memory(rs)
    rs.close(); s.close()
    assert combined >= 1000, combined            # the anchoring condition


def hand_table(entries, n=12):
    h = np.zeros(n, capi.HASH_ENTRY_DTYPE)
    h["ptr"] = -2
    for slot, (pos, off, ptr) in entries.items():
        h[slot]["pos"], h[slot]["offset"], h[slot]["ptr"] = pos, off, ptr
    return h


def hand_state(entries, blocks, lastFreeBlockId, lastFreeExcessListId, seed):
    """seed 0: a dst (8 heads + 4 excess entries); seed 1: a src (a table of 16 slots, its own random voxels)."""
    rng = np.random.default_rng(seed)
    vox = np.zeros(blocks * 512, capi.VOXEL_DTYPES[capi.VOXEL_S])
    vox["sdf"] = rng.integers(-32767, 32768, len(vox)); vox["w_depth"] = rng.integers(0, 101, len(vox))
    return dict(hash=hand_table(entries, 12 if seed == 0 else 16), voxels=vox, voxelType=capi.VOXEL_S, maxW=100, alloc=np.arange(blocks, dtype=np.int32),
                excess=np.arange(4, dtype=np.int32), lastFreeBlockId=lastFreeBlockId, lastFreeExcessListId=lastFreeExcessListId, bucketNum=8)


def table_of(state):
    return {i: (tuple(int(c) for c in e["pos"]), int(e["offset"]), int(e["ptr"])) for i, e in enumerate(state["hash"]) if e["ptr"] >= -1}


def test_restated_allocation_known_answers():
    """bucketNum = 8, four excess entries; (x, 0, 0) hashes to (5 x) mod 8, so x = 0, 8, 16 share head 0, x = 1, 9 head 5, x = 7, 15 head 3."""
    assert [M.hash_index((x, 0, 0), 7) for x in (0, 8, 16, 1, 9, 7, 15, 2)] == [0, 0, 0, 5, 5, 3, 3, 2]

    # (A) two positions on one occupied head (a chain of three after two rounds), two on one empty head (the loser becomes its child),
    # one present, one swapped out of src
    dst = hand_state({0: ((0, 0, 0), 0, 5)}, 6, 4, 3, 0)
    src = hand_state({0: ((0, 0, 0), 0, 0), 1: ((8, 0, 0), 0, 1), 2: ((16, 0, 0), 0, 2), 3: ((1, 0, 0), 0, 3), 4: ((9, 0, 0), 0, 4), 5: ((2, 0, 0), 0, -1)}, 6, -1, 3, 1)
    out, stats, where = M.merge(dst, src)
    assert table_of(out) == {0: ((0, 0, 0), 4, 5), 11: ((16, 0, 0), 2, 4), 9: ((8, 0, 0), 0, 1),        # round 1: slot 2 beats slot 1 on tail 0; round 2: slot 1 on tail 11
                             5: ((9, 0, 0), 3, 3), 10: ((1, 0, 0), 0, 2)}                               # round 1: slot 4 beats slot 3 on head 5; round 2: slot 3 on tail 5
    assert (out["lastFreeBlockId"], out["lastFreeExcessListId"]) == (0, 0)
    assert stats == dict(rounds=3, considered=5, alreadyPresent=1, allocated=4, combined=5, unserved=0, srcWithoutBlock=1, dstSwappedOut=0)
    assert where == {0: 0, 1: 9, 2: 11, 3: 10, 4: 5}
    # the combine: a block allocated by the merge held the initial voxels in a real scene; here the pool is random on both sides
    want = M.combine_voxels(src["voxels"][2 * 512:3 * 512], dst["voxels"][4 * 512:5 * 512], capi.VOXEL_S, 100)
    T.assert_fields_equal(out["voxels"][4 * 512:5 * 512], want, "block of src slot 2")
    T.assert_fields_equal(out["voxels"][:512], dst["voxels"][:512], "a block nobody took")

    # (B) the excess list runs dry while voxel blocks remain: the excess request on tail 3 is not served and takes NO voxel block,
    # the ordered request behind it (head 5) is served with the next one
    dst = hand_state({0: ((0, 0, 0), 0, 5), 3: ((7, 0, 0), 0, 6)}, 7, 4, 0, 0)
    src = hand_state({1: ((8, 0, 0), 0, 0), 2: ((15, 0, 0), 0, 1), 3: ((1, 0, 0), 0, 2)}, 3, -1, 3, 1)
    out, stats, where = M.merge(dst, src)
    assert table_of(out) == {0: ((0, 0, 0), 1, 5), 8: ((8, 0, 0), 0, 4), 3: ((7, 0, 0), 0, 6), 5: ((1, 0, 0), 0, 3)}
    assert (out["lastFreeBlockId"], out["lastFreeExcessListId"]) == (2, -1)
    assert stats == dict(rounds=2, considered=3, alreadyPresent=0, allocated=2, combined=2, unserved=1, srcWithoutBlock=0, dstSwappedOut=0)

    # (C) the voxel pool runs dry: head 2 takes the last block, head 5 stays empty; the counter stops at -1
    dst = hand_state({}, 1, 0, 3, 0)
    src = hand_state({1: ((1, 0, 0), 0, 0), 2: ((2, 0, 0), 0, 1)}, 2, -1, 3, 1)
    out, stats, where = M.merge(dst, src)
    assert table_of(out) == {2: ((2, 0, 0), 0, 0)}
    assert (out["lastFreeBlockId"], out["lastFreeExcessListId"]) == (-1, 3)
    assert stats == dict(rounds=2, considered=2, alreadyPresent=0, allocated=1, combined=1, unserved=1, srcWithoutBlock=0, dstSwappedOut=0)

    # a slot list: any order, duplicates once
    dst = hand_state({0: ((0, 0, 0), 0, 5)}, 6, 4, 3, 0)
    src = hand_state({0: ((0, 0, 0), 0, 0), 1: ((8, 0, 0), 0, 1), 3: ((1, 0, 0), 0, 3)}, 6, -1, 3, 1)
    out, stats, where = M.merge(dst, src, [3, 0, 3, 7])
    assert table_of(out) == {0: ((0, 0, 0), 0, 5), 5: ((1, 0, 0), 0, 4)} and stats["considered"] == 2 and stats["allocated"] == 1


def check_invariants(before, after, src, stats):
    h = after["hash"]
    live = h[h["ptr"] >= -1]
    pos = {tuple(p) for p in live["pos"].tolist()}
    assert len(pos) == len(live), "a position occurs twice"
    union = {tuple(p) for p in before["hash"]["pos"][before["hash"]["ptr"] >= -1].tolist()} | {tuple(p) for p in src["hash"]["pos"][src["hash"]["ptr"] >= 0].tolist()}
    if stats["unserved"] == 0:
        assert pos == union
    else:
        assert pos < union
    used = h["ptr"][h["ptr"] >= 0]
    free = after["alloc"][:max(after["lastFreeBlockId"] + 1, 0)]
    assert len(np.unique(used)) == len(used) and not np.intersect1d(used, free).size
    bucketNum = after["bucketNum"]
    for head in np.nonzero(h["ptr"][:bucketNum] >= -1)[0]:
        idx, steps = int(head), 0
        while h["offset"][idx] >= 1:
            idx = bucketNum + int(h["offset"][idx]) - 1
            steps += 1
            assert steps <= len(h) - bucketNum, "a chain does not end"
    assert before["lastFreeBlockId"] - after["lastFreeBlockId"] == stats["allocated"]
    new_excess = int(np.count_nonzero(h["ptr"][bucketNum:] >= -1)) - int(np.count_nonzero(before["hash"]["ptr"][bucketNum:] >= -1))
    assert before["lastFreeExcessListId"] - after["lastFreeExcessListId"] == new_excess


@pytest.mark.parametrize("bucketNum,excessNum", [(0, 0), (0x800, 0x1800)])
def test_restatement_invariants_on_oracle_scenes(oracle, bucketNum, excessNum):
    a, b = build(oracle, scenario_a(bucketNum=bucketNum, excessNum=excessNum)), build(oracle, scenario_b(bucketNum=bucketNum, excessNum=excessNum))
    sa, sb = M.state_of(a.scene), M.state_of(b.scene)
    out, stats, _ = M.merge(sa, sb)
    assert stats["alreadyPresent"] > 0 and stats["allocated"] > 0 and stats["unserved"] == 0
    assert stats["considered"] == stats["alreadyPresent"] + stats["allocated"] == stats["combined"]
    check_invariants(sa, out, sb, stats)
    a.close(); b.close()


def test_scene_merge_is_declared_and_bound(hip_host):
    assert "scene_merge" in capi.declared_functions() and "scene_merge" in capi._HOST_IO_SIGS
    assert "scene_merge" in hip_host.fn
    assert C.sizeof(capi.MergeStats) == 32


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("voxel", [capi.VOXEL_S, capi.VOXEL_F, capi.VOXEL_S_RGB, capi.VOXEL_F_RGB])
def test_merge_of_overlapping_scenes_equals_the_restatement(hip, voxel):
    colour = voxel in (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB)
    a, b = build(hip, scenario_a(voxelType=voxel, colour=colour)), build(hip, scenario_b(voxelType=voxel, colour=colour))
    stats, _ = merge_and_compare(a.scene, b.scene, what="case a, voxel type %d" % voxel)
    assert stats["alreadyPresent"] > 0 and stats["allocated"] > 0 and stats["rounds"] >= 2
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bucketNum,excessNum,runs_dry", [(0x800, 0x1800, False), (0x1000, 0x400, True)])
def test_merge_into_tiny_tables_equals_the_restatement(hip, bucketNum, excessNum, runs_dry):
    # runs_dry: B stands 0.5 m aside, so that few of its ~2 500 blocks are in A already; A has used 225 of the 1024 excess entries and
    # the 4096 heads cannot take the ~5 300 blocks of the union (the restatement on the oracle's scenes leaves 41 participants unserved)
    kw = dict(origin=(0.3, 0.1, -0.4)) if runs_dry else {}
    a, b = build(hip, scenario_a(bucketNum=bucketNum, excessNum=excessNum)), build(hip, scenario_b(bucketNum=bucketNum, excessNum=excessNum, **kw))
    stats, got = merge_and_compare(a.scene, b.scene, what="case b, %#x + %#x" % (bucketNum, excessNum))
    assert stats["rounds"] >= 3, "no chain grew by more than one entry"
    if runs_dry:
        assert stats["unserved"] > 0 and got["lastFreeExcessListId"] == -1 and got["lastFreeBlockId"] >= 0
    a.close(); b.close()


@pytest.mark.gpu
def test_merge_with_an_exhausted_voxel_pool_equals_the_restatement(hip):
    probe = build(hip, scenario_a())
    used = POOL - 1 - probe.scene.counters()["lastFreeBlockId"]
    probe.close()
    a, b = build(hip, scenario_a(localBlockNum=used + 100)), build(hip, scenario_b())
    stats, got = merge_and_compare(a.scene, b.scene, what="case c")           # (merge_from raises unless the call returned ITM_OK)
    assert stats["unserved"] > 0 and stats["allocated"] == 100 and got["lastFreeBlockId"] == -1
    a.close(); b.close()


@pytest.mark.gpu
def test_merge_of_a_visible_list_equals_the_restatement(hip):
    a, b = build(hip, scenario_a()), build(hip, scenario_b())
    n = b.scene.counters(b.rs)["noVisibleEntries"]
    ids = b.scene.download(capi.BUF_VISIBLE_IDS, b.rs)[:n].copy()
    rng = np.random.default_rng(7)
    ids = ids[: n // 2]                                                       # (a true subset of B)
    slots = rng.permutation(np.concatenate([ids, ids[:17], ids[5:9]])).astype(np.int32)
    stats, _ = merge_and_compare(a.scene, b.scene, slots, what="case d")
    assert stats["considered"] == len(ids) and stats["allocated"] > 0
    # the same through a device buffer the caller owns
    a2 = build(hip, scenario_a())
    dev = hip.to_backend(slots)
    stats2 = a2.scene.merge_from(b.scene, dev)
    assert stats2 == stats
    T.assert_fields_equal(a2.scene.download(capi.BUF_HASH_ENTRIES), a.scene.download(capi.BUF_HASH_ENTRIES), "device list vs host list")
    a.close(); b.close(); a2.close()


def upload_state(ses, st, live):
    """The scene state `st` and the visible list of the render state `live` (the merge leaves dst's render states as they are, and the
    next frame keeps what was visible before: the twin must start from the same list)."""
    for which, key in ((capi.BUF_HASH_ENTRIES, "hash"), (capi.BUF_EXCESS_LIST, "excess"), (capi.BUF_ALLOCATION_LIST, "alloc"), (capi.BUF_VOXEL_BLOCKS, "voxels")):
        ses.scene.upload(which, st[key])
    ses.scene.upload(capi.BUF_VISIBLE_IDS, live.scene.download(capi.BUF_VISIBLE_IDS, live.rs), ses.rs)
    ses.scene.upload(capi.BUF_VISIBLE_TYPE, live.scene.download(capi.BUF_VISIBLE_TYPE, live.rs), ses.rs)
    ses.scene.set_counters(ses.rs, st["lastFreeBlockId"], st["lastFreeExcessListId"], live.scene.counters(live.rs)["noVisibleEntries"])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "no directory", "no sdf mirror", "shifted origin"])
def test_derived_structures_after_a_merge_are_those_of_an_upload(hip, oracle, form):
    """Case e: the merged scene and a twin that received the merged state through itm_upload (which rebuilds the occupancy bits, the
    directories and the mirror from the table) run two further frames; every buffer stays identical, and the first frame's ray cast
    equals the oracle's on the same state."""
    key = {"no directory": 5, "no sdf mirror": 12}.get(form)
    if key:
        hip.check(hip.fn["debug_set"](key, 1), "debug_set")
    try:
        # shifted origin: B lies 6 m away, so most of its blocks are outside the cubes placed for A (512 / 256 blocks of 8 cm around A)
        origin = (25.0, -22.0, 30.0) if form == "shifted origin" else (0.05, 0.02, -0.1)
        sa, sb = scenario_a(), scenario_b(origin=origin)
        a, b = build(hip, sa), build(hip, sb)
        stats, merged = merge_and_compare(a.scene, b.scene, what="case e (%s)" % form)
        assert stats["allocated"] > 0
        if form == "shifted origin":
            org = np.array(a.scene.accel_info()["origin_directory"])
            pos = merged["hash"]["pos"][merged["hash"]["ptr"] >= 0].astype(np.int64)
            assert int(np.count_nonzero(np.any((pos < org) | (pos >= org + 512), axis=1))) > 0, "every block lies inside dst's cubes"
        twin, ref = T.Session(hip, sa), T.Session(oracle, sa)
        upload_state(twin, merged, a); upload_state(ref, merged, a)
        # further frames: one that looks where A looked, one that looks where B looked
        plan = [(sa, 3), (sb, 3)]
        for i, (sc, k) in enumerate(plan):
            for ses in (a, twin) + ((ref,) if i == 0 else ()):
                ses.sc = sc
                ses.frame(k, fused=True)
            ra, rt = a.snapshot(), twin.snapshot()
            ra.counters, rt.counters = [a.scene.counters(a.rs)], [twin.scene.counters(twin.rs)]
            T.assert_fields_equal(ra.hash, rt.hash, "frame %d: hash" % i)
            T.assert_fields_equal(ra.voxels, rt.voxels, "frame %d: voxels" % i)
            assert np.array_equal(ra.excess, rt.excess) and np.array_equal(ra.alloc_list, rt.alloc_list)
            assert ra.counters[0]["lastFreeBlockId"] == rt.counters[0]["lastFreeBlockId"] and ra.counters[0]["lastFreeExcessListId"] == rt.counters[0]["lastFreeExcessListId"]
            assert np.array_equal(ra.raycast, rt.raycast) and np.array_equal(ra.points, rt.points) and np.array_equal(ra.normals, rt.normals), "frame %d: maps" % i
            if i == 0:
                ro = ref.snapshot()
                assert np.array_equal(ra.raycast[..., 3], ro.raycast[..., 3]), "hit mask vs oracle"
                hit = ra.raycast[..., 3] > 0
                assert np.count_nonzero(hit) > 5000
                assert np.array_equal(ra.raycast[hit], ro.raycast[hit]) and np.array_equal(ra.points, ro.points), "ray cast vs oracle"
        a.close(); b.close(); twin.close(); ref.close()
    finally:
        if key:
            hip.check(hip.fn["debug_set"](key, 0), "debug_set")


assert (swapped_cases.W, swapped_cases.H, swapped_cases.POOL) == (W, H, POOL)


@pytest.mark.gpu
def test_merge_between_swapping_scenes_equals_the_restatement(hip):
    (src, rs_s), (dst, rs_d) = swapping_scene(hip, 1), swapping_scene(hip, 2)
    # what the set-up is for (stated from the inputs, not from the call under test; the two tables hold the scene's entries in the same slots)
    sp, dp = src.download(capi.BUF_HASH_ENTRIES)["ptr"], dst.download(capi.BUF_HASH_ENTRIES)["ptr"]
    assert np.count_nonzero(sp == -1) > 100 and np.count_nonzero((sp >= 0) & (dp == -1)) > 100 and np.count_nonzero((sp >= 0) & (dp >= 0)) > 100
    stats, _ = merge_and_compare(dst, src, what="case f")
    assert stats["srcWithoutBlock"] == int(np.count_nonzero(sp == -1)) and stats["dstSwappedOut"] == int(np.count_nonzero((sp >= 0) & (dp == -1)))
    rs_s.close(); rs_d.close(); src.close(); dst.close()


@pytest.mark.gpu
def test_merge_of_dense_scenes_equals_the_restatement(hip):
    kw = dict(indexType=capi.INDEX_DENSE, denseSize=(64, 64, 64), denseOffset=(-32, -32, 95), localBlockNum=0)
    a, b = build(hip, scenario_a(**kw)), build(hip, scenario_b(**kw))
    d0, s0 = M.state_of(a.scene), M.state_of(b.scene)
    assert np.count_nonzero(s0["voxels"]["w_depth"]) > 1000 and np.count_nonzero(d0["voxels"]["w_depth"]) > 1000
    want, wstats, _ = M.merge(d0, s0)
    stats = a.scene.merge_from(b.scene)
    assert (stats["considered"], stats["combined"]) == (1, 1) == (wstats["considered"], wstats["combined"])
    T.assert_fields_equal(a.scene.download(capi.BUF_VOXEL_BLOCKS), want["voxels"], "case g: voxels")
    T.assert_fields_equal(b.scene.download(capi.BUF_VOXEL_BLOCKS), s0["voxels"], "case g: src voxels")
    a.close(); b.close()


@pytest.mark.gpu
def test_merge_launches_recorded_frames_first(hip):
    """Case h: both scenes hold recorded, unflushed engine calls when merge_from is called; the result is that of the eager run."""
    results = []
    for recorded in (True, False):
        pair = []
        for sc in (scenario_a(), scenario_b()):
            ses = build(hip, sc, frames=2, deferred=recorded)
            v = ses.view(2)
            ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
            ses.scene.reco.IntegrateIntoScene(v, ses.rs)
            ses.scene.vis.CreateExpectedDepths(v.M_d, v.intr_d, ses.rs)        # recorded: nothing of frame 2 has been launched yet
            pair.append((ses, v))
        (a, _), (b, _) = pair
        if recorded:
            stats = a.scene.merge_from(b.scene)
            got = snapshot(a.scene)
        else:
            stats, got = merge_and_compare(a.scene, b.scene, what="case h (eager)")
        results.append((stats, got))
        a.close(); b.close()
    assert results[0][0] == results[1][0] and results[0][0]["allocated"] > 0
    M.assert_state_equal(results[0][1], results[1][1], "case h: recorded vs eager", T.assert_fields_equal)


@pytest.mark.gpu
def test_merge_refusals_leave_dst_untouched(hip):
    a = build(hip, scenario_a(), frames=1)
    before = snapshot(a.scene)
    entries = len(before["hash"])

    def refused(dst, src, slots=None):
        dev = hip.to_backend(np.asarray(slots, np.int32)) if slots is not None else None
        rc = hip.fn["scene_merge"](_P(dst.h), _P(src.h), _P(dev.ptr if dev else None), len(slots) if slots is not None else 0, None, None)
        hip.sync()
        return rc == capi.ERR_INVALID and len(hip.fn["last_error"]() or b"") > 0

    other_type = hip.create_scene(capi.VOXEL_F, capi.INDEX_HASH, capi.default_params(voxelSize=0.01), localBlockNum=POOL)
    other_size = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=float(np.nextafter(np.float32(0.01), np.float32(1)))), localBlockNum=POOL)
    same = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.01), localBlockNum=POOL)
    dense = hip.create_scene(capi.VOXEL_S, capi.INDEX_DENSE, capi.default_params(voxelSize=0.01), denseSize=(64, 64, 64))
    dense2 = hip.create_scene(capi.VOXEL_S, capi.INDEX_DENSE, capi.default_params(voxelSize=0.01), denseSize=(64, 64, 64))
    for s in (other_type, other_size, same, dense, dense2):
        s.reco.ResetScene()
    assert refused(a.scene, other_type), "voxel type mismatch"
    assert refused(a.scene, other_size), "voxelSize differing in the last bit"
    assert refused(a.scene, a.scene), "dst is src"
    assert refused(a.scene, dense), "hash with dense"
    assert refused(a.scene, same, [0, entries, 3]) and refused(a.scene, same, [-1]), "a slot outside the table"
    after = snapshot(a.scene)
    M.assert_state_equal(after, before, "refusals", T.assert_fields_equal)
    assert np.array_equal(after["alloc"], before["alloc"]) and np.array_equal(after["excess"], before["excess"])
    d0 = dense.download(capi.BUF_VOXEL_BLOCKS)
    assert refused(dense, dense2, [0]), "dense with a slot list"
    T.assert_fields_equal(dense.download(capi.BUF_VOXEL_BLOCKS), d0, "dense dst after a refusal")
    assert same.merge_from(a.scene)["allocated"] > 0            # and the call that is in order goes through
    for s in (other_type, other_size, same, dense, dense2):
        s.close()
    a.close()


DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "scene_merge_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "scene_merge_demo")


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_merge_adapters_compile_and_link():
    assert os.path.exists(build_demo())


def word_digest(arr):
    w = np.frombuffer(np.ascontiguousarray(arr).tobytes(), np.uint32).astype(np.uint64)
    return "%016x" % int((w * (2 * np.arange(len(w), dtype=np.uint64) + 1)).sum(dtype=np.uint64))


@pytest.mark.gpu
def test_cpp_merge_demo_equals_the_python_path(hip):
    exe = build_demo()
    got = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
    w, h, P = 160, 120, 160 * 120
    scenes = []
    for z, tx0 in ((1.5, 0.0), (1.52, -0.4)):
        s = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.01), localBlockNum=0x2000, bucketNum=0x1000, excessNum=0x400)
        s.reco.ResetScene()
        s.set_deferred_fusion(True)
        rs = s.vis.CreateRenderState((w, h))
        depth = hip.to_backend(np.full((h, w), z, np.float32))
        pts = capi.DevBuffer(hip, P * 16, np.float32, (P, 4)); nrm = capi.DevBuffer(hip, P * 16, np.float32, (P, 4))
        for k in range(2):
            Mk = np.eye(4, dtype=np.float32); Mk[0, 3] = np.float32(tx0) - np.float32(0.01) * np.float32(k)
            v = capi.View(depth, w, h, M_d=np.ascontiguousarray(Mk.T).reshape(16), intr_d=(145.0, 145.0, 80.0, 60.0))
            s.reco.AllocateSceneFromDepth(v, rs)
            s.reco.IntegrateIntoScene(v, rs)
            s.vis.CreateExpectedDepths(v.M_d, v.intr_d, rs)
            s.vis.CreateICPMaps(v, rs, pts, nrm)
        scenes.append((s, rs))
    (a, rs_a), (b, rs_b) = scenes
    n = b.counters(rs_b)["noVisibleEntries"]
    stats = a.merge_from(b, b.download(capi.BUF_VISIBLE_IDS, rs_b)[:n].copy())
    c = a.counters()
    assert stats["allocated"] > 0 and stats["alreadyPresent"] > 0
    for k, v in stats.items():
        assert got[k] == v, (k, got, stats)
    assert (got["lastFreeBlockId"], got["lastFreeExcessListId"]) == (c["lastFreeBlockId"], c["lastFreeExcessListId"])
    assert got["table"] == word_digest(a.download(capi.BUF_HASH_ENTRIES)) and got["voxels"] == word_digest(a.download(capi.BUF_VOXEL_BLOCKS))
    # two main engines: MergeSceneFrom brings B's blocks into A's scene, which goes on taking frames
    eng = json.loads(subprocess.run([exe, "--engines"], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
    assert eng["allocated"] > 0 and eng["alreadyPresent"] > 0 and eng["unserved"] == 0
    assert eng["considered"] == eng["src_blocks"] and eng["blocks_after"] == eng["blocks_before"] + eng["allocated"]
    for s, rs in scenes:
        rs.close(); s.close()
