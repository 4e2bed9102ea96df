"""itm_scene_coarsen (include/itm_hip.h): a TSDF scene resampled into one of twice the voxel size on the GPU (level of detail).

The product is compared, as whole arrays and bit for bit, with the restatement in tests/scene_coarsen_terms.py applied to the downloads
taken before the call; there is no tolerance anywhere.  The restatement itself is anchored without a GPU: its voxel arithmetic against
hand cases, its allocation against a hand-written table, its invariants and its mesh on oracle scenes."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import scene_coarsen_terms as K
import scene_merge_terms as M
import test_scene_merge as TM
import test_swapping
from infinitam_amd import capi
from infinitam_amd.capi import Mesh

W, H = TM.W, TM.H
FINE, COARSE, MU = 0.01, 0.02, 0.04
POOL = TM.POOL             # voxel blocks of a fine scene (whole pools are downloaded and compared)
CPOOL = 0x800              # ... of a coarse scene on the GPU: A needs 256
_P = C.c_void_p


def fine_a(**kw):
    return TM.scenario_a(mu=MU, **kw)


def fine_b(**kw):
    return TM.scenario_b(mu=MU, **kw)


def coarse(like=None, **kw):
    """The scenario of a coarse scene: twice the voxel size, the same mu; camera and trajectory of `like` (default A)."""
    like = like or fine_a()
    kw.setdefault("localBlockNum", CPOOL)
    return T.Scenario(name=like.name, w=W, h=H, voxelSize=COARSE, mu=MU, frames=like.frames, trajectory=like.trajectory, yaw_rate=like.yaw_rate,
                      origin=like.origin, voxelType=like.voxelType, colour=like.colour, indexType=like.indexType, **kw)


def dense_arg(dst, src):
    if dst.is_hash:
        return None
    return (tuple(src.cfg.denseSize), tuple(src.cfg.denseOffset), tuple(dst.cfg.denseSize), tuple(dst.cfg.denseOffset))


def coarsen_and_compare(dst, src, slots=None, what="coarsen"):
    """dst.coarsen_from(src) against the restatement on the downloads taken before the call; src must come out untouched."""
    d0, s0 = TM.snapshot(dst), TM.snapshot(src)
    want, wstats, where = K.coarsen(d0, s0, slots, dense_arg(dst, src))
    stats = dst.coarsen_from(src, slots)
    got, s1 = TM.snapshot(dst), TM.snapshot(src)
    print(what, "stats", stats, "restatement", wstats)
    assert stats == wstats, "%s: stats %s vs restatement %s" % (what, stats, wstats)
    if dst.is_hash:
        M.assert_state_equal(got, want, what, T.assert_fields_equal)
        M.assert_state_equal(s1, s0, what + " (src untouched)", T.assert_fields_equal)
        assert np.array_equal(s1["alloc"], s0["alloc"]) and np.array_equal(s1["excess"], s0["excess"])
    else:
        T.assert_fields_equal(got["voxels"], want["voxels"], what + ": voxels")
        T.assert_fields_equal(s1["voxels"], s0["voxels"], what + ": src voxels")
    if "swap" in d0:
        assert np.array_equal(got["swap"], d0["swap"]), what + ": swap states of dst changed"
    return stats, got, d0, where


def blocks_of(state, slots):
    return state["voxels"].reshape(-1, 512)[state["hash"]["ptr"][slots]]


def assert_only_D_changed(before, after, where, what):
    """Every voxel block of the pool outside D holds what it held."""
    touched = np.zeros(len(after["voxels"]) // 512, bool)
    ptr = after["hash"]["ptr"][sorted(set(where.values()))]
    touched[ptr[ptr >= 0]] = True
    T.assert_fields_equal(after["voxels"].reshape(-1, 512)[~touched].reshape(-1), before["voxels"].reshape(-1, 512)[~touched].reshape(-1), what + ": blocks outside D")


# ---- CPU: the restatement's voxel arithmetic -----------------------------------------------------------------------------------------

def hand_src(voxelType, blocks):
    """A src state holding `blocks` = {position: [8, 8, 8] structured voxels in z, y, x order}; a table as large as needed, no chains."""
    n = len(blocks)
    h = np.zeros(n, capi.HASH_ENTRY_DTYPE)
    vox = K.default_voxels((n, 8, 8, 8), voxelType)
    for i, (pos, v) in enumerate(sorted(blocks.items())):
        h[i]["pos"], h[i]["ptr"] = pos, i
        vox[i] = v
    return dict(hash=h, voxels=vox.reshape(-1), voxelType=voxelType, maxW=100)


def ramp_blocks(voxelType, lo, hi, f, w):
    """Blocks lo .. hi - 1 per axis whose voxel at p holds sdf f(px, py, pz) and weight w."""
    out = {}
    ax = np.arange(8)
    for bz in range(lo, hi):
        for by in range(lo, hi):
            for bx in range(lo, hi):
                v = K.default_voxels((8, 8, 8), voxelType)
                z, y, x = np.meshgrid(8 * bz + ax, 8 * by + ax, 8 * bx + ax, indexing="ij")
                v["sdf"], v["w_depth"] = f(x, y, z), w
                out[(bx, by, bz)] = v
    return out


@pytest.mark.parametrize("voxelType", [capi.VOXEL_S, capi.VOXEL_F])
def test_affine_sdf_and_constant_weight_are_reproduced_exactly(voxelType):
    """3^3 blocks around the origin, constant weight, an affine integer ramp: coarse == fine[2q] at every voxel whose 27 taps are stored."""
    def f(x, y, z):
        v = 3 * x - 5 * y + 7 * z + 11
        return v if voxelType == capi.VOXEL_S else v.astype(np.float32) * np.float32(0.03125)
    src = hand_src(voxelType, ramp_blocks(voxelType, -1, 2, f, 37))
    positions = np.array([(bx, by, bz) for bz in (-1, 0) for by in (-1, 0) for bx in (-1, 0)])
    got = K.coarse_blocks(src, positions, 100).reshape(-1, 8, 8, 8)
    checked = 0
    ax = np.arange(8)
    for B, blk in zip(positions, got):
        z, y, x = np.meshgrid(8 * B[2] + ax, 8 * B[1] + ax, 8 * B[0] + ax, indexing="ij")
        interior = (2 * x - 1 >= -8) & (2 * x + 1 < 16) & (2 * y - 1 >= -8) & (2 * y + 1 < 16) & (2 * z - 1 >= -8) & (2 * z + 1 < 16)
        assert np.array_equal(blk["sdf"][interior], f(2 * x, 2 * y, 2 * z)[interior]) and np.all(blk["w_depth"][interior] == 37)
        checked += int(np.count_nonzero(interior))
    assert checked == 11 ** 3            # fine voxels -8 .. 15 are stored: coarse voxels -3 .. 7 per axis have every tap (-4 reads -9)
    # a voxel at the edge of the stored cube has absent taps: its weight is smaller, its sdf is still a mean of stored values
    edge = K.coarse_blocks(src, np.array([(-1, -1, -1)]), 100).reshape(8, 8, 8)[4, 4, 4]          # coarse voxel (-4, -4, -4): tap -9 is absent
    assert 0 < edge["w_depth"] < 37


def one_tap(voxelType, p, sdf, w, wc=0, clr=(0, 0, 0)):
    """A src whose only observed voxel is p (inside block 0)."""
    v = K.default_voxels((8, 8, 8), voxelType)
    v[p[2], p[1], p[0]]["sdf"] = sdf
    v["w_depth"][p[2], p[1], p[0]] = w
    if K.has_colour(voxelType):
        v["w_color"][p[2], p[1], p[0]] = wc
        v["clr"][p[2], p[1], p[0]] = clr
    return hand_src(voxelType, {(0, 0, 0): v})


def test_single_tap_gives_the_tent_weights():
    """One observed fine voxel with weight w: A = 8w at the coarse voxel it is the centre of, 4w / 2w / w through a face / edge / corner."""
    w = 64                                            # (A + 32) div 64 = A / 64 exactly: w' = 8, 4, 2, 1
    for p, q, want in (((2, 2, 2), (1, 1, 1), 8), ((3, 2, 2), (1, 1, 1), 4), ((3, 3, 2), (1, 1, 1), 2), ((3, 3, 3), (1, 1, 1), 1),
                       ((3, 2, 2), (2, 1, 1), 4), ((3, 3, 3), (2, 2, 2), 1)):
        blk = K.coarse_blocks(one_tap(capi.VOXEL_S, p, -1234, w), np.array([(0, 0, 0)]), 255).reshape(8, 8, 8)
        assert blk["w_depth"][q[2], q[1], q[0]] == want and blk["sdf"][q[2], q[1], q[0]] == -1234, (p, q)
    blk = K.coarse_blocks(one_tap(capi.VOXEL_S, (2, 2, 2), -1234, w), np.array([(0, 0, 0)]), 255).reshape(8, 8, 8)
    assert np.count_nonzero(blk["w_depth"]) == 1 and blk["sdf"][0, 0, 0] == 32767        # an even voxel reaches its own coarse voxel only
    blk = K.coarse_blocks(one_tap(capi.VOXEL_S, (3, 3, 3), -1234, w), np.array([(0, 0, 0)]), 255).reshape(8, 8, 8)
    assert np.count_nonzero(blk["w_depth"]) == 8                                           # an odd one its eight neighbours


def two_taps(sdf0, w0, sdf1, w1, maxW=255):
    """Fine voxels (2, 2, 2) (centre, c = 8) and (3, 2, 2) (face, c = 4) of coarse voxel (1, 1, 1)."""
    v = K.default_voxels((8, 8, 8), capi.VOXEL_S)
    v[2, 2, 2] = (sdf0, w0)
    v[2, 2, 3] = (sdf1, w1)
    return K.coarse_blocks(hand_src(capi.VOXEL_S, {(0, 0, 0): v}), np.array([(0, 0, 0)]), maxW).reshape(8, 8, 8)[1, 1, 1]


def test_rounding_is_to_nearest_with_halves_away_from_zero():
    # a centre and a face tap of weight 1: A = 12, S = 8 s0 + 4 s1
    assert two_taps(3, 1, 0, 1)["sdf"] == 2 and two_taps(-3, 1, 0, 1)["sdf"] == -2                # 24 / 12
    assert two_taps(0, 1, 4, 1)["sdf"] == 1 and two_taps(0, 1, -4, 1)["sdf"] == -1                # 16 / 12 = 1.33
    assert two_taps(0, 1, 5, 1)["sdf"] == 2 and two_taps(0, 1, -5, 1)["sdf"] == -2                # 20 / 12 = 1.67

    # halves: the two face taps (3, 2, 2) and (1, 2, 2) of coarse voxel (1, 1, 1), a = 4 each: S / A = (s0 + s1) / 2
    def mean_of(s0, s1):
        v = K.default_voxels((8, 8, 8), capi.VOXEL_S)
        v[2, 2, 3] = (s0, 1)
        v[2, 2, 1] = (s1, 1)
        return int(K.coarse_blocks(hand_src(capi.VOXEL_S, {(0, 0, 0): v}), np.array([(0, 0, 0)]), 255).reshape(8, 8, 8)[1, 1, 1]["sdf"])
    assert [mean_of(1, 2), mean_of(-1, -2), mean_of(0, 1), mean_of(0, -1), mean_of(2, 2), mean_of(-7, 2)] == [2, -2, 1, -1, 2, -3]
    assert mean_of(32767, 32767) == 32767 and mean_of(-32767, -32767) == -32767


def test_weight_is_clamped_at_maxW_and_never_below_one():
    assert two_taps(5, 255, 5, 255, maxW=255)["w_depth"] == (12 * 255 + 32) // 64 == 48
    assert two_taps(5, 255, 5, 255, maxW=20)["w_depth"] == 20
    assert two_taps(5, 1, 5, 0)["w_depth"] == 1 and two_taps(5, 1, 5, 0)["sdf"] == 5                  # A = 8: (8 + 32) div 64 = 0 -> 1
    full = ramp_blocks(capi.VOXEL_S, -1, 2, lambda x, y, z: 0 * x + 9, 255)
    blk = K.coarse_blocks(hand_src(capi.VOXEL_S, full), np.array([(0, 0, 0)]), 1000).reshape(8, 8, 8)
    assert blk["w_depth"][3, 3, 3] == 255 and blk["sdf"][3, 3, 3] == 9                                   # A = 64 * 255: min(1000, 255, 255)


def test_colour_without_colour_weight_stays_zero():
    src = one_tap(capi.VOXEL_S_RGB, (2, 2, 2), 100, 50, wc=0, clr=(200, 100, 50))
    v = K.coarse_blocks(src, np.array([(0, 0, 0)]), 100).reshape(8, 8, 8)[1, 1, 1]
    assert v["w_depth"] == 6 and tuple(v["clr"]) == (0, 0, 0) and v["w_color"] == 0
    src = one_tap(capi.VOXEL_F_RGB, (2, 2, 2), 0.5, 50, wc=16, clr=(200, 100, 51))
    v = K.coarse_blocks(src, np.array([(0, 0, 0)]), 100).reshape(8, 8, 8)[1, 1, 1]
    assert v["sdf"] == np.float32(0.5) and tuple(v["clr"]) == (200, 100, 51) and v["w_color"] == 2     # Bc = 128


def test_block_coordinates_halve_with_an_arithmetic_shift():
    assert K.coarse_position([-1, -2, -3]).tolist() == [-1, -1, -2]
    assert K.coarse_position([0, 1, 2, 3, -4, -32768, 32767]).tolist() == [0, 0, 1, 1, -2, -16384, 16383]


def test_restated_allocation_known_answers():
    """bucketNum = 8 (as test_scene_merge's hand tables): the eight children of coarse position (1, 0, 0) -- hashIndex 5 -- in src slots
    0 .. 7, and the lone child (0, 0, 0) of coarse (0, 0, 0) in slot 8.  Round 1: slot 7 wins head 5, slot 8 head 0; round 2: the other
    seven find the entry."""
    assert M.hash_index((1, 0, 0), 7) == 5 and M.hash_index((0, 0, 0), 7) == 0
    dst = TM.hand_state({}, 4, 3, 3, 0)
    children = [(2 + (i & 1), (i >> 1) & 1, i >> 2) for i in range(8)]
    src = TM.hand_state({i: (c, 0, i) for i, c in enumerate(children)} | {8: ((0, 0, 0), 0, 8), 9: ((5, 5, 5), 0, -1)}, 9, -1, 3, 1)
    out, stats, where = K.coarsen(dst, src)
    assert TM.table_of(out) == {5: ((1, 0, 0), 0, 2), 0: ((0, 0, 0), 0, 3)}           # ascending sweep: slot 0 takes alloc[3], slot 5 alloc[2]
    assert (out["lastFreeBlockId"], out["lastFreeExcessListId"]) == (1, 3)
    assert stats == dict(rounds=2, considered=9, alreadyPresent=0, allocated=2, written=2, unserved=0, srcWithoutBlock=1, dstSwappedOut=0)
    assert where == {**{i: 5 for i in range(8)}, 8: 0}
    # the voxels: overwritten, not combined (dst's pool was random); blocks nobody took keep their content
    T.assert_fields_equal(out["voxels"][:2 * 512], dst["voxels"][:2 * 512], "blocks nobody took")
    want = K.coarse_blocks(src, np.array([(1, 0, 0), (0, 0, 0)]), 100)
    T.assert_fields_equal(out["voxels"][2 * 512:3 * 512], want[0], "coarse block (1, 0, 0)")
    T.assert_fields_equal(out["voxels"][3 * 512:], want[1], "coarse block (0, 0, 0)")
    # a dst that holds the position already, swapped out: found, counted, left alone
    dst = TM.hand_state({5: ((1, 0, 0), 0, -1)}, 4, 3, 3, 0)
    out, stats, where = K.coarsen(dst, src, [0, 3, 3])
    assert stats == dict(rounds=1, considered=2, alreadyPresent=2, allocated=0, written=0, unserved=0, srcWithoutBlock=0, dstSwappedOut=1)
    T.assert_fields_equal(out["voxels"], dst["voxels"], "nothing written")


# ---- CPU: oracle scenes ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_states(oracle):
    """A and B on the oracle, and the restated coarsening of each into an empty scene at twice the voxel size (computed once, read only)."""
    out = {}
    empty = T.Session(oracle, coarse(localBlockNum=POOL))
    e0 = M.state_of(empty.scene)
    empty.close()
    for name, sc in (("A", fine_a()), ("B", fine_b())):
        ses = TM.build(oracle, sc)
        s0 = M.state_of(ses.scene)
        ses.close()
        out[name] = (s0, e0) + K.coarsen(e0, s0)
    return out


@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_invariants_on_oracle_scenes(oracle_states, name):
    src, before, after, stats, where = oracle_states[name]
    sh = src["hash"]
    part = sh["pos"][sh["ptr"] >= 0].astype(np.int64)
    want = {tuple(p) for p in (part >> 1).tolist()}
    h = after["hash"]
    live = h[h["ptr"] >= -1]
    pos = [tuple(p) for p in live["pos"].tolist()]
    assert len(set(pos)) == len(pos), "a position occurs twice"
    assert set(pos) == want, "the positions are not exactly {b >> 1}"
    used = h["ptr"][h["ptr"] >= 0]
    free = after["alloc"][:after["lastFreeBlockId"] + 1]
    assert len(np.unique(used)) == len(used) and not np.intersect1d(used, free).size
    assert stats["allocated"] == stats["written"] == len(want) and stats["unserved"] == 0 and stats["considered"] == len(part)
    assert before["lastFreeBlockId"] - after["lastFreeBlockId"] == stats["allocated"]
    if name == "A":
        # what the scene is for, from the inputs alone
        print("A: participants", len(part), "coarse blocks", len(want), "rounds", stats["rounds"])
        assert np.count_nonzero(np.any((part < 0) & (part & 1 == 1), axis=1)) >= 100, "participants with a negative odd block coordinate"
        children = {}
        for p in part.tolist():
            children.setdefault(tuple(c >> 1 for c in p), []).append(p)
        sizes = np.array([len(v) for v in children.values()])
        assert np.count_nonzero(sizes == 1) >= 5 and np.count_nonzero(sizes == 8) >= 1, "single children / full octets"
        new_excess = int(np.count_nonzero(h["ptr"][after["bucketNum"]:] >= -1))
        assert new_excess >= 1 and before["lastFreeExcessListId"] - after["lastFreeExcessListId"] == new_excess, "no excess entry at the default table size"
        assert np.count_nonzero(after["voxels"]["w_depth"]) < np.count_nonzero(src["voxels"]["w_depth"]) / 4


def mesh_triangles(be, sc, state):
    ses = T.Session(be, sc)
    for which, key in ((capi.BUF_HASH_ENTRIES, "hash"), (capi.BUF_EXCESS_LIST, "excess"), (capi.BUF_ALLOCATION_LIST, "alloc"), (capi.BUF_VOXEL_BLOCKS, "voxels")):
        ses.scene.upload(which, state[key])
    ses.scene.set_counters(ses.rs, state["lastFreeBlockId"], state["lastFreeExcessListId"], 0)
    m = Mesh(ses.scene)
    m.MeshScene()
    tri = m.triangles()
    ses.close()
    return tri


def test_mesh_of_the_restated_coarse_scene(oracle, oracle_states):
    src, _, after, _, _ = oracle_states["A"]
    fine = mesh_triangles(oracle, fine_a(), src)
    crs = mesh_triangles(oracle, coarse(localBlockNum=POOL), after)
    print("triangles fine", len(fine), "coarse", len(crs))
    assert 0 < len(crs) < len(fine) / 2
    lo_f, hi_f = fine.reshape(-1, 3).min(0), fine.reshape(-1, 3).max(0)
    lo_c, hi_c = crs.reshape(-1, 3).min(0), crs.reshape(-1, 3).max(0)
    print("bounding boxes", lo_f, hi_f, lo_c, hi_c)
    assert np.all(np.abs(lo_c - lo_f) <= COARSE) and np.all(np.abs(hi_c - hi_f) <= COARSE)


def test_scene_coarsen_is_declared_and_bound(hip_host):
    assert "scene_coarsen" in capi.declared_functions() and "scene_coarsen" in capi._HOST_IO_SIGS
    assert "scene_coarsen" in hip_host.fn
    assert C.sizeof(capi.CoarsenStats) == 32
    assert "coarsen.hip" in open(os.path.join(T.ROOT, "infinitam_amd", "csrc", "Makefile")).read()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def empty(be, sc):
    return T.Session(be, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("voxel", [capi.VOXEL_S, capi.VOXEL_F, capi.VOXEL_S_RGB, capi.VOXEL_F_RGB])
def test_coarsening_into_an_empty_scene_equals_the_restatement(hip, voxel):
    """Case a."""
    colour = voxel in (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB)
    sc = fine_a(voxelType=voxel, colour=colour)
    a, d = TM.build(hip, sc), empty(hip, coarse(sc))
    stats, got, _, _ = coarsen_and_compare(d.scene, a.scene, what="case a, voxel type %d" % voxel)
    assert stats["allocated"] == stats["written"] > 100 and stats["rounds"] >= 2 and stats["unserved"] == 0
    assert np.count_nonzero(got["voxels"]["w_depth"]) > 10000
    if colour:
        assert np.count_nonzero(got["voxels"]["w_color"]) > 10000 and np.count_nonzero(got["voxels"]["clr"]) > 10000
    a.close(); d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bucketNum,excessNum,runs_dry", [(0x800, 0x1800, False), (0x400, 0x100, True)])
def test_coarsening_into_tiny_tables_equals_the_restatement(hip, bucketNum, excessNum, runs_dry):
    """Case b.  The 256 coarse blocks of A cannot use up 256 excess entries by themselves (at least one of them is a head; the restatement
    on the oracle's scene takes 77), so in the second case dst holds a scene already: B at the coarse voxel size from 0.5 m aside (605
    blocks, 141 of the 256 excess entries taken).  Restatement on the oracle's scenes: 5 rounds / 3 rounds with 220 participants unserved."""
    a = TM.build(hip, fine_a())
    if runs_dry:
        d = TM.build(hip, coarse(fine_b(origin=(0.3, 0.1, -0.4)), bucketNum=bucketNum, excessNum=excessNum))
    else:
        d = empty(hip, coarse(bucketNum=bucketNum, excessNum=excessNum))
    stats, got, before, where = coarsen_and_compare(d.scene, a.scene, what="case b, %#x + %#x" % (bucketNum, excessNum))
    assert stats["rounds"] >= 3, "no chain grew by more than one entry"
    if runs_dry:
        assert stats["unserved"] > 0 and got["lastFreeExcessListId"] == -1 and got["lastFreeBlockId"] >= 0
        assert_only_D_changed(before, got, where, "case b")
    a.close(); d.close()


@pytest.mark.gpu
def test_coarsening_with_an_exhausted_voxel_pool_equals_the_restatement(hip):
    """Case c: 100 voxel blocks for the 256 needed."""
    a, d = TM.build(hip, fine_a()), empty(hip, coarse(localBlockNum=100))
    stats, got, _, _ = coarsen_and_compare(d.scene, a.scene, what="case c")
    assert stats["allocated"] == 100 == stats["written"] and stats["unserved"] > 0 and got["lastFreeBlockId"] == -1
    a.close(); d.close()


@pytest.mark.gpu
def test_coarsening_a_visible_list_equals_the_restatement(hip):
    """Case d: half of A's visible list, permuted, with duplicates, into a dst that holds B; from a host array and a device buffer."""
    a = TM.build(hip, fine_a())
    n = a.scene.counters(a.rs)["noVisibleEntries"]
    ids = a.scene.download(capi.BUF_VISIBLE_IDS, a.rs)[:n].copy()
    ids = ids[: n // 2]                                                       # (a true subset of A)
    slots = np.random.default_rng(7).permutation(np.concatenate([ids, ids[:17], ids[5:9]])).astype(np.int32)
    d = TM.build(hip, coarse(fine_b()))
    stats, got, before, where = coarsen_and_compare(d.scene, a.scene, slots, what="case d")
    assert stats["considered"] == len(ids) and stats["allocated"] > 0 and stats["alreadyPresent"] > 0
    assert 0 < stats["written"] < np.count_nonzero(got["hash"]["ptr"] >= 0)
    assert_only_D_changed(before, got, where, "case d")
    d2 = TM.build(hip, coarse(fine_b()))
    dev = hip.to_backend(slots)
    assert d2.scene.coarsen_from(a.scene, dev) == stats
    T.assert_fields_equal(d2.scene.download(capi.BUF_HASH_ENTRIES), got["hash"], "device list vs host list: hash")
    T.assert_fields_equal(d2.scene.download(capi.BUF_VOXEL_BLOCKS), got["voxels"], "device list vs host list: voxels")
    a.close(); d.close(); d2.close()


@pytest.mark.gpu
def test_coarsening_twice_into_one_scene_overwrites_only_the_second_set(hip):
    """Case e: A, then B, into the same dst."""
    a, b, d = TM.build(hip, fine_a()), TM.build(hip, fine_b()), empty(hip, coarse())
    first, _, _, _ = coarsen_and_compare(d.scene, a.scene, what="case e, A")
    stats, got, before, where = coarsen_and_compare(d.scene, b.scene, what="case e, B")
    assert stats["alreadyPresent"] > 0 and stats["allocated"] > 0
    second = sorted(set(where.values()))
    held = np.nonzero(before["hash"]["ptr"] >= 0)[0]
    kept = np.setdiff1d(held, second)
    assert len(kept) > 0 and len(np.intersect1d(held, second)) > 0
    T.assert_fields_equal(blocks_of(got, kept).reshape(-1), blocks_of(before, kept).reshape(-1), "case e: blocks of A alone keep the first result")
    want = K.coarse_blocks(TM.snapshot(b.scene), got["hash"]["pos"][second].astype(np.int64), got["maxW"])
    T.assert_fields_equal(blocks_of(got, second).reshape(-1), want.reshape(-1), "case e: the blocks of the second D hold B alone")
    a.close(); b.close(); d.close()


FAR = (60.0, -55.0, 70.0)      # metres: 375 coarse blocks (16 cm) away on every axis, outside a directory cube of 512 blocks placed at the origin


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "no directory", "no sdf mirror", "shifted origin"])
def test_derived_structures_after_coarsening_are_those_of_an_upload(hip, oracle, form):
    """Case f: the coarsened scene and a twin that received the same state through itm_upload (which rebuilds the occupancy bits, the
    directories and the mirror from the table) take one further frame; every buffer stays identical, and the frame's ray cast equals the
    oracle's on the same state."""
    key = {"no directory": 5, "no sdf mirror": 12}.get(form)
    if key:
        hip.check(hip.fn["debug_set"](key, 1), "debug_set")
    try:
        if form == "shifted origin":      # dst has placed its cubes around a frame of its own; src lies far outside them
            sa = fine_a(origin=FAR)
            a, d = TM.build(hip, sa), TM.build(hip, coarse(), frames=1)
            org = np.array(d.scene.accel_info()["origin_directory"])
            sh = a.scene.download(capi.BUF_HASH_ENTRIES)
            pos = sh["pos"][sh["ptr"] >= 0].astype(np.int64) >> 1
            assert int(np.count_nonzero(np.any((pos < org) | (pos >= org + 512), axis=1))) > 100, "src lies inside dst's cubes"
        else:
            sa = fine_a()
            a, d = TM.build(hip, sa), empty(hip, coarse())
        stats, state, _, _ = coarsen_and_compare(d.scene, a.scene, what="case f (%s)" % form)
        assert stats["allocated"] > 100
        sc = coarse(sa)
        twin, ref = T.Session(hip, sc), T.Session(oracle, sc)
        TM.upload_state(twin, state, d); TM.upload_state(ref, state, d)
        for ses in (d, twin, ref):
            ses.sc = sc
            ses.frame(3, fused=True)
        rd, rt, ro = d.snapshot(), twin.snapshot(), ref.snapshot()
        T.assert_fields_equal(rd.hash, rt.hash, "hash")
        T.assert_fields_equal(rd.voxels, rt.voxels, "voxels")
        assert np.array_equal(rd.excess, rt.excess) and np.array_equal(rd.alloc_list, rt.alloc_list)
        assert rd.counters[0]["lastFreeBlockId"] == rt.counters[0]["lastFreeBlockId"] and rd.counters[0]["lastFreeExcessListId"] == rt.counters[0]["lastFreeExcessListId"]
        assert np.array_equal(rd.raycast, rt.raycast) and np.array_equal(rd.points, rt.points) and np.array_equal(rd.normals, rt.normals), "maps"
        assert np.array_equal(rd.raycast[..., 3], ro.raycast[..., 3]), "hit mask vs oracle"
        hit = rd.raycast[..., 3] > 0
        assert np.count_nonzero(hit) > 5000
        assert np.array_equal(rd.raycast[hit], ro.raycast[hit]) and np.array_equal(rd.points, ro.points), "ray cast vs oracle"
        a.close(); d.close(); twin.close(); ref.close()
    finally:
        if key:
            hip.check(hip.fn["debug_set"](key, 0), "debug_set")


def swapping_scene(be, voxelSize, transfer):
    """test_swapping's sequence: three frames on it, then one looking at a wall, in which `transfer` blocks leave for the host cache."""
    intr, seq = test_swapping.poses_and_depths()
    s = be.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=voxelSize, mu=MU), useSwapping=True, localBlockNum=POOL, transferBlockNum=transfer)
    s.reco.ResetScene()
    rs = s.vis.CreateRenderState((W, H))
    for Mk, depth in seq[:4]:
        v = capi.View(be.to_backend(depth), W, H, M_d=Mk, intr_d=intr)
        s.reco.AllocateSceneFromDepth(v, rs)
        s.reco.IntegrateIntoScene(v, rs)
        s.swap_integrate_global_into_local(rs)
        s.swap_save_to_global_memory(rs)
    return s, rs


@pytest.mark.gpu
def test_coarsening_between_swapping_scenes_equals_the_restatement(hip):
    """Case g (on the oracle's scenes: 512 entries of src and 64 of dst swapped out, 471 blocks written, 6 allocated)."""
    (src, rs_s), (dst, rs_d) = swapping_scene(hip, FINE, 0x200), swapping_scene(hip, COARSE, 0x40)
    # what the set-up is for, from the inputs
    sh, dh = src.download(capi.BUF_HASH_ENTRIES), dst.download(capi.BUF_HASH_ENTRIES)
    held = {tuple(p): int(q) for p, q in zip(dh["pos"][dh["ptr"] >= -1].tolist(), dh["ptr"][dh["ptr"] >= -1])}
    D = {tuple(c >> 1 for c in p) for p in sh["pos"][sh["ptr"] >= 0].tolist()}
    out_of_dst = sum(1 for p in D if held.get(p, -2) == -1)
    assert np.count_nonzero(sh["ptr"] == -1) > 100 and out_of_dst > 50 and sum(1 for p in D if held.get(p, -2) >= 0) > 100
    stats, _, _, _ = coarsen_and_compare(dst, src, what="case g")
    assert stats["srcWithoutBlock"] == int(np.count_nonzero(sh["ptr"] == -1)) and stats["dstSwappedOut"] == out_of_dst
    rs_s.close(); rs_d.close(); src.close(); dst.close()


@pytest.mark.gpu
def test_coarsening_dense_scenes_equals_the_restatement(hip):
    """Case h: 64^3 cells each; dst's array covers 1.28 m from another corner than src's 0.64 m, so taps leave src's array."""
    a = TM.build(hip, fine_a(indexType=capi.INDEX_DENSE, denseSize=(64, 64, 64), denseOffset=(-32, -32, 95), localBlockNum=0))
    d = empty(hip, coarse(a.sc, denseSize=(64, 64, 64), denseOffset=(-40, -20, 40), localBlockNum=0))
    q = [np.arange(64) + o for o in (-40, -20, 40)]
    inside = [(2 * q[i] - 1 >= lo) & (2 * q[i] + 1 < lo + 64) for i, lo in enumerate((-32, -32, 95))]
    partly = [((2 * q[i] + 1 >= lo) & (2 * q[i] - 1 < lo + 64)) & ~inside[i] for i, lo in enumerate((-32, -32, 95))]
    assert all(np.count_nonzero(m) > 10 for m in inside) and all(np.count_nonzero(m) == 2 for m in partly)
    assert np.count_nonzero(a.scene.download(capi.BUF_VOXEL_BLOCKS)["w_depth"]) > 1000
    stats, got, _, _ = coarsen_and_compare(d.scene, a.scene, what="case h")
    assert (stats["considered"], stats["written"]) == (1, 1)
    w = got["voxels"]["w_depth"].reshape(64, 64, 64)
    cube = lambda m: m[2][:, None, None] & m[1][None, :, None] & m[0][None, None, :]
    edge = cube([i | p for i, p in zip(inside, partly)]) & ~cube(inside)            # cells that read src with some taps outside its array
    assert np.count_nonzero(w) > 1000 and np.count_nonzero(w[edge]) > 0 and np.count_nonzero(w[~cube([i | p for i, p in zip(inside, partly)])]) == 0
    # a slot list is refused, dst untouched
    dev = hip.to_backend(np.zeros(1, np.int32))
    assert hip.fn["scene_coarsen"](_P(d.scene.h), _P(a.scene.h), _P(dev.ptr), 1, None, None) == capi.ERR_INVALID
    T.assert_fields_equal(d.scene.download(capi.BUF_VOXEL_BLOCKS), got["voxels"], "dense dst after a refusal")
    a.close(); d.close()


@pytest.mark.gpu
def test_coarsening_launches_recorded_frames_first(hip):
    """Case i: both scenes hold recorded, unflushed engine calls when coarsen_from is called; the result is that of the eager run."""
    results = []
    for recorded in (True, False):
        pair = []
        for sc in (coarse(fine_b()), fine_a()):
            ses = TM.build(hip, sc, frames=2, deferred=recorded)
            v = ses.view(2)
            ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
            ses.scene.reco.IntegrateIntoScene(v, ses.rs)
            ses.scene.vis.CreateExpectedDepths(v.M_d, v.intr_d, ses.rs)        # recorded: nothing of frame 2 has been launched yet
            pair.append(ses)
        d, a = pair
        if recorded:
            stats = d.scene.coarsen_from(a.scene)
            got = TM.snapshot(d.scene)
        else:
            stats, got, _, _ = coarsen_and_compare(d.scene, a.scene, what="case i (eager)")
        results.append((stats, got))
        a.close(); d.close()
    assert results[0][0] == results[1][0] and results[0][0]["allocated"] > 0 and results[0][0]["alreadyPresent"] > 0
    M.assert_state_equal(results[0][1], results[1][1], "case i: recorded vs eager", T.assert_fields_equal)


@pytest.mark.gpu
def test_coarsen_refusals_leave_dst_untouched(hip):
    """Case j."""
    a = TM.build(hip, fine_a(), frames=1)
    d = empty(hip, coarse())
    depth = [hip.to_backend(d.sc.depth(k)) for k in range(2)]
    v = [capi.View(depth[k], W, H, M_d=d.sc.pose(k), intr_d=d.sc.intr()) for k in range(2)]
    d.scene.process_frame_ahead(v[0], v[1], d.rs, d.points, d.normals)          # dst holds a frame and the requests of the next
    before = TM.snapshot(d.scene)
    entries = len(TM.snapshot(a.scene)["hash"])

    def refused(dst, src, slots=None, n=None):
        dev = hip.to_backend(np.asarray(slots, np.int32)) if slots is not None else None
        count = (len(slots) if slots is not None else 0) if n is None else n
        rc = hip.fn["scene_coarsen"](_P(dst.h if dst else None), _P(src.h if src else None), _P(dev.ptr if dev else None), count, None, None)
        hip.sync()
        return rc == capi.ERR_INVALID and len(hip.fn["last_error"]() or b"") > 0

    def scene(voxel=capi.VOXEL_S, index=capi.INDEX_HASH, size=FINE, mu=MU, **kw):
        s = hip.create_scene(voxel, index, capi.default_params(voxelSize=size, mu=mu), localBlockNum=POOL if index == capi.INDEX_HASH else 0, **kw)
        s.reco.ResetScene()
        return s

    up = lambda x: float(np.nextafter(np.float32(x), np.float32(1)))
    other_type, dense = scene(capi.VOXEL_F), scene(index=capi.INDEX_DENSE, denseSize=(64, 64, 64))
    same_size, off_size, other_mu, ok = scene(size=COARSE), scene(size=up(FINE)), scene(mu=up(MU)), scene()
    assert refused(d.scene, a.scene), "dst holds the block requests of a frame issued ahead"
    d.scene.cancel_ahead(d.rs)
    assert refused(None, a.scene) and refused(d.scene, None), "null scene"
    assert refused(d.scene, d.scene), "dst is src"
    assert refused(d.scene, other_type), "voxel type mismatch"
    assert refused(d.scene, dense), "hash with dense"
    assert refused(d.scene, same_size), "equal voxel sizes"
    assert refused(d.scene, off_size), "voxelSize not twice src's in the last bit"
    assert refused(d.scene, other_mu), "mu differing in the last bit"
    assert refused(ok, d.scene), "dst finer than src"
    assert refused(d.scene, ok, [0, entries, 3]) and refused(d.scene, ok, [-1]), "a slot outside the table"
    assert refused(d.scene, ok, [0, 1], n=-2), "a negative count"
    after = TM.snapshot(d.scene)
    M.assert_state_equal(after, before, "refusals", T.assert_fields_equal)
    assert np.array_equal(after["alloc"], before["alloc"]) and np.array_equal(after["excess"], before["excess"])
    assert d.scene.coarsen_from(a.scene)["allocated"] > 0            # and the call that is in order goes through
    for s in (other_type, dense, same_size, off_size, other_mu, ok):
        s.close()
    a.close(); d.close()


@pytest.mark.gpu
def test_mesh_of_the_coarsened_scene_is_the_mesh_of_the_uploaded_state(hip):
    """Case k: MeshVolume + Index, triangle for triangle."""
    a, d = TM.build(hip, fine_a()), empty(hip, coarse())
    d.scene.coarsen_from(a.scene)
    state = TM.snapshot(d.scene)
    twin = T.Session(hip, coarse())
    TM.upload_state(twin, state, d)
    meshes = []
    for ses in (d, twin):
        m = Mesh(ses.scene)
        m.MeshVolume(); m.Index()
        meshes.append((m.triangles(), m.vertices(), m.faces()))
        m.close()
    fine = Mesh(a.scene)
    fine.MeshVolume()
    assert 0 < len(meshes[0][0]) < fine.info()[0] / 2
    fine.close()
    for got, want, what in zip(meshes[0], meshes[1], ("triangles", "vertices", "faces")):
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
    a.close(); d.close(); twin.close()


# ---- the C++ adapters ----------------------------------------------------------------------------------------------------------------

DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "scene_coarsen_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "scene_coarsen_demo")


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_coarsen_adapters_compile_and_link():
    assert os.path.exists(build_demo())


def ply_counts(path):
    """(vertices, faces) from the header of a PLY file."""
    counts = {}
    with open(path, "rb") as f:
        for line in f:
            words = line.decode("ascii", "replace").split()
            if words[:1] == ["element"]:
                counts[words[1]] = int(words[2])
            if words[:1] == ["end_header"]:
                break
    return counts["vertex"], counts["face"]


@pytest.mark.gpu
def test_cpp_coarsen_demo_equals_the_python_path(hip, tmp_path):
    """Case l."""
    exe = build_demo()
    got = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
    w, h, P = 160, 120, 160 * 120
    scenes = []
    for z, tx0, size, table in ((1.5, 0.0, FINE, dict(localBlockNum=0x2000, bucketNum=0x1000, excessNum=0x400)),
                                (1.52, -0.4, COARSE, dict(localBlockNum=0x800, bucketNum=0x400, excessNum=0x100))):
        s = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=size, mu=MU), **table)
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
    (a, rs_a), (c, rs_c) = scenes
    n = a.counters(rs_a)["noVisibleEntries"]
    stats = c.coarsen_from(a, a.download(capi.BUF_VISIBLE_IDS, rs_a)[:n].copy())
    cnt = c.counters()
    assert stats["allocated"] > 0 and stats["alreadyPresent"] > 0 and stats["written"] > 0
    for k, v in stats.items():
        assert got[k] == v, (k, got, stats)
    assert (got["lastFreeBlockId"], got["lastFreeExcessListId"]) == (cnt["lastFreeBlockId"], cnt["lastFreeExcessListId"])
    assert got["table"] == TM.word_digest(c.download(capi.BUF_HASH_ENTRIES)) and got["voxels"] == TM.word_digest(c.download(capi.BUF_VOXEL_BLOCKS))
    for s, rs in scenes:
        rs.close(); s.close()
    # a main engine: CoarsenSceneInto and SaveSceneToCoarsePLY against the Python path on the scene its frames left (itm_scene_save)
    saved, ply = tmp_path / "fine", tmp_path / "coarse.ply"
    saved.mkdir()
    eng = json.loads(subprocess.run([exe, "--engine", str(saved), str(ply)], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
    fine = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=FINE, mu=MU), localBlockNum=0x4000)
    crs = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=COARSE, mu=MU), localBlockNum=0x4000)
    fine.reco.ResetScene(); crs.reco.ResetScene()
    fine.load(str(saved))
    stats = crs.coarsen_from(fine)
    assert stats["allocated"] == stats["written"] > 0 and stats["unserved"] == 0
    for k, v in stats.items():
        assert eng[k] == v, (k, eng, stats)
    assert eng["table"] == TM.word_digest(crs.download(capi.BUF_HASH_ENTRIES)) and eng["voxels"] == TM.word_digest(crs.download(capi.BUF_VOXEL_BLOCKS))
    m = Mesh(crs)
    m.MeshVolume(); m.Index()
    nv, nt = m.index_info()
    assert nt > 0 and ply_counts(str(ply)) == (nv, nt)
    m.close(); fine.close(); crs.close()
