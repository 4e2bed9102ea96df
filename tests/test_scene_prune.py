"""itm_scene_prune (include/itm_hip.h): empty and free-space blocks of a hash scene go back to the pool.

The product is compared, as whole arrays and bit for bit, with the restatement in tests/scene_prune_terms.py applied to the downloads
taken before the call.  The restatement itself is anchored without a GPU: against hand-written tables, and by its invariants on
oracle scenes, from whose pruned state the oracle goes on fusing."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import scene_merge_terms as M
import scene_prune_terms as P
import test_scene_merge as TM
from infinitam_amd import capi

W, H, POOL = TM.W, TM.H, TM.POOL
_P = C.c_void_p
SMALL = (0x800, 0x1800)
COVER = dict(classes=P.EMPTY | P.FREE, protect=0)          # the configuration the coverage counts are stated for


def scenario_b(frames=3, **kw):
    """merge_B of tests/test_scene_merge.py with any number of frames."""
    kw.setdefault("origin", (0.05, 0.02, -0.1))
    return TM.scenario("merge_B", frames=frames, trajectory="yaw", yaw_rate=0.1, **kw)


def table_sizes(sizes):
    return dict(bucketNum=sizes[0], excessNum=sizes[1])


# ---- CPU: the restatement ----------------------------------------------------------------------------------------------------------

BUCKETS, SLOTS = 8, 16


def block_of(kind):
    """512 short voxels: 'empty' (never observed), 'free' (every observed voxel at +1), 'surface', 'weak' (surface seen once)."""
    v = np.zeros(512, capi.VOXEL_DTYPES[capi.VOXEL_S])
    v["sdf"] = 32767
    if kind == "free":
        v["w_depth"][:100] = 3
    elif kind in ("surface", "weak"):
        v["sdf"][:64], v["w_depth"][:64] = 1200, (1 if kind == "weak" else 7)
    else:
        assert kind == "empty"
    return v


def hand_state(entries, kinds, lastFreeBlockId=None, lastFreeExcessListId=None):
    """entries: {slot: (pos, offset, ptr)}; kinds[ptr]: what voxel block ptr holds.  8 heads and 8 excess entries over a pool of
    len(kinds) + 4 blocks; the free lists hold what the table does not use, unless the counters say otherwise."""
    h = TM.hand_table(entries, SLOTS)
    blocks = len(kinds) + 4
    vox = np.concatenate([block_of(k) for k in kinds] + [block_of("empty")] * 4)
    used = sorted(p for _, _, p in entries.values() if p >= 0)
    free = [b for b in range(blocks) if b not in used]
    alloc = np.full(blocks, -7, np.int32); alloc[:len(free)] = free
    used_x = sorted(s - BUCKETS for s in entries if s >= BUCKETS)
    free_x = [x for x in range(SLOTS - BUCKETS) if x not in used_x]
    excess = np.full(SLOTS - BUCKETS, -7, np.int32); excess[:len(free_x)] = free_x
    st = dict(hash=h, voxels=vox, voxelType=capi.VOXEL_S, maxW=100, alloc=alloc, excess=excess, bucketNum=BUCKETS,
              lastFreeBlockId=len(free) - 1 if lastFreeBlockId is None else lastFreeBlockId,
              lastFreeExcessListId=len(free_x) - 1 if lastFreeExcessListId is None else lastFreeExcessListId)
    for slot, (pos, _, ptr) in entries.items():          # the hand-written table is a table: every entry is found where it stands
        assert P.find(tuple(pos), [tuple(p) for p in h["pos"].tolist()], h["offset"].tolist(), h["ptr"].tolist(), BUCKETS) == slot, (slot, pos)
    return st


def run(st, **kw):
    out, stats, dec, _ = P.prune(st, P.default_config(**kw))
    return out, stats, dec


CHAIN = {0: ((0, 0, 0), 1, 0), 8: ((8, 0, 0), 2, 1), 9: ((16, 0, 0), 3, 2), 10: ((24, 0, 0), 0, 3)}      # (x, 0, 0) hashes to (5 x) mod 8


def test_restated_prune_known_answers():
    assert [P.hash_index((x, 0, 0), 7) for x in (0, 8, 16, 24, 1, 2)] == [0, 0, 0, 0, 5, 2] and P.hash_index((2, 1, 1), 7) == 0
    assert P.short_threshold(1.0) == 32767 and P.short_threshold(0.5) == 16383 and P.short_threshold(-1.0) == -32767

    # a head alone: dropped, its block is the next one handed out, its voxels are initial again
    st = hand_state({3: ((7, 0, 0), 0, 0)}, ["free"])
    out, stats, dec = run(st)
    assert TM.table_of(out) == {} and dec[3] == P.BIT_FREE | P.BIT_CANDIDATE | P.BIT_DROPPED
    assert (stats["dropped"], stats["droppedHeads"], stats["droppedExcess"], stats["pinnedHeads"], stats["free_"]) == (1, 1, 0, 0, 1)
    assert out["lastFreeBlockId"] == st["lastFreeBlockId"] + 1 and out["alloc"][out["lastFreeBlockId"]] == 0 and out["lastFreeExcessListId"] == st["lastFreeExcessListId"]
    T.assert_fields_equal(out["voxels"][:512], block_of("empty"), "the dropped block")
    assert tuple(out["hash"][3]["pos"]) == (0, 0, 0) and out["hash"][3]["offset"] == 0 and out["hash"][3]["ptr"] == -2
    # ... and only FREE selected leaves an empty one alone
    assert run(hand_state({3: ((7, 0, 0), 0, 0)}, ["empty"]), classes=P.FREE)[1]["dropped"] == 0

    # a head pinned by a chain entry that stays, and by one that is swapped out
    for child, kinds in ((((8, 0, 0), 0, 1), ["empty", "surface"]), (((8, 0, 0), 0, -1), ["empty"])):
        st = hand_state({0: ((0, 0, 0), 1, 0), 8: child}, kinds)
        out, stats, dec = run(st)
        assert TM.table_of(out) == TM.table_of(st) and (stats["candidates"], stats["pinnedHeads"], stats["dropped"]) == (1, 1, 0)
        assert dec[0] == P.BIT_EMPTY | P.BIT_CANDIDATE and stats["withoutBlock"] == (1 if child[2] == -1 else 0)
        T.assert_fields_equal(out["voxels"], st["voxels"], "a pinned head keeps its voxels")
        assert (out["lastFreeBlockId"], out["lastFreeExcessListId"]) == (st["lastFreeBlockId"], st["lastFreeExcessListId"])

    # the first, a middle and the last entry of a chain of three, each alone
    for gone, want in ((8, {0: ((0, 0, 0), 2, 0), 9: ((16, 0, 0), 3, 2), 10: ((24, 0, 0), 0, 3)}),
                       (9, {0: ((0, 0, 0), 1, 0), 8: ((8, 0, 0), 3, 1), 10: ((24, 0, 0), 0, 3)}),
                       (10, {0: ((0, 0, 0), 1, 0), 8: ((8, 0, 0), 2, 1), 9: ((16, 0, 0), 0, 2)})):
        kinds = ["surface"] * 4
        kinds[CHAIN[gone][2]] = "empty"
        st = hand_state(CHAIN, kinds)
        out, stats, dec = run(st)
        assert TM.table_of(out) == want, gone
        assert (stats["dropped"], stats["droppedExcess"], stats["droppedHeads"]) == (1, 1, 0)
        assert out["excess"][out["lastFreeExcessListId"]] == gone - BUCKETS and out["alloc"][out["lastFreeBlockId"]] == CHAIN[gone][2]
        assert out["lastFreeExcessListId"] == st["lastFreeExcessListId"] + 1
    # all three: the head stays with offset 0 ...
    st = hand_state(CHAIN, ["surface", "empty", "free", "empty"])
    out, stats, dec = run(st)
    assert TM.table_of(out) == {0: ((0, 0, 0), 0, 0)} and (stats["dropped"], stats["droppedExcess"], stats["pinnedHeads"]) == (3, 3, 0)
    n, m = out["lastFreeBlockId"], out["lastFreeExcessListId"]
    assert out["alloc"][n - 2:n + 1].tolist() == [1, 2, 3] and out["excess"][m - 2:m + 1].tolist() == [0, 1, 2]          # ascending slot order
    # ... and goes too if it is a candidate itself
    st = hand_state(CHAIN, ["free", "empty", "free", "empty"])
    out, stats, dec = run(st)
    assert TM.table_of(out) == {} and (stats["dropped"], stats["droppedHeads"], stats["droppedExcess"], stats["pinnedHeads"]) == (4, 1, 3, 0)
    assert out["alloc"][out["lastFreeBlockId"] - 3:out["lastFreeBlockId"] + 1].tolist() == [0, 1, 2, 3]

    # both counters below -1 count as -1
    st = hand_state(CHAIN, ["surface", "empty", "surface", "empty"], lastFreeBlockId=-3, lastFreeExcessListId=-2)
    out, stats, dec = run(st)
    assert (out["lastFreeBlockId"], out["lastFreeExcessListId"]) == (1, 1) == (stats["lastFreeBlockId"], stats["lastFreeExcessListId"])
    assert out["alloc"][:2].tolist() == [1, 3] and out["excess"][:2].tolist() == [0, 2]

    # protection: a candidate beside a surface block stays; a forced box ignores that, and takes the surface block too when it covers it
    near = {5: ((1, 0, 0), 0, 0), 2: ((2, 0, 0), 0, 1)}
    st = hand_state(near, ["empty", "surface"])
    assert run(st)[1]["protectedByNeighbour"] == 1 and run(st)[1]["dropped"] == 0 and run(st)[2][5] == P.BIT_EMPTY
    assert run(st, protect=0)[1]["dropped"] == 1
    out, stats, dec = run(st, classes=P.EMPTY | P.BOX, boxMin=(1, 0, 0), boxMax=(1, 0, 0))
    assert TM.table_of(out) == {2: ((2, 0, 0), 0, 1)} and (stats["inBox"], stats["protectedByNeighbour"], stats["dropped"]) == (1, 0, 1)
    out, stats, dec = run(st, classes=P.BOX, boxMin=(1, -1, -1), boxMax=(2, 1, 1))
    assert TM.table_of(out) == {} and stats["dropped"] == 2 and dec[2] == P.BIT_SURFACE | P.BIT_INBOX | P.BIT_CANDIDATE | P.BIT_DROPPED
    # boxOnly: the classes apply inside the box only
    assert run(st, protect=0, boxOnly=1, boxMin=(5, 5, 5), boxMax=(6, 6, 6))[1]["dropped"] == 0
    assert run(st, protect=0, boxOnly=1, boxMin=(0, 0, 0), boxMax=(1, 1, 1))[1]["dropped"] == 1
    # a surface block that is a candidate itself (weak) protects nobody
    st = hand_state(near, ["empty", "weak"])
    assert run(st, classes=P.EMPTY | P.WEAK, weakMaxW=1)[1]["dropped"] == 2 and run(st, classes=P.EMPTY | P.WEAK, weakMaxW=1)[1]["protectedByNeighbour"] == 0
    assert run(st, classes=P.EMPTY)[1]["protectedByNeighbour"] == 1

    # protected by a DIAGONAL neighbour that lives in another bucket -- as the second entry of its chain
    # (the head of that chain is empty, so not a protector; it is a candidate and pinned by the chain)
    st = hand_state({5: ((1, 0, 0), 0, 0), 0: ((0, 0, 0), 1, 1), 8: ((2, 1, 1), 0, 2)}, ["free", "empty", "surface"])
    out, stats, dec = run(st)
    assert (stats["candidates"], stats["pinnedHeads"], stats["protectedByNeighbour"], stats["dropped"]) == (1, 1, 1, 0) and dec[5] == P.BIT_FREE
    # one step further away the same block protects nobody (there it is the chain of the candidate's own bucket, which pins it)
    assert P.hash_index((3, 1, 1), 7) == 5
    st = hand_state({5: ((1, 0, 0), 1, 0), 8: ((3, 1, 1), 0, 2)}, ["free", "surface", "surface"])
    assert run(st)[1]["dropped"] == 0 and run(st)[1]["pinnedHeads"] == 1 and run(st)[1]["protectedByNeighbour"] == 0

    # a dry run decides and counts, and changes nothing
    st = hand_state(CHAIN, ["free", "empty", "surface", "empty"])
    real, dry = run(st), run(st, dryRun=1)
    assert dry[1] == real[1] and np.array_equal(dry[2], real[2]) and real[1]["dropped"] == 2
    M.assert_state_equal(dry[0], st, "dry run", T.assert_fields_equal)


_oracle_scenes = {}


def oracle_scene(oracle, sizes):
    """merge_B, 6 frames, on the oracle: (state, render state) downloaded once and shared."""
    if sizes not in _oracle_scenes:
        ses = TM.build(oracle, scenario_b(frames=6, **table_sizes(sizes)))
        _oracle_scenes[sizes] = (M.state_of(ses.scene), P.render_state_of(ses.scene, ses.rs))
        ses.close()
    return _oracle_scenes[sizes]


def upload_pruned(ses, st, rs):
    """As test_scene_merge.upload_state, with the render state's list taken from the restatement."""
    for which, key in ((capi.BUF_HASH_ENTRIES, "hash"), (capi.BUF_EXCESS_LIST, "excess"), (capi.BUF_ALLOCATION_LIST, "alloc"), (capi.BUF_VOXEL_BLOCKS, "voxels")):
        ses.scene.upload(which, st[key])
    ses.scene.upload(capi.BUF_VISIBLE_IDS, rs["ids"], ses.rs)
    ses.scene.upload(capi.BUF_VISIBLE_TYPE, rs["types"], ses.rs)
    ses.scene.set_counters(ses.rs, st["lastFreeBlockId"], st["lastFreeExcessListId"], rs["n"])


def assert_coverage(stats, sizes, what):
    print(what, "coverage:", {k: stats[k] for k in ("considered", "empty", "free_", "candidates", "protectedByNeighbour", "pinnedHeads", "dropped", "droppedHeads", "droppedExcess")})
    assert stats["dropped"] >= 100, (what, stats)
    if sizes == SMALL:
        assert stats["droppedExcess"] >= 20 and stats["pinnedHeads"] >= 5, (what, stats)


@pytest.mark.parametrize("sizes", [(0, 0), SMALL])
def test_restatement_invariants_on_oracle_scenes(oracle, sizes):
    before, rs = oracle_scene(oracle, sizes)
    # protect = 0: in a noiseless synthetic scene every empty or free block touches a block of the surface (a block is 8 voxels wide, the
    # band 2), so with protection nothing at all goes -- asserted here, and COVER is what the comparisons below prune with
    assert P.prune(before, P.default_config())[1]["candidates"] == 0
    after, stats, dec, (rs_after,) = P.prune(before, P.default_config(**COVER), [rs])
    assert_coverage(stats, sizes, "oracle scene %#x + %#x" % sizes)
    assert stats["candidates"] == stats["dropped"] + stats["pinnedHeads"]
    h0, h1, bucketNum = before["hash"], after["hash"], after["bucketNum"]
    hpos, hoff, hptr = [tuple(p) for p in h1["pos"].tolist()], h1["offset"].tolist(), h1["ptr"].tolist()
    gone = (dec & P.BIT_DROPPED) != 0
    for e in np.nonzero(h0["ptr"] >= -1)[0]:
        found = P.find(tuple(h0["pos"][e].tolist()), hpos, hoff, hptr, bucketNum)
        assert found == (-1 if gone[e] else e), "entry %d: found at %d after the prune" % (e, found)
    assert np.array_equal(h1[~gone]["ptr"], h0[~gone]["ptr"]) and np.array_equal(h1[~gone]["pos"], h0[~gone]["pos"])
    # the pool and the excess entries: every one is either in use or on its list, exactly once
    free = after["alloc"][:after["lastFreeBlockId"] + 1]
    assert sorted(free.tolist() + h1["ptr"][h1["ptr"] >= 0].tolist()) == list(range(len(after["alloc"])))
    free_x = after["excess"][:after["lastFreeExcessListId"] + 1]
    assert sorted(free_x.tolist() + (np.nonzero(h1["ptr"][bucketNum:] >= -1)[0]).tolist()) == list(range(len(after["excess"])))
    assert after["lastFreeBlockId"] == before["lastFreeBlockId"] + stats["dropped"] and after["lastFreeExcessListId"] == before["lastFreeExcessListId"] + stats["droppedExcess"]
    # every dropped block reads as an absent one did: no observed voxel below +1 was in it
    v0 = before["voxels"].reshape(-1, 512)[h0["ptr"][gone]]
    assert not np.any((v0["w_depth"] > 0) & (v0["sdf"] < 32767))
    # the list of the render state: the old one without the dropped slots
    old = rs["ids"][:rs["n"]]
    assert np.array_equal(rs_after["ids"][:rs_after["n"]], old[~gone[old]]) and stats["visibleRemoved"] == rs["n"] - rs_after["n"] > 0
    # the reference's engines go on from the pruned state, and take the released blocks first
    sc = scenario_b(frames=8, **table_sizes(sizes))
    ses = T.Session(oracle, sc)
    upload_pruned(ses, after, rs_after)
    ses.frame(6, fused=False)
    c6 = ses.scene.counters(ses.rs)
    ses.frame(7, fused=False)
    c7 = ses.scene.counters(ses.rs)
    h2 = ses.scene.download(capi.BUF_HASH_ENTRIES)
    ses.close()
    assert c6["statusFlags"] == 0 and c7["statusFlags"] == 0
    taken = after["lastFreeBlockId"] - c7["lastFreeBlockId"]
    assert taken > 0, "the further frames allocated nothing"
    new = np.setdiff1d(h2["ptr"][h2["ptr"] >= 0], h1["ptr"][h1["ptr"] >= 0])
    handed = free[::-1][:taken]
    assert sorted(new.tolist()) == sorted(handed.tolist())
    assert len(np.intersect1d(new, h0["ptr"][gone])) == min(taken, stats["dropped"]), "the released blocks were not handed out first"


def test_scene_prune_is_declared_and_bound(hip_host):
    for name in ("scene_prune", "prune_default_config"):
        assert name in capi.declared_functions() and name in capi._HOST_IO_SIGS and name in hip_host.fn
    assert C.sizeof(capi.PruneConfig) == 48 and C.sizeof(capi.PruneStats) == 64
    cfg = capi.PruneConfig()
    hip_host.check(hip_host.fn["prune_default_config"](C.byref(cfg)), "prune_default_config")
    want = P.default_config()
    assert {k: (tuple(v) if isinstance(v, list) else v) for k, v in cfg.as_dict().items()} == want
    assert [n for n, _ in capi.PruneStats._fields_][:-1] == list(P.STATS)
    assert (capi.PRUNE_EMPTY, capi.PRUNE_FREE, capi.PRUNE_WEAK, capi.PRUNE_BOX) == (P.EMPTY, P.FREE, P.WEAK, P.BOX)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def prune_and_compare(scene, rss, what, before=None, **kw):
    """scene.prune against the restatement on the downloads taken before the call: statistics, decision bytes, table, both lists, both
    counters, the whole voxel pool and every render state's list.  Returns (stats, state after, decision bytes, state before)."""
    before = before if before is not None else M.state_of(scene)
    rs0 = [P.render_state_of(scene, rs) for rs in rss]
    want, wstats, wdec, wrs = P.prune(before, P.default_config(**kw), rs0)
    out = scene.prune(scene.prune_config(**kw), decisions=True)
    dec = out.pop("decisions")
    got = M.state_of(scene)
    print(what, "stats", out)
    assert out == wstats, "%s: stats %s vs restatement %s" % (what, out, wstats)
    assert np.array_equal(dec, wdec), "%s: decision bytes differ at slots %s" % (what, np.nonzero(dec != wdec)[0][:8])
    M.assert_state_equal(got, want, what, T.assert_fields_equal)
    for i, rs in enumerate(rss):
        P.assert_render_state_equal(P.render_state_of(scene, rs), wrs[i], "%s: render state %d" % (what, i))
    return out, got, dec, before


@pytest.mark.gpu
@pytest.mark.parametrize("voxel", [capi.VOXEL_S, capi.VOXEL_F, capi.VOXEL_S_RGB, capi.VOXEL_F_RGB])
def test_prune_equals_the_restatement(hip, voxel):
    """merge_B, 3 frames: empty and free blocks at freeSdf 1.0, then at 0.5, then -- with protection, which keeps everything at the
    thresholds above (see the oracle test) -- at 0.0, each from the state the call before left."""
    ses = TM.build(hip, scenario_b(voxelType=voxel, colour=voxel in (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB)))
    s1, st, _, _ = prune_and_compare(ses.scene, [ses.rs], "voxel type %d, freeSdf 1.0" % voxel, **COVER)
    assert s1["dropped"] >= 100 and s1["empty"] > 0 and s1["free_"] > 0 and s1["visibleRemoved"] > 0, s1
    s2, st, _, _ = prune_and_compare(ses.scene, [ses.rs], "voxel type %d, freeSdf 0.5" % voxel, before=st, freeSdf=0.5, **COVER)
    assert s2["dropped"] >= 100 and s2["empty"] <= s1["pinnedHeads"], s2
    s3, st, _, _ = prune_and_compare(ses.scene, [ses.rs], "voxel type %d, freeSdf 0.0, protected" % voxel, before=st, freeSdf=0.0)
    assert s3["protectedByNeighbour"] > 0 and s3["dropped"] > 0, s3
    ses.close()


@pytest.mark.gpu
def test_prune_in_small_tables_equals_the_restatement(hip):
    ses = TM.build(hip, scenario_b(frames=6, **table_sizes(SMALL)))
    stats, _, _, _ = prune_and_compare(ses.scene, [ses.rs], "small tables", **COVER)
    assert_coverage(stats, SMALL, "small tables")
    ses.close()


@pytest.mark.gpu
@pytest.mark.parametrize("voxel", [capi.VOXEL_S, capi.VOXEL_F, capi.VOXEL_S_RGB])
def test_prune_of_prepared_edges_equals_the_restatement(hip, voxel):
    """Chosen blocks of a built scene rewritten before the call: one observed voxel exactly at the threshold word and one just below
    it, a block whose only weight is w_color, largest weights of weakMaxW and weakMaxW + 1.  Each edge is seen on both sides."""
    colour = voxel == capi.VOXEL_S_RGB
    ses = TM.build(hip, scenario_b(voxelType=voxel, colour=colour))
    hsh, vox = ses.scene.download(capi.BUF_HASH_ENTRIES), ses.scene.download(capi.BUF_VOXEL_BLOCKS).reshape(-1, 512)
    slots = np.nonzero(hsh["ptr"] >= 0)[0][100:106]
    at, below, colour_only, weak, not_weak, far_below = (int(s) for s in slots)
    short = voxel in (capi.VOXEL_S, capi.VOXEL_S_RGB)
    thr = P.short_threshold(0.5) if short else np.float32(0.5)
    under = thr - 1 if short else np.nextafter(np.float32(0.5), np.float32(-1))
    WMAX = 3

    def rewrite(slot, sdf, w, w_color=0):
        b = vox[hsh["ptr"][slot]]
        b[:] = P.initial_voxel(voxel)
        b["sdf"][77], b["w_depth"][77] = sdf, w
        if colour:
            b["w_color"][300] = w_color
    rewrite(at, thr, 5); rewrite(below, under, 5); rewrite(colour_only, 0, 0, w_color=9)
    rewrite(weak, 0, WMAX); rewrite(not_weak, 0, WMAX + 1); rewrite(far_below, 0, 5)
    vox[hsh["ptr"][weak]]["w_depth"][:8] = 1          # (further observed voxels below the largest weight)
    ses.scene.upload(capi.BUF_VOXEL_BLOCKS, vox.reshape(-1))
    stats, _, dec, _ = prune_and_compare(ses.scene, [ses.rs], "prepared edges, voxel type %d" % voxel, classes=P.EMPTY | P.FREE | P.WEAK, freeSdf=0.5,
                                         weakMaxW=WMAX, protect=0)
    cls = dec & 0x1f
    assert cls[at] == P.BIT_FREE and dec[at] & P.BIT_CANDIDATE, "a voxel AT the threshold is free"
    assert cls[below] == P.BIT_SURFACE and not dec[below] & P.BIT_CANDIDATE, "a voxel one step below the threshold is surface"
    assert cls[colour_only] == P.BIT_EMPTY and dec[colour_only] & P.BIT_CANDIDATE, "colour weights make no observation"
    assert cls[weak] == P.BIT_SURFACE | P.BIT_WEAK and dec[weak] & P.BIT_CANDIDATE
    assert cls[not_weak] == P.BIT_SURFACE and not dec[not_weak] & P.BIT_CANDIDATE and cls[far_below] == P.BIT_SURFACE
    assert stats["dropped"] > 0
    ses.close()


def census_facts(c):
    return {k: c[k] for k in ("directory_cells", "slot_directory_cells", "mirror_blocks", "mirror_form", "has_directory")}


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "no directory", "no sdf mirror", "shifted origin", "paged mirror"])
def test_derived_structures_after_a_prune_are_those_of_an_upload(hip, oracle, form, monkeypatch):
    """Case e of the merge tests with the prune in the place of the merge: the pruned scene and a twin that received the pruned state
    through itm_upload run two further frames and stay identical; the first frame's ray cast is the oracle's; cubes and mirror are
    audited directly (tests/accel_terms.py) and read nothing at the dropped positions."""
    import accel_terms as A
    for var in ("ITM_MIRROR", "ITM_MIRROR_BITS", "ITM_MIRROR_PAGES", "ITM_NO_ACCELERATION_CUBES"):
        monkeypatch.delenv(var, raising=False)
    if form == "paged mirror":
        monkeypatch.setenv("ITM_MIRROR", "paged")
    key = {"no directory": 5, "no sdf mirror": 12}.get(form)
    if key:
        hip.check(hip.fn["debug_set"](key, 1), "debug_set")
    try:
        home, far = scenario_b(frames=5), scenario_b(frames=5, origin=(25.0, -22.0, 30.0))
        a = TM.build(hip, home, frames=3)
        plan = [(home, 3), (home, 4)]
        if form == "shifted origin":          # two frames 45 m away move both cubes: the blocks of the first three frames lie outside them
            a.sc = far
            a.frame(0, fused=True); a.frame(1, fused=True)
            plan = [(far, 2), (home, 3)]
        if form == "paged mirror":
            assert a.scene.accel_census()["mirror_form"] == "paged"
        stats, pruned, dec, before = prune_and_compare(a.scene, [a.rs], "derived structures (%s)" % form, **COVER)
        assert stats["dropped"] >= 100 and stats["visibleRemoved"] > 0
        gone = before["hash"]["pos"][(dec & P.BIT_DROPPED) != 0]
        facts = A.audit(a.scene, a.rs, pages_exact=False, what="after the prune (%s)" % form)
        probe = a.scene.accel_probe(gone)
        assert np.all(probe["dir_ptr"] == -1) and np.all(probe["dir_slot"] == -1), "a dropped position still has a directory cell"
        absent = np.int16(-32768) if before["voxelType"] in (capi.VOXEL_S, capi.VOXEL_S_RGB) else np.uint32(0xffffffff)
        assert np.all(probe["values"] == absent), "a dropped position still has mirror values"
        if form == "shifted origin":
            assert 0 < int(np.count_nonzero(probe["dir_covered"])) < len(gone), "dropped blocks inside AND outside the directory cube are wanted"
        elif form not in ("no directory",):
            assert np.all(probe["dir_covered"])
        twin, ref = T.Session(hip, home), T.Session(oracle, home)
        rs_state = P.render_state_of(a.scene, a.rs)
        upload_pruned(twin, pruned, rs_state); upload_pruned(ref, pruned, rs_state)
        tfacts = A.audit(twin.scene, twin.rs, what="the twin (%s)" % form)
        # the census of each was held against its own table at its own origin (the upload places the cubes by the table, the pruned scene
        # keeps those its frames placed); where as many blocks lie outside either, the two are the same numbers
        if (facts["outside_directory"], facts["outside_mirror"]) == (tfacts["outside_directory"], tfacts["outside_mirror"]):
            assert census_facts(facts["census"]) == census_facts(tfacts["census"])
        else:
            assert form == "shifted origin"
        for i, (sc, k) in enumerate(plan):
            for ses in (a, twin) + ((ref,) if i == 0 else ()):
                ses.sc = sc
                ses.frame(k, fused=True)
            ra, rt = a.snapshot(), twin.snapshot()
            T.assert_fields_equal(ra.hash, rt.hash, "frame %d: hash" % i)
            T.assert_fields_equal(ra.voxels, rt.voxels, "frame %d: voxels" % i)
            n, m = ra.counters[0]["lastFreeBlockId"] + 1, ra.counters[0]["lastFreeExcessListId"] + 1
            assert np.array_equal(ra.excess[:m], rt.excess[:m]) and np.array_equal(ra.alloc_list[:n], rt.alloc_list[:n])
            assert ra.counters[0] == rt.counters[0], (ra.counters, rt.counters)
            assert np.array_equal(ra.raycast, rt.raycast) and np.array_equal(ra.points, rt.points) and np.array_equal(ra.normals, rt.normals), "frame %d: maps" % i
            if i == 0:
                ro = ref.snapshot()
                assert np.array_equal(ra.raycast[..., 3], ro.raycast[..., 3]), "hit mask vs oracle"
                hit = ra.raycast[..., 3] > 0
                assert np.count_nonzero(hit) > 5000
                assert np.array_equal(ra.raycast[hit], ro.raycast[hit]) and np.array_equal(ra.points, ro.points), "ray cast vs oracle"
                T.assert_fields_equal(ra.hash, ro.hash, "frame 0: hash vs oracle")
            A.audit(a.scene, a.rs, pages_exact=False, what="frame %d after the prune (%s)" % (i, form))
        a.close(); twin.close(); ref.close()
    finally:
        if key:
            hip.check(hip.fn["debug_set"](key, 0), "debug_set")


@pytest.mark.gpu
def test_prune_repairs_every_render_state(hip):
    """Two render states on one scene, each with its own list: each list is the old one without the dropped slots, in order, and the
    next fused frame through each equals that of a twin which received the pruned state and lists through itm_upload."""
    sc = scenario_b(frames=7)
    a = TM.build(hip, sc, frames=3)
    rs2 = a.scene.vis.CreateRenderState((W, H))
    a.scene.process_frame(a.view(5), rs2, a.points, a.normals)          # another view: another list
    l1, l2 = (P.render_state_of(a.scene, rs) for rs in (a.rs, rs2))
    assert l1["n"] > 500 and l2["n"] > 500 and not np.array_equal(l1["ids"][:l1["n"]], l2["ids"][:l2["n"]])
    stats, pruned, dec, _ = prune_and_compare(a.scene, [a.rs, rs2], "two render states", **COVER)
    gone = (dec & P.BIT_DROPPED) != 0
    removed = 0
    for old, rs in ((l1, a.rs), (l2, rs2)):
        new = P.render_state_of(a.scene, rs)
        ids = old["ids"][:old["n"]]
        assert np.array_equal(new["ids"][:new["n"]], ids[~gone[ids]]) and new["n"] < old["n"]
        assert not np.any(new["types"][gone]) and np.array_equal(new["types"][~gone], old["types"][~gone])
        removed += old["n"] - new["n"]
    assert stats["visibleRemoved"] == removed > 0
    twin = T.Session(hip, sc)
    trs2 = twin.scene.vis.CreateRenderState((W, H))
    upload_pruned(twin, pruned, P.render_state_of(a.scene, a.rs))
    new2 = P.render_state_of(a.scene, rs2)
    twin.scene.upload(capi.BUF_VISIBLE_IDS, new2["ids"], trs2)
    twin.scene.upload(capi.BUF_VISIBLE_TYPE, new2["types"], trs2)
    c = twin.scene.counters()
    twin.scene.set_counters(trs2, c["lastFreeBlockId"], c["lastFreeExcessListId"], new2["n"])
    for k, (ra, rt) in ((3, (a.rs, twin.rs)), (6, (rs2, trs2))):
        for ses, rs in ((a, ra), (twin, rt)):
            ses.scene.process_frame(ses.view(k), rs, ses.points, ses.normals)
        T.assert_fields_equal(a.scene.download(capi.BUF_HASH_ENTRIES), twin.scene.download(capi.BUF_HASH_ENTRIES), "frame %d: hash" % k)
        T.assert_fields_equal(a.scene.download(capi.BUF_VOXEL_BLOCKS), twin.scene.download(capi.BUF_VOXEL_BLOCKS), "frame %d: voxels" % k)
        assert a.scene.counters(ra) == twin.scene.counters(rt)
        n = a.scene.counters(ra)["noVisibleEntries"]
        assert np.array_equal(a.scene.download(capi.BUF_VISIBLE_IDS, ra)[:n], twin.scene.download(capi.BUF_VISIBLE_IDS, rt)[:n])
        assert np.array_equal(a.scene.download(capi.BUF_VISIBLE_TYPE, ra), twin.scene.download(capi.BUF_VISIBLE_TYPE, rt))
        assert np.array_equal(a.scene.download(capi.BUF_RAYCAST_RESULT, ra), twin.scene.download(capi.BUF_RAYCAST_RESULT, rt))
        assert np.array_equal(a.points.numpy(), twin.points.numpy())
    rs2.close(); trs2.close(); a.close(); twin.close()


@pytest.mark.gpu
def test_prune_refills_an_exhausted_pool(hip, oracle):
    """lastFreeBlockId = -3: the pool ran dry and requests went unserved.  The prune leaves dropped - 1, and the next frame allocates
    out of the released blocks exactly as the oracle does from the same state."""
    sc = scenario_b(frames=4)
    a = TM.build(hip, sc, frames=3)
    c = a.scene.counters(a.rs)
    a.scene.set_counters(a.rs, -3, c["lastFreeExcessListId"], c["noVisibleEntries"])
    stats, pruned, _, _ = prune_and_compare(a.scene, [a.rs], "exhausted pool", **COVER)
    assert stats["dropped"] >= 100 and pruned["lastFreeBlockId"] == stats["dropped"] - 1 == stats["lastFreeBlockId"]
    ref = T.Session(oracle, sc)
    upload_pruned(ref, pruned, P.render_state_of(a.scene, a.rs))
    a.frame(3, fused=True); ref.frame(3, fused=True)
    ra, ro = a.snapshot(), ref.snapshot()
    assert ra.counters[0]["lastFreeBlockId"] < stats["dropped"] - 1, "the frame allocated nothing"
    for key in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries"):
        assert ra.counters[0][key] == ro.counters[0][key], (key, ra.counters, ro.counters)
    T.assert_fields_equal(ra.hash, ro.hash, "hash vs oracle"); T.assert_fields_equal(ra.voxels, ro.voxels, "voxels vs oracle")
    n = max(ra.counters[0]["lastFreeBlockId"] + 1, 0)
    assert np.array_equal(ra.alloc_list[:n], ro.alloc_list[:n]) and np.array_equal(ra.raycast, ro.raycast)
    a.close(); ref.close()


def everything(scene, rss):
    st = M.state_of(scene)
    return st, [P.render_state_of(scene, rs) for rs in rss]


def assert_everything_equal(got, want, what):
    (g, grs), (w, wrs) = got, want
    M.assert_state_equal(g, w, what, T.assert_fields_equal)
    assert np.array_equal(g["alloc"], w["alloc"]) and np.array_equal(g["excess"], w["excess"]), what + ": the whole lists"
    for a, b in zip(grs, wrs):
        assert a["n"] == b["n"] and np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["types"], b["types"]), what + ": render state"


@pytest.mark.gpu
def test_dry_run_changes_nothing_and_decides_as_the_real_run(hip):
    a = TM.build(hip, scenario_b())
    rs2 = a.scene.vis.CreateRenderState((W, H))
    a.scene.process_frame(a.view(4), rs2, a.points, a.normals)
    before = everything(a.scene, [a.rs, rs2])
    dry = a.scene.prune(a.scene.prune_config(dryRun=1, **COVER), decisions=True)
    assert_everything_equal(everything(a.scene, [a.rs, rs2]), before, "dry run")
    real = a.scene.prune(a.scene.prune_config(**COVER), decisions=True)
    assert np.array_equal(dry.pop("decisions"), real.pop("decisions")) and dry == real and real["dropped"] >= 100 and real["visibleRemoved"] > 0
    c = a.scene.counters()
    assert (c["lastFreeBlockId"], c["lastFreeExcessListId"]) == (real["lastFreeBlockId"], real["lastFreeExcessListId"])
    rs2.close(); a.close()


@pytest.mark.gpu
def test_prune_refusals_leave_everything_untouched(hip):
    a = TM.build(hip, scenario_b(), frames=2)
    before = everything(a.scene, [a.rs])

    def refused(scene, **kw):
        cfg = scene.prune_config().replace(**kw)
        stats = capi.PruneStats()
        rc = hip.fn["scene_prune"](_P(scene.h), C.byref(cfg), None, C.byref(stats), None)
        hip.sync()
        return rc == capi.ERR_INVALID and len(hip.fn["last_error"]() or b"") > 0

    for kw in (dict(classes=0), dict(classes=16), dict(freeSdf=float("nan")), dict(freeSdf=float("inf")), dict(freeSdf=1.5), dict(freeSdf=-1.25),
               dict(classes=P.WEAK, weakMaxW=0), dict(classes=P.EMPTY | P.WEAK, weakMaxW=-2), dict(classes=P.BOX, boxMin=(0, 3, 0), boxMax=(5, 2, 5)),
               dict(boxOnly=1, boxMin=(1, 0, 0), boxMax=(0, 0, 0))):
        assert refused(a.scene, **kw), kw
    assert hip.fn["scene_prune"](_P(a.scene.h), None, None, None, None) == capi.ERR_INVALID
    assert_everything_equal(everything(a.scene, [a.rs]), before, "bad configs")
    # (weakMaxW and the box are not looked at where they are not used)
    assert a.scene.prune(a.scene.prune_config(dryRun=1, weakMaxW=0, boxMin=(1, 1, 1), boxMax=(0, 0, 0), **COVER))["candidates"] > 0
    # a frame issued ahead
    v = [a.view(k) for k in (2, 3)]
    a.scene.process_frame_ahead(v[0], v[1], a.rs, a.points, a.normals)
    st = M.state_of(a.scene)
    assert refused(a.scene) and b"ahead" in hip.fn["last_error"]()
    M.assert_state_equal(M.state_of(a.scene), st, "ahead frame pending", T.assert_fields_equal)
    a.scene.cancel_ahead(a.rs)
    assert a.scene.prune(a.scene.prune_config(**COVER))["dropped"] > 0          # and the call that is in order goes through
    # a dense scene, a swapping scene
    dense = hip.create_scene(capi.VOXEL_S, capi.INDEX_DENSE, capi.default_params(voxelSize=0.01), denseSize=(64, 64, 64))
    dense.reco.ResetScene()
    d0 = dense.download(capi.BUF_VOXEL_BLOCKS)
    assert refused(dense)
    T.assert_fields_equal(dense.download(capi.BUF_VOXEL_BLOCKS), d0, "dense scene after a refusal")
    swap, rs = TM.swapping_scene(hip, 1)
    s0 = TM.snapshot(swap)
    assert refused(swap) and refused(swap, dryRun=1)
    s1 = TM.snapshot(swap)
    M.assert_state_equal(s1, s0, "swapping scene", T.assert_fields_equal)
    assert np.array_equal(s1["swap"], s0["swap"])
    rs.close(); swap.close(); dense.close(); a.close()


@pytest.mark.gpu
def test_prune_launches_recorded_frames_first(hip):
    """The scene holds recorded, unflushed engine calls when prune is called; the result is that of the eager run."""
    results = []
    for recorded in (True, False):
        ses = TM.build(hip, scenario_b(), frames=2, deferred=recorded)
        v = ses.view(2)
        ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
        ses.scene.reco.IntegrateIntoScene(v, ses.rs)
        ses.scene.vis.CreateExpectedDepths(v.M_d, v.intr_d, ses.rs)        # recorded: nothing of frame 2 has been launched yet
        if recorded:
            stats = ses.scene.prune(ses.scene.prune_config(**COVER))
            got = M.state_of(ses.scene)
        else:
            stats, got, _, _ = prune_and_compare(ses.scene, [ses.rs], "recorded frames (eager)", **COVER)
        results.append((stats, got, P.render_state_of(ses.scene, ses.rs)))
        ses.close()
    assert results[0][0] == results[1][0] and results[0][0]["dropped"] >= 100
    M.assert_state_equal(results[0][1], results[1][1], "recorded vs eager", T.assert_fields_equal)
    P.assert_render_state_equal(results[0][2], results[1][2], "recorded vs eager")


@pytest.mark.gpu
def test_box_erases_a_region(hip):
    """ITM_PRUNE_BOX over the blocks of the sphere (radius 0.5 m around (0.05, 0.02, 1.4) m, blocks of 8 cm) with protect = 1: nothing
    is left inside but pinned heads, queries inside read no block, and a mesh has no vertex there."""
    a = TM.build(hip, scenario_b())
    lo, hi = np.array((-7, -7, 10)), np.array((7, 7, 24))

    def inside(blocks):
        return np.all((blocks >= lo) & (blocks <= hi), axis=1)

    def mesh_blocks():
        mesh = capi.Mesh(a.scene)
        mesh.MeshScene()
        tri = mesh.triangles().reshape(-1, 3)
        mesh.close()
        # (a vertex ON a block's first voxel plane, 0.64 m say, is a float32 just below it: a thousandth of a voxel decides for that block)
        return np.floor((tri.astype(np.float64) / 0.01 + 1e-3) / 8).astype(np.int64), tri

    blocks0, _ = mesh_blocks()
    assert np.count_nonzero(inside(blocks0)) > 1000, "the sphere is not where the box is"
    stats, pruned, dec, before = prune_and_compare(a.scene, [a.rs], "box erase", classes=P.BOX, boxMin=tuple(lo), boxMax=tuple(hi), protect=1)
    assert stats["inBox"] > 300 and stats["candidates"] == stats["inBox"] and stats["protectedByNeighbour"] == 0
    assert stats["dropped"] == stats["inBox"] - stats["pinnedHeads"] and (dec[(dec & P.BIT_DROPPED) != 0] & P.BIT_SURFACE).any()
    h = pruned["hash"]
    left = np.nonzero((h["ptr"] >= -1) & inside(h["pos"].astype(np.int64)))[0]
    pinned = np.nonzero(((dec & P.BIT_CANDIDATE) != 0) & ((dec & P.BIT_DROPPED) == 0))[0]
    assert np.array_equal(left, pinned) and len(pinned) == stats["pinnedHeads"] and np.all(pinned < pruned["bucketNum"])
    # the centre voxel of every dropped block reads "no block"
    gone = before["hash"]["pos"][(dec & P.BIT_DROPPED) != 0].astype(np.float32)
    q = a.scene.query_points(gone * 8 + 4, units="voxels", want=("sdf_nearest", "weight", "flags"))
    assert not np.any(q["flags"] & 1) and not np.any(q["weight"])
    blocks1, _ = mesh_blocks()
    keep = {tuple(p) for p in h["pos"][pinned].tolist()}
    stray = [tuple(b) for b in blocks1[inside(blocks1)].tolist() if tuple(b) not in keep]
    assert not stray, "mesh vertices inside the erased box: %s" % stray[:5]
    assert len(blocks1) > 1000, "the wall outside the box is still meshed"
    a.close()


DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "scene_prune_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "scene_prune_demo")


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_prune_adapters_compile_and_link():
    assert os.path.exists(build_demo())


@pytest.mark.gpu
@pytest.mark.parametrize("every", [2, 0])
def test_cpp_engine_with_prune_every_n_frames_equals_the_python_path(hip, every):
    """ITMMainEngine_HIP over six frames with pruneEveryNFrames = 2 ends in the state the binding reaches with the same calls; with 0
    in the state of a run that never prunes."""
    exe = build_demo()
    got = json.loads(subprocess.run([exe, str(every)], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
    w, h, n = 160, 120, 160 * 120
    s = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.01), localBlockNum=0x4000)
    s.reco.ResetScene()
    s.set_deferred_fusion(True)
    rs = s.vis.CreateRenderState((w, h))
    raw = hip.to_backend(np.full((h, w), 1500, np.int16))
    depth = capi.DevBuffer(hip, n * 4, np.float32, (h, w))
    hip.check(hip.fn["convert_depth_affine"](_P(raw.ptr), _P(depth.ptr), w, h, 0.001, 0.0, None), "convert_depth_affine")
    pts = capi.DevBuffer(hip, n * 16, np.float32, (n, 4)); nrm = capi.DevBuffer(hip, n * 16, np.float32, (n, 4))
    kw = dict(classes=P.EMPTY | P.FREE | P.WEAK, weakMaxW=1, protect=0)          # once-seen blocks too: the flat wall leaves no empty ones
    cfg = s.prune_config(**kw)
    prunes = dropped = removed = 0
    for k in range(6):
        Mk = np.eye(4, dtype=np.float32); Mk[0, 3] = -np.float32(0.05) * np.float32(k)
        v = capi.View(depth, w, h, M_d=np.ascontiguousarray(Mk.T).reshape(16), intr_d=(145.0, 145.0, 80.0, 60.0))
        s.process_frame(v, rs, pts, nrm)
        if every and (k + 1) % every == 0:
            st = s.prune(cfg)
            prunes += 1; dropped += st["dropped"]; removed += st["visibleRemoved"]
    dry = s.prune(s.prune_config(dryRun=1, **kw))
    c = s.counters(rs)
    want = dict(prunes=prunes, dropped=dropped, visibleRemoved=removed, lastFreeBlockId=c["lastFreeBlockId"], lastFreeExcessListId=c["lastFreeExcessListId"],
                noVisibleEntries=c["noVisibleEntries"], table=TM.word_digest(s.download(capi.BUF_HASH_ENTRIES)), voxels=TM.word_digest(s.download(capi.BUF_VOXEL_BLOCKS)),
                dry_considered=dry["considered"], dry_candidates=dry["candidates"], dry_dropped=dry["dropped"])
    print(got)
    assert got == want
    assert (prunes, dropped > 0, removed > 0) == ((3, True, True) if every else (0, False, False)) and dry["considered"] > 100
    assert every or dry["candidates"] > 0
    rs.close(); s.close()
