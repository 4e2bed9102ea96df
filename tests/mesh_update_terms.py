"""Numpy restatement of the incremental mesh's bookkeeping (include/itm_hip.h, itm_mesh_update: steps 1-3 and 6 of the definition) from
two downloads of the hash table -- as it was when the run table was made, as it is now -- and the marked slots.  The triangles are never
restated: the expected buffer is MeshScene of the same scene.  Also the triangle count of every listed block from its voxels (the
per-configuration counts of mesh_dense_cases.ntri_table), to split a soup into the runs of its blocks."""
import numpy as np

import mesh_dense_cases as MD
from infinitam_amd.capi import MESH_CHANGED_DTYPE, MESH_REMOVED_DTYPE, MESH_UPDATE_ALL_MARKED, MESH_UPDATE_NO_RUN_TABLE, MESH_UPDATE_OVERFLOW

F = np.float32
STAT_NAMES = ("full", "allocated", "marked", "ignoredMarks", "appeared", "vanished", "remeshed", "kept", "noChanged", "noRemoved")


def keys(pos):
    """one int64 per block position [..., 3]; neighbours at +-1 of any int16 position keep distinct keys"""
    p = np.asarray(pos, np.int64) + 40000
    return p[..., 0] | (p[..., 1] << 20) | (p[..., 2] << 40)


def listed(table):
    """the slots with ptr >= 0, ascending"""
    return np.nonzero(table["ptr"] >= 0)[0]


def terms(table0, table1, marks, run_current=True, everything=False, overflow=False):
    """table0: the table when the run table was made (ignored unless run_current), table1: the table now, marks: every value handed to
    Touch since the last update (any order, duplicates, values outside the table).  Returns the statistics that do not count triangles,
    `dirty` (the slots of D, ascending) and the delta's `changed` (slot, pos) and `removed` records."""
    n = len(table1)
    marks = np.asarray(marks, np.int64).reshape(-1)
    inside = (marks >= 0) & (marks < n)
    marked = np.unique(marks[inside])
    a1 = listed(table1)
    pos1 = table1["pos"][a1].astype(np.int64)
    out = dict(full=0, allocated=len(a1), marked=len(marked), ignoredMarks=int((~inside).sum()), appeared=0, vanished=0)
    removed = np.zeros(0, MESH_REMOVED_DTYPE)
    dirty = a1
    if run_current:
        a0 = listed(table0)
        both = np.intersect1d(a0, a1)
        moved = both[np.any(table0["pos"][both] != table1["pos"][both], axis=1)]
        appeared = np.union1d(np.setdiff1d(a1, a0), moved)
        vanished = np.union1d(np.setdiff1d(a0, a1), moved)
        out.update(appeared=len(appeared), vanished=len(vanished))
        seeds = np.concatenate([keys(table1["pos"][np.intersect1d(marked, a1)]), keys(table1["pos"][appeared]), keys(table0["pos"][vanished])])
        hit = np.zeros(len(a1), bool)
        for d in range(8):
            hit |= np.isin(keys(pos1 + np.array([d & 1, (d >> 1) & 1, d >> 2])), seeds)
        dirty = a1[hit]
        gone = vanished[~np.isin(keys(table0["pos"][vanished]), keys(pos1))]
        removed = np.zeros(len(gone), MESH_REMOVED_DTYPE)
        removed["slot"] = gone
        removed["pos"] = table0["pos"][gone]
    if not run_current:
        out["full"] = MESH_UPDATE_NO_RUN_TABLE
    elif everything:
        out["full"] = MESH_UPDATE_ALL_MARKED
    elif overflow:                                                        # (the caller knows: the triangles are not restated)
        out["full"] = MESH_UPDATE_OVERFLOW
    if out["full"]:
        dirty = a1
    changed = np.zeros(len(dirty), MESH_CHANGED_DTYPE)
    changed["slot"] = dirty
    changed["pos"] = table1["pos"][dirty]
    out.update(remeshed=len(dirty), kept=len(a1) - len(dirty), noChanged=len(dirty), noRemoved=len(removed))
    return out, dirty, changed, removed


def block_counts(table, voxels):
    """triangles of every listed block, in slot order: its 512 cells read its own voxels and one layer of the seven blocks at +d; a
    corner without a voxel or equal to 1.0f kills the cell"""
    a = listed(table)
    pos = table["pos"][a].astype(np.int64)
    order = np.argsort(keys(pos))
    sorted_keys = keys(pos)[order]
    sdf = MD.to_float(np.asarray(voxels)["sdf"]).reshape(-1, 8, 8, 8)              # [block, z, y, x]
    val = np.full((len(a), 9, 9, 9), np.nan, F)
    for d in range(8):
        dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
        k = keys(pos + np.array([dx, dy, dz]))
        at = np.searchsorted(sorted_keys, k)
        at[at >= len(a)] = 0
        found = sorted_keys[at] == k
        ptr = table["ptr"][a[order[at]]]
        sx, sy, sz = (slice(8, 9) if dx else slice(0, 8)), (slice(8, 9) if dy else slice(0, 8)), (slice(8, 9) if dz else slice(0, 8))
        src = sdf[ptr[found]][:, (slice(0, 1) if dz else slice(0, 8)), (slice(0, 1) if dy else slice(0, 8)), (slice(0, 1) if dx else slice(0, 8))]
        sub = val[:, sz, sy, sx]
        sub[found] = src
        val[:, sz, sy, sx] = sub
    ok = np.ones((len(a), 8, 8, 8), bool)
    cube = np.zeros((len(a), 8, 8, 8), np.int64)
    for j, (dx, dy, dz) in enumerate(MD.CORNERS):
        c = val[:, dz:dz + 8, dy:dy + 8, dx:dx + 8]
        ok &= ~np.isnan(c) & (c != F(1))
        cube |= (c < 0).astype(np.int64) << j
    return a, np.where(ok, MD.ntri_table()[cube], 0).reshape(len(a), -1).sum(axis=1)


def runs(table, voxels, tri):
    """{slot: the bytes of its run} of a soup in slot order; the counts must add up to the soup's length"""
    a, cnt = block_counts(table, voxels)
    assert int(cnt.sum()) == len(tri), f"per-block total {int(cnt.sum())} != the soup's {len(tri)}"
    start = np.cumsum(cnt) - cnt
    raw = np.ascontiguousarray(tri, F).view(np.uint32).reshape(len(tri), 9)
    return {int(s): raw[b:b + c].tobytes() for s, b, c in zip(a, start, cnt)}, dict(zip(a.tolist(), cnt.tolist()))
