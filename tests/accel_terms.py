"""The invariant of the acceleration cubes (infinitam_amd/csrc/accel_device.h, scene.hip), restated in numpy on DOWNLOADED buffers -- the
hash table, the voxel pool and accel_info() -- and compared with what the read-only probe and census of include/itm_debug.h find in
device memory:

    the only non-empty cells are those of table entries with ptr >= 0, at the scene's current origin, and a mirror cell holds the raw
    sdf of its voxel.

Spelled out:
  * an entry with ptr >= 0 inside the directory cube (512 blocks per side at origin_directory) has dirPtr == ptr and dirSlot == its
    table index; outside the cube it has no cell;
  * an entry with ptr >= 0 inside the mirror cube (256 per side paged, the side that follows from mirror_bytes dense) whose page is
    mapped (or in the dense form) has its 512 mirror values equal to the raw sdf fields of voxels ptr * 512 ... of the pool, bit for
    bit, in the block's own order; with page entry -3 ("unmappable": the pool had run dry) it has no place; its page is never -1;
  * entries with ptr == -1 (swapped out), removed entries and positions that were never allocated have empty directory cells (-1) and
    a mirror block that is all "absent" (-32768 / 0xffffffff) wherever it has a place;
  * census: the non-empty cells of either directory number the ptr >= 0 entries inside the directory cube, the mirror blocks with a
    cell that is not "absent" number the ptr >= 0 entries that have a place -- over the WHOLE cube / every page of the pool, so a
    dirty page that went back to the pool, or a cell left behind at an old origin, is counted;
  * page table: no entry is -2 outside a kernel; the entries >= 0 are distinct, lie below mirror_pages_mapped, and number exactly
    mirror_pages_mapped (every page the pool handed out sits in the table); mirror_pages_mapped <= mirror_pages.
  * pages_exact (after ResetScene, after a cube move followed by the refill, and at any time in a scene whose blocks never leave):
    the pages that are not -1 are exactly the pages that hold an entry with ptr >= 0.  Otherwise -- BETWEEN such events in a scene
    that swaps -- a page may stay mapped (or marked unmappable) although every block in it has been swapped out and all its cells are
    "absent": the page goes back to the pool only at the next unfill.  That is allowed here, and only there.
"""
import numpy as np

from infinitam_amd import capi

DIR_SIDE = 512
PAGED_SIDE = 256
PAGE = 16                    # blocks per side of a page
TABLE_SIDE = PAGED_SIDE // PAGE
PAGE_NONE, PAGE_CLAIMING, PAGE_UNMAPPABLE = -1, -2, -3
NEIGHBOURS = np.array([(x, y, z) for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.int64)


def is_short(voxel_type):
    return voxel_type in (capi.VOXEL_S, capi.VOXEL_S_RGB)


def geometry(info, voxel_type):
    """Where the cubes lie and which form the mirror has, from accel_info() alone."""
    elem = 2 if is_short(voxel_type) else 4
    g = dict(dir=info["directory_bytes"] > 0, slot=info["slot_directory_bytes"] > 0,
             dir_org=np.asarray(info["origin_directory"], np.int64), mir_org=np.asarray(info["origin_mirror"], np.int64),
             pages=int(info["mirror_pages"]), mapped=int(info["mirror_pages_mapped"]),
             absent=np.int16(-32768) if elem == 2 else np.uint32(0xffffffff))
    if info["mirror_bytes"] == 0:
        g["form"], g["side"] = "none", 0
    elif info["mirror_pages"] > 0:
        g["form"], g["side"] = "paged", PAGED_SIDE
    else:
        blocks = info["mirror_bytes"] // (512 * elem)
        side = int(round(blocks ** (1.0 / 3.0)))
        assert side ** 3 == blocks and side & (side - 1) == 0, "mirror_bytes %d is no cube of blocks" % info["mirror_bytes"]
        g["form"], g["side"] = "dense", side
    return g


def keys_of(pos):
    p = np.asarray(pos, np.int64).reshape(-1, 3) + (1 << 17)
    return (p[:, 0] << 40) | (p[:, 1] << 20) | p[:, 2]


def raw_sdf(voxels):
    """The sdf fields of the pool as the mirror stores them: int16 as they are, float32 as their bits."""
    s = np.ascontiguousarray(voxels["sdf"])
    return s if s.dtype == np.int16 else s.view(np.uint32)


def positions_to_probe(hsh):
    """Every entry with ptr >= 0 or ptr == -1 (slot and position), then the 26 neighbours of each that are not in the table themselves
    (slot -1)."""
    slots = np.nonzero(hsh["ptr"] >= -1)[0]
    pos = hsh["pos"][slots].astype(np.int64).reshape(-1, 3)
    if len(pos) == 0:
        return slots.astype(np.int64), pos
    nb = (pos[:, None, :] + NEIGHBOURS[None, :, :]).reshape(-1, 3)
    k, first = np.unique(keys_of(nb), return_index=True)
    nb = nb[first[~np.isin(k, keys_of(pos))]]
    return np.concatenate([slots.astype(np.int64), np.full(len(nb), -1, np.int64)]), np.concatenate([pos, nb])


def table_index(rel):
    """Page-table index of cube-relative block coordinates (inside the paged cube)."""
    p = rel // PAGE
    return (p[:, 2] * TABLE_SIDE + p[:, 1]) * TABLE_SIDE + p[:, 0]


def expected_cells(hsh, voxels, geo, positions, page_table):
    """What the probe must find at `positions` ([n][3]): arrays dir_covered, dir_ptr, dir_slot, mirror_covered, page, no_place,
    values[n][512], and slot (the table index of the resident entry there, -1 if none) / out_slot (of a swapped-out one)."""
    pos = np.asarray(positions, np.int64).reshape(-1, 3)
    n = len(pos)
    live = np.nonzero(hsh["ptr"] >= -1)[0]
    lk = keys_of(hsh["pos"][live])
    order = np.argsort(lk, kind="stable")
    lk, live = lk[order], live[order]
    assert len(np.unique(lk)) == len(lk), "a position occurs twice in the table"
    pk = keys_of(pos)
    at = np.searchsorted(lk, pk)
    found = (at < len(lk)) & (lk[np.minimum(at, max(len(lk) - 1, 0))] == pk) if len(lk) else np.zeros(n, bool)
    entry = np.where(found, live[np.minimum(at, max(len(lk) - 1, 0))] if len(lk) else -1, -1)
    ptr = np.where(found, hsh["ptr"][np.maximum(entry, 0)], -2).astype(np.int64)
    resident = ptr >= 0
    rel_d = pos - geo["dir_org"]
    dir_covered = np.all((rel_d >= 0) & (rel_d < DIR_SIDE), axis=1) & geo["dir"]
    rel_m = pos - geo["mir_org"]
    mirror_covered = np.all((rel_m >= 0) & (rel_m < max(geo["side"], 1)), axis=1) & (geo["form"] != "none")
    page = np.full(n, PAGE_NONE, np.int64)
    if geo["form"] == "paged":
        page[mirror_covered] = np.asarray(page_table, np.int64)[table_index(rel_m[mirror_covered])]
    no_place = ~mirror_covered | ((geo["form"] == "paged") & (page < 0))
    raw = raw_sdf(voxels).reshape(-1, 512)
    values = np.full((n, 512), geo["absent"], raw.dtype)
    filled = resident & ~no_place
    values[filled] = raw[ptr[filled]]
    return dict(dir_covered=dir_covered, dir_ptr=np.where(resident & dir_covered, ptr, -1), dir_slot=np.where(resident & dir_covered & geo["slot"], entry, -1),
                mirror_covered=mirror_covered, page=page, no_place=no_place, values=values, slot=np.where(resident, entry, -1),
                out_slot=np.where(found & (ptr == -1), entry, -1))


def expected_census(hsh, geo, page_table):
    """The census the whole table implies, and what the test cases want to know about the situation (all from the inputs)."""
    res = np.nonzero(hsh["ptr"] >= 0)[0]
    pos = hsh["pos"][res].astype(np.int64).reshape(-1, 3)
    in_dir = np.all((pos - geo["dir_org"] >= 0) & (pos - geo["dir_org"] < DIR_SIDE), axis=1)
    rel_m = pos - geo["mir_org"]
    in_mir = np.all((rel_m >= 0) & (rel_m < max(geo["side"], 1)), axis=1) & (geo["form"] != "none")
    placed = in_mir.copy()
    pages_wanted = np.zeros(0, np.int64)
    unmappable = 0
    if geo["form"] == "paged":
        t = table_index(rel_m[in_mir])
        e = np.asarray(page_table, np.int64)[t]
        placed[in_mir] = e >= 0
        unmappable = int(np.count_nonzero(e == PAGE_UNMAPPABLE))
        pages_wanted = np.unique(t)
    return dict(directory_cells=int(np.count_nonzero(in_dir)) if geo["dir"] else 0, slot_directory_cells=int(np.count_nonzero(in_dir)) if geo["slot"] else 0,
                mirror_blocks=int(np.count_nonzero(placed)), resident=len(res), swapped_out=int(np.count_nonzero(hsh["ptr"] == -1)),
                outside_directory=int(np.count_nonzero(~in_dir)), outside_mirror=int(np.count_nonzero(~in_mir)),
                in_unmappable_pages=unmappable, pages_wanted=pages_wanted)


def page_table_failures(page_table, page_counter, geo, pages_wanted, pages_exact):
    t = np.asarray(page_table, np.int64)
    out = []
    if geo["form"] != "paged":
        if np.any(t != PAGE_NONE) or page_counter != 0:
            out.append("page table: a scene without a paged mirror reports entries %s, counter %d" % (np.unique(t).tolist()[:8], page_counter))
        return out
    mapped, pages = geo["mapped"], geo["pages"]
    if not mapped <= pages:
        out.append("page table: mirror_pages_mapped %d > mirror_pages %d" % (mapped, pages))
    if mapped != min(max(page_counter, 0), pages):
        out.append("page table: mirror_pages_mapped %d, but the pool's counter is %d of %d pages" % (mapped, page_counter, pages))
    for i in np.nonzero(t == PAGE_CLAIMING)[0][:4]:
        out.append("page table: entry %d is -2 (being claimed) outside a kernel" % i)
    bad = np.nonzero((t < PAGE_UNMAPPABLE) | (t >= mapped))[0]
    for i in bad[:4]:
        out.append("page table: entry %d is %d, mirror_pages_mapped is %d" % (i, t[i], mapped))
    v = t[t >= 0]
    if len(np.unique(v)) != len(v):
        u, c = np.unique(v, return_counts=True)
        d = int(u[c > 1][0])
        out.append("page table: page %d of the pool is mapped by entries %s" % (d, np.nonzero(t == d)[0].tolist()))
    if len(v) != mapped:
        out.append("page table: %d entries >= 0, mirror_pages_mapped is %d (a page was handed out and is not in the table, or the reverse)" % (len(v), mapped))
    for i in pages_wanted[t[pages_wanted] == PAGE_NONE][:4]:
        out.append("page table: entry %d is -1 but the page holds an entry with ptr >= 0" % i)
    if pages_exact:
        stale = np.setdiff1d(np.nonzero(t != PAGE_NONE)[0], pages_wanted)
        for i in stale[:4]:
            out.append("page table: entry %d is %d but no entry with ptr >= 0 lies in that page (pages must be exactly those that hold a block here)" % (i, t[i]))
    return out


def compare(slots, positions, want, got, census_want, census_got, limit=8):
    """Failure messages: each names the entry, its position, the structure and the two values (expected, found)."""
    out = []

    def who(i):
        e = int(want["slot"][i]) if want["slot"][i] >= 0 else int(want["out_slot"][i])
        kind = "entry %d (ptr >= 0)" % e if want["slot"][i] >= 0 else "entry %d (swapped out)" % e if e >= 0 else "no entry (a neighbour of one)"
        return "%s at block %s" % (kind, tuple(int(c) for c in positions[i]))

    for key, name in (("dir_covered", "directory cube covers"), ("dir_ptr", "dirPtr"), ("dir_slot", "dirSlot"), ("mirror_covered", "mirror cube covers"),
                      ("page", "page-table entry"), ("no_place", "mirror 'no place' flag")):
        bad = np.nonzero(np.asarray(want[key]) != np.asarray(got[key]))[0]
        for i in bad[:limit]:
            out.append("%s: %s: expected %s, found %s" % (who(i), name, want[key][i], got[key][i]))
        if len(bad) > limit:
            out.append("... %s differs at %d positions in all" % (name, len(bad)))
    bad = np.nonzero(np.any(want["values"] != got["values"], axis=1))[0]
    for i in bad[:limit]:
        v = int(np.nonzero(want["values"][i] != got["values"][i])[0][0])
        out.append("%s: sdf mirror: %d of 512 values differ, first at voxel %d: expected %s, found %s"
                   % (who(i), int(np.count_nonzero(want["values"][i] != got["values"][i])), v, want["values"][i][v], got["values"][i][v]))
    if len(bad) > limit:
        out.append("... sdf mirror differs at %d positions in all" % len(bad))
    for key, name in (("directory_cells", "block directory"), ("slot_directory_cells", "slot directory"), ("mirror_blocks", "sdf mirror")):
        if census_want[key] != census_got[key]:
            out.append("census: %s: %d entries with ptr >= 0 have a cell there, the cube holds %d non-empty ones" % (name, census_want[key], census_got[key]))
    return out


def audit(scene, rs=None, pages_exact=None, what=""):
    """Census, downloads, probe and restatement of one scene, as it is now (recorded engine calls are launched by the census: it runs
    first).  pages_exact: see the module's text; by default true unless the scene swaps.  Raises AssertionError listing what differs;
    returns the expected census with the facts about the situation (resident, swapped_out, outside_directory, outside_mirror,
    in_unmappable_pages, moves, form ...) and the downloads it was computed from (hash, voxels, info, census)."""
    if pages_exact is None:
        pages_exact = not scene.cfg.useSwapping
    census = scene.accel_census()
    info = scene.accel_info()
    hsh = scene.download(capi.BUF_HASH_ENTRIES, rs)
    voxels = scene.download(capi.BUF_VOXEL_BLOCKS, rs)
    geo = geometry(info, scene.cfg.voxelType)
    assert census["mirror_form"] == geo["form"] and census["has_directory"] == geo["dir"], (what, census["mirror_form"], geo["form"], info)
    slots, pos = positions_to_probe(hsh)
    got = scene.accel_probe(pos)
    want = expected_cells(hsh, voxels, geo, pos, census["page_table"])
    cw = expected_census(hsh, geo, census["page_table"])
    fails = compare(slots, pos, want, got, cw, census)
    fails += page_table_failures(census["page_table"], census["page_counter"], geo, cw["pages_wanted"], pages_exact)
    assert not fails, "%s: %d finding(s) [form %s, origins %s / %s, %d resident, %d swapped out]:\n  %s" % (
        what or "audit", len(fails), geo["form"], info["origin_directory"], info["origin_mirror"], cw["resident"], cw["swapped_out"], "\n  ".join(fails[:40]))
    cw.update(form=geo["form"], side=geo["side"], moves=int(info["moves"]), placed=info["placed"], probed=len(pos), info=info, census=census, hash=hsh, voxels=voxels)
    return cw
