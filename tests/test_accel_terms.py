"""tests/accel_terms.py (the invariant of the block directory, the slot directory and the sdf mirror, restated in numpy) against values
written out by hand: tables of a dozen entries that straddle a face of either cube and a page boundary, with one swapped-out entry
and one entry in a page the pool could not map.  No GPU: what the probe and the census would report is written out here too."""
import numpy as np

import accel_terms as A
from infinitam_amd import capi

ABSENT = -32768


def table(entries, n=16):
    h = np.zeros(n, capi.HASH_ENTRY_DTYPE)
    h["ptr"] = -2
    for slot, (pos, ptr) in entries.items():
        h[slot]["pos"], h[slot]["ptr"] = pos, ptr
    return h


def pool(blocks):
    """voxel v of block b holds sdf 100 b + (v mod 97): every block is recognisable, no value is "absent"."""
    vox = np.zeros(blocks * 512, capi.VOXEL_DTYPES[capi.VOXEL_S])
    vox["sdf"] = (100 * (np.arange(blocks * 512) // 512) + np.arange(blocks * 512) % 512 % 97).astype(np.int16)
    vox["w_depth"] = 7
    return vox


# the directory cube covers x, y, z in [0, 512), the paged mirror cube [0, 256); pages are 16 blocks wide
ENTRIES = {
    0: ((0, 0, 0), 3),        # page 0
    1: ((15, 0, 0), 0),       # page 0, last block before the page boundary
    2: ((16, 0, 0), 5),       # page 1, first block behind it
    3: ((255, 0, 0), 1),      # page 15: the last block inside the mirror cube
    4: ((256, 0, 0), 2),      # outside the mirror cube, inside the directory cube
    5: ((511, 0, 0), 4),      # the last block inside the directory cube
    6: ((512, 0, 0), 6),      # outside both
    7: ((-1, 0, 0), 7),       # outside both, on the other side
    8: ((0, 16, 0), -1),      # swapped out; its page (16) was never mapped
    9: ((0, 0, 16), 8),       # page 256: the pool had run dry (-3)
    10: ((17, 0, 0), 9),      # page 1
    12: ((3, 3, 3), 10),      # page 0
}
INFO = dict(directory_bytes=512 ** 3 * 4, slot_directory_bytes=512 ** 3 * 4, mirror_bytes=3 * 4096 * 1024 + 16384, mirror_pages=3, mirror_pages_mapped=3,
            origin_directory=[0, 0, 0], origin_mirror=[0, 0, 0], placed=True, moves=0)


def page_table():
    t = np.full(4096, -1, np.int32)
    t[0], t[1], t[15], t[256] = 1, 0, 2, -3
    return t


def test_geometry_from_accel_info():
    g = A.geometry(INFO, capi.VOXEL_S)
    assert (g["form"], g["side"], g["pages"], g["mapped"], g["dir"], g["slot"]) == ("paged", 256, 3, 3, True, True)
    dense = dict(INFO, mirror_bytes=64 ** 3 * 1024, mirror_pages=0, mirror_pages_mapped=0)
    assert (A.geometry(dense, capi.VOXEL_S)["form"], A.geometry(dense, capi.VOXEL_S)["side"]) == ("dense", 64)
    assert A.geometry(dict(dense, mirror_bytes=32 ** 3 * 2048), capi.VOXEL_F)["side"] == 32          # float bits: two kilobytes per block
    off = dict(INFO, mirror_bytes=0, mirror_pages=0, mirror_pages_mapped=0)
    assert A.geometry(off, capi.VOXEL_F_RGB)["form"] == "none"
    nodir = dict(off, directory_bytes=0, slot_directory_bytes=0)
    assert not A.geometry(nodir, capi.VOXEL_S)["dir"]


def test_positions_cover_every_entry_and_its_free_neighbours():
    slots, pos = A.positions_to_probe(table(ENTRIES))
    assert slots[:12].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12] and np.all(slots[12:] == -1)
    assert [tuple(p) for p in pos[:12].tolist()] == [ENTRIES[s][0] for s in slots[:12]]
    nb = {tuple(p) for p in pos[12:].tolist()}
    assert len(nb) == len(pos) - 12, "a neighbour is probed twice"
    assert not nb & {e[0] for e in ENTRIES.values()}, "an entry's position is listed as a free neighbour"
    # (15, 0, 0), (16, 0, 0) and (17, 0, 0) are entries and each other's neighbours: the union of the 3 x 3 x 3 boxes around x = 15, 16, 17 is x in 14 .. 18, 45 positions, 3 of them entries
    box = {(x, y, z) for x in range(14, 19) for y in (-1, 0, 1) for z in (-1, 0, 1)} - {(15, 0, 0), (16, 0, 0), (17, 0, 0)}
    assert box <= nb and len(box) == 42
    assert (1, 1, 1) in nb and (2, 2, 2) in nb and (-2, 0, 0) in nb and (513, 1, -1) in nb


def test_expected_cells_known_answers():
    h, vox = table(ENTRIES), pool(11)
    geo = A.geometry(INFO, capi.VOXEL_S)
    pos = [(0, 0, 0), (15, 0, 0), (16, 0, 0), (255, 0, 0), (256, 0, 0), (511, 0, 0), (512, 0, 0), (-1, 0, 0), (0, 16, 0), (0, 0, 16), (1, 0, 0), (300, 300, 300), (0, 255, 255)]
    w = A.expected_cells(h, vox, geo, pos, page_table())
    assert w["dir_covered"].tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1]
    assert w["dir_ptr"].tolist() == [3, 0, 5, 1, 2, 4, -1, -1, -1, 8, -1, -1, -1]
    assert w["dir_slot"].tolist() == [0, 1, 2, 3, 4, 5, -1, -1, -1, 9, -1, -1, -1]
    assert w["mirror_covered"].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 1]
    assert w["page"].tolist() == [1, 1, 0, 2, -1, -1, -1, -1, -1, -3, 1, -1, -1]
    assert w["no_place"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1]
    assert w["slot"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, -1, 9, -1, -1, -1] and w["out_slot"].tolist() == [-1] * 8 + [8] + [-1] * 4
    v = w["values"]
    assert v.dtype == np.int16 and v.shape == (13, 512)
    assert v[0].tolist() == [300 + t % 97 for t in range(512)]                      # block 3 of the pool, in the pool's own order
    assert (v[1][0], v[1][96], v[1][97], v[1][511]) == (0, 96, 0, 511 % 97)         # block 0
    assert v[2][5] == 505 and v[3][0] == 100
    for i in (4, 5, 6, 7, 8, 9, 10, 11, 12):                                        # outside, swapped out, unmappable, free neighbour, empty space
        assert np.all(v[i] == ABSENT), i


def test_expected_census_known_answers():
    h = table(ENTRIES)
    c = A.expected_census(h, A.geometry(INFO, capi.VOXEL_S), page_table())
    assert (c["directory_cells"], c["slot_directory_cells"], c["mirror_blocks"]) == (9, 9, 6)
    assert (c["resident"], c["swapped_out"], c["outside_directory"], c["outside_mirror"], c["in_unmappable_pages"]) == (11, 1, 2, 4, 1)
    assert c["pages_wanted"].tolist() == [0, 1, 15, 256]
    # the dense form, a cube of 32 blocks at (-16, -16, -16): x = -1, 0, 3, 15 are inside, 16 and 17 are not; every covered block has a place
    dense = dict(INFO, mirror_bytes=32 ** 3 * 1024, mirror_pages=0, mirror_pages_mapped=0, origin_mirror=[-16, -16, -16])
    g = A.geometry(dense, capi.VOXEL_S)
    c = A.expected_census(h, g, np.full(4096, -1, np.int32))
    assert (c["mirror_blocks"], c["outside_mirror"], c["in_unmappable_pages"]) == (4, 7, 0)
    w = A.expected_cells(h, pool(11), g, [(-1, 0, 0), (15, 0, 0), (16, 0, 0), (0, 0, 15), (0, 0, 16), (0, 16, 0)], np.full(4096, -1, np.int32))
    assert w["mirror_covered"].tolist() == [1, 1, 0, 1, 0, 0] and w["no_place"].tolist() == [0, 0, 1, 0, 1, 1]
    assert w["values"][0][0] == 700 and w["values"][1][1] == 1 and np.all(w["values"][2:] == ABSENT)
    # no mirror, no directories: nothing is expected anywhere
    none = dict(INFO, directory_bytes=0, slot_directory_bytes=0, mirror_bytes=0, mirror_pages=0, mirror_pages_mapped=0)
    c = A.expected_census(h, A.geometry(none, capi.VOXEL_S), np.full(4096, -1, np.int32))
    assert (c["directory_cells"], c["slot_directory_cells"], c["mirror_blocks"]) == (0, 0, 0)


def observed():
    h, vox = table(ENTRIES), pool(11)
    geo = A.geometry(INFO, capi.VOXEL_S)
    slots, pos = A.positions_to_probe(h)
    want = A.expected_cells(h, vox, geo, pos, page_table())
    got = {k: np.array(v, copy=True) for k, v in want.items()}
    cw = A.expected_census(h, geo, page_table())
    return slots, pos, want, got, cw, dict(directory_cells=9, slot_directory_cells=9, mirror_blocks=6)


def test_compare_names_entry_position_structure_and_values():
    slots, pos, want, got, cw, cg = observed()
    assert A.compare(slots, pos, want, got, cw, cg) == []
    got["values"][8][100] = 32767                       # the swapped-out entry's block was not emptied
    got["dir_ptr"][3] = 77                              # a wrong pointer
    i = int(np.nonzero(np.all(pos == (1, 0, 0), axis=1))[0][0])
    got["dir_slot"][i] = 5                              # a cell left behind where no entry is
    cg["mirror_blocks"] = 7
    msgs = A.compare(slots, pos, want, got, cw, cg)
    assert len(msgs) == 4
    assert "entry 3 (ptr >= 0) at block (255, 0, 0): dirPtr: expected 1, found 77" in msgs
    assert "no entry (a neighbour of one) at block (1, 0, 0): dirSlot: expected -1, found 5" in msgs
    assert "entry 8 (swapped out) at block (0, 16, 0): sdf mirror: 1 of 512 values differ, first at voxel 100: expected -32768, found 32767" in msgs
    assert "census: sdf mirror: 6 entries with ptr >= 0 have a cell there, the cube holds 7 non-empty ones" in msgs


def test_page_table_rules():
    geo = A.geometry(INFO, capi.VOXEL_S)
    wanted = np.array([0, 1, 15, 256])
    assert A.page_table_failures(page_table(), 4, geo, wanted, True) == []
    t = page_table(); t[16] = -3                         # a page that holds no resident block (its only entry is swapped out)
    assert A.page_table_failures(t, 5, geo, wanted, False) == [], "allowed between unfills in a scene that swaps"
    assert any("entry 16 is -3 but no entry" in m for m in A.page_table_failures(t, 5, geo, wanted, True))
    t = page_table(); t[15] = -1
    m = A.page_table_failures(t, 4, geo, wanted, False)
    assert any("entry 15 is -1 but the page holds" in x for x in m) and any("2 entries >= 0, mirror_pages_mapped is 3" in x for x in m)
    t = page_table(); t[15] = 1
    assert any("page 1 of the pool is mapped by entries [0, 15]" in x for x in A.page_table_failures(t, 4, geo, wanted, False))
    t = page_table(); t[7] = -2
    assert any("entry 7 is -2" in x for x in A.page_table_failures(t, 4, geo, wanted, False))
    t = page_table(); t[15] = 3
    assert any("entry 15 is 3, mirror_pages_mapped is 3" in x for x in A.page_table_failures(t, 4, geo, wanted, False))
    assert any("counter is 2" in x for x in A.page_table_failures(page_table(), 2, geo, wanted, False))
    assert any("mirror_pages_mapped 3 > mirror_pages 2" in x for x in A.page_table_failures(page_table(), 4, dict(geo, pages=2), wanted, False))
    dense = A.geometry(dict(INFO, mirror_bytes=32 ** 3 * 1024, mirror_pages=0, mirror_pages_mapped=0), capi.VOXEL_S)
    assert A.page_table_failures(np.full(4096, -1), 0, dense, np.zeros(0, np.int64), True) == []
    assert A.page_table_failures(page_table(), 0, dense, np.zeros(0, np.int64), True) != []


def test_float_mirror_values_are_the_bits():
    vox = np.zeros(512, capi.VOXEL_DTYPES[capi.VOXEL_F])
    vox["sdf"] = np.float32(-0.25)
    assert A.raw_sdf(vox).dtype == np.uint32 and int(A.raw_sdf(vox)[0]) == 0xBE800000
