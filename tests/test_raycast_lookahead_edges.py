"""The empty-space look-ahead of the hash ray cast at its boundaries, HIP against the oracle bit for bit.

The scenes are PREPARED, not fused: a table and a voxel pool built here and uploaded into both backends (the upload path of
tests/prepared_state_cases.py and tests/test_accel_origin.py), so that the length of the runs of "no block" steps is chosen.  Camera
at block C looking along +z; a NEAR slab of allocated blocks at z = C + 10 whose voxels all hold the initial value (found, sdf 1: the
ray walks through it in steps of mu / voxelSize voxels and every step resets its count of misses), then GAP block layers without any
block, then a FAR slab one block thick that holds a plane (sdf falling from +0.875 to -0.875 across the block).  A step without a
block is 8 voxels along the unit direction: the ray through the image centre moves 8 * dz ~ 8 voxels in z per step and takes GAP
(at most GAP + 1) of them between the slabs, rays towards the image corners (dz down to 0.84) up to a fifth more -- every case
therefore covers the run lengths GAP .. GAP + 3 at least.  With a streak of 2 before the wave-wide probe of 10 cells, parking at 12
misses and 12 cells per parked round, the probe ends at run length 12 and the first two parked rounds at 24 and 36: the gaps
9 .. 13 and 21 .. 25 end just before, at and just after those boundaries.

What is compared (tests/itm_testlib.py compare_results): the in-frame ray cast of CreateICPMaps (the kernel with the parked phase), its
points and normals, the range image, and a free-view FindSurface of the same pose.  The reference tree is not read."""

import numpy as np
import pytest

import itm_testlib as T
import mesh_dense_cases as MD
from infinitam_amd import capi, synth

F = np.float32
W, H, VOXEL, MU = 64, 48, 0.005, 0.02
NEAR, POOL = 10, 0x800
GAPS = (9, 10, 11, 12, 13, 21, 22, 23, 24, 25)
SHORT = (capi.VOXEL_S, capi.VOXEL_S_RGB)


def slab(C, depth, margin=1):
    """Block positions of the layer `depth` blocks in front of the camera block C that the 64 x 48 frustum can touch (its half
    angles: 32 / 58 and 24 / 58), plus a margin."""
    hx, hy = int(np.ceil((depth + 1) * 32 / 58)) + margin, int(np.ceil((depth + 1) * 24 / 58)) + margin
    y, x = np.meshgrid(np.arange(-hy, hy + 1), np.arange(-hx, hx + 1), indexing="ij")
    return np.stack([C[0] + x.reshape(-1), C[1] + y.reshape(-1), np.full(x.size, C[2] + depth)], -1)


def plane_block(voxelType):
    """512 voxels of a block crossed by the plane z = 3.5 (block-local), truncation band 4 voxels"""
    z = np.repeat(np.arange(8), 64)
    f = np.clip((3.5 - z) / 4.0, -1.0, 1.0)
    v = np.zeros(512, capi.VOXEL_DTYPES[voxelType])
    v["sdf"] = np.rint(f * 32767).astype(np.int16) if voxelType in SHORT else f.astype(F)
    v["w_depth"] = 1
    if "clr" in v.dtype.names:
        v["clr"] = np.stack([(z * 31) & 255, (np.arange(512) * 7) & 255, np.full(512, 90)], -1).astype(np.uint8)
        v["w_color"] = 1
    return v


def prepared(voxelType, C, gap, half_far=False, anchor=None):
    """(table, voxel pool, block positions): near slab, `gap` empty layers, far slab (half_far: only the blocks with x < C.x, so that
    rays beside its edge run on through empty space until their range ends); anchor: one more block, voxels at the initial value"""
    C = np.asarray(C, np.int64)
    near, far = slab(C, NEAR), slab(C, NEAR + gap + 1)
    if half_far:
        far = far[far[:, 0] < C[0]]
    pos = np.concatenate([near, far] + ([np.asarray(anchor, np.int64)[None, :]] if anchor is not None else []))
    assert len(pos) <= POOL and np.abs(pos).max() < 32000
    table, _ = MD.build_table(pos)
    pool = MD.default_voxels(POOL * 512, voxelType)
    pool[len(near) * 512:(len(near) + len(far)) * 512] = np.tile(plane_block(voxelType), len(far))
    return table, pool, pos


def scenario(voxelType, C):
    # the camera stands at the low corner of block C plus (2.3, 1.9, 0.7) voxels: metres whose float32 image is what both engines get
    t = tuple(F((8 * c + o) * VOXEL) for c, o in zip(C, (2.3, 1.9, 0.7)))
    return T.Scenario(name="lookahead_edges", w=W, h=H, voxelType=voxelType, voxelSize=VOXEL, mu=MU, frames=1, localBlockNum=POOL,
                      colour=voxelType in (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB), origin=t)


def cast(be, sc, table, pool):
    """Upload, then FindVisibleBlocks / CreateExpectedDepths / CreateICPMaps from the scenario's pose: (snapshot, free-view result,
    accel_info or None)."""
    ses = T.Session(be, sc)
    try:
        s, rs = ses.scene, ses.rs
        s.upload(capi.BUF_HASH_ENTRIES, table)
        s.upload(capi.BUF_VOXEL_BLOCKS, pool)
        M = synth.pose_matrix(sc.origin)
        v = capi.View(be.to_backend(np.zeros((H, W), F)), W, H, M_d=M, intr_d=sc.intr(), rgb=ses.rgb, w_rgb=W, h_rgb=H, intr_rgb=sc.intr())
        s.vis.FindVisibleBlocks(M, sc.intr(), rs)
        s.vis.CreateExpectedDepths(M, sc.intr(), rs)
        s.vis.FindSurface(M, sc.intr(), rs)
        free = s.download(capi.BUF_RAYCAST_RESULT, rs).copy()
        s.vis.CreateICPMaps(v, rs, ses.points, ses.normals)
        snap = ses.snapshot(with_voxels=False)
        info = s.accel_info() if be.fn.get("scene_accel_info") else None
        return snap, free, info
    finally:
        ses.close()


_oracle = {}


def oracle_cast(oracle, key, sc, table, pool):
    """one oracle run per scene, shared by the mirror forms and never modified"""
    if key not in _oracle:
        _oracle[key] = cast(oracle, sc, table, pool)[:2]
    return _oracle[key]


def check(hip, oracle, key, sc, table, pool, gap, min_hits):
    want, want_free = oracle_cast(oracle, key, sc, table, pool)
    got, got_free, info = cast(hip, sc, table, pool)
    T.compare_results(got, want, sc, what="%s gap %d" % (key[0], gap))
    assert np.array_equal(got_free, want_free), "free-view ray cast"
    hit = want.raycast[..., 3] > 0
    assert hit.sum() >= min_hits, hit.sum()
    # the hits lie on the far slab's plane: the rays did cross the gap
    zs = want.raycast[hit][:, 2]
    z_plane = 8 * (key[2][2] + NEAR + gap + 1) + 3.5
    assert np.abs(zs - z_plane).max() < 1.0, (zs.min(), zs.max(), z_plane)
    return info


ORIGINS = {"origin": (0, 0, 0), "negative": (-37, 21, -15)}      # "negative": blocks with x < 0, y around 21, and z crossing 0 inside the gap


@pytest.mark.gpu
@pytest.mark.parametrize("where", list(ORIGINS))
@pytest.mark.parametrize("gap", GAPS)
def test_runs_that_end_around_a_look_ahead_boundary(hip, oracle, gap, where):
    C = ORIGINS[where]
    if where == "negative":
        assert C[2] + NEAR < 0 < C[2] + NEAR + gap + 1
    sc = scenario(capi.VOXEL_S, C)
    table, pool, _ = prepared(capi.VOXEL_S, C, gap)
    info = check(hip, oracle, ("s", gap, C), sc, table, pool, gap, min_hits=W * H * 9 // 10)
    assert info["placed"] and info["directory_bytes"] > 0 and info["mirror_bytes"] > 0 and info["mirror_pages"] == 0      # the dense mirror


@pytest.mark.gpu
@pytest.mark.parametrize("gap", (10, 12, 23, 24))
def test_the_same_runs_with_the_paged_mirror(hip, oracle, gap, monkeypatch):
    """ITM_MIRROR is read when a scene is created (tests/test_paged_mirror.py sets it the same way)."""
    monkeypatch.setenv("ITM_MIRROR", "paged")
    C = ORIGINS["negative"]
    sc = scenario(capi.VOXEL_S, C)
    table, pool, _ = prepared(capi.VOXEL_S, C, gap)
    info = check(hip, oracle, ("s", gap, C), sc, table, pool, gap, min_hits=W * H * 9 // 10)
    assert info["mirror_pages"] > 0 and info["mirror_pages_mapped"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("gap", (11, 24))
def test_float_colour_voxels_have_the_directory_only(hip, oracle, gap):
    C = ORIGINS["negative"]
    sc = scenario(capi.VOXEL_F_RGB, C)
    table, pool, _ = prepared(capi.VOXEL_F_RGB, C, gap)
    info = check(hip, oracle, ("f_rgb", gap, C), sc, table, pool, gap, min_hits=W * H * 9 // 10)
    assert info["directory_bytes"] > 0 and info["mirror_bytes"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("gap", (14, 17, 30))
def test_a_range_that_ends_inside_a_look_ahead(hip, oracle, gap):
    """Half a far slab: the range image of the tiles along its edge reaches to the far slab's back, and the rays of those tiles that
    pass beside the edge find no block until total >= totalMax -- after about gap + 2 steps without a block, i.e. inside the probe's
    cells (14), inside the first parked round (17) and inside the second (30)."""
    C = ORIGINS["origin"]
    sc = scenario(capi.VOXEL_S, C)
    table, pool, _ = prepared(capi.VOXEL_S, C, gap, half_far=True)
    want, _ = oracle_cast(oracle, ("s_half", gap, C), sc, table, pool)
    check(hip, oracle, ("s_half", gap, C), sc, table, pool, gap, min_hits=W * H // 3)
    # columns right of the centre saw the near slab (their tiles have a range) and hit nothing
    right = want.raycast[:, W // 2 + 2:, 3]
    assert (right == 0).all()
    rng = T.range_region(want.range_image, W, H)
    assert (rng[:, :, 1] > rng[:, :, 0]).all(), "every tile has a range: rays without a hit marched until it ended"


@pytest.mark.gpu
@pytest.mark.parametrize("face", ["leaving", "entering"])
@pytest.mark.parametrize("gap", (12, 23))
def test_look_ahead_cells_outside_the_directory_cube(hip, oracle, gap, face):
    """After an upload the directory cube (512 blocks per side) is centred on the bounding box of the table's blocks, rounded to 4
    (scene.hip, accel_place_for_table; tests/test_accel_origin.py reaches the cube's edges by walking, this test by one far ANCHOR
    block behind or far in front of the camera that shifts the box): the cube's last (leaving) or first (entering) covered layer is put
    in the middle of the gap.  The rays' look-ahead rounds then hold cells on both sides of the face: the address of a cell outside is
    the cell's image modulo the cube -- always readable -- and its value is ignored; beyond the face every read walks the table."""
    C = np.array(ORIGINS["origin"], np.int64)
    n0, far = C[2] + NEAR, C[2] + NEAR + gap + 1
    if face == "leaving":                         # first layer NOT covered: c + 256, with c the centre of [anchor, far], a multiple of 4
        c = (n0 + 1 + gap // 2 - 256) // 4 * 4
        anchor_z = 2 * c - far
        first_out = c + 256
        assert n0 + 1 < first_out <= far - 2
    else:                                         # first layer covered: c - 256, the centre of [near, anchor]
        c = -((-(n0 + 1 + gap // 2 + 256)) // 4 * 4)
        anchor_z = 2 * c - n0
        first_in = c - 256
        assert n0 + 2 <= first_in < far
    anchor = (int(C[0]), int(C[1]), int(anchor_z))
    sc = scenario(capi.VOXEL_S, tuple(C))
    table, pool, _ = prepared(capi.VOXEL_S, tuple(C), gap, anchor=anchor)
    info = check(hip, oracle, ("s_" + face, gap, tuple(C)), sc, table, pool, gap, min_hits=W * H * 9 // 10)
    oz = info["origin_directory"][2]
    if face == "leaving":
        assert oz + 512 == first_out, (info, first_out)
    else:
        assert oz == first_in, (info, first_in)
