"""Half-swapped scenes in everything that reads or persists a scene.

Host swapping leaves a hash scene in a state nothing else produces: table entries with ptr == -1 that have no directory or mirror cell,
scattered among resident blocks (swap-out takes the first N entries in TABLE order), their voxels in the host cache alone.
tests/test_swapping.py follows that state through allocation, integration and the camera's own ray cast; here every other reader meets
it (part A), the fused frame paths run on it (part B), it is checkpointed and resumed (part C) and reset and filled again (part D).
The scene is swapped_cases' "half-swapped scene"; every test states from its inputs that the scene is what it is for (anchors())."""
import os
import shutil

import numpy as np
import pytest

import esdf_cases as EC
import esdf_terms as ET
import itm_testlib as T
import mesh_attr_terms as MT
import pose_quality_terms as PQT
import ren_cases as RC
import scene_query_terms as QT
import swapped_cases as SC
import test_distance_field as DF
import test_mesh_attributes as MA
import test_pose_quality as PQ
import test_scene_query as SQ
import test_tracker_terms as TTT
import tracker_terms as TT
from infinitam_amd import capi
from infinitam_amd.capi import Mesh
from test_engine_api import compare as api_compare

VOXELS = [(capi.VOXEL_S, False), (capi.VOXEL_F_RGB, True)]
VOXEL_IDS = ["s", "f_rgb"]


def swap_reference(ref):
    """The `ref` fixture with the reference build of swapped_cases' pool and transfer sizes (the reference's are compile-time constants)."""
    return T.ReferenceCheck(ref.records, ref.test_id, T.reference_swap_backend())


def hits_from(run, pose_k=0):
    """Pixels FindSurface hits from the pose of frame `pose_k`, on a render state of its own."""
    s = run.scene
    rs = s.vis.CreateRenderState((SC.W, SC.H))
    M, _ = run.seq[pose_k]
    s.vis.FindVisibleBlocks(M, run.intr, rs)
    s.vis.CreateExpectedDepths(M, run.intr, rs)
    s.vis.FindSurface(M, run.intr, rs)
    n = int(np.count_nonzero(s.download(capi.BUF_RAYCAST_RESULT, rs)[..., 3] > 0))
    rs.close()
    return n


_unswapped_hits = {}


def unswapped_hits(be, voxel, colour):
    """Ray hits from pose 0 on the same scene before anything is swapped (three frames), once per backend and voxel type."""
    key = (be.prefix, voxel)
    if key not in _unswapped_hits:
        run = SC.build(be, 0, voxel, colour)
        _unswapped_hits[key] = hits_from(run)
        run.close()
    return _unswapped_hits[key]


def anchors(run, voxel, colour):
    """The conditions the half-swapped scene is built for, from the inputs of the call under test."""
    swapped, beside = SC.neighbour_census(run.scene.download(capi.BUF_HASH_ENTRIES))
    assert swapped > 400, swapped
    assert beside > 300, beside
    hits, before = hits_from(run), unswapped_hits(run.be, voxel, colour)
    assert 20000 < hits < before, (hits, before)
    return swapped, beside, hits


# ---- the fixture itself (CPU) ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_the_half_swapped_scene_is_what_it_is_for(oracle, voxel, colour):
    run = SC.build(oracle, 1, voxel, colour)
    swapped, beside, hits = anchors(run, voxel, colour)
    assert swapped == SC.TRANSFER                     # one swap-out call's worth
    flags = run.scene.global_cache_flags()
    table = run.scene.download(capi.BUF_HASH_ENTRIES)
    assert np.all(flags[table["ptr"] == -1] == 1), "a swapped-out entry without a cached block"
    run.close()


# ---- A1. the free-view family ---------------------------------------------------------------------------------------------------------

def find_surface(run):
    """FindSurface from pose 0 on a second render state: the result with the misses' coordinates zeroed (they are not defined)"""
    s = run.scene
    rs = s.vis.CreateRenderState((SC.W, SC.H))
    M, _ = run.seq[0]
    s.vis.FindVisibleBlocks(M, run.intr, rs)
    s.vis.CreateExpectedDepths(M, run.intr, rs)
    s.vis.FindSurface(M, run.intr, rs)
    ray = s.download(capi.BUF_RAYCAST_RESULT, rs)
    ray[ray[..., 3] <= 0, :3] = 0
    rs.close()
    return ray


def free_view(run):
    """Every free-view entry point on a second render state of the half-swapped scene, as test_engine_api.api_sequence calls them."""
    be, s = run.be, run.scene
    W, H, P = SC.W, SC.H, SC.W * SC.H
    out = {}
    rs = s.vis.CreateRenderState((W, H))
    M, intr = run.seq[0][0], run.intr
    s.vis.FindVisibleBlocks(M, intr, rs)
    c = s.counters(rs)
    out["visible_count"] = c["noVisibleEntries"]
    out["visible_ids"] = s.download(capi.BUF_VISIBLE_IDS, rs)[: c["noVisibleEntries"]]
    s.vis.CreateExpectedDepths(M, intr, rs)
    out["range"] = T.range_region(s.download(capi.BUF_RANGE_IMAGE, rs), W, H)
    s.vis.FindSurface(M, intr, rs)
    ray = s.download(capi.BUF_RAYCAST_RESULT, rs)
    out["find_surface_w"] = ray[..., 3].copy()
    ray[ray[..., 3] <= 0, :3] = 0
    out["find_surface"] = ray
    img = capi.DevBuffer(be, P * 4, np.uint8, (H, W, 4))
    for name, typ in (("grey", capi.RENDER_SHADED_GREYSCALE), ("volume", capi.RENDER_COLOUR_FROM_VOLUME), ("normal", capi.RENDER_COLOUR_FROM_NORMAL)):
        be.check(be.fn["memcpy_h2d"](img.ptr, np.full((H, W, 4), 7, np.uint8).ctypes.data, P * 4, None), "h2d")
        be.sync()
        s.vis.RenderImage(M, intr, rs, img, typ)
        out["render_" + name] = img.numpy()
    # ForwardRender into the second pose, from the ray cast of the first
    s.vis.FindSurface(M, intr, rs)
    v1 = run.view(1)
    s.vis.CreateExpectedDepths(v1.M_d, v1.intr_d, rs)
    s.vis.ForwardRender(v1, rs)
    c = s.counters(rs)
    out["fwd_missing_count"] = c["noFwdProjMissingPoints"]
    out["fwd_missing"] = s.download(capi.BUF_MISSING_POINTS, rs)[: c["noFwdProjMissingPoints"]]
    out["fwd_projection"] = s.download(capi.BUF_FORWARD_PROJECTION, rs)
    # the colour tracker's point cloud
    v0 = run.view(0)
    loc, col = capi.DevBuffer(be, P * 16, np.float32, (P, 4)), capi.DevBuffer(be, P * 16, np.float32, (P, 4))
    for skip in (False, True):
        s.vis.CreateExpectedDepths(v0.M_d, v0.intr_d, rs)
        s.vis.CreatePointCloud(v0, rs, loc, col, skipPoints=skip)
        n = s.counters(rs)["noTotalPoints"]
        out[f"pc_count_{int(skip)}"] = n
        out[f"pc_locations_{int(skip)}"] = loc.numpy()[:n]
        out[f"pc_colours_{int(skip)}"] = col.numpy()[:n]
        out[f"pc_image_{int(skip)}"] = s.download(capi.BUF_RAYCAST_IMAGE, rs)
    for b in (img, loc, col):
        b.close()
    rs.close()
    return out


def check_free_view_is_what_it_is_for(out):
    hit = out["find_surface_w"] > 0
    assert np.count_nonzero(hit) > 20000 and out["fwd_missing_count"] > 0 and out["pc_count_0"] > out["pc_count_1"] > 1000
    assert out["visible_count"] > 300


_oracle_free_view = {}


def oracle_free_view(voxel, colour):
    """The oracle's free-view outputs and ray cast of the half-swapped scene, computed once and left unchanged"""
    if voxel not in _oracle_free_view:
        run = SC.build(T.oracle_backend(), 1, voxel, colour)
        _oracle_free_view[voxel] = (free_view(run), find_surface(run))
        run.close()
    return _oracle_free_view[voxel]


@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_oracle_free_view_of_the_half_swapped_scene_equals_the_reference_engine(oracle, ref, voxel, colour):
    ref = swap_reference(ref)
    a, _ = oracle_free_view(voxel, colour)
    check_free_view_is_what_it_is_for(a)
    if ref.backend is not None:
        run = SC.build(ref.backend, 1, voxel, colour)
        anchors(run, voxel, colour)
        api_compare(a, free_view(run), "oracle vs reference")
        run.close()
    ref.check("free_view", a)


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_hip_free_view_of_the_half_swapped_scene_equals_the_oracle(hip, voxel, colour):
    run = SC.build(hip, 1, voxel, colour)
    anchors(run, voxel, colour)
    want, _ = oracle_free_view(voxel, colour)
    check_free_view_is_what_it_is_for(want)
    api_compare(free_view(run), want, "hip vs oracle")
    run.close()


SINGLE_PASS_RAYCAST = 8            # include/itm_debug.h (test_hip_parity.test_single_pass_ray_cast_path)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "paged_few", "mirror_off", "no_cubes", "single_pass"])
@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_hip_find_surface_of_the_half_swapped_scene_in_every_mirror_form(hip, voxel, colour, form):
    """The ray cast through the mirror in its default form, paged with 5 pages, without a mirror, without the acceleration cubes
    (the table walk), and in one pass."""
    env = {"no_cubes": {"ITM_NO_ACCELERATION_CUBES": "1"}, "single_pass": {}}[form] if form in ("no_cubes", "single_pass") else SQ.FORMS[form]
    if form == "single_pass":
        hip.check(hip.fn["debug_set"](SINGLE_PASS_RAYCAST, 1), "debug_set")
    try:
        with SQ.environment(env):
            run = SC.build(hip, 1, voxel, colour)
        info = run.scene.accel_info()
        if form == "no_cubes":
            assert info["directory_bytes"] == 0 and info["mirror_bytes"] == 0, info
        elif form == "mirror_off" or voxel != capi.VOXEL_S:          # (the float voxel types get no mirror: their ray cast reads the pool)
            assert info["mirror_bytes"] == 0 and info["directory_bytes"] > 0, info
        elif form == "paged_few":
            assert info["mirror_pages"] == 5, info
        else:
            assert info["mirror_bytes"] > 0, info
        got = find_surface(run)
    finally:
        if form == "single_pass":
            hip.check(hip.fn["debug_set"](SINGLE_PASS_RAYCAST, 0), "debug_set")
    swapped, beside = SC.neighbour_census(run.scene.download(capi.BUF_HASH_ENTRIES))
    assert swapped > 400 and beside > 300
    _, want = oracle_free_view(voxel, colour)
    hits = int(np.count_nonzero(want[..., 3] > 0))
    assert 20000 < hits < unswapped_hits(T.oracle_backend(), voxel, colour)
    assert np.array_equal(got[..., 3], want[..., 3]), "%s: hit mask differs at %d pixels" % (form, np.count_nonzero(got[..., 3] != want[..., 3]))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), form
    run.close()


# ---- A2 / A3. hash meshing and the mesh's attributes ------------------------------------------------------------------------------------

def mesh_of(run, max_triangles=0):
    m = Mesh(run.scene, max_triangles)
    m.MeshScene()
    return m, m.triangles(), m.info()


_oracle_mesh = {}


def oracle_mesh(voxel, colour):
    """(table, voxels, triangles, info, the first 999 triangles of a full buffer and its info) of the oracle's half-swapped scene"""
    if voxel not in _oracle_mesh:
        run = SC.build(T.oracle_backend(), 1, voxel, colour)
        m, tri, info = mesh_of(run)
        mf, trif, infof = mesh_of(run, 1000)
        _oracle_mesh[voxel] = dict(table=run.scene.download(capi.BUF_HASH_ENTRIES), voxels=run.scene.download(capi.BUF_VOXEL_BLOCKS), tri=tri, info=info,
                                   full_tri=trif, full_info=infof)
        m.close(); mf.close(); run.close()
    return _oracle_mesh[voxel]


_restated = {}


def restated_attributes(voxel, colour):
    """mesh_attr_terms on the oracle's half-swapped scene and mesh: (triangles, gradients, normals, colour floats | None)"""
    if voxel not in _restated:
        o = oracle_mesh(voxel, colour)
        reader = MT.MeshVoxelReader(o["voxels"], o["table"])           # (blocks with ptr >= 0: a swapped-out block reads as absent)
        _restated[voxel] = (o["tri"],) + MT.attributes(reader, o["tri"], SC.VOXEL_SIZE, colours=colour)
    return _restated[voxel]


@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_oracle_mesh_of_the_half_swapped_scene_equals_the_reference_engine(oracle, ref, voxel, colour):
    ref = swap_reference(ref)
    o = oracle_mesh(voxel, colour)
    assert o["info"][0] > 50000 and o["full_info"] == (999, 1000) and np.array_equal(o["full_tri"], o["tri"][:999])
    if ref.backend is not None:
        run = SC.build(ref.backend, 1, voxel, colour)
        anchors(run, voxel, colour)
        m, tri, info = mesh_of(run)                      # (the reference's buffer size is a compile-time constant: no full-buffer run)
        assert info == o["info"] and np.array_equal(tri.view(np.uint32), o["tri"].view(np.uint32)), "oracle vs reference"
        m.close()
        run.close()
    ref.check("mesh", (o["info"], o["tri"], o["full_info"], o["full_tri"]))


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_hip_mesh_and_attributes_of_the_half_swapped_scene(hip, voxel, colour):
    """2, 3: MeshScene == the oracle's (also into a full buffer), MeshVolume == MeshScene as on every hash scene, normals and colours
    == mesh_attr_terms on both vertex paths."""
    run = SC.build(hip, 1, voxel, colour)
    anchors(run, voxel, colour)
    o = oracle_mesh(voxel, colour)
    assert o["info"][0] > 50000
    m, tri, info = mesh_of(run)
    assert info == o["info"] and np.array_equal(tri.view(np.uint32), o["tri"].view(np.uint32)), "MeshScene"
    mf, trif, infof = mesh_of(run, 1000)
    assert infof == o["full_info"] == (999, 1000) and np.array_equal(trif.view(np.uint32), o["full_tri"].view(np.uint32)), "MeshScene, full buffer"
    # MeshVolume of a hash scene is MeshScene (test_mesh_dense.test_hip_unchanged_behaviour_and_staleness), attributes included
    mv = Mesh(run.scene)
    mv.MeshVolume()
    assert mv.info() == info and np.array_equal(mv.triangles().view(np.uint32), tri.view(np.uint32)), "MeshVolume"
    what = capi.MESH_NORMALS | (capi.MESH_COLOURS if colour else 0)
    want = restated_attributes(voxel, colour)
    m.ComputeAttributes(what); mv.ComputeAttributes(capi.MESH_NORMALS)
    normals = m.normals()
    assert np.array_equal(mv.normals().view(np.uint32), normals.view(np.uint32))
    MA.assert_equals_restatement("half-swapped", tri, normals, m.colours() if colour else None, restatement=want)
    hip.check(hip.fn["debug_set"](MA.DEBUG_MESH_ATTR_PER_VERTEX, 1), "debug_set")
    try:
        m.MeshScene()
        m.ComputeAttributes(what)
        MA.assert_equals_restatement("half-swapped, per vertex", m.triangles(), m.normals(), m.colours() if colour else None, restatement=want)
    finally:
        hip.check(hip.fn["debug_set"](MA.DEBUG_MESH_ATTR_PER_VERTEX, 0), "debug_set")
    for x in (m, mf, mv):
        x.close()
    run.close()


# ---- A4 - A6. queries, distance field, pose quality, Ren energy -----------------------------------------------------------------------

class HalfSwapped:
    """What the query, distance-field and pose-quality tests read from their `Built` objects, around the half-swapped scene: the helpers
    of those modules run on it unchanged."""

    def __init__(self, be, voxel, colour):
        self.be = be
        self.run = SC.build(be, 1, voxel, colour)
        self.scene = self.run.scene
        self.sc = T.Scenario(name="half_swapped", w=SC.W, h=SC.H, voxelSize=SC.VOXEL_SIZE, voxelType=voxel, colour=colour)   # its parameters
        assert tuple(self.sc.intr()) == tuple(self.run.intr) and np.array_equal(self.sc.pose(0), self.run.seq[0][0])
        assert (np.float32(self.sc.mu), np.float32(self.sc.voxelSize)) == (np.float32(self.scene.params.mu), np.float32(self.scene.params.voxelSize))
        self.table = self.scene.download(capi.BUF_HASH_ENTRIES)
        self.reader = PQT.reader_of(self.scene)                     # blocks with ptr >= 0: a swapped-out block reads as absent
        self.mesh = Mesh(self.scene)
        self.mesh.MeshScene()
        self.vertices = self.mesh.triangles().reshape(-1, 3)
        self.depth = self.run.seq[0][1]
        self.depth_dev = self.run.view(0).depth
        self.handle = capi.PoseQuality(be) if "pose_quality_create" in be.fn else None

    bounds = SQ.Built.bounds
    blocks = SQ.Built.blocks

    def swapped_blocks(self):
        return self.table["pos"][self.table["ptr"] == -1].astype(np.int64)

    def view(self, pose, depth_dev=None, w=None, h=None):
        return capi.View(depth_dev or self.depth_dev, w or SC.W, h or SC.H, M_d=pose, intr_d=self.run.intr)

    def boxes(self):
        """{name: (origin, size)} for test_distance_field.check_scene: the box of esdf_cases on the fused surface (40 x 33 x 17, origin
        not block-aligned) placed on the swapped-out block nearest to the sphere's front, and a smaller one astride the first resident
        block that has a swapped-out positive neighbour"""
        out = self.swapped_blocks()
        near = out[np.argmin(((out * 8 + 4 - np.array([0, 0, 100])) ** 2).sum(1))]
        resident = {tuple(p) for p in self.blocks()}
        gone = {tuple(p) for p in out}
        first = min(p for p in resident if any((p[0] + dx, p[1] + dy, p[2] + dz) in gone for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)))
        return {"surface": (tuple(int(a) for a in near * 8 - (13, 11, 5)), (40, 33, 17)),
                "astride": (tuple(int(a) for a in np.array(first) * 8 + (3, 2, 1)), (21, 14, 13))}

    def restated(self, box, sites, min_weight, R):
        return ET.esdf(self.reader, box, EC.SITE_MASKS[sites], min_weight, R, self.sc.voxelSize)

    def close(self):
        if self.handle is not None:
            self.handle.close()
        self.mesh.close()
        self.run.close()


def block_keys(pos):
    pos = np.asarray(pos, np.int64)
    return ((pos[..., 0] + 32768) << 32) | ((pos[..., 1] + 32768) << 16) | (pos[..., 2] + 32768)


def straddling(b, p):
    """Of the positions p (voxels): those whose 8 trilinear corners lie in a resident block AND in a swapped-out block."""
    with np.errstate(all="ignore"):
        ok = np.all(np.abs(p) < 30000, axis=1)
    base = np.floor(np.where(ok[:, None], p, 0)).astype(np.int64)
    corners = np.stack([(base + d) >> 3 for d in np.ndindex(2, 2, 2)], 1)           # [n, 8, 3] block positions
    keys = block_keys(corners)
    resident, gone = np.isin(keys, block_keys(b.blocks())), np.isin(keys, block_keys(b.swapped_blocks()))
    return ok & resident.any(1) & gone.any(1)


def boxes_hold_swapped_blocks(b):
    """from the table and the restatement alone"""
    gone = b.swapped_blocks()
    for name, (origin, size) in b.boxes().items():
        lo, hi = np.array(origin), np.array(origin) + np.array(size)
        inside = np.all((gone * 8 + 8 > lo) & (gone * 8 < hi), axis=1)
        res = b.blocks()
        assert inside.any() and np.all((res * 8 + 8 > lo) & (res * 8 < hi), axis=1).any(), name
        # a voxel of a swapped-out block is unobserved: not STORED, and a site of the unobserved-site mask
        blk = gone[np.nonzero(inside)[0][0]]
        v = np.clip(blk * 8 + 4, lo, hi - 1) - lo
        for R in (0, EC.R_NEAR):
            st = b.restated((origin, size), "unknown", 1, R)["state"]
            cell = st[v[2], v[1], v[0]]
            assert (cell & ET.STORED) == 0 and (cell & ET.OBSERVED) == 0, (name, cell)
    got = b.restated(b.boxes()["surface"], "surface", 1, EC.R_NEAR)
    assert np.count_nonzero(got["state"] & ET.SITE) > 50, "the first box lies on the surface"


@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_the_point_set_and_the_boxes_meet_swapped_out_blocks(oracle, voxel, colour):
    """On the CPU: the inputs of tests 4 and 5 are what they are for."""
    b = HalfSwapped(oracle, voxel, colour)
    v, p = SQ.point_sets(b)
    n = int(np.count_nonzero(straddling(b, p))) + int(np.count_nonzero(straddling(b, QT.positions(v, "metres", SC.VOXEL_SIZE))))
    print("points whose trilinear corners straddle a resident and a swapped-out block:", n)
    assert n >= 200, n
    boxes_hold_swapped_blocks(b)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_hip_queries_and_distance_field_of_the_half_swapped_scene(hip, voxel, colour):
    """4, 5: test_scene_query's check_points / check_rays and test_distance_field's check_scene."""
    b = HalfSwapped(hip, voxel, colour)
    anchors(b.run, voxel, colour)
    v, p = SQ.check_points(b, SQ.wants(b.sc), "half-swapped")
    n = int(np.count_nonzero(straddling(b, p))) + int(np.count_nonzero(straddling(b, QT.positions(v, "metres", SC.VOXEL_SIZE))))
    print("points whose trilinear corners straddle a resident and a swapped-out block:", n)
    assert n >= 200, n
    SQ.check_rays(b, "half-swapped")
    boxes_hold_swapped_blocks(b)
    DF.check_scene(b, "half-swapped")
    b.close()


def perturbed(pose):
    """4 cm along x and -1.5 cm along y: the pixels read other voxels, many across a block face"""
    return PQT.shifted(pose, tx=0.04, ty=-0.015)


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_hip_pose_quality_and_ren_energy_of_the_half_swapped_scene(hip, voxel, colour):
    """6: test_pose_quality's check_against_restatement and test_tracker_terms' Ren comparison (their bounds), at pose 0 and at one
    perturbed pose."""
    b = HalfSwapped(hip, voxel, colour)
    anchors(b.run, voxel, colour)
    pose0 = b.run.seq[0][0]
    seen = [PQ.check_against_restatement(b, b.depth, pose, "half-swapped, " + name, b.depth_dev) for name, pose in (("pose 0", pose0), ("perturbed", perturbed(pose0)))]
    # what the swapped-out blocks cost: fewer known pixels than valid ones, but thousands of each
    assert 5000 < seen[0]["noKnown"] < seen[0]["noValid"] and seen[1]["noKnown"] > 5000, seen
    reader = TT.VoxelReader(b.scene.download(capi.BUF_VOXEL_BLOCKS), entries=b.table)
    trk = TTT.Ren(hip)
    try:
        cache = {}
        poses = {"pose 0": RC.inv_col(pose0), "perturbed": RC.inv_col(perturbed(pose0))}
        depths = {(SC.W, SC.H): (np.ascontiguousarray(b.depth, np.float32), np.asarray(b.run.intr, np.float32))}
        worst = TTT.ren_compare(hip, trk, b.scene, b.sc, reader, depths, poses, "half-swapped", cache)
        assert all(t.n > 1000 for t in cache.values()), [t.n for t in cache.values()]
        print(f"Ren, half-swapped: worst ratio {worst:.3f}")
    finally:
        trk.close()
    b.close()


# ---- B. frame paths on a swapping scene ----------------------------------------------------------------------------------------------

def lockstep(a, b, frames, order_a, order_b, what, announce=None):
    """Runs two Runs through `frames`, comparing everything (all cached blocks) after every frame."""
    for k in frames:
        a.frame(k, order_a, announce=None if announce is None else announce(k))
        b.frame(k, order_b)
        SC.compare(a.snapshot(), b.snapshot(), "%s, frame %d" % (what, k))


def swapped_and_back(run):
    """The sequence did what it is for: blocks left (more than one transfer's worth at the peak is not required here: the pool is
    small) and came back into resident entries."""
    table = run.scene.download(capi.BUF_HASH_ENTRIES)
    states = run.scene.download(capi.BUF_SWAP_STATES)
    assert int(np.count_nonzero(run.scene.global_cache_flags())) > 900
    assert int(np.count_nonzero((states == 2) & (table["ptr"] >= 0))) > 400


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_fused_frames_with_swap_calls_equal_the_oracle(hip, oracle, voxel, colour):
    """7: process_frame, then the two swap calls, against the oracle's six calls."""
    a, b = SC.Run(hip, voxel, colour), SC.Run(oracle, voxel, colour)
    lockstep(a, b, range(SC.FRAMES), "fused", "calls", "fused frames vs oracle")
    swapped_and_back(a)
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_frames_announced_ahead_on_a_swapping_scene_equal_the_plain_sequence(hip, oracle, voxel, colour):
    """8: on swapping scenes the requests ahead are dropped, so an announced next view changes nothing -- whether it is the view that
    follows (even frames) or another one (odd frames announce the frame after next; the last announces frame 0)."""
    def announce(k):
        return (k + 1 if k % 2 == 0 else k + 2) % SC.FRAMES
    a, b = SC.Run(hip, voxel, colour), SC.Run(oracle, voxel, colour)
    lockstep(a, b, range(SC.FRAMES), "ahead", "calls", "frames announced ahead vs oracle", announce)
    swapped_and_back(a)
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_the_reference_order_with_deferred_fusion_on_equals_the_oracle(hip, oracle, voxel, colour):
    """9: allocate, integrate, swap, swap, expected depths, ICP maps on a scene that accepted deferred fusion: swapping scenes never
    record, so every call has run when it returns."""
    a, b = SC.Run(hip, voxel, colour, deferred=True), SC.Run(oracle, voxel, colour)
    lockstep(a, b, range(SC.FRAMES), "reference", "reference", "deferred fusion on vs oracle")
    swapped_and_back(a)
    a.close(); b.close()


# ---- C. checkpoint of a swapping scene -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_resume_of_a_half_swapped_scene_is_bit_identical(hip, oracle, tmp_path, voxel, colour):
    """10: saved at the half-swapped state, loaded into a fresh swapping scene and render state; the remaining six frames (three away,
    three back, with the swap calls) equal the uninterrupted run and the oracle's, every cached block included.
    (While the checkpoint held neither the swap states nor the host cache, this failed in the first frame resumed, both voxel types:
    lastFreeBlockId 14877 against 15297 -- with every state zero again the 420 scene blocks still resident never left.)"""
    full, orc = SC.build(hip, 1, voxel, colour, order="reference"), SC.build(oracle, 1, voxel, colour, order="reference")
    anchors(full, voxel, colour)
    full.scene.save(str(tmp_path), full.rs)
    assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp") or f.endswith(".new")]
    resumed = SC.Run(hip, voxel, colour)
    resumed.scene.load(str(tmp_path), resumed.rs)
    for k in range(SC.HALF, SC.FRAMES):
        full.frame(k); orc.frame(k)
        resumed.frame(k, count_combined=True)
        x = full.snapshot()
        SC.compare(resumed.snapshot(), x, "resumed vs uninterrupted, frame %d" % k)
        SC.compare(x, orc.snapshot(), "uninterrupted vs oracle, frame %d" % k)
    assert resumed.combined >= 500, resumed.combined
    for r in (full, orc, resumed):
        r.close()


def check_refused_loads_of_a_swapping_scene(hip, tmp_path):
    """12 (called by test_checkpoint.test_rejected_checkpoints_leave_the_scene_untouched): a swapping victim refuses corrupt and
    incomplete checkpoints and then continues exactly as its undisturbed twin, cache included."""
    src = SC.build(hip, 3, order="reference")               # another state than the victim's: a load that went through would show
    good = str(tmp_path / "swap_good"); os.makedirs(good)
    src.scene.save(good, src.rs)
    names = set(os.listdir(good))
    assert {"swap_states.dat", "cache_flags.dat", "cache_blocks.dat"} <= names and not [f for f in names if f.endswith((".tmp", ".new"))]
    flags = np.frombuffer(open(os.path.join(good, "cache_flags.dat"), "rb").read(), np.uint8)
    blocks = os.path.getsize(os.path.join(good, "cache_blocks.dat"))
    stored = int(np.count_nonzero(flags[4:]))
    assert stored > 900 and blocks == 4 + stored * 512 * src.scene.voxel_dtype.itemsize, "the cache is stored compactly"
    victim, twin = SC.build(hip, 1, order="reference"), SC.build(hip, 1, order="reference")
    made = []

    def corrupt(name, fn):
        made.append(name)
        bad = str(tmp_path / ("swap_bad%d_%s" % (len(made), name))); shutil.copytree(good, bad)
        fn(os.path.join(bad, name))
        with pytest.raises(capi.ItmError):
            victim.scene.load(bad, victim.rs)

    corrupt("cache_blocks.dat", lambda p: os.truncate(p, 4 + 100 * 512 * 4 + 17))       # a truncated block file

    def bad_state(p):
        raw = bytearray(open(p, "rb").read()); raw[4 + 12345] = 7
        open(p, "wb").write(bytes(raw))
    corrupt("swap_states.dat", bad_state)

    def one_flag_more(p):
        raw = bytearray(open(p, "rb").read())
        free = int(np.nonzero(np.frombuffer(bytes(raw[4:]), np.uint8) == 0)[0][0])
        raw[4 + free] = 1                                                                   # 0/1 still, but one more than there are blocks
        open(p, "wb").write(bytes(raw))
    corrupt("cache_flags.dat", one_flag_more)

    def not_a_flag(p):
        raw = bytearray(open(p, "rb").read()); raw[4 + int(np.nonzero(flags[4:])[0][0])] = 2
        open(p, "wb").write(bytes(raw))
    corrupt("cache_flags.dat", not_a_flag)
    for name in ("swap_states.dat", "cache_flags.dat", "cache_blocks.dat"):                  # a swapping scene's checkpoint without them
        corrupt(name, os.remove)
    corrupt("voxel.dat", lambda p: os.truncate(p, 100))                                      # and a plain file after the swap files were read

    for r in (victim, twin):
        r.frame(SC.HALF)
    SC.compare(victim.snapshot(), twin.snapshot(), "after refused loads")
    victim.scene.load(good, victim.rs)                                                      # the intact checkpoint still loads, wholesale
    src.frame(6); victim.frame(6)
    SC.compare(victim.snapshot(), src.snapshot(), "after the intact load")
    for r in (src, victim, twin):
        r.close()


@pytest.mark.gpu
def test_a_checkpoint_of_a_plain_scene_is_refused_by_a_swapping_scene_and_back(hip, tmp_path):
    """The configuration in config.dat tells the two apart before any block is read."""
    plain = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=SC.VOXEL_SIZE), localBlockNum=SC.POOL)
    plain.reco.ResetScene()
    d_plain, d_swap = str(tmp_path / "plain"), str(tmp_path / "swap")
    os.makedirs(d_plain); os.makedirs(d_swap)
    plain.save(d_plain)
    assert not [f for f in os.listdir(d_plain) if f.startswith(("swap_", "cache_"))]
    run = SC.Run(hip)
    run.scene.save(d_swap)
    with pytest.raises(capi.ItmError):
        run.scene.load(d_plain)
    with pytest.raises(capi.ItmError):
        plain.load(d_swap)
    plain.close(); run.close()


# ---- D. second life ------------------------------------------------------------------------------------------------------------------

def second_life(be, voxel, colour):
    """ResetScene on the half-swapped scene, then the first five frames again: (run, states and flags before / after the reset)."""
    run = SC.build(be, 1, voxel, colour, order="reference")
    before = (run.scene.download(capi.BUF_SWAP_STATES), run.scene.global_cache_flags())
    run.scene.reco.ResetScene()
    after = (run.scene.download(capi.BUF_SWAP_STATES), run.scene.global_cache_flags())
    return run, before, after


@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_oracle_reset_of_a_half_swapped_scene_equals_the_reference_engine(oracle, ref, voxel, colour):
    """13 on the CPU.  The reference's ResetScene leaves the swap states and the cache flags as they were; so does the oracle."""
    ref = swap_reference(ref)
    a, before, after = second_life(oracle, voxel, colour)
    assert int(np.count_nonzero(before[0] == 2)) > 900 and int(np.count_nonzero(before[1])) >= SC.TRANSFER
    b = None
    if ref.backend is not None:
        b, _, ref_after = second_life(ref.backend, voxel, colour)
        assert np.array_equal(after[0], ref_after[0]) and np.array_equal(after[1], ref_after[1]), "states / flags after ResetScene"
    frames = []
    for k in range(5):
        a.frame(k)
        frames.append(a.snapshot())
        if b is not None:
            b.frame(k)
            SC.compare(frames[-1], b.snapshot(), "oracle vs reference, second life, frame %d" % k)
    ref.check("after_reset", dict(states=after[0], flags=after[1]))
    # (the cached blocks as one array per frame: a digest per field instead of one per block)
    ref.check("frames", [dict(f, blocks=np.stack(f["blocks"])) for f in frames])
    a.close()
    if b is not None:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,colour", VOXELS, ids=VOXEL_IDS)
def test_hip_reset_of_a_half_swapped_scene_equals_the_oracle(hip, oracle, voxel, colour):
    """13: HIP == oracle after ResetScene and after every frame of the second life."""
    (a, _, after_a), (b, before, after_b) = second_life(hip, voxel, colour), second_life(oracle, voxel, colour)
    assert int(np.count_nonzero(before[0] == 2)) > 900 and int(np.count_nonzero(before[1])) >= SC.TRANSFER
    assert np.array_equal(after_a[0], after_b[0]), "swap states after ResetScene"
    assert np.array_equal(after_a[1], after_b[1]), "cache flags after ResetScene"
    lockstep(a, b, range(5), "reference", "reference", "second life")
    a.close(); b.close()
