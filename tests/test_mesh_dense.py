"""Dense meshing (include/itm_hip.h: itm_mesh_volume; tests/mesh_dense_cases.py states the expectation).

The mesh of a dense volume is defined by the reference's per-cell function, so every comparison is bit for bit, as whole arrays: the
expected triangles are the oracle's MeshScene of the equivalent hash scene, reordered per cell into the brick order of the definition.
  * CPU: the helper's table is consistent, the triangles-per-case table comes out of the oracle as it must, the per-cell total equals
    the oracle's, the header and the binding declare the entry point.
  * GPU: all 256 sign configurations, a ragged volume at an offset that is no multiple of 8, fused scenes of all four voxel types and
    a wider one (2 048 bricks: several grid strides), an uploaded volume of 8 602 bricks (three sweeps of the scan), the full buffer, what stays as it was (itm_mesh_scene, staleness, recorded frames), and everything
    downstream of the triangles (attributes, index, writers)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import mesh_attr_cases as MC
import mesh_attr_terms as MT
import mesh_dense_cases as MD
import mesh_index_terms as MI
from infinitam_amd import capi
from infinitam_amd.capi import BUF_HASH_ENTRIES, BUF_VOXEL_BLOCKS, MESH_COLOURS, MESH_NORMALS, Mesh

F = np.float32
COLOUR = (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB)
ALL_TYPES = (capi.VOXEL_S, capi.VOXEL_F, capi.VOXEL_S_RGB, capi.VOXEL_F_RGB)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


_expected = {}


def expected_ragged(voxelType):
    key = ("ragged", voxelType)
    if key not in _expected:
        v = MD.ragged_volume(voxelType)
        _expected[key] = (v,) + MD.expected_mesh(v, MD.RAGGED_SIZE, MD.RAGGED_OFFSET, voxelType, MD.RAGGED_VOXEL_SIZE)
    return _expected[key]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------

def test_equivalent_table_is_consistent():
    """every block is found again by a walk from hashIndex; chains are used where heads collide"""
    v = MD.ragged_volume(capi.VOXEL_F)
    table, blocks, runs = MD.dense_as_hash(v, MD.RAGGED_SIZE, MD.RAGGED_OFFSET, capi.VOXEL_F)
    assert len(runs) == 3 * 3 * 2 == len(blocks) // 512                 # x: -7 .. 12, y: 3 .. 19, z: 95 .. 103 in 8-aligned blocks
    assert int((table["ptr"] >= 0).sum()) == len(runs) and len({s for s, _ in runs}) == len(runs)
    for slot, pos in runs:
        assert MD.walk(table, pos) == slot
    assert MD.walk(table, (100, 100, 100)) == -1
    # array voxels sit where they fall, the rest is the default voxel
    got = blocks[table["ptr"][MD.walk(table, (0, 1, 12))] * 512 + 1 + 2 * 8 + 3 * 64]      # global (1, 10, 99) = array (8, 7, 4)
    assert got == v.reshape(9, 17, 20)[4, 7, 8]
    assert int((blocks["sdf"] != 1.0).sum()) == int((v["sdf"] != 1.0).sum())
    # colliding positions: the later block goes to the top of the excess list and is found through the chain (30^3 positions in
    # 2^20 buckets collide some hundred times, also three to a bucket)
    g = np.arange(-15, 15)
    many = np.stack([a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij")], -1)
    t2, r2 = MD.build_table(many)
    in_excess = [(s, p) for s, p in r2 if s >= MD.BUCKET_NUM]
    assert len(in_excess) > 100 and in_excess[0][0] == MD.BUCKET_NUM + MD.EXCESS_NUM - 1
    assert len({s for s, _ in r2}) == len(r2) and all(MD.walk(t2, p) == s for s, p in in_excess) and all(MD.walk(t2, p) == s for s, p in r2[::37])
    heads = np.bincount(MD.hash_index(many), minlength=MD.BUCKET_NUM)
    assert heads.max() >= 3 and int((heads - 1).clip(0).sum()) == len(in_excess)
    big, _, runs_big = MD.dense_as_hash(MD.default_voxels(64 * 64 * 64, capi.VOXEL_S), (64, 64, 64), (-32, -32, 95), capi.VOXEL_S)
    assert len(runs_big) == 8 * 8 * 9 and all(MD.walk(big, p) == s for s, p in runs_big)


def test_triangles_per_case_come_from_the_oracle():
    ntri = MD.ntri_table()
    assert ntri.shape == (256,) and ntri[0] == 0 and ntri[255] == 0
    assert np.all((ntri[1:255] >= 1) & (ntri[1:255] <= 5))
    assert all(ntri[1 << j] == 1 and ntri[255 ^ (1 << j)] == 1 for j in range(8))      # one corner apart from the rest: one triangle


def test_per_cell_total_equals_the_oracle_total():
    for vt in (capi.VOXEL_F, capi.VOXEL_S_RGB):
        v, tri, table, blocks = expected_ragged(vt)                      # expected_mesh asserts the equality
        uncut = int(MD.cell_counts(MD.ragged_volume(vt, cut=False), MD.RAGGED_SIZE).sum())
        assert tri.shape[0] == int(MD.cell_counts(v, MD.RAGGED_SIZE).sum()) > 100 and tri.shape[0] != uncut
    # the early returns of sdfInterp are in the data: vertices that sit exactly on lattice points
    v, tri, _, _ = expected_ragged(capi.VOXEL_F)
    p = (tri.reshape(-1, 3) / F(MD.RAGGED_VOXEL_SIZE)).astype(np.float64)
    assert int(np.all(np.abs(p - np.rint(p)) < 1e-4, axis=1).sum()) > 10


def test_binding_and_header_declare_the_entry_point():
    declared = capi.declared_functions()
    assert "mesh_volume" in declared and "mesh_volume" in capi._HOST_IO_SIGS and "mesh_volume" not in capi._SIGS
    assert hasattr(Mesh, "MeshVolume")
    text = open(os.path.join(T.ROOT, "include", "itm_hip.h")).read()
    assert "int ITM_FN(mesh_volume)(const itm_scene* scene, itm_mesh* mesh, itm_stream stream);" in text


def test_adapters_compile(tmp_path):
    src = tmp_path / "volume.cpp"
    src.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_s, ITMPlainVoxelArray>::SaveVolumeToMesh(const char*);\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_f_rgb, ITMVoxelBlockHash>::SaveVolumeToMesh(const char*);\n'
                   'template class ITMMeshingEngine_HIP<ITMVoxel_s, ITMPlainVoxelArray>;\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def upload_dense(hip, voxels, size, offset, voxelType, voxelSize):
    s = hip.create_scene(voxelType, capi.INDEX_DENSE, capi.default_params(voxelSize=voxelSize), denseSize=size, denseOffset=offset)
    s.reco.ResetScene()
    s.upload(BUF_VOXEL_BLOCKS, voxels)
    return s


def assert_triangles(got, want, what):
    assert got.shape == want.shape, f"{what}: {got.shape[0]} triangles, expected {want.shape[0]}"
    bad = np.nonzero(np.any(bits(got).reshape(len(got), 9) != bits(want).reshape(len(want), 9), axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} triangles differ, first at {bad[:5]}: {got[bad[:2]]} vs {want[bad[:2]]}"


def fused_dense(hip, sc, frames=None):
    """(session, voxels downloaded from the HIP scene after fusing)"""
    ses = MC.fuse(hip, sc, frames=frames)
    return ses, ses.scene.download(BUF_VOXEL_BLOCKS)


def fused_expected(hip, sc):
    key = ("fused", sc.name, sc.voxelType)
    if key not in _expected:
        ses, v = fused_dense(hip, sc)
        ses.close()
        _expected[key] = (v,) + MD.expected_mesh(v, sc.denseSize, sc.denseOffset, sc.voxelType, sc.voxelSize)
    return _expected[key]


@pytest.mark.gpu
@pytest.mark.parametrize("vt", [capi.VOXEL_F, capi.VOXEL_S])
def test_hip_all_256_cases(hip, vt):
    v = MD.case_volume(vt)
    want, _, _ = MD.expected_mesh(v, MD.CASE_SIZE, (0, 0, 0), vt, MD.CASE_VOXEL_SIZE)
    assert want.shape[0] == int(MD.ntri_table().sum()) > 256
    s = upload_dense(hip, v, MD.CASE_SIZE, (0, 0, 0), vt, MD.CASE_VOXEL_SIZE)
    m = Mesh(s, want.shape[0] + 2)
    m.MeshVolume()
    assert_triangles(m.triangles(), want, "256 cases")


@pytest.mark.gpu
@pytest.mark.parametrize("vt", [capi.VOXEL_F, capi.VOXEL_S_RGB])
def test_hip_ragged_and_unaligned(hip, vt):
    v, want, _, _ = expected_ragged(vt)
    assert want.shape[0] > 100
    s = upload_dense(hip, v, MD.RAGGED_SIZE, MD.RAGGED_OFFSET, vt, MD.RAGGED_VOXEL_SIZE)
    m = Mesh(s, want.shape[0] + 2)
    m.MeshVolume()
    assert_triangles(m.triangles(), want, "ragged volume")


@pytest.mark.gpu
@pytest.mark.parametrize("vt", ALL_TYPES)
def test_hip_fused_scenes(hip, vt):
    sc = MD.dense_scenario(MC.DENSE, vt)
    v, want, _, _ = fused_expected(hip, sc)
    assert want.shape[0] > 1000
    ses, v2 = fused_dense(hip, sc)
    assert v2.tobytes() == v.tobytes()
    m = Mesh(ses.scene, want.shape[0] + 2)
    m.MeshVolume()
    assert_triangles(m.triangles(), want, sc.name)


@pytest.mark.gpu
def test_hip_wide_fused_scene(hip):
    sc = MD.WIDE                                                         # denseOffset (-64, -64, 96)
    v, want, _, _ = fused_expected(hip, sc)
    assert want.shape[0] > 1000
    ses, _ = fused_dense(hip, sc)
    m = Mesh(ses.scene, want.shape[0] + 2)
    m.MeshVolume()
    assert_triangles(m.triangles(), want, sc.name)


def expected_sweeps():
    if "sweeps" not in _expected:
        v = MD.sweeps_volume()
        _expected["sweeps"] = (v,) + MD.expected_mesh(v, MD.SWEEPS_SIZE, MD.SWEEPS_OFFSET, capi.VOXEL_S, MD.SWEEPS_VOXEL_SIZE)
    return _expected["sweeps"]


@pytest.mark.gpu
def test_hip_scan_over_several_sweeps(hip):
    """8 602 bricks: the scan carries base and list position over three sweeps of 4 096 bricks (the last partial), bit for bit; with
    a full buffer the last slot's triangle comes from a brick of the last sweep"""
    v, want, _, _ = expected_sweeps()
    per_brick = MD.brick_counts(v, MD.SWEEPS_SIZE)
    assert len(per_brick) == 23 * 22 * 17 == 8602 and len(per_brick) % MD.SWEEP_BRICKS != 0
    listed = np.nonzero(per_brick)[0]
    assert set(listed // MD.SWEEP_BRICKS) == {0, 1, 2} and int(per_brick.sum()) == want.shape[0] > 50000
    assert min(int((listed // MD.SWEEP_BRICKS == k).sum()) for k in range(3)) >= 10
    s = upload_dense(hip, v, MD.SWEEPS_SIZE, MD.SWEEPS_OFFSET, capi.VOXEL_S, MD.SWEEPS_VOXEL_SIZE)
    m = Mesh(s, want.shape[0] + 2)
    m.MeshVolume()
    assert_triangles(m.triangles(), want, "three sweeps")
    # the cap inside the second sweep's triangles: the buffer is expected[:cap - 1], the last slot holds the last triangle of all
    cap = int(per_brick[:MD.SWEEP_BRICKS + 1000].sum()) + 3
    assert int(per_brick[:MD.SWEEP_BRICKS].sum()) < cap - 1 < want.shape[0]
    m2 = Mesh(s, cap)
    m2.MeshVolume()
    assert m2.info() == (cap - 1, cap)
    assert_triangles(m2.triangles(), want[:cap - 1], "three sweeps, full buffer")
    assert np.array_equal(bits(last_slot(s, m2, cap)), bits(want[-1]))


@pytest.mark.gpu
def test_hip_full_buffer(hip):
    sc = MD.dense_scenario(MC.DENSE, capi.VOXEL_S)
    v, want, _, _ = fused_expected(hip, sc)
    ses, _ = fused_dense(hip, sc)
    m = Mesh(ses.scene, 1000)
    m.MeshVolume()
    assert m.info() == (999, 1000)
    assert_triangles(m.triangles(), want[:999], "full buffer")
    n_all = want.shape[0]
    m2 = Mesh(ses.scene, n_all + 1)
    m2.MeshVolume()
    assert m2.info() == (n_all, n_all + 1)
    assert_triangles(m2.triangles(), want, "max_triangles = n_all + 1")


def last_slot(s, m, cap):
    """slot cap - 1 of a mesh's buffer: past the counted triangles, so read from the device"""
    last = np.zeros((1, 3, 3), F)
    dev = capi._P()
    s.be.check(s.be.fn["mesh_info"](capi._P(m.h), None, None, C.byref(dev), None), "mesh_info")
    s.be.check(s.be.fn["memcpy_d2h"](last.ctypes.data_as(capi._P), capi._P(dev.value + (cap - 1) * 36), 36, None), "memcpy_d2h")
    s.be.sync()
    return last[0]


def sorted_rows(tri):
    rows = bits(tri).reshape(len(tri), 9)
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.gpu
@pytest.mark.parametrize("vt", [capi.VOXEL_S, capi.VOXEL_F_RGB])
def test_hip_dense_and_hash_meshers_emit_the_same_cells(hip, vt):
    """the ragged volume as a dense scene and as its equivalent hash scene: both meshers go through one cell function, handed positions
    and samples their own way (clipped bricks, a non-zero offset, corners in a neighbouring block) -- the same triangles bit for bit as
    multisets, and with a full buffer each keeps ITS last generated triangle in the last slot"""
    v, want, table, blocks = expected_ragged(vt)
    n = want.shape[0]
    assert n > 100
    key = ("ragged hash order", vt)
    if key not in _expected:
        _expected[key] = MD.oracle_mesh(table, blocks, vt, MD.RAGGED_VOXEL_SIZE, n + 2)
    want_hash = _expected[key]                                           # table-slot order: the hash mesher's
    assert want_hash.shape == want.shape and not np.array_equal(bits(want_hash), bits(want))
    d = upload_dense(hip, v, MD.RAGGED_SIZE, MD.RAGGED_OFFSET, vt, MD.RAGGED_VOXEL_SIZE)
    h = hip.create_scene(vt, capi.INDEX_HASH, capi.default_params(voxelSize=MD.RAGGED_VOXEL_SIZE), localBlockNum=max(len(blocks) // 512 + 1, 16))
    h.reco.ResetScene()
    h.upload(BUF_HASH_ENTRIES, table)
    h.upload(BUF_VOXEL_BLOCKS, blocks)
    md, mh = Mesh(d, n + 2), Mesh(h, n + 2)
    md.MeshVolume(); mh.MeshScene()
    assert md.info() == (n, n + 2) == mh.info()
    td, th = md.triangles(), mh.triangles()
    assert np.array_equal(sorted_rows(td), sorted_rows(th))
    assert_triangles(td, want, "dense order"); assert_triangles(th, want_hash, "hash order")
    # three too small: cap - 1 counted triangles, the last slot keeps the mesher's own last triangle (the two orders end differently)
    cap = n - 3
    assert not np.array_equal(bits(want[-1]), bits(want_hash[-1]))
    for s, m, mesh, expected, what in ((d, Mesh(d, cap), "MeshVolume", want, "dense"), (h, Mesh(h, cap), "MeshScene", want_hash, "hash")):
        getattr(m, mesh)()
        assert m.info() == (cap - 1, cap)
        assert_triangles(m.triangles(), expected[:cap - 1], what + ", full buffer")
        assert np.array_equal(bits(last_slot(s, m, cap)), bits(expected[-1])), what + ": last slot"


@pytest.mark.gpu
def test_hip_unchanged_behaviour_and_staleness(hip):
    sc = MD.dense_scenario(MC.DENSE, capi.VOXEL_S)
    v, want, _, _ = fused_expected(hip, sc)
    ses, _ = fused_dense(hip, sc)
    m = Mesh(ses.scene, 1000000)
    m.MeshScene()
    assert m.info()[0] == 0                                              # itm_mesh_scene: empty, as in the reference
    m.MeshVolume()
    assert_triangles(m.triangles(), want, "after an empty MeshScene")
    with pytest.raises(capi.ItmError, match=r"\(-1\)"):                  # meshed, attributes not computed
        m.normals()
    m.ComputeAttributes(MESH_NORMALS)
    m.Index()
    m.ComputeIndexedAttributes(MESH_NORMALS)
    assert m.normals().shape == want.shape and m.index_info()[1] == want.shape[0]
    m.MeshVolume()                                                       # makes attributes and index stale
    for call in (m.normals, m.index_info, m.vertices, m.vertex_normals):
        with pytest.raises(capi.ItmError, match=r"\(-1\)"):
            call()
    m.MeshScene()                                                        # replaces the mesh: empty again
    assert m.info()[0] == 0 and m.triangles().shape == (0, 3, 3)
    m.ComputeAttributes(MESH_NORMALS); m.Index()
    assert m.normals().shape == (0, 3, 3) and m.index_info() == (0, 0)
    # two more frames, mesh again: the expected array of the new voxels
    ses.frame(2); ses.frame(3)
    v4 = ses.scene.download(BUF_VOXEL_BLOCKS)
    assert v4.tobytes() != v.tobytes()
    want4, _, _ = MD.expected_mesh(v4, sc.denseSize, sc.denseOffset, sc.voxelType, sc.voxelSize)
    m.MeshVolume()
    assert_triangles(m.triangles(), want4, "four frames")
    # a hash scene: MeshVolume is MeshScene
    hs = MC.fuse(hip, MC.SCENES["mesh_micro"])
    a, b = Mesh(hs.scene), Mesh(hs.scene)
    a.MeshScene(); b.MeshVolume()
    assert a.info() == b.info() and a.info()[0] > 1000 and np.array_equal(bits(a.triangles()), bits(b.triangles()))
    b.ComputeAttributes(MESH_NORMALS); a.ComputeAttributes(MESH_NORMALS)
    assert np.array_equal(bits(a.normals()), bits(b.normals()))


@pytest.mark.gpu
def test_hip_recorded_frames_are_fused_before_meshing(hip):
    sc = MD.dense_scenario(MC.DENSE, capi.VOXEL_S)
    v, want, _, _ = fused_expected(hip, sc)
    ses = T.Session(hip, sc, deferred_fusion=True)
    ses.frame(0, fused="four")
    vw = ses.view(1)
    ses.scene.reco.AllocateSceneFromDepth(vw, ses.rs)                    # recorded, not launched
    ses.scene.reco.IntegrateIntoScene(vw, ses.rs)
    m = Mesh(ses.scene, want.shape[0] + 2)
    m.MeshVolume()
    assert_triangles(m.triangles(), want, "deferred fusion")


def read_stl(path):
    data = open(path, "rb").read()
    n = struct.unpack("<I", data[80:84])[0]
    rec = np.frombuffer(data[84:], np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    assert len(rec) == n and data[:80] == b" " * 80
    return rec["v"][:, ::-1, :]                                          # WriteSTL stores p2, p1, p0


def downstream_case(hip, name):
    if name == "ragged":
        vt = capi.VOXEL_S_RGB
        v, want, table, blocks = expected_ragged(vt)
        s = upload_dense(hip, v, MD.RAGGED_SIZE, MD.RAGGED_OFFSET, vt, MD.RAGGED_VOXEL_SIZE)
        return s, s, vt, MD.RAGGED_VOXEL_SIZE, want, table, blocks
    vt = {"s": capi.VOXEL_S, "f_rgb": capi.VOXEL_F_RGB}[name]
    sc = MD.dense_scenario(MC.DENSE, vt)
    v, want, table, blocks = fused_expected(hip, sc)
    ses, _ = fused_dense(hip, sc)
    return ses, ses.scene, vt, sc.voxelSize, want, table, blocks


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s", "f_rgb", "ragged"])
def test_hip_downstream_of_a_dense_mesh(hip, tmp_path, name):
    keep, scene, vt, voxelSize, want, table, blocks = downstream_case(hip, name)
    colour = vt in COLOUR
    m = Mesh(scene, want.shape[0] + 2)
    m.MeshVolume()
    tri = m.triangles()
    assert_triangles(tri, want, name)
    g, n, c = MT.attributes(MT.MeshVoxelReader(blocks, table), tri, voxelSize, colours=colour)
    what = MESH_NORMALS | (MESH_COLOURS if colour else 0)
    m.ComputeAttributes(what)
    got = bits(m.normals()).reshape(-1, 3)
    bad = np.nonzero(np.any(got != bits(n), axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(n)} normals differ, first at vertex {bad[:5]}: {m.normals().reshape(-1, 3)[bad[:3]]} vs {n[bad[:3]]}"
    if colour:
        assert np.array_equal(m.colours().reshape(-1, 4), MT.colour_bytes(c))
    else:
        with pytest.raises(capi.ItmError, match=r"\(-1\).*colour"):
            m.ComputeAttributes(MESH_COLOURS)
    assert np.array_equal(bits(m.triangles()), bits(tri))
    # index
    m.Index()
    vertices, faces, first = m.vertices(), m.faces(), m.first()
    assert np.array_equal(bits(vertices[faces.astype(np.int64)]), bits(tri)) and np.all(np.diff(first.astype(np.int64)) > 0)
    wv, wf, wfirst = MI.index(tri)
    assert np.array_equal(bits(vertices), bits(wv)) and np.array_equal(faces, wf) and np.array_equal(first, wfirst)
    m.ComputeIndexedAttributes(what)
    fi = first.astype(np.int64)
    assert np.array_equal(bits(m.vertex_normals()), bits(n[fi]))
    if colour:
        assert np.array_equal(m.vertex_colours(), MT.colour_bytes(c)[fi])
    # writers
    p = str(tmp_path / "m")
    m.WritePLY(p + ".ply")
    assert open(p + ".ply", "rb").read() == MT.ply_bytes(tri, n, MT.colour_bytes(c) if colour else None)
    m.WriteIndexedPLY(p + "_i.ply")
    assert open(p + "_i.ply", "rb").read() == MI.ply_bytes_indexed(vertices, faces, n[fi], MT.colour_bytes(c)[fi] if colour else None)
    m.WriteSTL(p + ".stl")
    assert np.array_equal(bits(read_stl(p + ".stl")), bits(tri))
    m.WriteIndexedOBJ(p + "_i.obj")
    assert open(p + "_i.obj", "rb").read() == MI.obj_text_indexed(vertices, faces)
    m.WriteOBJ(p + ".obj")
    lines = open(p + ".obj").read().split("\n")
    nt = tri.shape[0]
    assert lines[0] == "v %f %f %f" % tuple(float(x) for x in tri[0, 0]) and lines[3 * nt - 1] == "v %f %f %f" % tuple(float(x) for x in tri[-1, 2])
    assert lines[3 * nt] == "f 3 2 1" and lines[4 * nt - 1] == f"f {3 * nt} {3 * nt - 1} {3 * nt - 2}" and lines[4 * nt:] == [""]
    got_v = np.array([[float(t) for t in ln.split()[1:]] for ln in lines[:3 * nt]])
    assert np.array_equal(got_v, np.array([[float("%f" % x) for x in row] for row in tri.reshape(-1, 3)]))
