"""Indexed mesh (include/itm_hip.h: itm_mesh_index / itm_mesh_indexed_attributes / itm_mesh_write_ply_indexed / _obj_indexed).

The index is defined in terms of the triangle buffer -- bit-equal positions are one vertex, unique vertices numbered by first
occurrence, every triangle kept -- so everything is compared bit for bit, as whole arrays, no vertex or triangle left out:
  * CPU: the numpy restatement (tests/mesh_index_terms.py) on the oracle's meshes gives the distinct-position counts that
    tests/golden/g_mesh_attributes.json records for the reference's meshes, and is lossless; the Python writers' layout.
  * GPU: vertices / faces / first equal the restatement of the same soup for the five scenes of test_meshing, under the weak-hash debug
    key, for a full buffer, after re-meshing, for the dense scene; the indexed attributes equal the float32 restatement of
    tests/mesh_attr_terms.py taken at `first`; staleness is refused; the files equal the Python writers' bytes."""
import json
import os
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import mesh_attr_cases as MC
import mesh_attr_terms as MT
import mesh_index_terms as MI
from infinitam_amd import capi
from infinitam_amd.capi import MESH_COLOURS, MESH_NORMALS, Mesh
from test_mesh_attributes import bits, restated, what_of

F = np.float32
GOLDEN = os.path.join(T.GOLDEN_DIR, "g_mesh_attributes")
DEBUG_MESH_INDEX_WEAK_HASH = 27          # include/itm_debug.h
NEW_FNS = ("mesh_index", "mesh_index_info", "mesh_download_indexed", "mesh_indexed_attributes", "mesh_download_indexed_attributes",
           "mesh_write_ply_indexed", "mesh_write_obj_indexed")


def assert_is_the_index_of(tri, vertices, faces, first):
    """vertices / faces / first are the restatement's for the soup `tri`, whole arrays, and reproduce the soup"""
    wv, wf, wfirst = MI.index(tri)
    assert vertices.shape == wv.shape and faces.shape == wf.shape == (tri.shape[0], 3) and first.shape == wfirst.shape
    assert np.array_equal(first, wfirst), f"first: {int((first != wfirst).sum())} of {len(wfirst)} differ"
    assert np.array_equal(faces, wf), f"faces: {int((faces != wf).sum())} of {wf.size} differ"
    assert np.array_equal(bits(vertices), bits(wv))
    assert np.all(np.diff(first.astype(np.int64)) > 0)
    assert np.array_equal(bits(vertices[faces.astype(np.int64)]), bits(tri))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MC.GOLDEN_SCENES))
def test_restatement_on_the_oracle_meshes(name):
    tri = restated(name)[0]
    meta = json.load(open(GOLDEN + ".json"))["scenes"][name]
    vertices, faces, first = MI.index(tri)
    assert tri.shape[0] * 3 == meta["vertices"]
    assert len(vertices) == len(first) == meta["distinct_positions"] == {"mesh_micro": 38875, "mesh_f_rgb": 38030, "mesh_s_rgb_yaw": 404553}[name]
    assert first[0] == 0 and np.all(np.diff(first.astype(np.int64)) > 0)
    assert faces.shape == (tri.shape[0], 3) and faces.dtype == np.uint32 and int(faces.max()) == len(vertices) - 1
    assert np.array_equal(bits(vertices[faces.astype(np.int64)]), bits(tri))              # lossless
    assert np.array_equal(bits(vertices), bits(tri.reshape(-1, 3)[first]))
    # numbered by first occurrence: the first time index k is used, every smaller index has been used
    flat = faces.reshape(-1).astype(np.int64)
    assert np.array_equal(np.maximum.accumulate(flat)[first], np.arange(len(first)))


def test_restatement_compares_bits_not_values():
    tri = np.zeros((2, 3, 3), F)
    tri[0, 1, 0] = F(-0.0)                      # equal as a value, another vertex by the definition
    tri[1, 2] = (1, 2, 3)
    vertices, faces, first = MI.index(tri)
    assert first.tolist() == [0, 1, 5] and faces.tolist() == [[0, 1, 0], [0, 0, 2]]
    assert np.array_equal(bits(vertices), bits(tri.reshape(-1, 3)[[0, 1, 5]]))
    assert all(a.shape[0] == 0 for a in MI.index(np.zeros((0, 3, 3), F)))


def test_python_indexed_writer_layout():
    # two triangles sharing an edge: 4 vertices, 2 faces
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F)
    tri = np.stack([quad[[0, 1, 2]], quad[[0, 2, 3]]])
    vertices, faces, first = MI.index(tri)
    assert first.tolist() == [0, 1, 2, 5] and faces.tolist() == [[0, 1, 2], [0, 2, 3]] and np.array_equal(vertices, quad)
    nrm = -np.arange(12, dtype=F).reshape(4, 3)
    col = np.arange(16, dtype=np.uint8).reshape(4, 4)
    for n_, c_, vb in ((nrm, col, 27), (nrm, None, 24), (None, None, 12)):
        data = MI.ply_bytes_indexed(vertices, faces, n_, c_)
        head, body = data.split(b"end_header\n", 1)
        lines = head.decode().split("\n")
        assert lines[:4] == ["ply", "format binary_little_endian 1.0", "comment itm-hip mesh", "element vertex 4"]
        assert ("property float nx" in lines) == (n_ is not None) and ("property uchar red" in lines) == (c_ is not None)
        assert lines[-3:] == ["element face 2", "property list uchar int vertex_indices", ""]
        assert len(body) == 4 * vb + 2 * 13
        assert np.array_equal(np.frombuffer(body[vb:vb + 12], "<f4"), quad[1])
        assert body[4 * vb] == 3 and np.array_equal(np.frombuffer(body[4 * vb + 1:4 * vb + 13], "<i4"), [2, 1, 0])
        assert body[4 * vb + 13] == 3 and np.array_equal(np.frombuffer(body[4 * vb + 14:4 * vb + 26], "<i4"), [3, 2, 0])
    both = MI.ply_bytes_indexed(vertices, faces, nrm, col)[-26 - 4 * 27:]
    assert both[27 + 12:27 + 24] == nrm[1].tobytes() and both[27 + 24:27 + 27] == bytes([4, 5, 6])
    # the same header lines and property order as the soup's file
    soup_head = MT.ply_bytes(tri, np.zeros((2, 3, 3), F), np.zeros((2, 3, 4), np.uint8)).split(b"end_header\n")[0].decode().split("\n")
    mine = MI.ply_bytes_indexed(vertices, faces, nrm, col).split(b"end_header\n")[0].decode().split("\n")
    assert [l for l in mine if not l.startswith("element vertex")] == [l for l in soup_head if not l.startswith("element vertex")]
    assert MI.obj_text_indexed(vertices, faces).decode() == ("v 0.000000 0.000000 0.000000\nv 1.000000 0.000000 0.000000\nv 1.000000 1.000000 0.000000\n"
                                                            "v 0.000000 1.000000 0.000000\nf 3 2 1\nf 4 3 1\n")


def test_binding_header_and_library_declare_the_entry_points(hip_host):
    declared = capi.declared_functions()
    for fn in NEW_FNS:
        assert fn in declared and fn in capi._HOST_IO_SIGS and fn not in capi._SIGS and fn in hip_host.fn
    for method in ("Index", "vertices", "faces", "first", "ComputeIndexedAttributes", "vertex_normals", "vertex_colours", "WriteIndexedPLY",
                   "WriteIndexedOBJ"):
        assert callable(getattr(Mesh, method))
    text = open(os.path.join(T.ROOT, "include", "itm_debug.h")).read()
    assert f"#define ITM_DEBUG_MESH_INDEX_WEAK_HASH {DEBUG_MESH_INDEX_WEAK_HASH} " in text


def test_main_engine_indexed_export_compiles(tmp_path):
    src = tmp_path / "save_indexed.cpp"
    src.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>::SaveSceneToIndexedPLY(const char*);\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_f_rgb, ITMVoxelBlockHash>::SaveSceneToIndexedPLY(const char*);\n'
                   'template void ITMMesh::ComputeIndexedAttributes(const ITMScene<ITMVoxel_s_rgb, ITMVoxelBlockHash>*, int);\n'
                   'void f(ITMMesh* m) { m->Index(); m->WriteIndexedPLY("a"); m->WriteIndexedOBJ("b"); }\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def hip_index(hip, sc, max_triangles=0, frames=None):
    ses = MC.fuse(hip, sc, frames=frames)
    m = Mesh(ses.scene, max_triangles)
    m.MeshScene()
    tri = m.triangles()
    m.Index()
    return ses, m, tri


def weak_hash(hip, on):
    hip.check(hip.fn["debug_set"](DEBUG_MESH_INDEX_WEAK_HASH, 1 if on else 0), "debug_set")


def raises_invalid():
    return pytest.raises(capi.ItmError, match=r"\(-1\)")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MC.SCENES))
def test_hip_index_equals_the_restatement(hip, name):
    ses, m, tri = hip_index(hip, MC.SCENES[name])
    assert tri.shape[0] > 1000 and np.array_equal(tri, restated(name)[0])          # the soup is the oracle's, as today
    vertices, faces, first = m.vertices(), m.faces(), m.first()
    assert m.index_info() == (len(vertices), tri.shape[0])
    print(f"{name}: {tri.shape[0]} triangles, {3 * tri.shape[0]} soup vertices, {len(vertices)} unique")
    assert_is_the_index_of(tri, vertices, faces, first)
    assert np.array_equal(bits(m.triangles()), bits(tri))                          # the call leaves the triangle buffer alone
    if name in MC.GOLDEN_SCENES:
        assert len(vertices) == json.load(open(GOLDEN + ".json"))["scenes"][name]["distinct_positions"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mesh_micro", "mesh_f_rgb"])
def test_hip_index_weak_hash(hip, name):
    """ITM_DEBUG_MESH_INDEX_WEAK_HASH: 256 start slots, probe chains hundreds of slots long, the last chain wraps round the table"""
    weak_hash(hip, True)
    try:
        ses, m, tri = hip_index(hip, MC.SCENES[name])
        vertices, faces, first = m.vertices(), m.faces(), m.first()
    finally:
        weak_hash(hip, False)
    assert np.array_equal(tri, restated(name)[0])
    assert_is_the_index_of(tri, vertices, faces, first)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MC.SCENES))
def test_hip_indexed_attributes(hip, name):
    sc = MC.SCENES[name]
    ses, m, tri = hip_index(hip, sc)
    first = m.first().astype(np.int64)
    rtri, g, n, c = restated(name)
    with raises_invalid():                                                         # indexed, not computed
        m.vertex_normals()
    m.ComputeIndexedAttributes(what_of(sc))
    with raises_invalid():                                                         # the soup's attributes are another matter
        m.normals()
    vn = m.vertex_normals()
    assert vn.shape == (len(first), 3)
    got, want = bits(vn), bits(n[first])
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} of {len(want)} vertex normals differ, first at {bad[:5]}: {vn[bad[:3]]} vs {n[first][bad[:3]]}"
    vc = None
    if sc.colour:
        vc = m.vertex_colours()
        assert vc.shape == (len(first), 4) and np.array_equal(vc, MT.colour_bytes(c)[first])
    else:
        with pytest.raises(capi.ItmError, match=r"\(-1\).*colour"):
            m.ComputeIndexedAttributes(MESH_COLOURS)
        with raises_invalid():
            m.vertex_colours()
    # the soup attributes of the same handle, taken at first; computing them leaves the indexed ones alone
    m.ComputeAttributes(what_of(sc))
    assert np.array_equal(bits(m.normals().reshape(-1, 3)[first]), bits(vn))
    if sc.colour:
        assert np.array_equal(m.colours().reshape(-1, 4)[first], vc)
        assert np.array_equal(m.vertex_colours(), vc)
    assert np.array_equal(bits(m.vertex_normals()), bits(vn))
    # ... and the other way round: a new index makes the indexed attributes stale, not the soup's
    soup_normals = m.normals()
    m.Index()
    with raises_invalid():
        m.vertex_normals()
    assert np.array_equal(bits(m.normals()), bits(soup_normals))
    m.ComputeIndexedAttributes(MESH_NORMALS)
    assert np.array_equal(bits(m.vertex_normals()), bits(vn)) and np.array_equal(bits(m.normals()), bits(soup_normals))
    assert np.array_equal(bits(m.triangles()), bits(tri))
    with raises_invalid():
        m.ComputeIndexedAttributes(0)
    with raises_invalid():
        m.ComputeIndexedAttributes(4)


@pytest.mark.gpu
def test_hip_index_of_a_full_buffer(hip):
    sc = MC.SCENES["mesh_f_rgb"]
    ses, m, tri = hip_index(hip, sc, max_triangles=1000)
    assert m.info() == (999, 1000) and np.array_equal(tri, restated("mesh_f_rgb")[0][:999])
    assert_is_the_index_of(tri, m.vertices(), m.faces(), m.first())
    first = m.first().astype(np.int64)
    m.ComputeIndexedAttributes(what_of(sc))
    rtri, g, n, c = restated("mesh_f_rgb")
    assert np.array_equal(bits(m.vertex_normals()), bits(n[first])) and np.array_equal(m.vertex_colours(), MT.colour_bytes(c)[first])


@pytest.mark.gpu
def test_hip_index_stale_remesh_and_dense(hip, tmp_path):
    sc = MC.SCENES["mesh_micro"]
    ses = MC.fuse(hip, sc)
    m = Mesh(ses.scene)
    path = str(tmp_path / "x")

    def assert_refused():
        for call in (m.index_info, m.vertices, m.faces, m.first, m.vertex_normals, lambda: m.ComputeIndexedAttributes(MESH_NORMALS),
                     lambda: m.WriteIndexedPLY(path), lambda: m.WriteIndexedOBJ(path)):
            with raises_invalid():
                call()

    assert_refused()                                                  # never meshed, never indexed
    m.MeshScene()
    assert_refused()                                                  # meshed, not indexed
    m.Index()
    m.ComputeIndexedAttributes(MESH_NORMALS)
    assert_is_the_index_of(restated("mesh_micro")[0], m.vertices(), m.faces(), m.first())
    m.MeshScene()
    assert_refused()                                                  # stale after a re-mesh
    # two more frames, re-mesh, re-index: equal to a fresh session of five frames
    ses.frame(3); ses.frame(4)
    m.MeshScene()
    m.Index()
    m.ComputeIndexedAttributes(MESH_NORMALS)
    fses, fm, ftri = hip_index(hip, sc, frames=5)
    fm.ComputeIndexedAttributes(MESH_NORMALS)
    assert ftri.shape[0] != restated("mesh_micro")[0].shape[0] and np.array_equal(m.triangles(), ftri)
    assert_is_the_index_of(ftri, m.vertices(), m.faces(), m.first())
    for a, b in ((m.vertices(), fm.vertices()), (m.vertex_normals(), fm.vertex_normals())):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(m.faces(), fm.faces()) and np.array_equal(m.first(), fm.first())
    # dense scenes: an empty mesh, an empty index, files with zero elements, no error
    dses = MC.fuse(hip, MC.DENSE)
    dm = Mesh(dses.scene)
    dm.MeshScene()
    dm.Index()
    dm.ComputeIndexedAttributes(MESH_NORMALS)
    assert dm.index_info() == (0, 0)
    assert dm.vertices().shape == (0, 3) and dm.faces().shape == (0, 3) and dm.first().shape == (0,) and dm.vertex_normals().shape == (0, 3)
    dm.WriteIndexedPLY(path + ".ply"); dm.WriteIndexedOBJ(path + ".obj")
    empty = np.zeros((0, 3), F)
    assert open(path + ".ply", "rb").read() == MI.ply_bytes_indexed(empty, np.zeros((0, 3), np.uint32), empty)
    assert open(path + ".obj", "rb").read() == b""
    with pytest.raises(capi.ItmError, match=r"\(-1\).*colour"):
        dm.ComputeIndexedAttributes(MESH_COLOURS)


@pytest.mark.gpu
def test_hip_recorded_frames_are_fused_before_indexed_attributes(hip):
    sc = MC.SCENES["mesh_f_rgb"]
    # frame 1 recorded after the mesh and the index of frame 0, then the attributes: they read the scene with frame 1 in it
    ses = T.Session(hip, sc, deferred_fusion=True)
    ses.frame(0, fused="four")
    m = Mesh(ses.scene)
    m.MeshScene()
    m.Index()
    v = ses.view(1)
    ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)                 # recorded, not launched
    ses.scene.reco.IntegrateIntoScene(v, ses.rs)
    m.ComputeIndexedAttributes(what_of(sc))
    imm = T.Session(hip, sc, deferred_fusion=False)
    imm.frame(0)
    m2 = Mesh(imm.scene)
    m2.MeshScene()
    m2.Index()
    imm.frame(1)
    m2.ComputeIndexedAttributes(what_of(sc))
    m2.ComputeAttributes(what_of(sc))
    first = m2.first().astype(np.int64)
    assert np.array_equal(m.triangles(), m2.triangles()) and np.array_equal(m.first(), m2.first())
    assert np.array_equal(bits(m.vertex_normals()), bits(m2.vertex_normals())) and np.array_equal(m.vertex_colours(), m2.vertex_colours())
    assert np.array_equal(bits(m2.normals().reshape(-1, 3)[first]), bits(m.vertex_normals()))
    # and they differ from what frame 0 alone gives: the recorded frame was really fused first
    only0 = T.Session(hip, sc, deferred_fusion=False)
    only0.frame(0)
    m3 = Mesh(only0.scene)
    m3.MeshScene()
    m3.Index()
    m3.ComputeIndexedAttributes(MESH_NORMALS)
    assert np.array_equal(m3.first(), m.first()) and not np.array_equal(bits(m3.vertex_normals()), bits(m.vertex_normals()))


@pytest.mark.gpu
def test_hip_indexed_files(hip, tmp_path):
    sc = MC.SCENES["mesh_f_rgb"]
    ses = MC.fuse(hip, sc)
    m = Mesh(ses.scene)
    m.MeshScene()
    tri = m.triangles()
    soup_files = {}
    for ext, fn in (("ply", "WritePLY"), ("obj", "WriteOBJ"), ("stl", "WriteSTL")):
        getattr(m, fn)(str(tmp_path / ("before." + ext)))
        soup_files[ext] = open(str(tmp_path / ("before." + ext)), "rb").read()
    m.Index()
    vertices, faces, first = MI.index(tri)
    rtri, g, n, c = restated("mesh_f_rgb")
    path = str(tmp_path / "i.ply")
    m.WriteIndexedPLY(path)
    assert open(path, "rb").read() == MI.ply_bytes_indexed(vertices, faces)                                   # neither attribute
    m.ComputeAttributes(what_of(sc))                                                                          # the soup's do not count
    m.WriteIndexedPLY(path)
    assert open(path, "rb").read() == MI.ply_bytes_indexed(vertices, faces)
    m.MeshScene(); m.Index()
    m.ComputeIndexedAttributes(MESH_NORMALS)
    m.WriteIndexedPLY(path)
    assert open(path, "rb").read() == MI.ply_bytes_indexed(vertices, faces, n[first])                         # normals only
    m.ComputeIndexedAttributes(MESH_COLOURS)
    m.WriteIndexedPLY(path)
    data = open(path, "rb").read()
    assert data == MI.ply_bytes_indexed(vertices, faces, n[first], MT.colour_bytes(c)[first])                 # both
    print(f"mesh_f_rgb: indexed PLY {len(data)} bytes, soup PLY with both attributes {len(MT.ply_bytes(tri, n, MT.colour_bytes(c)))} bytes")
    opath = str(tmp_path / "i.obj")
    m.WriteIndexedOBJ(opath)
    assert open(opath, "rb").read() == MI.obj_text_indexed(vertices, faces)
    # the soup's files are what they were before the index existed
    for ext, fn in (("ply", "WritePLY"), ("obj", "WriteOBJ"), ("stl", "WriteSTL")):
        getattr(m, fn)(str(tmp_path / ("after." + ext)))
        assert open(str(tmp_path / ("after." + ext)), "rb").read() == soup_files[ext]


@pytest.mark.gpu
def test_hip_index_is_deterministic(hip):
    sc = MC.SCENES["mesh_s_rgb_yaw"]
    ses, m, tri = hip_index(hip, sc)
    a = (m.vertices(), m.faces(), m.first())
    m.Index()
    b = (m.vertices(), m.faces(), m.first())
    m2 = Mesh(ses.scene)
    m2.MeshScene()
    m2.Index()
    c = (m2.vertices(), m2.faces(), m2.first())
    for other in (b, c):
        assert np.array_equal(bits(a[0]), bits(other[0])) and np.array_equal(a[1], other[1]) and np.array_equal(a[2], other[2])
