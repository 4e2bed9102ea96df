"""Mesh vertex attributes (include/itm_hip.h: itm_mesh_attributes / itm_mesh_download_attributes / itm_mesh_write_ply).

The attributes have reference semantics -- computeSingleNormalFromSDF and readFromSDF_color4u_interpolated at vertex / voxelSize --
so everything is compared bit for bit, as whole arrays, no vertex left out:
  * CPU: the float32 numpy restatement (tests/mesh_attr_terms.py), fed the oracle's scene and mesh, reproduces the reference's values
    (tests/golden/g_mesh_attributes.*: digests of the full arrays, values of a subset) -- and from the reference's own scene where
    its build exists.  That pins the restatement before it is the yardstick on the GPU.
  * GPU: HIP normals / colours equal the restatement's for the five scenes of test_meshing, the full-buffer mesh, re-meshing,
    deferred fusion, the dense scene; staleness and colourless scenes are refused; the PLY files equal the Python writer's bytes."""
import json
import os
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import mesh_attr_cases as MC
import mesh_attr_terms as MT
from infinitam_amd import capi
from infinitam_amd.capi import BUF_HASH_ENTRIES, BUF_VOXEL_BLOCKS, MESH_COLOURS, MESH_NORMALS, Mesh

F = np.float32
GOLDEN = os.path.join(T.GOLDEN_DIR, "g_mesh_attributes")
DEBUG_MESH_ATTR_PER_VERTEX = 26          # include/itm_debug.h

_restated = {}


def golden():
    return json.load(open(GOLDEN + ".json")), np.load(GOLDEN + ".npz")


def restate(table, voxels, tri, sc):
    reader = MT.MeshVoxelReader(voxels, table)
    return MT.attributes(reader, tri, sc.voxelSize, colours=sc.colour)


def restated(name):
    """(triangles, gradients, normals, colour floats | None) of a scene of MC.SCENES from the oracle's scene and mesh"""
    if name not in _restated:
        sc = MC.SCENES[name]
        table, voxels, tri = MC.scene_and_mesh(T.oracle_backend(), sc)
        _restated[name] = (tri,) + restate(table, voxels, tri, sc)
    return _restated[name]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_matches_golden(name, tri, g, c):
    meta, arr = golden()
    e = meta["scenes"][name]
    p = MT.sample_positions(tri, MC.SCENES[name].voxelSize)
    every, halo = MT.subset_indices(name, p)
    assert g.shape[0] == e["vertices"] and MT.sha256(tri) == e["mesh_sha256"]
    assert np.array_equal(halo, arr[f"{name}_halo_index"])
    assert np.array_equal(bits(g[every]), bits(arr[f"{name}_every_gradient"])), "gradient, every k-th vertex"
    assert np.array_equal(bits(g[halo]), bits(arr[f"{name}_halo_gradient"])), "gradient, vertices with a high fractional part"
    assert MT.sha256(g) == e["gradient_sha256"]
    if "colour_sha256" in e:
        assert np.array_equal(bits(c[every]), bits(arr[f"{name}_every_colour"])) and np.array_equal(bits(c[halo]), bits(arr[f"{name}_halo_colour"]))
        assert MT.sha256(c) == e["colour_sha256"]
    else:
        assert c is None


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MC.GOLDEN_SCENES))
def test_restatement_reproduces_the_reference_values(name, ref):
    tri, g, n, c = restated(name)
    assert_matches_golden(name, tri, g, c)
    if ref.backend is not None:           # the same from the scene the reference's own engines fused and meshed
        sc = MC.SCENES[name]
        table, voxels, rtri = MC.scene_and_mesh(ref.backend, sc)
        assert np.array_equal(rtri, tri)
        rg, rn, rc = restate(table, voxels, rtri, sc)
        assert_matches_golden(name, rtri, rg, rc)
        assert np.array_equal(bits(rn), bits(n))


@pytest.mark.parametrize("name,over_1e3,over_1e5", [("mesh_micro", 22605, 22581), ("mesh_f_rgb", 22186, 22186), ("mesh_s_rgb_yaw", 347229, None)])
def test_the_low_floor_case_is_in_the_data(name, over_1e3, over_1e5):
    """Vertices on a lattice plane whose `* voxelSize / voxelSize` came back one ulp low: floor(p) sits one voxel under the cell's
    corner, the staged neighbourhood must reach planes -2 and +10 of the block."""
    tri = restated(name)[0]
    meta, arr = golden()
    p = MT.sample_positions(tri, MC.SCENES[name].voxelSize)
    assert int(MT.high_fraction(p, 1e-3).sum()) == over_1e3 == meta["scenes"][name]["high_fraction_1e-3"]
    if over_1e5 is not None:
        assert int(MT.high_fraction(p, 1e-5).sum()) == over_1e5
    halo = arr[f"{name}_halo_index"]
    assert len(halo) == 2000 == len(arr[f"{name}_halo_gradient"]) and np.all(MT.high_fraction(p[halo], 1e-3))
    assert MT.high_fraction(p[halo], 1e-5).any()
    # such a vertex really reads below the cell: floor(p) is under the lattice coordinate the vertex lies on
    q = p[halo][MT.high_fraction(p[halo], 1e-5)]
    assert np.any(np.floor(q) < np.rint(q))


def test_python_ply_writer_layout():
    tri = np.arange(18, dtype=F).reshape(2, 3, 3)
    nrm = -tri
    col = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    for n_, c_, vb in ((nrm, col, 27), (nrm, None, 24), (None, None, 12)):
        data = MT.ply_bytes(tri, n_, c_)
        head, body = data.split(b"end_header\n", 1)
        lines = head.decode().split("\n")
        assert lines[:4] == ["ply", "format binary_little_endian 1.0", "comment itm-hip mesh", "element vertex 6"]
        assert ("property float nx" in lines) == (n_ is not None) and ("property uchar red" in lines) == (c_ is not None)
        assert lines[-3:] == ["element face 2", "property list uchar int vertex_indices", ""]
        assert len(body) == 6 * vb + 2 * 13
        assert np.array_equal(np.frombuffer(body[:12], "<f4"), tri[0, 0])
        assert body[6 * vb] == 3 and np.array_equal(np.frombuffer(body[6 * vb + 1:6 * vb + 13], "<i4"), [2, 1, 0])
        assert np.array_equal(np.frombuffer(body[6 * vb + 14:6 * vb + 26], "<i4"), [5, 4, 3])
    assert MT.ply_bytes(tri, nrm, col)[-26 - 6 * 27:][12:24] == nrm[0, 0].tobytes()
    assert MT.ply_bytes(tri, nrm, col)[-26 - 6 * 27:][24:27] == bytes([0, 1, 2])


def test_binding_and_header_declare_the_entry_points():
    declared = capi.declared_functions()
    for fn in ("mesh_attributes", "mesh_download_attributes", "mesh_write_ply"):
        assert fn in declared and fn in capi._HOST_IO_SIGS and fn not in capi._SIGS
    assert (capi.MESH_NORMALS, capi.MESH_COLOURS) == (1, 2)


DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "mesh_ply_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "mesh_ply_demo")


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_demo_and_main_engine_export_compile(tmp_path):
    assert os.path.exists(build_demo())
    # ITMMainEngine_HIP::SaveSceneToMesh / SaveSceneToPLY are templates: instantiate them
    src = tmp_path / "save.cpp"
    src.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>::SaveSceneToPLY(const char*);\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_f_rgb, ITMVoxelBlockHash>::SaveSceneToPLY(const char*);\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>::SaveSceneToMesh(const char*);\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def what_of(sc):
    return MESH_NORMALS | (MESH_COLOURS if sc.colour else 0)


def hip_attributes(hip, sc, max_triangles=0, frames=None):
    ses = MC.fuse(hip, sc, frames=frames)
    m = Mesh(ses.scene, max_triangles)
    m.MeshScene()
    tri = m.triangles()
    m.ComputeAttributes(what_of(sc))
    return ses, m, tri, m.normals(), (m.colours() if sc.colour else None)


def assert_equals_restatement(name, tri, normals, colours, restatement=None):
    """restatement: (triangles, gradients, normals, colour floats | None) of a scene that is not one of MC.SCENES"""
    rtri, g, n, c = restatement if restatement is not None else restated(name)
    assert np.array_equal(tri, rtri)
    got, want = bits(normals).reshape(-1, 3), bits(n)
    if not np.array_equal(got, want):
        bad = np.nonzero(np.any(got != want, axis=1))[0]
        raise AssertionError(f"{name}: {len(bad)} of {len(want)} normals differ, first at vertex {bad[:5]}: {normals.reshape(-1, 3)[bad[:3]]} vs {n[bad[:3]]}")
    if c is not None:
        want_c = MT.colour_bytes(c)
        got_c = colours.reshape(-1, 4)
        bad = np.nonzero(np.any(got_c != want_c, axis=1))[0]
        assert len(bad) == 0, f"{name}: {len(bad)} colours differ, first at vertex {bad[:5]}: {got_c[bad[:3]]} vs {want_c[bad[:3]]}"


def assert_properties(name, tri, normals):
    nrm = normals.reshape(-1, 3)
    # equal positions get equal attributes
    keys = np.ascontiguousarray(tri.reshape(-1, 3)).view(np.dtype((np.void, 12))).reshape(-1)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    assert np.array_equal(bits(nrm[first][inverse.reshape(-1)]), bits(nrm))
    # unit length or exactly zero.  Bound: the reciprocal square root and the three products round once each, a few float32 ulps
    # (< 5e-7) of the length; 1e-6 is derived, not measured
    length = np.sqrt((nrm.astype(np.float64) ** 2).sum(1))
    zero = np.all(nrm == 0, axis=1)
    assert np.all(zero | (np.abs(length - 1.0) <= 1e-6)), np.abs(length[~zero] - 1.0).max()
    # the normal points out of the surface: agreement with the triangles' geometric normals (WriteOBJ's winding) is at least the
    # share the restatement itself reaches on this scene
    geo = np.repeat(MC.geometric_normals(tri), 3, axis=0)
    share = float(((nrm.astype(np.float64) * geo).sum(1) > 0).mean())
    want = float(((restated(name)[2].astype(np.float64) * np.repeat(MC.geometric_normals(restated(name)[0]), 3, axis=0)).sum(1) > 0).mean())
    print(f"{name}: normals agree with the geometric normal for {share:.4f} of the vertices (restatement {want:.4f}), {int(zero.sum())} zero normals")
    assert share >= want and share > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MC.SCENES))
def test_hip_attributes_equal_the_restatement(hip, name):
    sc = MC.SCENES[name]
    ses, m, tri, normals, colours = hip_attributes(hip, sc)
    assert tri.shape[0] > 1000
    assert_equals_restatement(name, tri, normals, colours)
    assert np.array_equal(m.triangles(), tri)                       # the pass writes nothing into the triangle buffer
    assert_properties(name, tri, normals)
    if name in MC.GOLDEN_SCENES:                                    # and therefore the reference's values
        meta, arr = golden()
        every, halo = MT.subset_indices(name, MT.sample_positions(tri, sc.voxelSize))
        nrm = normals.reshape(-1, 3)
        for idx, key in ((every, "every"), (halo, "halo")):
            assert np.array_equal(bits(nrm[idx]), bits(MT.normals_from_gradient(arr[f"{name}_{key}_gradient"])))
            if sc.colour:
                assert np.array_equal(colours.reshape(-1, 4)[idx], MT.colour_bytes(arr[f"{name}_{key}_colour"]))
        assert MT.sha256(restated(name)[1]) == meta["scenes"][name]["gradient_sha256"]
    if not sc.colour:
        with pytest.raises(capi.ItmError, match=r"\(-1\).*colour"):
            m.ComputeAttributes(MESH_COLOURS)
        with pytest.raises(capi.ItmError, match=r"\(-1\)"):
            m.colours()
        assert np.array_equal(bits(m.normals()), bits(normals))     # the refused request left the normals as they were


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mesh_micro", "mesh_f_rgb"])
def test_hip_one_lane_per_vertex_path(hip, name):
    """ITM_DEBUG_MESH_ATTR_PER_VERTEX: every vertex through the hash (the path vertices outside the staged planes take)"""
    hip.check(hip.fn["debug_set"](DEBUG_MESH_ATTR_PER_VERTEX, 1), "debug_set")
    try:
        ses, m, tri, normals, colours = hip_attributes(hip, MC.SCENES[name])
    finally:
        hip.check(hip.fn["debug_set"](DEBUG_MESH_ATTR_PER_VERTEX, 0), "debug_set")
    assert_equals_restatement(name, tri, normals, colours)


@pytest.mark.gpu
def test_hip_full_buffer(hip):
    sc = MC.SCENES["mesh_f_rgb"]
    full = hip_attributes(hip, sc)
    ses, m, tri, normals, colours = hip_attributes(hip, sc, max_triangles=1000)
    assert m.info() == (999, 1000) and normals.shape == (999, 3, 3) and colours.shape == (999, 3, 4)
    assert np.array_equal(tri, full[2][:999])
    assert np.array_equal(bits(normals), bits(full[3][:999])) and np.array_equal(colours, full[4][:999])


@pytest.mark.gpu
def test_hip_stale_remesh_and_dense(hip):
    sc = MC.SCENES["mesh_micro"]
    ses = MC.fuse(hip, sc)
    m = Mesh(ses.scene)
    with pytest.raises(capi.ItmError, match=r"\(-1\)"):              # never computed, never meshed
        m.normals()
    m.MeshScene()
    with pytest.raises(capi.ItmError, match=r"\(-1\)"):              # meshed, not computed
        m.normals()
    m.ComputeAttributes(MESH_NORMALS)
    assert_equals_restatement("mesh_micro", m.triangles(), m.normals(), None)
    m.MeshScene()
    with pytest.raises(capi.ItmError, match=r"\(-1\)"):              # stale after a re-mesh
        m.normals()
    with pytest.raises(capi.ItmError, match=r"\(-1\)"):
        m.ComputeAttributes(0)
    with pytest.raises(capi.ItmError, match=r"\(-1\)"):
        m.ComputeAttributes(4)
    # two more frames, re-mesh, recompute: equal to a fresh session of five frames
    ses.frame(3); ses.frame(4)
    m.MeshScene()
    m.ComputeAttributes(MESH_NORMALS)
    fresh = hip_attributes(hip, sc, frames=5)
    assert fresh[2].shape[0] != restated("mesh_micro")[0].shape[0]
    assert np.array_equal(m.triangles(), fresh[2]) and np.array_equal(bits(m.normals()), bits(fresh[3]))
    # ... and to the restatement on the oracle's five-frame scene
    ref = MC.fuse(T.oracle_backend(), sc, frames=5)
    mo = Mesh(ref.scene); mo.MeshScene()
    g, n, _ = restate(ref.scene.download(BUF_HASH_ENTRIES), ref.scene.download(BUF_VOXEL_BLOCKS), mo.triangles(), sc)
    assert np.array_equal(mo.triangles(), fresh[2]) and np.array_equal(bits(n), bits(fresh[3]).reshape(-1, 3))
    # dense scenes: an empty mesh, empty attributes, no error
    dses = MC.fuse(hip, MC.DENSE)
    dm = Mesh(dses.scene)
    dm.MeshScene()
    dm.ComputeAttributes(MESH_NORMALS)
    assert dm.info()[0] == 0 and dm.normals().shape == (0, 3, 3)
    with pytest.raises(capi.ItmError, match=r"\(-1\).*colour"):
        dm.ComputeAttributes(MESH_COLOURS)


@pytest.mark.gpu
def test_hip_recorded_frames_are_fused_first(hip):
    sc = MC.SCENES["mesh_f_rgb"]
    want = hip_attributes(hip, sc)                                   # every call launched before the next
    ses = T.Session(hip, sc, deferred_fusion=True)
    ses.frame(0, fused="four")
    v = ses.view(1)
    ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)                 # recorded, not launched
    ses.scene.reco.IntegrateIntoScene(v, ses.rs)
    m = Mesh(ses.scene)
    m.MeshScene()
    m.ComputeAttributes(what_of(sc))
    assert np.array_equal(m.triangles(), want[2])
    assert np.array_equal(bits(m.normals()), bits(want[3])) and np.array_equal(m.colours(), want[4])
    # the attribute call itself launches what is recorded: frame 1 recorded after the mesh of frame 0, then attributes
    ses2 = T.Session(hip, sc, deferred_fusion=True)
    ses2.frame(0, fused="four")
    m2 = Mesh(ses2.scene)
    m2.MeshScene()
    v2 = ses2.view(1)
    ses2.scene.reco.AllocateSceneFromDepth(v2, ses2.rs)
    ses2.scene.reco.IntegrateIntoScene(v2, ses2.rs)
    m2.ComputeAttributes(MESH_NORMALS)
    imm = T.Session(hip, sc, deferred_fusion=False)
    imm.frame(0)
    m3 = Mesh(imm.scene)
    m3.MeshScene()
    imm.frame(1)
    m3.ComputeAttributes(MESH_NORMALS)
    assert np.array_equal(m2.triangles(), m3.triangles()) and np.array_equal(bits(m2.normals()), bits(m3.normals()))


@pytest.mark.gpu
def test_hip_ply_files(hip, tmp_path):
    sc = MC.SCENES["mesh_f_rgb"]
    ses = MC.fuse(hip, sc)
    m = Mesh(ses.scene)
    m.MeshScene()
    tri = m.triangles()
    path = str(tmp_path / "m.ply")
    m.WritePLY(path)
    assert open(path, "rb").read() == MT.ply_bytes(tri)                                   # neither attribute
    m.ComputeAttributes(MESH_NORMALS)
    rtri, g, n, c = restated("mesh_f_rgb")
    m.WritePLY(path)
    assert open(path, "rb").read() == MT.ply_bytes(rtri, n)                               # normals only
    m.ComputeAttributes(MESH_COLOURS)
    m.WritePLY(path)
    assert open(path, "rb").read() == MT.ply_bytes(rtri, n, MT.colour_bytes(c))           # both
    m.MeshScene()
    m.WritePLY(path)
    assert open(path, "rb").read() == MT.ply_bytes(tri)                                   # stale attributes are not written
    # OBJ and STL are what they were
    full = hip_attributes(hip, sc)[1]
    for ext, fn in (("obj", "WriteOBJ"), ("stl", "WriteSTL")):
        pa, pb = str(tmp_path / ("a." + ext)), str(tmp_path / ("b." + ext))
        getattr(m, fn)(pa); getattr(full, fn)(pb)
        assert open(pa, "rb").read() == open(pb, "rb").read()


@pytest.mark.gpu
def test_cpp_demo_ply_equals_the_python_one(hip, tmp_path):
    exe = build_demo()
    path = str(tmp_path / "demo.ply")
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    W, H, P = 160, 120, 160 * 120
    s = hip.create_scene(capi.VOXEL_S_RGB, capi.INDEX_HASH, capi.default_params(voxelSize=0.01))
    s.reco.ResetScene()
    rs = s.vis.CreateRenderState((W, H))
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    depth = (F(1.5) + F(0.002) * ((x * 7 + y * 13) % 50).astype(F)).astype(F)
    rgb = np.stack([(x * 3) & 255, (y * 5) & 255, (x + y) & 255, np.full_like(x, 255)], -1).astype(np.uint8)
    d_depth, d_rgb = hip.to_backend(depth), hip.to_backend(rgb)
    pts = capi.DevBuffer(hip, P * 16, F, (P, 4)); nrm = capi.DevBuffer(hip, P * 16, F, (P, 4))
    for k in range(2):
        M = np.eye(4, dtype=F); M[0, 3] = F(-0.01) * F(k)
        v = capi.View(d_depth, W, H, M_d=np.ascontiguousarray(M.T).reshape(16), intr_d=(145.0, 145.0, 80.0, 60.0), rgb=d_rgb,
                      w_rgb=W, h_rgb=H, intr_rgb=(145.0, 145.0, 80.0, 60.0))
        s.process_frame(v, rs, pts, nrm)
    m = Mesh(s)
    m.MeshScene()
    tri = m.triangles()
    assert got["triangles"] == tri.shape[0] > 1000
    sc = T.Scenario(voxelSize=0.01, voxelType=capi.VOXEL_S_RGB, colour=True)
    g, n, c = restate(s.download(BUF_HASH_ENTRIES), s.download(BUF_VOXEL_BLOCKS), tri, sc)
    assert open(path, "rb").read() == MT.ply_bytes(tri, n, MT.colour_bytes(c))
    assert got["sum_red"] == int(MT.colour_bytes(c)[:, 0].astype(np.int64).sum()) > 0
