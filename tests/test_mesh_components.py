"""Connected components of the indexed mesh and the fragment filter (include/itm_hip.h: itm_mesh_components / itm_mesh_components_info /
itm_mesh_download_components / itm_mesh_filter_components; include/itm_debug.h: itm_debug_mesh_components, key 30).

The components are defined on the index -- vertices linked iff a triangle names both, numbered by ascending smallest vertex, integer
counts and a box in the order of the float bits -- so everything is compared bit for bit, as whole arrays:
  * CPU: the numpy restatement (tests/mesh_components_terms.py) on the oracle's meshes gives the component counts and sizes measured for
    the three golden scenes (cross-checked against scipy where it is importable); its properties; hand cases; the boundary.
  * GPU: the three arrays equal the restatement of the same downloaded index for four scenes, under the per-lane statistics key and under
    the weak-hash index key; adversarial graphs through the hook; the filter's buffer, attributes, index, components and files against
    the restatements of the packed soup; staleness and refusals; lifecycle, memory, failed allocations; determinism."""
import ctypes as C
import gc
import os
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import mesh_attr_cases as MC
import mesh_attr_terms as MT
import mesh_components_terms as MK
import mesh_index_terms as MI
from infinitam_amd import capi
from infinitam_amd.capi import MESH_COLOURS, MESH_NORMALS, Mesh
from test_mesh_attributes import bits, restated, what_of

F = np.float32
DEBUG_MESH_ATTR_PER_VERTEX = 26          # include/itm_debug.h
DEBUG_MESH_INDEX_WEAK_HASH = 27
DEBUG_FAIL_ALLOCATION = 28
DEBUG_MESH_COMPONENTS_PER_LANE = 30
NEW_FNS = ("mesh_components", "mesh_components_info", "mesh_download_components", "mesh_filter_components", "debug_mesh_components")
# measured on the oracle's meshes with a numpy union-find, cross-checked against scipy.sparse.csgraph.connected_components:
# triangles, unique vertices, components, the three largest (number, triangles, vertices), (components, triangles) with >= 100 triangles
MEASURED = {
    "mesh_micro": (72769, 38875, 99, [(8, 59516, 30595), (0, 12688, 7514), (11, 72, 71)], (2, 72204)),
    "mesh_f_rgb": (71311, 38030, 93, [(6, 58848, 30261), (0, 11809, 6913), (15, 142, 148)], (3, 70799)),
    "mesh_s_rgb_yaw": (819263, 404553, 1322, [(1, 506352, 254840), (6, 97576, 51191), (14, 81656, 26649)], (25, 805335)),
}
_labelled = {}


def labelled(name):
    """(triangles, vertices, faces, vertexComponent, triangleComponent, stats) of the oracle's mesh of a golden scene"""
    if name not in _labelled:
        tri = restated(name)[0]
        vertices, faces, first = MI.index(tri)
        _labelled[name] = (tri, vertices, faces) + MK.components(faces, vertices)
    return _labelled[name]


def words(stats):
    """the component records as uint32 words: compared by bits"""
    return np.ascontiguousarray(stats).view(np.uint32).reshape(-1, 10)


def same_labelling(got, want):
    (gv, gt, gs), (wv, wt, ws) = got, want
    assert gv.shape == wv.shape and gt.shape == wt.shape and gs.shape == ws.shape
    assert np.array_equal(gv, wv), f"vertexComponent: {int((gv != wv).sum())} of {len(wv)} differ"
    assert np.array_equal(gt, wt), f"triangleComponent: {int((gt != wt).sum())} of {len(wt)} differ"
    bad = np.nonzero(np.any(words(gs) != words(ws), axis=1))[0]
    assert len(bad) == 0, f"components: {len(bad)} of {len(ws)} differ, first {bad[:3]}: {gs[bad[:3]]} vs {ws[bad[:3]]}"


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MC.GOLDEN_SCENES))
def test_restatement_on_the_oracle_meshes(name):
    tri, vertices, faces, vc, tc, stats = labelled(name)
    n_tri, n_vtx, n_comp, three, (n_big, tri_big) = MEASURED[name]
    assert (tri.shape[0], len(vertices), len(stats)) == (n_tri, n_vtx, n_comp)
    order = np.argsort(-stats["noTriangles"].astype(np.int64), kind="stable")[:3]
    assert [(int(c), int(stats["noTriangles"][c]), int(stats["noVertices"][c])) for c in order] == three
    big = stats["noTriangles"] >= 100
    assert (int(big.sum()), int(stats["noTriangles"][big].sum())) == (n_big, tri_big)
    if name == "mesh_s_rgb_yaw":
        assert int((stats["noTriangles"] == 1).sum()) == 28
        single = stats["noVertices"] == 1                           # triangles whose three corners welded to one position
        assert int(single.sum()) >= 1 and np.all(stats["noTriangles"][single] >= 1)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return
    f = faces.astype(np.int64)
    rows, cols = np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]])
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_vtx, n_vtx))
    assert connected_components(graph, directed=False)[0] == n_comp


@pytest.mark.parametrize("name", list(MC.GOLDEN_SCENES))
def test_restatement_properties(name):
    tri, vertices, faces, vc, tc, stats = labelled(name)
    nC = len(stats)
    roots = stats["firstVertex"].astype(np.int64)
    assert roots[0] == 0 and np.all(np.diff(roots) > 0)                                  # numbered by ascending root ...
    assert np.array_equal(vc[roots], np.arange(nC)) and np.array_equal(np.maximum.accumulate(vc)[roots], np.arange(nC))
    seen, first_use = np.unique(tc, return_index=True)                                   # ... = the order of first appearance in the buffer
    assert np.array_equal(seen, np.arange(nC)) and np.all(np.diff(first_use) > 0)
    assert np.array_equal(np.maximum.accumulate(tc)[first_use], np.arange(nC))
    assert int(stats["noTriangles"].sum()) == tri.shape[0] and int(stats["noVertices"].sum()) == len(vertices)
    assert not stats["reserved"].any()
    f = faces.astype(np.int64)
    assert np.array_equal(vc[f[:, 0]], vc[f[:, 1]]) and np.array_equal(vc[f[:, 0]], vc[f[:, 2]]) and np.array_equal(tc, vc[f[:, 0]])
    # the boxes contain their vertices and every face of a box is attained
    key = MK.order_key(bits(vertices))
    lo, hi = MK.order_key(bits(stats["bbMin"])), MK.order_key(bits(stats["bbMax"]))
    assert np.all(lo[vc] <= key) and np.all(key <= hi[vc])
    for axis in range(3):
        assert np.all(np.bincount(vc, weights=key[:, axis] == lo[vc, axis], minlength=nC) > 0)
        assert np.all(np.bincount(vc, weights=key[:, axis] == hi[vc, axis], minlength=nC) > 0)


def test_restatement_hand_cases():
    # two triangles that share one corner only as a VALUE (-0.0 against +0.0): two vertices, two components
    tri = np.zeros((2, 3, 3), F)
    tri[0, 1] = (1, 0, 0); tri[0, 2] = (0, 1, 0)
    tri[1, 0] = (F(-0.0), 0, 0); tri[1, 1] = (-1, 0, 0); tri[1, 2] = (0, -1, 0)
    vertices, faces, first = MI.index(tri)
    vc, tc, stats = MK.components(faces, vertices)
    assert len(vertices) == 6 and vc.tolist() == [0, 0, 0, 1, 1, 1] and tc.tolist() == [0, 1]
    assert stats["firstVertex"].tolist() == [0, 3] and stats["noVertices"].tolist() == [3, 3] and stats["noTriangles"].tolist() == [1, 1]
    # the same corner bit for bit: one component
    tri[1, 0, 0] = 0.0
    vertices, faces, first = MI.index(tri)
    vc, tc, stats = MK.components(faces, vertices)
    assert len(vertices) == 5 and len(stats) == 1 and (int(stats["noVertices"][0]), int(stats["noTriangles"][0])) == (5, 2)
    # a triangle (k, k, k): a component of one vertex; (k, k, j) links k and j
    vc, tc, stats = MK.components(np.array([[0, 1, 2], [3, 3, 3], [4, 4, 5]]), np.zeros((6, 3), F))
    assert vc.tolist() == [0, 0, 0, 1, 2, 2] and tc.tolist() == [0, 1, 2]
    assert stats["noVertices"].tolist() == [3, 1, 2] and stats["noTriangles"].tolist() == [1, 1, 1] and stats["firstVertex"].tolist() == [0, 3, 4]
    # the order of the box is that of the bit patterns: -0.0 < +0.0, and the stored floats are the vertices' own bits
    vertices = np.array([[0.0, -1.0, 2.0], [-0.0, -2.0, 0.0], [0.0, -0.0, -0.0]], F)
    vc, tc, stats = MK.components(np.array([[0, 1, 2]]), vertices)
    assert bits(stats["bbMin"][0]).tolist() == [0x80000000, int(bits(F(-2.0))[0]), 0x80000000]
    assert bits(stats["bbMax"][0]).tolist() == [0, 0x80000000, int(bits(F(2.0))[0])]
    assert MK.order_key(bits(F(-0.0))) + 1 == MK.order_key(bits(F(0.0)))
    assert np.array_equal(MK.order_bits(MK.order_key(bits(vertices))), bits(vertices))
    # a vertex no triangle names is a component of its own; an empty mesh has none
    vc, tc, stats = MK.components(np.array([[0, 2, 3]]), np.zeros((5, 3), F))
    assert vc.tolist() == [0, 1, 0, 0, 2] and stats["noTriangles"].tolist() == [1, 0, 0]
    vc, tc, stats = MK.components(np.zeros((0, 3), np.uint32), np.zeros((0, 3), F))
    assert vc.shape == (0,) and tc.shape == (0,) and stats.shape == (0,) and stats.dtype.itemsize == 40
    assert MK.filtered(np.zeros((0, 3, 3), F), tc, stats, 5).shape == (0, 3, 3)


def test_restatement_of_the_filter():
    tri = np.arange(5 * 9, dtype=F).reshape(5, 3, 3)
    tc = np.array([0, 1, 0, 2, 1])
    stats = np.zeros(3, MK.COMPONENT)
    stats["noTriangles"] = [2, 2, 1]
    assert np.array_equal(MK.filtered(tri, tc, stats, 2), tri[[0, 1, 2, 4]])
    assert np.array_equal(MK.filtered(tri, tc, stats, 0, [0, 1, 1]), tri[[1, 3, 4]])
    assert np.array_equal(MK.filtered(tri, tc, stats, 2, [0, 1, 1]), tri[[1, 4]])
    assert MK.filtered(tri, tc, stats, 3).shape == (0, 3, 3)
    assert MK.largest(stats, 1).tolist() == [1, 0, 0] and MK.largest(stats, 2).tolist() == [1, 1, 0]      # ties: the lower number


def test_binding_header_and_library_declare_the_entry_points(hip_host):
    declared = capi.declared_functions()
    for fn in NEW_FNS:
        assert fn in declared and fn in capi._HOST_IO_SIGS and fn not in capi._SIGS and fn in hip_host.fn
    for method in ("Components", "components_info", "vertex_component", "triangle_component", "components", "FilterComponents", "KeepLargest"):
        assert callable(getattr(Mesh, method))
    text = open(os.path.join(T.ROOT, "include", "itm_debug.h")).read()
    assert f"#define ITM_DEBUG_MESH_COMPONENTS_PER_LANE {DEBUG_MESH_COMPONENTS_PER_LANE} " in text
    assert hip_host.fn["debug_set"](DEBUG_MESH_COMPONENTS_PER_LANE, 0) == 0
    assert "mesh_components.hip" in open(os.path.join(T.ROOT, "infinitam_amd", "csrc", "Makefile")).read()


def test_component_record_layout_matches_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "itm_hip.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   'sizeof(itm_mesh_component), offsetof(itm_mesh_component, noTriangles), offsetof(itm_mesh_component, bbMin),'
                   'offsetof(itm_mesh_component, bbMax)); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [40, 8, 16, 28]
    assert got == [C.sizeof(capi.MeshComponent), capi.MeshComponent.noTriangles.offset, capi.MeshComponent.bbMin.offset, capi.MeshComponent.bbMax.offset]
    d = capi.MESH_COMPONENT_DTYPE
    assert got == [d.itemsize, d.fields["noTriangles"][1], d.fields["bbMin"][1], d.fields["bbMax"][1]] and d == MK.COMPONENT


def test_main_engine_clean_export_compiles(tmp_path):
    src = tmp_path / "save_clean.cpp"
    src.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>::SaveSceneToCleanPLY(const char*, uint32_t);\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_f_rgb, ITMVoxelBlockHash>::SaveSceneToCleanPLY(const char*, uint32_t);\n'
                   'uint32_t f(ITMMesh* m, const uint8_t* keep) { m->Index(); m->Components(); m->FilterComponents(100); m->Index(); m->Components();\n'
                   '  m->FilterComponents(0, keep, m->noComponents); return m->noComponents + m->noTotalTriangles; }\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def debug_set(hip, key, value):
    hip.check(hip.fn["debug_set"](key, value), "debug_set")


def raises_invalid():
    return pytest.raises(capi.ItmError, match=r"\(-1\)")


def meshed(hip, sc, max_triangles=0, frames=None, volume=False):
    ses = MC.fuse(hip, sc, frames=frames)
    m = Mesh(ses.scene, max_triangles)
    m.MeshVolume() if volume else m.MeshScene()
    return ses, m


def labelling(m):
    return m.vertex_component(), m.triangle_component(), m.components()


def restatement_of_the_index(m):
    return MK.components(m.faces(), m.vertices())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mesh_micro", "mesh_f_rgb", "mesh_f", "mesh_s_rgb_yaw"])
def test_hip_components_equal_the_restatement(hip, name):
    ses, m = meshed(hip, MC.SCENES[name])
    m.Index()
    vertices, faces = m.vertices(), m.faces()
    want = MK.components(faces, vertices)
    m.Components()
    nC, rounds = m.components_info()
    print(f"{name}: {len(faces)} triangles, {len(vertices)} vertices, {nC} components, {rounds} union round(s)")
    assert nC == len(want[2]) and rounds >= 1
    if name in MEASURED:
        assert (len(faces), len(vertices), nC) == MEASURED[name][:3]
    same_labelling(labelling(m), want)
    assert np.array_equal(m.faces(), faces) and np.array_equal(bits(m.vertices()), bits(vertices))      # the call leaves the index alone
    debug_set(hip, DEBUG_MESH_COMPONENTS_PER_LANE, 1)                     # the statistics with one atomic per lane
    try:
        m.Components()
        per_lane = labelling(m)
    finally:
        debug_set(hip, DEBUG_MESH_COMPONENTS_PER_LANE, 0)
    same_labelling(per_lane, want)
    debug_set(hip, DEBUG_MESH_INDEX_WEAK_HASH, 1)                         # the components do not care how the index was built
    try:
        m.Index()
        m.Components()
        weak = labelling(m)
        print(f"{name}: weak-hash index, {m.components_info()[1]} union round(s)")
    finally:
        debug_set(hip, DEBUG_MESH_INDEX_WEAK_HASH, 0)
    assert np.array_equal(m.faces(), faces)
    same_labelling(weak, want)


def hook(hip, faces, n_vertices, cap=None):
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    cap = n_vertices if cap is None else cap
    vc = np.full(n_vertices, 0xFFFFFFFF, np.uint32)
    stats = np.zeros(cap, capi.MESH_COMPONENT_DTYPE)
    nC, rounds = C.c_uint32(), C.c_uint32()
    hip.check(hip.fn["debug_mesh_components"](f.ctypes.data_as(C.c_void_p), len(f), n_vertices, vc.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p),
                                              cap, C.byref(nC), C.byref(rounds), None), "debug_mesh_components")
    return vc, stats[:min(nC.value, cap)], nC.value, rounds.value


def strip(n, base=0):
    i = np.arange(n, dtype=np.int64) + base
    return np.stack([i, i + 1, i + 2], axis=1)


def shuffled(faces, n_vertices, seed):
    """vertex numbers and triangle order shuffled"""
    rng = np.random.RandomState(seed)
    return rng.permutation(n_vertices)[faces][rng.permutation(len(faces))]


def graph_cases():
    cases = {}
    cases["strip"] = (shuffled(strip(4096), 4098, 1), 4098)                                                   # diameter ~ 4096, one component
    isolated = 4098 + 3 * np.arange(3000)[:, None] + np.arange(3)[None, :]
    cases["strip_and_isolated"] = (shuffled(np.concatenate([strip(4096), isolated]), 4098 + 9000, 2), 4098 + 9000)
    rim = 1 + 2 * np.arange(2048)
    star = np.stack([np.zeros(2048, np.int64), rim, rim + 1], axis=1)
    cases["star"] = (shuffled(star, 4097, 3), 4097)
    cases["star_hub_last"] = (4096 - star, 4097)                                                              # every link points away from the root
    cases["two_chains"] = (np.concatenate([strip(2048), strip(2048, 2050), [[2049, 4099, 4099]]]), 4100)      # joined by the LAST triangle only
    cases["degenerate"] = (np.array([[5, 5, 5], [1, 1, 3], [3, 1, 1], [0, 0, 0], [7, 2, 7], [2, 2, 6], [4, 4, 4]]), 9)
    cases["unreferenced"] = (shuffled(strip(300), 302, 4) * 3 + 1, 3 * 302 + 5)
    cases["no_triangles"] = (np.zeros((0, 3), np.int64), 5)
    cases["one_triangle"] = (np.array([[2, 0, 1]]), 3)
    cases["one_vertex"] = (np.array([[0, 0, 0]]), 1)
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(graph_cases()))
def test_hip_hook_on_adversarial_graphs(hip, case):
    faces, nV = graph_cases()[case]
    wv, wt, ws = MK.components(faces, np.zeros((nV, 3), F))           # no positions: the box stays zero
    for per_lane in (0, 1):
        debug_set(hip, DEBUG_MESH_COMPONENTS_PER_LANE, per_lane)
        try:
            vc, stats, nC, rounds = hook(hip, faces, nV)
        finally:
            debug_set(hip, DEBUG_MESH_COMPONENTS_PER_LANE, 0)
        print(f"{case}: {len(faces)} triangles, {nV} vertices, {nC} components, {rounds} union round(s)")
        assert nC == len(ws) and rounds >= 1
        assert np.array_equal(vc, wv), f"{int((vc != wv).sum())} of {nV} differ"
        assert np.array_equal(words(stats), words(ws))
    if case == "strip":
        assert nC == 1
    if case == "two_chains":
        assert nC == 1 and len(MK.components(faces[:-1], np.zeros((nV, 3), F))[2]) == 2
    if case == "strip_and_isolated":
        assert nC == 3001
        vc, stats, nC2, _ = hook(hip, faces, nV, cap=7)                # a short component array: the first 7 records, the full count
        assert nC2 == nC and np.array_equal(words(stats), words(ws[:7])) and np.array_equal(vc, wv)


@pytest.mark.gpu
def test_hip_hook_refuses_an_index_out_of_range(hip):
    with raises_invalid():
        hook(hip, np.array([[0, 1, 2], [2, 3, 4]]), 4)
    assert hook(hip, np.zeros((0, 3), np.int64), 0)[2:] == (0, 0)      # no vertices: no components, no error


# the soup's files as itm_mesh_write_obj / itm_mesh_write_stl write them (ITMMesh::WriteOBJ / WriteSTL)
def obj_text(tri):
    v = np.asarray(tri, F).reshape(-1, 3).astype(np.float64)
    out = ["v %f %f %f\n" % (p[0], p[1], p[2]) for p in v]
    out += ["f %d %d %d\n" % (3 * i + 3, 3 * i + 2, 3 * i + 1) for i in range(len(v) // 3)]
    return "".join(out).encode()


def stl_bytes(tri):
    t = np.ascontiguousarray(tri, "<f4").reshape(-1, 3, 3)
    rec = np.zeros(len(t), np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    rec["v"] = t[:, ::-1]
    return b" " * 80 + np.uint32(len(t)).tobytes() + rec.tobytes()


def assert_files(m, tmp_path, tri, normals, colours, vertices, faces, vertex_normals, vertex_colours):
    """the five files of the handle equal the Python writers' bytes"""
    p = lambda ext: str(tmp_path / ("f." + ext))
    m.WritePLY(p("ply")); m.WriteOBJ(p("obj")); m.WriteSTL(p("stl")); m.WriteIndexedPLY(p("i.ply")); m.WriteIndexedOBJ(p("i.obj"))
    assert open(p("ply"), "rb").read() == MT.ply_bytes(tri, normals, colours)
    assert open(p("obj"), "rb").read() == obj_text(tri)
    assert open(p("stl"), "rb").read() == stl_bytes(tri)
    assert open(p("i.ply"), "rb").read() == MI.ply_bytes_indexed(vertices, faces, vertex_normals, vertex_colours)
    assert open(p("i.obj"), "rb").read() == MI.obj_text_indexed(vertices, faces)


def assert_behaves_as_meshed(m, sc, packed, normals_before, colours_before, kept_mask, want_sizes, tmp_path=None):
    """after a filter the handle is a mesh of exactly the packed triangles: stale marks, then attributes, index, components, files"""
    assert m.info()[0] == len(packed) and np.array_equal(bits(m.triangles()), bits(packed))
    for call in (m.normals, m.index_info, m.vertices, m.components_info, m.components, m.vertex_normals, lambda: m.FilterComponents(0), m.Components):
        with raises_invalid():
            call()
    what = what_of(sc)
    m.ComputeAttributes(what)
    normals = m.normals()
    assert np.array_equal(bits(normals), bits(normals_before[kept_mask]))          # functions of the position alone
    colours = None
    if sc.colour:
        colours = m.colours()
        assert np.array_equal(colours, colours_before[kept_mask])
    m.Index()
    vertices, faces, first = m.vertices(), m.faces(), m.first()
    wv, wf, wfirst = MI.index(packed)
    assert np.array_equal(first, wfirst) and np.array_equal(faces, wf) and np.array_equal(bits(vertices), bits(wv))
    m.ComputeIndexedAttributes(what)
    vn = m.vertex_normals()
    assert np.array_equal(bits(vn), bits(normals.reshape(-1, 3)[first.astype(np.int64)]))
    vcol = m.vertex_colours() if sc.colour else None
    if sc.colour:
        assert np.array_equal(vcol, colours.reshape(-1, 4)[first.astype(np.int64)])
    m.Components()
    got = labelling(m)
    same_labelling(got, MK.components(faces, vertices))
    assert [(int(s["noTriangles"]), int(s["noVertices"])) for s in got[2]] == want_sizes
    if tmp_path is not None:
        assert_files(m, tmp_path, packed, normals, colours, vertices, faces, vn, vcol)


def attributes_and_labelling(m, sc):
    """(triangles, normals, colours | None, labelling) of a freshly meshed handle: attributes, index and components computed"""
    tri = m.triangles()
    m.ComputeAttributes(what_of(sc))
    normals, colours = m.normals(), (m.colours() if sc.colour else None)
    m.Index()
    m.Components()
    lab = labelling(m)
    same_labelling(lab, restatement_of_the_index(m))
    return tri, normals, colours, lab


@pytest.mark.gpu
@pytest.mark.parametrize("per_vertex", [0, 1])
def test_hip_filter_drops_the_fragments(hip, tmp_path, per_vertex):
    """mesh_f_rgb, minTriangles = 100: 3 of 93 components, 70 799 of 71 311 triangles; block-staged attributes and key 26"""
    sc = MC.SCENES["mesh_f_rgb"]
    debug_set(hip, DEBUG_MESH_ATTR_PER_VERTEX, per_vertex)
    try:
        ses, m = meshed(hip, sc)
        tri, normals, colours, (vc, tc, stats) = attributes_and_labelling(m, sc)
        assert (tri.shape[0], len(stats)) == (71311, 93)
        assert m.FilterComponents(100) == (70799, 3)
        assert m.info()[0] == 70799
        kept = MK.kept_components(stats, 100)[tc]
        packed = MK.filtered(tri, tc, stats, 100)
        sizes = [(int(s["noTriangles"]), int(s["noVertices"])) for s in stats[MK.kept_components(stats, 100)]]
        assert sizes == [(11809, 6913), (58848, 30261), (142, 148)]
        assert_behaves_as_meshed(m, sc, packed, normals, colours, kept, sizes, tmp_path)
    finally:
        debug_set(hip, DEBUG_MESH_ATTR_PER_VERTEX, 0)


@pytest.mark.gpu
def test_hip_filter_masks_largest_all_and_nothing(hip, tmp_path):
    sc = MC.SCENES["mesh_f_rgb"]
    ses, m = meshed(hip, sc)
    tri, normals, colours, (vc, tc, stats) = attributes_and_labelling(m, sc)
    sizes = lambda keep: [(int(s["noTriangles"]), int(s["noVertices"])) for s in stats[keep]]

    def again():
        m.MeshScene(); m.Index(); m.Components()

    # a mask that selects component 0 alone
    keep = np.zeros(len(stats), np.uint8); keep[0] = 1
    assert m.FilterComponents(0, keep) == (11809, 1)
    assert_behaves_as_meshed(m, sc, MK.filtered(tri, tc, stats, 0, keep), normals, colours, tc == 0, [(11809, 6913)])
    # the mask and the threshold together: nothing of components 0 .. 5 has 20 000 triangles
    again()
    keep = np.zeros(len(stats), np.uint8); keep[:6] = 1
    assert m.FilterComponents(20000, keep) == (0, 0) and m.info()[0] == 0
    # the largest one
    again()
    assert m.KeepLargest(1) == (58848, 1)
    assert_behaves_as_meshed(m, sc, MK.filtered(tri, tc, stats, 0, MK.largest(stats, 1)), normals, colours, tc == 6, [(58848, 30261)])
    again()
    assert m.KeepLargest(2) == (58848 + 11809, 2)
    assert np.array_equal(bits(m.triangles()), bits(MK.filtered(tri, tc, stats, 0, MK.largest(stats, 2))))
    # a threshold above every size: a valid empty mesh, empty files
    again()
    assert m.FilterComponents(58849) == (0, 0) and m.info()[0] == 0 and m.triangles().shape == (0, 3, 3)
    empty = np.zeros((0, 3, 3), F)
    assert_behaves_as_meshed(m, sc, empty, normals, colours, np.zeros(len(tri), bool), [], tmp_path)
    assert m.components_info() == (0, 0) and m.FilterComponents(0) == (0, 0)
    # threshold 0, no mask: the identity -- and stale all the same
    again()
    assert m.FilterComponents() == (len(tri), len(stats))
    everything = np.ones(len(tri), bool)
    assert_behaves_as_meshed(m, sc, tri, normals, colours, everything, sizes(np.ones(len(stats), bool)))


@pytest.mark.gpu
def test_hip_filter_of_a_full_buffer(hip):
    sc = MC.SCENES["mesh_f_rgb"]
    ses, m = meshed(hip, sc, max_triangles=1000)
    assert m.info() == (999, 1000)
    tri, normals, colours, (vc, tc, stats) = attributes_and_labelling(m, sc)
    assert tri.shape[0] == 999 and int(stats["noTriangles"].sum()) == 999 and len(stats) > 1
    big = int(np.sort(stats["noTriangles"])[-2])                          # keeps the two largest (and what ties with the second)
    keep = MK.kept_components(stats, big)
    print(f"full buffer: {len(stats)} components of {sorted(stats['noTriangles'].tolist())[-5:]} triangles at most, threshold {big}")
    assert m.FilterComponents(big) == (int(stats["noTriangles"][keep].sum()), int(keep.sum()))
    sizes = [(int(s["noTriangles"]), int(s["noVertices"])) for s in stats[keep]]
    assert_behaves_as_meshed(m, sc, MK.filtered(tri, tc, stats, big), normals, colours, keep[tc], sizes)


@pytest.mark.gpu
def test_hip_filter_of_a_dense_mesh(hip, tmp_path):
    sc = MC.DENSE
    ses, m = meshed(hip, sc, volume=True)
    tri, normals, colours, (vc, tc, stats) = attributes_and_labelling(m, sc)
    assert tri.shape[0] > 1000 and len(stats) > 1
    big = int(np.sort(stats["noTriangles"])[-1])                          # the largest component alone (and what ties with it)
    keep = MK.kept_components(stats, big)
    print(f"dense: {tri.shape[0]} triangles, {len(stats)} components, the largest {big} triangles")
    assert 0 < int(stats["noTriangles"][keep].sum()) < tri.shape[0]
    assert m.FilterComponents(big) == (int(stats["noTriangles"][keep].sum()), int(keep.sum()))
    sizes = [(int(s["noTriangles"]), int(s["noVertices"])) for s in stats[keep]]
    assert_behaves_as_meshed(m, sc, MK.filtered(tri, tc, stats, big), normals, colours, keep[tc], sizes, tmp_path)
    # itm_mesh_scene leaves a dense scene empty: an empty index, no components, nothing to filter, no error
    m.MeshScene(); m.Index(); m.Components()
    assert m.components_info() == (0, 0) and m.components().shape == (0,) and m.vertex_component().shape == (0,) and m.FilterComponents(1) == (0, 0)


@pytest.mark.gpu
def test_hip_components_stale_and_refused(hip):
    sc = MC.SCENES["mesh_micro"]
    ses = MC.fuse(hip, sc)
    m = Mesh(ses.scene)

    def assert_refused(with_the_call=False):
        for call in (m.components_info, m.vertex_component, m.triangle_component, m.components, lambda: m.FilterComponents(10), lambda: m.KeepLargest(1)):
            with raises_invalid():
                call()
        if with_the_call:
            with raises_invalid():
                m.Components()

    assert_refused(True)                                                  # never meshed
    m.MeshScene()
    assert_refused(True)                                                  # meshed, no index
    m.Index()
    assert_refused()                                                      # an index, no components: the readers and the filter refuse
    m.Components()
    nC = m.components_info()[0]
    assert nC == 99
    for bad in (np.ones(nC - 1, np.uint8), np.ones(nC + 1, np.uint8), np.ones(0, np.uint8)):
        with raises_invalid():
            m.FilterComponents(0, bad)
    assert m.components_info()[0] == nC and m.info()[0] == 72769          # a refused filter changes nothing
    m.Index()
    assert_refused()                                                      # stale after a new index
    m.Components()
    m.MeshScene()
    assert_refused(True)                                                  # stale after a re-mesh
    m.Index(); m.Components()
    assert m.FilterComponents(100) == (72204, 2)
    assert_refused(True)                                                  # stale after a filter, with the index
    m.MeshVolume(); m.Index(); m.Components()
    assert m.components_info()[0] == nC


@pytest.mark.gpu
def test_hip_components_lifecycle(hip):
    """two more fused frames, then re-mesh, re-index, re-label (a filter in between): equal to a fresh session"""
    sc = MC.SCENES["mesh_micro"]
    ses, m = meshed(hip, sc)
    m.Index(); m.Components()
    assert m.FilterComponents(100) == (72204, 2)
    ses.frame(3); ses.frame(4)
    m.MeshScene(); m.Index(); m.Components()
    fses, fm = meshed(hip, sc, frames=5)
    fm.Index(); fm.Components()
    assert np.array_equal(bits(m.triangles()), bits(fm.triangles())) and m.info()[0] != 72769
    same_labelling(labelling(m), labelling(fm))
    same_labelling(labelling(m), restatement_of_the_index(m))


def live(be):
    """(live allocations, live bytes) of the library, process-wide.  The figures are compared with each other, so nothing else may free
    memory in between: sessions and meshes that earlier tests left to the cycle collector are collected first."""
    gc.collect()
    out = (C.c_int64 * 3)()
    be.check(be.fn["debug_memory"](out), "debug_memory")
    return tuple(out)[:2]


@pytest.mark.gpu
def test_hip_components_memory(hip):
    sc = MC.SCENES["mesh_micro"]
    debug_set(hip, DEBUG_FAIL_ALLOCATION, 0)
    ses = MC.fuse(hip, sc)
    start = live(hip)
    m = Mesh(ses.scene)
    m.MeshScene(); m.Index()
    indexed = live(hip)
    want = restatement_of_the_index(m)
    # every allocation of the labelling may fail: the call reports it, keeps none of the new buffers, and the handle stays usable
    failures = 0
    for n in range(1, 20):
        debug_set(hip, DEBUG_FAIL_ALLOCATION, n)
        try:
            m.Components()
        except capi.ItmError as e:
            assert "(-2)" in str(e)
            failures += 1
            assert live(hip) == indexed, f"allocation {n}: the failed call kept memory"
            with raises_invalid():
                m.components_info()
            assert m.index_info() == (len(want[0]), len(want[1]))
            continue
        finally:
            debug_set(hip, DEBUG_FAIL_ALLOCATION, 0)
        break
    assert failures == 8                                                  # the eight buffers of a labelling
    same_labelling(labelling(m), want)
    labelled_bytes = live(hip)
    assert labelled_bytes[0] == indexed[0] + 8
    m.Components()                                                        # again: nothing grows
    assert live(hip) == labelled_bytes
    # the filter's buffers: had before the mesh is touched, or the mesh and its labelling stay as they were
    tri = m.triangles()
    for n in (1, 2, 3):
        debug_set(hip, DEBUG_FAIL_ALLOCATION, n)
        try:
            with pytest.raises(capi.ItmError, match=r"\(-2\)"):
                m.FilterComponents(100)
        finally:
            debug_set(hip, DEBUG_FAIL_ALLOCATION, 0)
        assert live(hip) == labelled_bytes and m.components_info()[0] == 99 and np.array_equal(bits(m.triangles()), bits(tri))
    assert m.FilterComponents(100) == (72204, 2)
    m.close()
    assert live(hip) == start


@pytest.mark.gpu
def test_hip_components_are_deterministic(hip):
    sc = MC.SCENES["mesh_s_rgb_yaw"]
    ses, m = meshed(hip, sc)
    m.Index(); m.Components()
    a = labelling(m)
    assert (len(a[1]), len(a[0]), len(a[2])) == MEASURED["mesh_s_rgb_yaw"][:3]
    m.Components()
    same_labelling(labelling(m), a)
    m2 = Mesh(ses.scene)
    m2.MeshScene(); m2.Index(); m2.Components()
    same_labelling(labelling(m2), a)
    print(f"mesh_s_rgb_yaw: {m.components_info()[1]} and {m2.components_info()[1]} union round(s)")
