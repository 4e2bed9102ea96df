"""Fixed-point smoothing of the indexed mesh (include/itm_hip.h: itm_mesh_smooth / itm_mesh_smooth_default_config; include/itm_debug.h:
itm_debug_mesh_smooth, key 31).

The smoothing is defined on the index in integers -- neighbour entries of the proper triangles, positions quantised once, every pass the
rounded mean offset times a Q16 factor, dequantised once -- so everything is compared bit for bit, as whole arrays:
  * CPU: the numpy restatement (tests/mesh_smooth_terms.py) on hand cases with values worked out by hand, on a noisy icosphere (the
    figures of the prototype: Taubin keeps the volume, Laplacian shrinks), on the oracle's meshes (pinned vertices, translation by whole
    quanta, statistics, the measured numbers of irregular vertices); the boundary.
  * GPU: the hook against the restatement (vertices, flags, statistics) on the hand cases, random face soups, a double cone whose apex
    rows span many waves, sizes around the wave and the workgroup, all again as a scatter (key 31); refusals; the product on four
    scenes -- vertices, soup, state, attributes at the new positions, files --, a dense and a full mesh, failed allocations, determinism."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import mesh_attr_cases as MC
import mesh_attr_terms as MT
import mesh_index_terms as MI
import mesh_smooth_terms as MS
from infinitam_amd import capi
from infinitam_amd.capi import MESH_COLOURS, MESH_NORMALS, Mesh
from mesh_smooth_terms import bits
from test_mesh_attributes import restated, what_of
from test_mesh_components import assert_files, debug_set, live, meshed, raises_invalid

F = np.float32
DEBUG_MESH_ATTR_PER_VERTEX = 26          # include/itm_debug.h
DEBUG_FAIL_ALLOCATION = 28
DEBUG_MESH_SMOOTH_SCATTER = 31
NEW_FNS = ("mesh_smooth", "mesh_smooth_default_config", "debug_mesh_smooth")
# measured on the oracle's meshes with the restatement's topology: unique vertices, irregular, isolated, max entries
MEASURED = {
    "mesh_micro": (38875, 6052, 0, 18),
    "mesh_f_rgb": (38030, 5910, 0, 18),
    "mesh_s_rgb_yaw": (404553, 40545, 23, 40),
}
_indexed = {}


def indexed(name):
    """(vertices, faces) of the oracle's mesh of a golden scene"""
    if name not in _indexed:
        vertices, faces, first = MI.index(restated(name)[0])
        _indexed[name] = (vertices, faces)
    return _indexed[name]


def same(got, want, what=""):
    """(vertices, flags, stats) bit for bit"""
    gv, gf, gs = got
    wv, wf, ws = want
    assert gs == ws, f"{what}: statistics {gs} vs {ws}"
    assert np.array_equal(gf, wf), f"{what}: {int((gf != wf).sum())} of {len(wf)} flags differ"
    bad = np.nonzero(np.any(bits(gv).reshape(-1, 3) != bits(wv).reshape(-1, 3), axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(wv)} vertices differ, first {bad[:3]}: {gv[bad[:3]]} vs {wv[bad[:3]]}"


# ---- CPU: hand cases ------------------------------------------------------------------------------------------------------------------

TETRA_V = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0, 0, 5]], F)
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
ONE = dict(quantum=1.0)                  # one unit per quantum: the integers are the coordinates


def test_hand_tetrahedron_lands_on_the_rounded_mean():
    out, flags, stats = MS.smooth(TETRA_V, TETRA_F, MS.config(1, 1.0, 1.0, **ONE))
    # mean of the other three, half up: (1, 4/3, 5/3), (0, 4/3, 5/3), (1, 0, 5/3), (1, 4/3, 0)
    assert out.tolist() == [[1, 1, 2], [0, 1, 2], [1, 0, 2], [1, 1, 0]]
    assert flags.tolist() == [0, 0, 0, 0] and stats == dict(noVertices=4, noMoving=4, noIrregular=0, noIsolated=0, maxEntries=6, steps=1)


def test_hand_single_triangle_pinned_and_free():
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 6, 0]], F)
    f = np.array([[0, 1, 2]])
    out, flags, stats = MS.smooth(v, f, MS.config(7, 1.0, 1.0, **ONE))
    assert np.array_equal(bits(out), bits(v)) and flags.tolist() == [1, 1, 1]
    assert stats == dict(noVertices=3, noMoving=0, noIrregular=3, noIsolated=0, maxEntries=2, steps=7)
    out, flags, stats = MS.smooth(v, f, MS.config(1, 1.0, 1.0, pin=False, **ONE))
    assert out.tolist() == [[2, 3, 0], [0, 3, 0], [2, 0, 0]] and flags.tolist() == [1, 1, 1] and stats["noMoving"] == 3


def test_hand_fan_and_three_triangles_on_an_edge():
    v, f = MS.fan(6, closed=True)
    q = F(1.0 / 1024)
    out, flags, stats = MS.smooth(v, f, MS.config(1, 1.0, 1.0, quantum=q))
    assert flags.tolist() == [0, 1, 1, 1, 1, 1, 1] and stats["noMoving"] == 1 and stats["maxEntries"] == 12
    assert np.array_equal(bits(out[1:]), bits(v[1:]))                    # the rim is a border: pinned
    x = [[int(c) for c in np.rint(p.astype(np.float64) / np.float64(q))] for p in v]
    centre = []
    for axis in range(3):
        a = 2 * sum(x[k][axis] for k in range(1, 7)) - 12 * x[0][axis]   # every rim vertex twice
        centre.append(x[0][axis] + (2 * a + 12) // 24)                   # lambda = 1: s = d
    assert x[0][2] == 256 and centre[2] == 0
    assert out[0].tolist() == [F(np.float64(c) * np.float64(q)) for c in centre]
    # an open fan: the centre is on the border too
    v, f = MS.fan(6, closed=False)
    assert MS.smooth(v, f, MS.config(1))[1].tolist() == [1] * 7
    # three triangles on the edge (0, 1): its ends see each other three times, the others see everything once
    out, flags, stats = MS.smooth(np.arange(15, dtype=F).reshape(5, 3), np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]]), MS.config(3, **ONE))
    assert flags.tolist() == [1] * 5 and stats["noIrregular"] == 5 and stats["noMoving"] == 0 and stats["maxEntries"] == 6


def test_hand_degenerate_faces_and_unnamed_vertices():
    v = (np.arange(21, dtype=F).reshape(7, 3) * F(0.37)).astype(F)
    f = np.array([[0, 0, 0], [1, 1, 2], [3, 4, 5], [3, 3, 4], [5, 5, 5]])
    out, flags, stats = MS.smooth(v, f, MS.config(5, pin=False, quantum=0.01))
    assert flags.tolist() == [2, 2, 2, 1, 1, 1, 2]                       # 0, 1, 2: degenerate faces only; 6: no face names it
    assert stats == dict(noVertices=7, noMoving=3, noIrregular=3, noIsolated=4, maxEntries=2, steps=5)
    assert np.array_equal(bits(out[[0, 1, 2, 6]]), bits(v[[0, 1, 2, 6]])) and not np.array_equal(out[3:6], v[3:6])


def test_hand_half_up_roundings_below_zero():
    v = np.array([[0, 0, 0], [-4, -5, -6], [0, 0, 0]], F)
    f = np.array([[0, 1, 2]])
    # vertex 0: n = 2, a = (-4, -5, -6): a / n = -2 (exact), -2.5 (a half: up, to -2), -3 (exact)  ->  d = (-2, -2, -3)
    out = MS.smooth(v, f, MS.config(1, 1.0, 1.0, pin=False, **ONE))[0]
    assert out.tolist() == [[-2, -2, -3], [0, 0, 0], [-2, -2, -3]]
    # lambda = 0.5: f d / 65536 = (-1, -1, -1.5) -> s = (-1, -1, -1): the half goes up.  Vertex 1: d = (4, 5, 6) -> s = (2, 3, 3)
    out = MS.smooth(v, f, MS.config(1, 0.5, 0.5, pin=False, **ONE))[0]
    assert out.tolist() == [[-1, -1, -1], [-2, -2, -3], [-1, -1, -1]]
    # a negative factor: d = -3, f = -0.5 -> 1.5 -> 2
    assert MS.smooth(v, f, MS.config(1, -0.5, -0.5, pin=False, **ONE))[0][0].tolist() == [1, 1, 2]
    # the second pass uses mu
    two = MS.smooth(v, f, MS.config(2, 1.0, 0.0, pin=False, **ONE))[0]
    assert np.array_equal(two, MS.smooth(v, f, MS.config(1, 1.0, 1.0, pin=False, **ONE))[0])
    # the clamp: at the limit a vertex stays inside
    far = np.array([[2.0 ** 30, 0, 0], [2.0 ** 30, 0, 0], [-2.0 ** 30, 0, 0]], F)
    assert MS.smooth(far, f, MS.config(1, -1.0, -1.0, pin=False, **ONE))[0][:, 0].tolist() == [2.0 ** 30, 2.0 ** 30, -2.0 ** 30]


def test_hand_minus_zero_steps_zero_and_empty():
    v = np.array([[-0.0, 1, 2], [4, -0.0, 0], [0, 6, -0.0]], F)
    f = np.array([[0, 1, 2]])
    out = MS.smooth(v, f, MS.config(4, **ONE))[0]
    assert np.array_equal(bits(out), bits(v)) and int((bits(out) == 0x80000000).sum()) == 3
    assert int((bits(MS.smooth(v, f, MS.config(4, pin=False, **ONE))[0]) == 0x80000000).sum()) == 0     # a moving vertex is rewritten
    out, flags, stats = MS.smooth(TETRA_V * F(np.nan), TETRA_F, MS.config(0))     # steps == 0: the statistics only, positions are not read
    assert stats == dict(noVertices=4, noMoving=4, noIrregular=0, noIsolated=0, maxEntries=6, steps=0) and np.isnan(out).all()
    out, flags, stats = MS.smooth(np.zeros((0, 3), F), np.zeros((0, 3), np.int64), MS.config(3))
    assert out.shape == (0, 3) and flags.shape == (0,) and not any(stats.values())
    out, flags, stats = MS.smooth(np.ones((1, 3), F), np.zeros((0, 3), np.int64), MS.config(3))
    assert flags.tolist() == [2] and stats == dict(noVertices=1, noMoving=0, noIrregular=0, noIsolated=1, maxEntries=0, steps=3)


LEAST_Q = F(1.0) - F(2.0 ** -24)           # the float below 1


def refusals():
    """name -> (vertices, faces, cfg): every one is refused"""
    ok = (TETRA_V, TETRA_F)
    # Coordinates beyond the limit.  No pair of floats has rint(v / q) == 2^30 + 1: with v = m 2^e and q = k 2^g, m and k below 2^24
    # and k of b bits, a quotient near 2^30 needs m 2^(e-g) >= k 2^30 >= 2^(29+b), so m 2^(e-g) is a multiple of 2^(6+b) and so is
    # k 2^30 (b <= 24); their difference would have to lie within k / 2 of k < 2^b: there is no such multiple.  The same count gives
    # 2^30 + 64 as the least that can be reached, by q = 1 - 2^-24 under v = 2^30 (quotient 2^30 + 64.000004): the very float that
    # quantum 1 accepts (test_restatement_accepts_the_limits, the hook's "clamp" case).  At quantum 1 the next float is 2^30 + 128.
    big = TETRA_V.copy(); big[2, 1] = F(2.0 ** 30 + 128)
    least = TETRA_V.copy(); least[1, 2] = F(-2.0 ** 30)
    nan = TETRA_V.copy(); nan[3, 0] = np.nan
    inf = TETRA_V.copy(); inf[0, 2] = -np.inf
    return {
        "steps": ok + (dict(MS.config(1, **ONE), steps=MS.MAX_STEPS + 1),), "steps_garbage": ok + (dict(MS.config(1, **ONE), steps=0xffffffff),),
        "lambda": ok + (dict(MS.config(1, **ONE), lambdaQ16=65537),), "mu": ok + (dict(MS.config(1, **ONE), muQ16=-65537),),
        "quantum_zero": ok + (MS.config(1, quantum=0.0),), "quantum_negative": ok + (MS.config(1, quantum=-1.0),),
        "quantum_nan": ok + (MS.config(1, quantum=np.nan),), "quantum_inf": ok + (MS.config(1, quantum=np.inf),),
        "reserved": ok + (MS.config(1, reserved=(0, 0, 1), **ONE),), "flags": ok + (MS.config(1, pin=3, **ONE),),
        "face_index": (TETRA_V, np.array([[0, 1, 2], [1, 2, 4]]), MS.config(1, **ONE)),
        "coordinate_beyond": (big, TETRA_F, MS.config(1, **ONE)), "coordinate_least_beyond": (least, TETRA_F, MS.config(1, quantum=LEAST_Q)),
        "coordinate_nan": (nan, TETRA_F, MS.config(1, **ONE)),
        "coordinate_inf": (inf, TETRA_F, MS.config(1, **ONE)),
    }


@pytest.mark.parametrize("case", list(refusals()))
def test_restatement_refuses(case):
    v, f, cfg = refusals()[case]
    with pytest.raises(MS.Refused):
        MS.smooth(v, f, cfg)


def test_restatement_accepts_the_limits():
    assert np.rint(np.float64(F(-2.0 ** 30)) / np.float64(LEAST_Q)) == -(2.0 ** 30 + 64)               # "coordinate_least_beyond" is what it says
    MS.check_config(dict(MS.config(1, **ONE), steps=MS.MAX_STEPS))
    assert MS.MAX_STEPS == 65536 and f"#define ITM_MESH_SMOOTH_MAX_STEPS {MS.MAX_STEPS}\n" in open(os.path.join(T.ROOT, "include", "itm_hip.h")).read()
    at = TETRA_V.copy(); at[2, 1] = F(2.0 ** 30); at[1, 0] = F(-2.0 ** 30)
    out = MS.smooth(at, TETRA_F, dict(MS.config(2, **ONE), lambdaQ16=65536, muQ16=-65536))[0]
    assert np.all(np.abs(out) <= 2.0 ** 30)


# ---- CPU: the prototype's figures -------------------------------------------------------------------------------------------------------

SPHERE_Q = 0.005 / 1024


def radius_std(v):
    return float(np.linalg.norm(np.asarray(v, np.float64), axis=1).std())


def test_icosphere_taubin_keeps_the_volume_and_laplacian_shrinks():
    v, f = MS.noisy_icosphere()
    assert v.shape == (2562, 3) and f.shape == (5120, 3)
    vol0, std0 = MS.enclosed_volume(v, f), radius_std(v)
    out, flags, stats = MS.smooth(v, f, MS.config(quantum=SPHERE_Q))
    assert stats == dict(noVertices=2562, noMoving=2562, noIrregular=0, noIsolated=0, maxEntries=12, steps=20) and not flags.any()
    vol, std = MS.enclosed_volume(out, f), radius_std(out)
    print(f"taubin: radius std {std0:.4f} -> {std:.4f}, volume {100 * (vol / vol0 - 1):+.2f} %")
    assert std < 0.5 * std0 and abs(vol / vol0 - 1) < 0.01
    lap = MS.smooth(v, f, MS.config(20, 0.5, 0.5, quantum=SPHERE_Q))[0]
    print(f"laplacian: radius std {radius_std(lap):.4f}, volume {100 * (MS.enclosed_volume(lap, f) / vol0 - 1):+.2f} %")
    assert MS.enclosed_volume(lap, f) / vol0 - 1 < -0.05


def test_icosphere_with_a_hole():
    v, f = MS.noisy_icosphere()
    around = np.any(f == 0, axis=1)                                       # vertex 0 is one of the icosahedron's twelve: five triangles
    ring = np.setdiff1d(np.unique(f[around]), [0])
    assert int(around.sum()) == 5 and len(ring) == 5
    out, flags, stats = MS.smooth(v, f[~around], MS.config(quantum=SPHERE_Q))
    assert flags[0] == 2 and np.all(flags[ring] == 1) and int(flags.astype(bool).sum()) == 6
    assert stats["noIrregular"] == 5 and stats["noIsolated"] == 1 and stats["noMoving"] == 2562 - 6
    pinned = np.concatenate([[0], ring])
    assert np.array_equal(bits(out[pinned]), bits(v[pinned]))
    moved = np.setdiff1d(np.arange(2562), pinned)
    assert np.all(np.any(bits(out[moved]) != bits(v[moved]), axis=1))
    # with the flag clear the ring moves, the centre does not
    out = MS.smooth(v, f[~around], MS.config(quantum=SPHERE_Q, pin=False))[0]
    assert np.array_equal(bits(out[0]), bits(v[0])) and np.all(np.any(bits(out[ring]) != bits(v[ring]), axis=1))


# ---- CPU: the oracle's meshes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MC.GOLDEN_SCENES))
def test_restatement_on_the_oracle_meshes(name):
    vertices, faces = indexed(name)
    nV = len(vertices)
    steps = 2 if name == "mesh_s_rgb_yaw" else 4
    cfg = MS.config(steps, quantum=MC.SCENES[name].voxelSize / 1024)
    out, flags, stats = MS.smooth(vertices, faces, cfg)
    irregular, isolated = (flags & 1) != 0, (flags & 2) != 0
    print(f"{name}: {stats}")
    assert (nV, stats["noIrregular"], stats["noIsolated"], stats["maxEntries"]) == MEASURED[name]
    # the statistics add up: a vertex is isolated, pinned (irregular) or moving; an isolated vertex has no entry, so it is not irregular
    assert stats["noVertices"] == nV and stats["steps"] == steps and not np.any(irregular & isolated)
    assert stats["noMoving"] + stats["noIrregular"] + stats["noIsolated"] == nV
    assert (int(irregular.sum()), int(isolated.sum())) == (stats["noIrregular"], stats["noIsolated"])
    still = irregular | isolated
    assert np.array_equal(bits(out[still]), bits(vertices[still]))
    assert np.any(bits(out[~still]) != bits(vertices[~still]))
    free = MS.smooth(vertices, faces, dict(cfg, flags=0))[2]
    assert free["noMoving"] == nV - stats["noIsolated"] and free["noIrregular"] == stats["noIrregular"]
    # translation by whole quanta: with a power of two as the quantum and the coordinates on its grid every sum is exact
    q = 2.0 ** -18
    snapped = (np.rint(vertices.astype(np.float64) / q) * q).astype(F)
    shift = np.array([3, -70000, 1 << 20], np.float64) * q
    moved = (snapped.astype(np.float64) + shift).astype(F)
    assert np.array_equal(moved.astype(np.float64), snapped.astype(np.float64) + shift)                # representable
    a = MS.smooth(snapped, faces, dict(cfg, quantum=F(q)))[0]
    b = MS.smooth(moved, faces, dict(cfg, quantum=F(q)))[0]
    assert np.array_equal(b.astype(np.float64), a.astype(np.float64) + shift)


# ---- CPU: build and binding -----------------------------------------------------------------------------------------------------------

def test_binding_header_and_library_declare_the_entry_points(hip_host):
    declared = capi.declared_functions()
    for fn in NEW_FNS:
        assert fn in declared and fn in capi._HOST_IO_SIGS and fn not in capi._SIGS and fn in hip_host.fn
    assert callable(Mesh.Smooth)
    text = open(os.path.join(T.ROOT, "include", "itm_debug.h")).read()
    assert f"#define ITM_DEBUG_MESH_SMOOTH_SCATTER {DEBUG_MESH_SMOOTH_SCATTER} " in text
    assert hip_host.fn["debug_set"](DEBUG_MESH_SMOOTH_SCATTER, 0) == 0
    assert "mesh_smooth.hip" in open(os.path.join(T.ROOT, "infinitam_amd", "csrc", "Makefile")).read()
    cfg = capi.MeshSmoothConfig()
    assert hip_host.fn["mesh_smooth_default_config"](0.005, C.byref(cfg)) == 0                      # host only: no device is touched
    assert (cfg.steps, cfg.lambdaQ16, cfg.muQ16, cfg.flags, tuple(cfg.reserved)) == (20, 32768, -34734, 1, (0, 0, 0))
    assert F(cfg.quantum) == F(0.005) / F(1024)
    want = MS.config(quantum=F(0.005) / F(1024))
    assert (want["steps"], want["lambdaQ16"], want["muQ16"], want["flags"]) == (cfg.steps, cfg.lambdaQ16, cfg.muQ16, cfg.flags)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert hip_host.fn["mesh_smooth_default_config"](bad, C.byref(cfg)) == -1
    assert capi.MESH_SMOOTH_PIN_IRREGULAR == MS.PIN_IRREGULAR == 1


def test_record_layouts_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "itm_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d\\n",'
                   'sizeof(itm_mesh_smooth_config), sizeof(itm_mesh_smooth_stats), offsetof(itm_mesh_smooth_config, quantum),'
                   'offsetof(itm_mesh_smooth_config, reserved), offsetof(itm_mesh_smooth_stats, maxEntries), offsetof(itm_mesh_smooth_stats, reserved),'
                   'ITM_MESH_SMOOTH_PIN_IRREGULAR); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 32, 12, 20, 16, 24, 1]
    assert got[:6] == [C.sizeof(capi.MeshSmoothConfig), C.sizeof(capi.MeshSmoothStats), capi.MeshSmoothConfig.quantum.offset,
                       capi.MeshSmoothConfig.reserved.offset, capi.MeshSmoothStats.maxEntries.offset, capi.MeshSmoothStats.reserved.offset]


DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "mesh_smooth_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "mesh_smooth_demo")


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
    src = tmp_path / "save_smooth.cpp"
    src.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>::SaveSceneToSmoothPLY(const char*, uint32_t, uint32_t);\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_f_rgb, ITMVoxelBlockHash>::SaveSceneToSmoothPLY(const char*, uint32_t, uint32_t);\n'
                   'uint32_t f(ITMMesh* m) { m->Index(); itm_mesh_smooth_stats a = m->Smooth(), b = m->Smooth(10, 0.5f, 0.5f, 1e-5f, false);\n'
                   '  return a.noMoving + b.noIrregular; }\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)


# ---- GPU: the hook ----------------------------------------------------------------------------------------------------------------------

PATTERN = F(-77.125)


def as_struct(cfg):
    return capi.MeshSmoothConfig(cfg["steps"], cfg["lambdaQ16"], cfg["muQ16"], float(cfg["quantum"]), cfg["flags"], (C.c_uint32 * 3)(*cfg["reserved"]))


def hook(hip, vertices, faces, cfg):
    """(vertices', flags, stats) of itm_debug_mesh_smooth; the output arrays are returned with the error when the call is refused"""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    out = np.full(v.shape, PATTERN, F)
    flags = np.full(len(v), 0xEE, np.uint8)
    stats = capi.MeshSmoothStats()
    rc = hip.fn["debug_mesh_smooth"](v.ctypes.data_as(C.c_void_p), len(v), f.ctypes.data_as(C.c_void_p), len(f), C.byref(as_struct(cfg)),
                                     out.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), C.byref(stats), None)
    if rc != 0:
        raise capi.ItmError(f"({rc})", out, flags)
    return out, flags, stats.as_dict()


def soup(n_vertices, n_triangles, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((n_vertices, 3)) * 0.3).astype(F), rng.randint(0, n_vertices, (n_triangles, 3))


def strip_mesh(n_vertices, n_triangles, seed):
    """a closed sphere-like random mesh is not needed: a soup whose faces name near vertices, so that rows stay short and many vertices move"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, n_vertices, n_triangles)
    f = np.stack([a, (a + rng.randint(1, 4, n_triangles)) % n_vertices, (a + rng.randint(4, 8, n_triangles)) % n_vertices], 1)
    return (rng.standard_normal((n_vertices, 3)) * 0.1).astype(F), f


def hook_cases():
    cases = {}
    cases["tetrahedron"] = (TETRA_V, TETRA_F, MS.config(1, 1.0, 1.0, **ONE))
    cases["triangle_pinned"] = (np.array([[-0.0, 1, 2], [4, -0.0, 0], [0, 6, -0.0]], F), np.array([[0, 1, 2]]), MS.config(7, **ONE))
    cases["triangle_free"] = (np.array([[0, 0, 0], [4, 0, 0], [0, 6, 0]], F), np.array([[0, 1, 2]]), MS.config(1, 1.0, 1.0, pin=False, **ONE))
    cases["half_up_below_zero"] = (np.array([[0, 0, 0], [-4, -5, -6], [0, 0, 0]], F), np.array([[0, 1, 2]]), MS.config(1, 0.5, 0.5, pin=False, **ONE))
    cases["negative_factor"] = (np.array([[0, 0, 0], [-4, -5, -6], [0, 0, 0]], F), np.array([[0, 1, 2]]), MS.config(3, -0.5, 1.0, pin=False, **ONE))
    cases["clamp"] = (np.array([[2.0 ** 30, 0, 0], [2.0 ** 30, 0, 0], [-2.0 ** 30, 0, 0]], F), np.array([[0, 1, 2]]), MS.config(2, -1.0, -1.0, pin=False, **ONE))
    cases["fan_closed"] = MS.fan(6, True) + (MS.config(1, 1.0, 1.0, quantum=1.0 / 1024),)
    cases["fan_open"] = MS.fan(6, False) + (MS.config(5),)
    cases["edge_of_three"] = (np.arange(15, dtype=F).reshape(5, 3), np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]]), MS.config(3, pin=False, **ONE))
    cases["degenerate"] = ((np.arange(21, dtype=F).reshape(7, 3) * F(0.37)).astype(F), np.array([[0, 0, 0], [1, 1, 2], [3, 4, 5], [3, 3, 4], [5, 5, 5]]),
                           MS.config(5, pin=False, quantum=0.01))
    cases["steps_zero"] = (TETRA_V * F(np.nan), TETRA_F, MS.config(0))
    cases["one_vertex"] = (np.ones((1, 3), F), np.zeros((0, 3), np.int64), MS.config(3))
    cases["icosphere"] = MS.noisy_icosphere() + (MS.config(quantum=SPHERE_Q),)
    cases["icosphere_laplacian"] = MS.noisy_icosphere() + (MS.config(20, 0.5, 0.5, quantum=SPHERE_Q),)
    for pin in (True, False):
        cases[f"soup_pin_{int(pin)}"] = soup(1000, 3000, 11) + (MS.config(33, pin=pin, quantum=1e-4),)
        cases[f"near_soup_pin_{int(pin)}"] = strip_mesh(5000, 9000, 12) + (MS.config(33, pin=pin, quantum=1e-4),)
    cases["double_cone"] = MS.double_cone(5000) + (MS.config(5, quantum=1e-5),)
    cases["double_cone_free"] = (MS.double_cone(5000)[0], MS.double_cone(5000)[1][:-1], MS.config(4, pin=False, quantum=1e-5))
    for nv, nt in ((63, 255), (65, 257), (255, 63), (257, 65), (1023, 2047), (1025, 2049)):     # one below / above the wave, the workgroup, the chunk
        cases[f"sizes_{nv}_{nt}"] = strip_mesh(nv, nt, nv) + (MS.config(3, pin=False, quantum=1e-4),)
    return cases


_wanted = {}


def wanted(case):
    if case not in _wanted:
        _wanted[case] = MS.smooth(*hook_cases()[case])
    return _wanted[case]


@pytest.mark.gpu
@pytest.mark.parametrize("scatter", [0, 1])
@pytest.mark.parametrize("case", list(hook_cases()))
def test_hip_hook_equals_the_restatement(hip, case, scatter):
    v, f, cfg = hook_cases()[case]
    want = wanted(case)
    debug_set(hip, DEBUG_MESH_SMOOTH_SCATTER, scatter)
    try:
        got = hook(hip, v, f, cfg)
    finally:
        debug_set(hip, DEBUG_MESH_SMOOTH_SCATTER, 0)
    print(f"{case}: {got[2]}")
    if case == "steps_zero":                                              # NaN input passes through: compared as bits below
        assert np.isnan(got[0]).all()
    same(got, want, case)
    if case.startswith("double_cone"):
        assert got[2]["maxEntries"] in (10000, 9998)
    if case == "double_cone":
        assert got[2]["noMoving"] == 5002 and np.any(bits(got[0][:2]) != bits(v[:2]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(refusals()))
def test_hip_hook_refusals_write_nothing(hip, case):
    v, f, cfg = refusals()[case]
    for scatter in (0, 1):
        debug_set(hip, DEBUG_MESH_SMOOTH_SCATTER, scatter)
        try:
            with pytest.raises(capi.ItmError, match=r"\(-1\)") as e:
                hook(hip, v, f, cfg)
        finally:
            debug_set(hip, DEBUG_MESH_SMOOTH_SCATTER, 0)
        out, flags = e.value.args[1:]
        assert np.all(bits(out) == bits(PATTERN)) and np.all(flags == 0xEE)      # the caller's pattern
    assert hook(hip, TETRA_V, TETRA_F, MS.config(1, 1.0, 1.0, **ONE))[0].tolist() == [[1, 1, 2], [0, 1, 2], [1, 0, 2], [1, 1, 0]]


# ---- GPU: the product -------------------------------------------------------------------------------------------------------------------

def smooth_kwargs(cfg):
    return dict(steps=cfg["steps"], lam=cfg["lambdaQ16"] / 65536, mu=cfg["muQ16"] / 65536, quantum=float(cfg["quantum"]), pin_irregular=bool(cfg["flags"] & 1))


def state(m):
    return m.vertices(), m.faces(), m.first(), m.triangles()


def assert_state(m, vertices, faces, first, tri=None):
    """the index is served and unchanged but for the positions, the soup is the vertices through the faces"""
    assert m.index_info() == (len(vertices), len(faces))
    assert np.array_equal(m.faces(), faces) and np.array_equal(m.first(), first)
    got = m.vertices()
    bad = np.nonzero(np.any(bits(got) != bits(vertices), axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(vertices)} vertices differ, first {bad[:3]}: {got[bad[:3]]} vs {vertices[bad[:3]]}"
    want_tri = vertices[faces.astype(np.int64)] if tri is None else tri
    assert m.info()[0] == len(faces) and np.array_equal(bits(m.triangles()), bits(want_tri))
    soup_vertices = m.triangles().reshape(-1, 3)
    assert np.array_equal(bits(soup_vertices[first.astype(np.int64)]), bits(vertices))          # first[k] names a soup vertex that holds vertices[k]


def assert_stale(m):
    for call in (m.normals, m.vertex_normals, m.components_info, m.components, lambda: m.FilterComponents(0)):
        with raises_invalid():
            call()


def reader_of(ses):
    return MT.MeshVoxelReader(ses.scene.download(capi.BUF_VOXEL_BLOCKS), ses.scene.download(capi.BUF_HASH_ENTRIES))


def assert_attributes(hip, m, sc, reader, vertices, faces, tmp_path=None):
    """soup and indexed attributes at the moved positions equal mesh_attr_terms, through the per-block kernel and one lane per vertex"""
    what = what_of(sc)
    g, n, c = MT.attributes(reader, vertices, sc.voxelSize, colours=sc.colour)       # per unique vertex: functions of the position alone
    f = faces.astype(np.int64)
    for per_vertex in (0, 1):
        debug_set(hip, DEBUG_MESH_ATTR_PER_VERTEX, per_vertex)
        try:
            m.ComputeAttributes(what)
            m.ComputeIndexedAttributes(what)
        finally:
            debug_set(hip, DEBUG_MESH_ATTR_PER_VERTEX, 0)
        vn, normals = m.vertex_normals(), m.normals()
        bad = np.nonzero(np.any(bits(vn) != bits(n), axis=1))[0]
        assert len(bad) == 0, f"per_vertex {per_vertex}: {len(bad)} of {len(n)} vertex normals differ, first {bad[:3]}: {vn[bad[:3]]} vs {n[bad[:3]]}"
        assert np.array_equal(bits(normals), bits(n[f]))
        vcol = colours = None
        if sc.colour:
            vcol, colours = m.vertex_colours(), m.colours()
            assert np.array_equal(vcol, MT.colour_bytes(c)) and np.array_equal(colours, MT.colour_bytes(c)[f])
    if tmp_path is not None:
        assert_files(m, tmp_path, vertices[f], normals, colours, vertices, faces, vn, vcol)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mesh_micro", "mesh_f_rgb", "mesh_f", "mesh_s_rgb_yaw"])
def test_hip_product_equals_the_restatement(hip, tmp_path, name):
    sc = MC.SCENES[name]
    big = name == "mesh_s_rgb_yaw"
    ses, m = meshed(hip, sc)
    with raises_invalid():
        m.Smooth()                                                        # no index
    m.Index()
    m.MeshScene()
    with raises_invalid():
        m.Smooth()                                                        # a stale index: the buffer was generated anew
    m.Index(); m.Components(); m.FilterComponents(0)
    with raises_invalid():
        m.Smooth()                                                        # a stale index: the buffer was packed by the filter
    m.Index()
    vertices, faces, first, tri = state(m)
    m.ComputeAttributes(MESH_NORMALS); m.ComputeIndexedAttributes(MESH_NORMALS); m.Components()
    cfg = MS.config(3 if big else 5, quantum=F(sc.voxelSize) / F(1024))
    # steps == 0: the statistics, and nothing changes, the state included
    want0 = MS.smooth(vertices, faces, dict(cfg, steps=0))
    assert m.Smooth(steps=0) == want0[2]
    assert_state(m, vertices, faces, first, tri)
    m.normals(); m.vertex_normals(); m.components_info()
    # refused configurations leave everything as it was
    for kw in (dict(lam=1.01), dict(mu=-1.01), dict(quantum=0.0), dict(quantum=float("nan")), dict(quantum=1e-12), dict(steps=MS.MAX_STEPS + 1)):
        with raises_invalid():
            m.Smooth(**kw)
    assert_state(m, vertices, faces, first, tri)
    m.normals(); m.vertex_normals(); m.components_info()
    # the call with the default quantum (voxelSize / 1024)
    want = MS.smooth(vertices, faces, cfg)
    stats = m.Smooth(steps=cfg["steps"])
    print(f"{name}: {stats}")
    assert stats == want[2]
    if name in MEASURED:
        assert (stats["noVertices"], stats["noIrregular"], stats["noIsolated"], stats["maxEntries"]) == MEASURED[name]
    assert_state(m, want[0], faces, first)
    assert_stale(m)
    assert_attributes(hip, m, sc, reader_of(ses), want[0], faces, tmp_path)
    m.Components()
    assert m.components_info()[0] >= 1
    # a second call: the restatement applied twice
    twice = MS.smooth(want[0], faces, cfg)
    assert m.Smooth(steps=cfg["steps"]) == twice[2]
    assert_state(m, twice[0], faces, first)
    assert_stale(m)
    # a fresh index of the smoothed soup is accepted and describes it
    m.Index()
    wv, wf, wfirst = MI.index(twice[0][faces.astype(np.int64)])
    assert np.array_equal(m.faces(), wf) and np.array_equal(m.first(), wfirst) and np.array_equal(bits(m.vertices()), bits(wv))
    print(f"{name}: {len(wv)} vertices after re-indexing the smoothed mesh ({len(vertices)} before)")


@pytest.mark.gpu
def test_hip_attributes_serve_vertices_that_left_their_block(hip):
    """Laplacian passes without pinning at a coarse quantum move border vertices by more than a voxel: the per-block kernel must send
    them down the global path"""
    sc = MC.SCENES["mesh_f_rgb"]
    ses, m = meshed(hip, sc)
    m.Index()
    vertices, faces, first, tri = state(m)
    cfg = MS.config(40, 1.0, 1.0, quantum=F(sc.voxelSize) / F(16), pin=False)
    want = MS.smooth(vertices, faces, cfg)
    assert m.Smooth(**smooth_kwargs(cfg)) == want[2]
    assert_state(m, want[0], faces, first)
    travelled = np.abs(want[0].astype(np.float64) - vertices).max(axis=1) / sc.voxelSize
    block = lambda p: np.floor(MT.sample_positions(p, sc.voxelSize) / F(8)).astype(np.int64)
    left = int(np.any(block(want[0]) != block(vertices), axis=1).sum())
    print(f"mesh_f_rgb: {int((travelled > 1).sum())} vertices moved by more than a voxel (max {travelled.max():.2f}), {left} changed block")
    assert int((travelled > 1).sum()) > 0 and left > 0
    assert_attributes(hip, m, sc, reader_of(ses), want[0], faces)


@pytest.mark.gpu
def test_hip_smooth_of_a_dense_mesh_and_of_a_full_buffer(hip, tmp_path):
    sc = MC.DENSE
    ses, m = meshed(hip, sc, volume=True)
    m.Index()
    vertices, faces, first, tri = state(m)
    assert len(faces) > 1000
    cfg = MS.config(5, quantum=F(sc.voxelSize) / F(1024))
    want = MS.smooth(vertices, faces, cfg)
    assert m.Smooth(steps=5) == want[2]
    assert_state(m, want[0], faces, first)
    assert_stale(m)
    m.ComputeAttributes(MESH_NORMALS); m.ComputeIndexedAttributes(MESH_NORMALS)          # through the voxel array, at the new positions
    vn = m.vertex_normals()
    assert np.array_equal(bits(m.normals()), bits(vn[faces.astype(np.int64)])) and np.all(np.isfinite(vn))
    m.MeshScene(); m.Index()                                              # itm_mesh_scene leaves a dense scene empty: zero statistics, no error
    assert not any(m.Smooth().values()) and m.index_info() == (0, 0)
    # a full buffer: the count stops one below the capacity; the last slot is not part of the mesh and stays as it is
    sc = MC.SCENES["mesh_f_rgb"]
    ses, m = meshed(hip, sc, max_triangles=1000)
    assert m.info() == (999, 1000)
    m.Index()
    vertices, faces, first, tri = state(m)
    want = MS.smooth(vertices, faces, MS.config(5, quantum=F(sc.voxelSize) / F(1024), pin=False))
    assert m.Smooth(steps=5, pin_irregular=False) == want[2]
    assert_state(m, want[0], faces, first)
    assert_attributes(hip, m, sc, reader_of(ses), want[0], faces, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("scatter,buffers", [(0, 9), (1, 10)])
def test_hip_smooth_memory(hip, scatter, buffers):
    sc = MC.SCENES["mesh_micro"]
    debug_set(hip, DEBUG_FAIL_ALLOCATION, 0)
    ses = MC.fuse(hip, sc)
    start = live(hip)
    m = Mesh(ses.scene)
    m.MeshScene(); m.Index(); m.ComputeIndexedAttributes(MESH_NORMALS); m.Components()
    before = live(hip)
    vertices, faces, first, tri = state(m)
    want = MS.smooth(vertices, faces, MS.config(5, quantum=F(sc.voxelSize) / F(1024)))
    debug_set(hip, DEBUG_MESH_SMOOTH_SCATTER, scatter)
    try:
        # every allocation of the call may fail: the call reports it, keeps none of its buffers, and the mesh is as it was
        failures = 0
        for n in range(1, 20):
            debug_set(hip, DEBUG_FAIL_ALLOCATION, n)
            try:
                m.Smooth(steps=5)
            except capi.ItmError as e:
                assert "(-2)" in str(e)
                failures += 1
                assert live(hip) == before, f"allocation {n}: the failed call kept memory"
                assert_state(m, vertices, faces, first, tri)
                m.vertex_normals(); m.components_info()               # the state too
                continue
            finally:
                debug_set(hip, DEBUG_FAIL_ALLOCATION, 0)
            break
        assert failures == buffers                                     # every buffer of the call
        assert_state(m, want[0], faces, first)                         # the same call then succeeds with the clean result
        assert_stale(m)
        held = live(hip)
        assert held[0] == before[0] + buffers
        m.Smooth(steps=0)                                              # again: nothing grows
        assert live(hip) == held
    finally:
        debug_set(hip, DEBUG_MESH_SMOOTH_SCATTER, 0)
    m.close()
    assert live(hip) == start


@pytest.mark.gpu
def test_hip_smooth_is_deterministic(hip):
    sc = MC.SCENES["mesh_s_rgb_yaw"]
    ses, m = meshed(hip, sc)
    digests = []
    for scatter in (0, 0, 1):
        debug_set(hip, DEBUG_MESH_SMOOTH_SCATTER, scatter)
        try:
            m.MeshScene(); m.Index()
            stats = m.Smooth()
        finally:
            debug_set(hip, DEBUG_MESH_SMOOTH_SCATTER, 0)
        digests.append((MT.sha256(m.vertices()), MT.sha256(m.triangles()), tuple(stats.items())))
    print(f"mesh_s_rgb_yaw: {digests[0]}")
    assert digests[0] == digests[1] == digests[2]
    assert stats["noVertices"] == 404553 and stats["steps"] == 20


@pytest.mark.gpu
def test_cpp_demo_ply_equals_the_python_one(hip, tmp_path):
    exe = build_demo()
    path, mine = str(tmp_path / "demo.ply"), str(tmp_path / "python.ply")
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
    m.MeshScene(); m.Index()
    vertices, faces = m.vertices(), m.faces()
    want = MS.smooth(vertices, faces, MS.config(quantum=F(0.01) / F(1024)))
    stats = m.Smooth()
    assert stats == want[2] and np.array_equal(bits(m.vertices()), bits(want[0]))
    assert got == dict(triangles=len(faces), vertices=stats["noVertices"], moving=stats["noMoving"], irregular=stats["noIrregular"],
                       isolated=stats["noIsolated"], max_entries=stats["maxEntries"], steps=20) and len(faces) > 1000
    m.ComputeIndexedAttributes(MESH_NORMALS | MESH_COLOURS)
    m.WriteIndexedPLY(mine)
    assert open(path, "rb").read() == open(mine, "rb").read() == MI.ply_bytes_indexed(want[0], faces, m.vertex_normals(), m.vertex_colours())
