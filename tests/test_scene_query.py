"""Scene queries (include/itm_hip.h: itm_scene_query_points / itm_scene_cast_rays): sdf, gradient, colour, weight and flags at
caller-supplied points, castRay along caller-supplied segments.  Everything is compared bit for bit, no tolerances:

  * CPU: the float32 numpy restatement (tests/scene_query_terms.py) of the ray cast, fed camera rays built from castRay's own preamble,
    reproduces the oracle's FindSurface; the trilinear restatement returns the stored voxel at integer positions; the invalid rule at
    its boundary values.  That pins the restatement and the ray input convention before they are the yardstick on the GPU.
  * GPU: points and rays equal the restatement for every output, every voxel type, the dense index and every access path (dense
    mirror, paged mirror, no mirror, no directory, table walk); camera rays equal the oracle's FindSurface; queries launch recorded
    frames first; the C++ adapter gives what the Python binding gives."""
import contextlib
import json
import os
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import mesh_attr_cases as MC
import scene_query_terms as Q
from infinitam_amd import capi, synth
from infinitam_amd.capi import BUF_HASH_ENTRIES, BUF_RANGE_IMAGE, BUF_RAYCAST_RESULT, MESH_COLOURS, MESH_NORMALS, Mesh

F = np.float32
DEBUG_NO_DIRECTORY = 5          # include/itm_debug.h
SCENES = dict(MC.SCENES, dense=MC.DENSE)
SCENES.pop("mesh_vga_4mm")
ALL = ("sdf", "sdf_nearest", "gradient", "normal", "colour", "weight", "flags")
N_POINTS = 20011
N_RAYS = 5003


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
            raise AssertionError(f"{what}: {k}: {len(bad)} of {len(g)} differ, first at {bad[:5]}: {got[k][bad[:3]]} vs {want[k][bad[:3]]}")


def wants(sc):
    """the subsets of outputs with a kernel instance of their own (query.hip: nothing / trilinear / gradient / colour and their unions)"""
    subsets = [("sdf",), ("gradient",), ("sdf_nearest", "weight"), ("flags", "normal")]
    if sc.colour:
        subsets += [("colour",), ("sdf", "colour"), ALL]
    else:
        subsets += [tuple(w for w in ALL if w != "colour")]
    return subsets


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------

FORMS = {"default": {}, "paged": {"ITM_MIRROR": "paged"}, "paged_few": {"ITM_MIRROR": "paged", "ITM_MIRROR_PAGES": "5"}, "mirror_off": {"ITM_MIRROR": "off"}}


@contextlib.contextmanager
def environment(values):
    """The mirror's form is read from the environment when a scene is created."""
    keys = ("ITM_MIRROR", "ITM_MIRROR_BITS", "ITM_MIRROR_PAGES", "ITM_NO_ACCELERATION_CUBES")
    old = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(values)
    try:
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


class Built:
    """A fused scene on a backend with what the tests read from it: the restatement's reader and the mesh vertices (metres)."""

    def __init__(self, be, sc, form="default", moved_away=False):
        self.sc = sc
        with environment(FORMS[form]):
            if moved_away:
                # fused 40 m from the origin, then one frame at the origin: both cubes are re-placed around the new camera and every
                # block of the first place lies outside them
                far = T.Scenario(**{**sc.__dict__, "origin": (40.0, -30.0, 20.0)})
                self.ses = MC.fuse(be, far)
                self.old_blocks = self.ses.scene.download(BUF_HASH_ENTRIES)
                self.old_blocks = self.old_blocks["pos"][self.old_blocks["ptr"] >= 0].astype(np.int32)
                self.ses.sc = sc
                self.ses.frame(0, fused=True)
            else:
                self.ses = MC.fuse(be, sc)
        self.scene = self.ses.scene
        self.reader = Q.reader_of(self.scene)
        self.mesh = None
        if "mesh_volume" in be.fn:               # the product: the mesh of either index type
            self.mesh = Mesh(self.scene)
            self.mesh.MeshVolume()
            self.vertices = self.mesh.triangles().reshape(-1, 3)

    def bounds(self):
        """(lo, hi) of the stored voxels, in voxels"""
        if self.scene.is_hash:
            e = self.scene.download(BUF_HASH_ENTRIES)
            pos = e["pos"][e["ptr"] >= 0].astype(np.int64)
            return pos.min(0) * 8, (pos.max(0) + 1) * 8
        lo = np.array(self.scene.cfg.denseOffset[:], np.int64)
        return lo, lo + np.array(self.scene.cfg.denseSize[:], np.int64)

    def blocks(self):
        if self.scene.is_hash:
            e = self.scene.download(BUF_HASH_ENTRIES)
            return e["pos"][e["ptr"] >= 0].astype(np.int64)
        lo, hi = self.bounds()
        g = np.stack(np.meshgrid(*[np.arange(lo[a] // 8, hi[a] // 8 + 1) for a in range(3)], indexing="ij"), -1)
        return g.reshape(-1, 3)

    def close(self):
        if self.mesh is not None:
            self.mesh.close()
        self.ses.close()


_built = {}


def built(be, name, form="default", moved_away=False):
    key = (id(be), name, form, moved_away)
    if key not in _built:
        _built[key] = Built(be, SCENES[name], form, moved_away)
    return _built[key]


@pytest.fixture(scope="module", autouse=True)
def close_scenes():
    yield
    for b in _built.values():
        b.close()
    _built.clear()


# ---- the point set --------------------------------------------------------------------------------------------------------------------

INVALID_VALUES = [262135.9, 262136.0, -262136.0, np.nan, np.inf, -np.inf]


def invalid_points(inside):
    """each boundary value of the invalid rule on each axis of a point inside the scene, and on all three"""
    pts = []
    for v in INVALID_VALUES:
        for axis in range(3):
            p = np.array(inside, F)
            p[axis] = v
            pts.append(p)
        pts.append(np.full(3, v, F))
    return np.array(pts, F)


def voxel_points(b, n, seed=11):
    """n positions in voxels: uniform in the bounding box +- 2 blocks, integer lattice points, positions within 1e-3 of block faces,
    edges and corners on both sides (8k +- e, 8k - 1 +- e), negative coordinates, unallocated blocks, the shell 3 voxels around the
    box (the outside of a dense array) and the values of the invalid rule"""
    rng = np.random.default_rng(seed)
    lo, hi = b.bounds()
    blocks = b.blocks()
    parts = [invalid_points((lo + hi) / 2)]
    # near block faces (one axis at a boundary), edges (two) and corners (three)
    m = 4500
    blk = blocks[rng.integers(0, len(blocks), m)]
    p = blk * 8 + rng.uniform(0, 8, (m, 3))
    at = rng.integers(1, 8, m)                                   # which axes sit at a boundary: bit per axis, never none
    edge = blk * 8 + rng.choice([0, 8], (m, 3)) - rng.choice([0, 1], (m, 3)) + rng.choice([-1, 1], (m, 3)) * rng.uniform(0, 1e-3, (m, 3))
    for a in range(3):
        p[:, a] = np.where((at >> a) & 1, edge[:, a], p[:, a])
    parts.append(p)
    # integer lattice points, inside and around the box
    parts.append(rng.integers(lo - 4, hi + 4, (2500, 3)).astype(np.float64))
    # the shell around the box: up to 3 voxels outside on every side
    m = 1500
    p = rng.uniform(lo - 3, hi + 3, (m, 3))
    a = rng.integers(0, 3, m)
    side = np.where(rng.integers(0, 2, m) == 0, rng.uniform(-3, 0, m) + lo[a], rng.uniform(0, 3, m) + hi[a])
    p[np.arange(m), a] = side
    parts.append(p)
    # unallocated space far from the scene, and all-negative coordinates
    parts.append(rng.uniform(lo, hi, (500, 3)) + rng.choice([-1, 1], (500, 3)) * 3000.0)
    parts.append(-np.abs(rng.uniform(lo - 16, hi + 16, (1000, 3))))
    rest = n - sum(len(q) for q in parts)
    assert rest > 3000
    parts.append(rng.uniform(lo - 16, hi + 16, (rest, 3)))
    return np.concatenate(parts).astype(F)


def point_sets(b):
    """(vertices in metres, positions in voxels): N_POINTS together"""
    v = b.vertices[::16][:6000]
    return np.ascontiguousarray(v, F), voxel_points(b, N_POINTS - len(v))


def check_points(b, subsets, what):
    v, p = point_sets(b)
    assert len(v) + len(p) == N_POINTS and len(v) > 500
    for units, pts in (("metres", v), ("voxels", p)):
        for want in subsets:
            got = b.scene.query_points(pts, units, want)
            assert_same(got, Q.query_points(b.reader, pts, units, b.sc.voxelSize, want), f"{what}, {units}, {want}")
    return v, p


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------

def oracle_surface(ses, M, free_view):
    """(range image, FindSurface result) of the oracle's scene at pose M"""
    sc = ses.sc
    if free_view:
        ses.scene.vis.FindVisibleBlocks(M, sc.intr(), ses.rs)
    ses.scene.vis.CreateExpectedDepths(M, sc.intr(), ses.rs)
    ses.scene.vis.FindSurface(M, sc.intr(), ses.rs)
    return ses.scene.download(BUF_RANGE_IMAGE, ses.rs).copy(), ses.scene.download(BUF_RAYCAST_RESULT, ses.rs).reshape(-1, 4).copy()


def assert_hits_equal(got, want, what, min_hits=1000):
    assert np.array_equal(got[:, 3], want[:, 3]), f"{what}: hit mask differs at {np.count_nonzero(got[:, 3] != want[:, 3])} rays"
    hit = want[:, 3] > 0
    assert hit.sum() >= min_hits, (what, int(hit.sum()))
    bad = np.nonzero((bits(got[hit]) != bits(want[hit])).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {int(hit.sum())} hits differ, first {got[hit][bad[:3]]} vs {want[hit][bad[:3]]}"


@pytest.mark.parametrize("name", ["mesh_micro", "mesh_f_rgb", "dense"])
def test_ray_restatement_reproduces_the_oracles_find_surface(oracle, name):
    b = built(oracle, name)
    sc = b.sc
    M = sc.pose(sc.frames - 1)
    rng_img, want = oracle_surface(b.ses, M, free_view=False)
    rays = Q.camera_rays(M, sc.intr(), sc.w, sc.h, rng_img)
    assert_hits_equal(Q.cast_rays(b.reader, rays, sc.voxelSize, sc.mu), want, name)


@pytest.mark.parametrize("name", ["mesh_micro", "mesh_f_rgb", "dense"])
def test_trilinear_restatement_at_integer_positions_is_the_stored_voxel(oracle, name):
    b = built(oracle, name)
    rng = np.random.default_rng(3)
    lo, hi = b.bounds()
    blocks = b.blocks()
    inside = blocks[rng.integers(0, len(blocks), 10000)] * 8 + rng.integers(0, 8, (10000, 3))
    p = np.concatenate([inside, rng.integers(lo - 8, hi + 8, (10000, 3))]).astype(F)
    tri, corners = Q.trilinear(b.reader, p)
    near, found, _ = Q.nearest(b.reader, p)
    assert found.sum() > 2000 and (~found).sum() > 2000
    assert np.array_equal(bits(tri), bits(near))
    assert np.array_equal((corners & 1) != 0, found)
    assert np.all(near[~found] == F(1))


def test_invalid_rule_at_its_boundary_values():
    p = invalid_points((1.0, 2.0, 3.0))
    bad = Q.invalid(p).reshape(len(INVALID_VALUES), 4)
    assert not bad[0].any(), "262135.9 is a valid coordinate"
    assert bad[1:].all(), "262136, -262136, NaN and +-Inf are not"
    # floor(p) - 1 .. floor(p) + 2 of the largest valid coordinate stays inside the table's short block coordinates
    top = np.nextafter(Q.POINT_LIMIT, F(0))
    assert (int(np.floor(top)) + 2) >> 3 <= 32767 and (int(np.floor(-top)) - 1) >> 3 >= -32768


def test_binding_and_header_declare_the_entry_points():
    declared = capi.declared_functions()
    for fn in ("scene_query_points", "scene_cast_rays"):
        assert fn in declared and fn in capi._HOST_IO_SIGS and fn not in capi._SIGS
    assert (capi.QUERY_METRES, capi.QUERY_VOXELS, capi.QUERY_INVALID) == (0, 1, 0x80000000)
    assert set(capi.QUERY_OUTPUTS) == {n for n, _ in capi.QueryOut._fields_}


DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "scene_query_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "scene_query_demo")


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_demo_and_main_engine_queries_compile(tmp_path):
    assert os.path.exists(build_demo())
    src = tmp_path / "query.cpp"
    src.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>::QueryPoints(const float*, uint32_t, const itm_query_out&, int) const;\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_f_rgb, ITMPlainVoxelArray>::CastRays(const float*, uint32_t, float*) const;\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)


# ---- GPU: points ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_points_equal_the_restatement(hip, name):
    b = built(hip, name)
    sc = b.sc
    v, p = check_points(b, wants(sc), name)
    # the point set is what it claims to be
    flags = b.scene.query_points(p, "voxels", ("flags",))["flags"]
    assert np.count_nonzero(flags == capi.QUERY_INVALID) == 5 * 4, "the invalid values"
    assert np.count_nonzero(flags & 2) > 1000 and np.count_nonzero(flags == 0) > 1000, "cells with all corners, cells with none"
    corners = (flags >> 8) & 0xff
    assert np.count_nonzero((corners != 0) & (corners != 0xff) & (flags != capi.QUERY_INVALID)) > 200, "cells that straddle allocated and unallocated blocks"
    # n = 0 and n = 1
    none = b.scene.query_points(np.zeros((0, 3), F), "voxels", ALL if sc.colour else ALL[:4])
    assert all(len(a) == 0 for a in none.values())
    one = b.scene.query_points(v[:1], "metres", ("sdf", "gradient", "flags"))
    assert_same(one, Q.query_points(b.reader, v[:1], "metres", sc.voxelSize, ("sdf", "gradient", "flags")), name + ", one point")
    # at the mesh's own vertices: what itm_mesh_attributes computes
    b.mesh.ComputeAttributes(MESH_NORMALS | (MESH_COLOURS if sc.colour else 0))
    got = b.scene.query_points(b.vertices, "metres", ("normal", "colour") if sc.colour else ("normal",))
    assert len(b.vertices) > 3000
    assert np.array_equal(bits(got["normal"]), bits(b.mesh.normals().reshape(-1, 3)))
    if sc.colour:
        assert np.array_equal(got["colour"], b.mesh.colours().reshape(-1, 4))
    else:
        with pytest.raises(capi.ItmError, match=r"\(-1\).*colour"):
            b.scene.query_points(v[:4], "metres", ("colour",))
    with pytest.raises(capi.ItmError, match=r"\(-1\)"):
        hip.check(hip.fn["scene_query_points"](capi._P(b.scene.h), None, 4, 7, None, None), "scene_query_points")


def all_blocks_outside_the_cubes(b):
    probe = b.scene.accel_probe(b.old_blocks)
    return not probe["dir_covered"].any() and not probe["mirror_covered"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mesh_micro", "mesh_s_rgb_yaw"])
@pytest.mark.parametrize("path", ["paged", "paged_few", "mirror_off", "directory_off", "table_walk"])
def test_points_under_every_access_path(hip, name, path):
    sc = SCENES[name]
    subsets = [("sdf",), ("gradient",), tuple(w for w in ALL if sc.colour or w != "colour")]
    if path == "directory_off":
        b = built(hip, name)
        hip.check(hip.fn["debug_set"](DEBUG_NO_DIRECTORY, 1), "debug_set")
        try:
            check_points(b, subsets, f"{name}, {path}")
        finally:
            hip.check(hip.fn["debug_set"](DEBUG_NO_DIRECTORY, 0), "debug_set")
        return
    b = built(hip, name, form=path if path in FORMS else "default", moved_away=path == "table_walk")
    info = b.scene.accel_info()
    if path.startswith("paged"):
        assert info["mirror_pages"] == (5 if path == "paged_few" else info["mirror_pages"]) > 0, info
    elif path == "mirror_off":
        assert info["mirror_bytes"] == 0 and info["directory_bytes"] > 0, info
    else:
        assert info["moves"] >= 1 and all_blocks_outside_the_cubes(b), info
    check_points(b, subsets, f"{name}, {path}")


# ---- GPU: rays ------------------------------------------------------------------------------------------------------------------------

def arbitrary_rays(b, n, seed=5):
    """n rays in metres: origins inside the volume, outside it and behind the surface, random directions, t0 = 0, segments shorter than a
    voxel, segments wholly in unallocated space, t0 >= t1 and the invalid cases"""
    rng = np.random.default_rng(seed)
    vs = float(b.sc.voxelSize)
    lo, hi = (np.asarray(a, np.float64) * vs for a in b.bounds())
    span = hi - lo
    s = rng.uniform(lo - 0.3 * span, hi + 0.3 * span, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    length = rng.uniform(0.05, 2.5, n)
    t0 = rng.uniform(0.0, 1.0, n)
    kind = rng.integers(0, 10, n)
    # from the camera side towards mesh vertices, ending behind the surface (kind 0-2); from behind the surface (kind 3)
    tgt = b.vertices[rng.integers(0, len(b.vertices), n)].astype(np.float64)
    cam = np.array([0.0, 0.0, 0.0]) + rng.normal(scale=0.2, size=(n, 3))
    to = tgt - cam
    to /= np.linalg.norm(to, axis=1)[:, None]
    front = kind <= 2
    s[front] = (tgt - to * rng.uniform(0.1, 0.8, n)[:, None])[front]
    d[front] = to[front]
    back = kind == 3
    s[back] = (tgt + to * rng.uniform(0.0, 0.04, n)[:, None])[back]
    length[kind == 4] = rng.uniform(0.0, vs, n)[kind == 4]                  # shorter than one voxel
    t0[kind == 5] = 0.0
    far = kind == 6                                                        # wholly in unallocated space
    s[far] += 50.0
    e = s + d * length[:, None]
    t1 = t0 + length
    swap = kind == 7                                                       # t0 >= t1
    t1[swap] = t0[swap] - rng.uniform(0.0, 0.5, n)[swap]
    rays = np.concatenate([s, t0[:, None], e, t1[:, None]], 1).astype(F)
    # the invalid cases: each of the eight values not finite, s == e, an end point at the limit, a length beyond the limit
    lim = F(131072.0 * vs * 1.001)
    k = 0
    for col in range(8):
        for v in (np.nan, np.inf, -np.inf):
            rays[k, col] = v
            k += 1
    rays[k, 4:7] = rays[k, 0:3]; k += 1
    for col in (0, 1, 2, 4, 5, 6):
        rays[k, col] = lim; rays[k + 1, col] = -lim
        k += 2
    for col in (3, 7):
        rays[k, col] = F(4194304.0 * vs * 1.001)
        k += 1
    rays[k, 0:3] = 0; rays[k, 4:7] = F(1e-30)                              # d.d underflows to 0: the normalised direction is not finite
    return rays, k + 1


def check_rays(b, what):
    rays, n_invalid = arbitrary_rays(b, N_RAYS)
    want = Q.cast_rays(b.reader, rays, b.sc.voxelSize, b.sc.mu)
    got = b.scene.cast_rays(rays)
    assert np.all(got[:n_invalid] == 0), "invalid rays take no step"
    assert_hits_equal(got, want, what, min_hits=800)
    assert np.count_nonzero(want[:, 3] == 0) > 1500
    assert b.scene.cast_rays(np.zeros((0, 8), F)).shape == (0, 4)
    assert_hits_equal(b.scene.cast_rays(rays[-1:]), want[-1:], what + ", one ray", min_hits=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,moved", [("mesh_micro", "default", False), ("mesh_f_rgb", "default", False), ("dense", "default", False),
                                             ("mesh_micro", "paged_few", False), ("mesh_micro", "mirror_off", False), ("mesh_micro", "default", True)])
def test_arbitrary_rays_equal_the_restatement(hip, name, form, moved):
    b = built(hip, name, form=form, moved_away=moved)
    if moved:
        assert all_blocks_outside_the_cubes(b)
    check_rays(b, f"{name}, {form}{', table walk' if moved else ''}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mesh_micro", "mesh_f_rgb", "dense"])
def test_camera_rays_equal_the_oracles_find_surface(hip, oracle, name):
    b, ref = built(hip, name), built(oracle, name)
    sc = b.sc
    free = synth.pose_matrix_yaw(tuple(F(a) + F(d) for a, d in zip(sc.position(0), (0.15, -0.05, -0.1))), 0.12)
    rng = np.random.default_rng(9)
    for M, free_view in ((sc.pose(sc.frames - 1), False), (sc.pose(0), True), (free, True)):
        rng_img, want = oracle_surface(ref.ses, M, free_view)
        rays = Q.camera_rays(M, sc.intr(), sc.w, sc.h, rng_img)
        got = b.scene.cast_rays(rays)
        assert_hits_equal(got, want, f"{name}, pose {M[12:15]}")
        # no lane depends on its neighbours: a random permutation and a random third give the same per-ray results
        hit = got[:, 3] > 0
        perm = rng.permutation(len(rays))
        again = b.scene.cast_rays(rays[perm])
        assert np.array_equal(again[:, 3], got[perm][:, 3]) and np.array_equal(bits(again[hit[perm]]), bits(got[perm][hit[perm]]))
        third = np.sort(rng.choice(len(rays), len(rays) // 3, replace=False))
        again = b.scene.cast_rays(rays[third])
        assert np.array_equal(again[:, 3], got[third][:, 3]) and np.array_equal(bits(again[hit[third]]), bits(got[third][hit[third]]))


# ---- GPU: recorded frames, the C++ adapter ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_queries_launch_recorded_frames_first(hip):
    sc = SCENES["mesh_f_rgb"]
    b = built(hip, "mesh_f_rgb")
    v, p = point_sets(b)
    rays, _ = arbitrary_rays(b, 2001)
    results = []
    for deferred in (True, False):
        ses = T.Session(hip, sc, deferred_fusion=deferred)
        ses.frame(0, fused="four" if deferred else False)
        view = ses.view(1)
        ses.scene.reco.AllocateSceneFromDepth(view, ses.rs)          # deferred: recorded, not launched
        ses.scene.reco.IntegrateIntoScene(view, ses.rs)
        ses.scene.vis.CreateExpectedDepths(view.M_d, view.intr_d, ses.rs)
        if deferred:
            results.append((ses.scene.cast_rays(rays), ses.scene.query_points(p, "voxels", ALL)))
            ses2 = T.Session(hip, sc, deferred_fusion=True)          # the point query as the call that meets the recorded frame
            ses2.frame(0, fused="four")
            view2 = ses2.view(1)
            ses2.scene.reco.AllocateSceneFromDepth(view2, ses2.rs)
            ses2.scene.reco.IntegrateIntoScene(view2, ses2.rs)
            ses2.scene.vis.CreateExpectedDepths(view2.M_d, view2.intr_d, ses2.rs)
            first = ses2.scene.query_points(p, "voxels", ALL)
            ses2.close()
        else:
            results.append((ses.scene.cast_rays(rays), ses.scene.query_points(p, "voxels", ALL)))
        ses.close()
    (ra, pa), (rb, pb) = results
    assert_same(pa, pb, "recorded frame, points after rays")
    assert_same(first, pb, "recorded frame, points first")
    assert_hits_equal(ra, rb, "recorded frame, rays", min_hits=300)
    # and the second frame is really in what they saw
    before = b.scene.query_points(p, "voxels", ("weight",))["weight"]
    one = T.Session(hip, sc, deferred_fusion=False)
    one.frame(0)
    w1 = one.scene.query_points(p, "voxels", ("weight",))["weight"]
    one.close()
    assert np.array_equal(pb["weight"], before) and not np.array_equal(pb["weight"], w1)


def fnv(a):
    h = 1469598103934665603
    for byte in np.ascontiguousarray(a).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


@pytest.mark.gpu
def test_cpp_demo_equals_the_python_binding(hip):
    out = subprocess.run([build_demo()], check=True, capture_output=True, text=True).stdout
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
    k, j, i = np.meshgrid(np.arange(21), np.arange(31), np.arange(41), indexing="ij")
    points = np.stack([F(-0.6) + F(0.03) * i.astype(F), F(-0.45) + F(0.03) * j.astype(F), F(1.45) + F(0.01) * k.astype(F)], -1).reshape(-1, 3).astype(F)
    j, i = np.meshgrid(np.arange(31), np.arange(41), indexing="ij")
    dx, dy = (F(-0.4) + F(0.02) * i.astype(F)).reshape(-1), (F(-0.3) + F(0.02) * j.astype(F)).reshape(-1)
    half, three = np.full_like(dx, F(0.5)), np.full_like(dx, F(3.0))
    rays = np.stack([F(0.5) * dx, F(0.5) * dy, half, half, F(3.0) * dx, F(3.0) * dy, three, three], -1).astype(F)
    res = s.query_points(points, "metres", ("sdf", "gradient", "normal", "colour", "weight", "flags"))
    hits = s.cast_rays(rays)
    hits[hits[:, 3] == 0] = 0
    assert got["points"] == len(points) and got["rays"] == len(rays)
    assert got["hits"] == int((hits[:, 3] > 0).sum()) > 800
    assert got["all_corners"] == int(np.count_nonzero(res["flags"] & 2)) > 1000
    for name in ("sdf", "gradient", "normal", "colour", "weight", "flags"):
        assert got[name] == fnv(res[name]), name
    assert got["hit_points"] == fnv(hits)
    # ... and both are the restatement's
    reader = Q.reader_of(s)
    assert_same(res, Q.query_points(reader, points, "metres", 0.01, tuple(res)), "demo scene")
    assert_hits_equal(hits, Q.cast_rays(reader, rays, 0.01, 0.02), "demo scene")
    rs.close(); s.close()
