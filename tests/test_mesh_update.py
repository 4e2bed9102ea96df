"""Incremental mesh (include/itm_hip.h: itm_mesh_touch / itm_mesh_update / itm_mesh_update_info / itm_mesh_download_update).

The expected buffer is never restated: it is MeshScene on a second handle of the same scene, compared bit for bit, order included.  The
bookkeeping -- which blocks appeared, vanished, are dirty, were removed -- is restated in numpy (tests/mesh_update_terms.py) from two
downloads of the table and the marked slots, and the call's statistics and delta equal it in every case.
  * CPU: the boundary; the restatement on the oracle's tables of consecutive frames: the dirty set made from the visible list contains
    every block whose run of the oracle's soup differs, and is at most half the map at the last frame.
  * GPU: frame by frame; every voxel type; fused and recorded frames; accumulated marks (and a missing one, which must show);  the
    neighbour rule on a constructed case; presence changes (prune); the full paths with their reasons; refusals; the adapters."""
import ctypes as C
import json
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import itm_testlib as T
import mesh_attr_cases as MC
import mesh_dense_cases as MD
import mesh_update_terms as MU
from infinitam_amd import capi
from infinitam_amd.capi import Mesh
from itm_testlib import Scenario
from test_mesh_components import raises_invalid

F = np.float32
SC = Scenario(name="mesh_update", w=160, h=120, voxelSize=0.01, frames=6, trajectory="yaw", yaw_rate=0.3)
NEW_FNS = ("mesh_touch", "mesh_update", "mesh_update_info", "mesh_download_update")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def table_of(ses):
    return ses.scene.download(capi.BUF_HASH_ENTRIES)


def visible(ses):
    n = ses.scene.counters(ses.rs)["noVisibleEntries"]
    return ses.scene.download(capi.BUF_VISIBLE_IDS, ses.rs)[:n].copy()


# ---- CPU: the boundary ----------------------------------------------------------------------------------------------------------------

def test_binding_header_and_library_declare_the_entry_points(hip_host):
    declared = capi.declared_functions()
    for fn in NEW_FNS:
        assert fn in declared and fn in capi._HOST_IO_SIGS and fn not in capi._SIGS and fn in hip_host.fn
    assert callable(Mesh.Touch) and callable(Mesh.Update) and callable(Mesh.update_delta)
    assert "mesh_update.hip" in open(os.path.join(T.ROOT, "infinitam_amd", "csrc", "Makefile")).read()
    # a null handle is refused before anything touches a device
    assert hip_host.fn["mesh_touch"](None, None, None, None, -1, None) == -1
    assert b"null" in hip_host.fn["last_error"]()
    assert hip_host.fn["mesh_update"](None, None, None, None) == -1
    assert hip_host.fn["mesh_update_info"](None, None, None, None, None, None) == -1


def test_record_layouts_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "itm_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\\n",'
                   'sizeof(itm_mesh_update_stats), sizeof(itm_mesh_changed_block), sizeof(itm_mesh_removed_block),'
                   'offsetof(itm_mesh_update_stats, trianglesBefore), offsetof(itm_mesh_update_stats, noChanged),'
                   'offsetof(itm_mesh_changed_block, firstTriangle), offsetof(itm_mesh_removed_block, pos),'
                   'ITM_MESH_UPDATE_NO_RUN_TABLE, ITM_MESH_UPDATE_ALL_MARKED, ITM_MESH_UPDATE_OVERFLOW); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [64, 20, 12, 32, 48, 12, 4, 1, 2, 3]
    assert got[:7] == [C.sizeof(capi.MeshUpdateStats), C.sizeof(capi.MeshChangedBlock), C.sizeof(capi.MeshRemovedBlock),
                       capi.MeshUpdateStats.trianglesBefore.offset, capi.MeshUpdateStats.noChanged.offset, capi.MeshChangedBlock.firstTriangle.offset,
                       capi.MeshRemovedBlock.pos.offset]
    assert (capi.MESH_CHANGED_DTYPE.itemsize, capi.MESH_REMOVED_DTYPE.itemsize) == (20, 12)
    assert got[7:] == [capi.MESH_UPDATE_NO_RUN_TABLE, capi.MESH_UPDATE_ALL_MARKED, capi.MESH_UPDATE_OVERFLOW]


def test_restatement_hand_case():
    """four slots: 0 stays, 1 vanishes, 2 changes its position, 3 appears; slot 0 sits at -x of the block that vanished"""
    t0 = np.zeros(8, capi.HASH_ENTRY_DTYPE); t0["ptr"] = -2
    t1 = t0.copy()
    for tab, entries in ((t0, {0: (4, 0, 0), 1: (5, 0, 0), 2: (9, 9, 9), 5: (20, 0, 0)}), (t1, {0: (4, 0, 0), 2: (9, 9, 10), 3: (30, 0, 0), 5: (20, 0, 0)})):
        for k, (slot, pos) in enumerate(entries.items()):
            tab["pos"][slot] = pos; tab["ptr"][slot] = k
    t1["ptr"][1] = -1                                                     # swapped out: vanished
    out, dirty, changed, removed = MU.terms(t0, t1, [7, 7, -1, 8, 99])
    assert out == dict(full=0, allocated=4, marked=1, ignoredMarks=3, appeared=2, vanished=2, remeshed=3, kept=1, noChanged=3, noRemoved=2)
    assert dirty.tolist() == [0, 2, 3] and removed["slot"].tolist() == [1, 2] and removed["pos"].tolist() == [[5, 0, 0], [9, 9, 9]]
    assert changed["pos"].tolist() == [[4, 0, 0], [9, 9, 10], [30, 0, 0]]
    # a mark on slot 5 makes it dirty, and nothing else: no listed block has it at +d
    assert MU.terms(t0, t1, [5])[1].tolist() == [0, 2, 3, 5]
    assert MU.terms(t0, t1, [], run_current=False)[0]["full"] == capi.MESH_UPDATE_NO_RUN_TABLE
    full = MU.terms(t0, t1, [], everything=True)
    assert full[0]["full"] == capi.MESH_UPDATE_ALL_MARKED and full[1].tolist() == [0, 2, 3, 5] and len(full[3]) == 2


_oracle = {}


def oracle_frames(oracle):
    """per frame of SC on the CPU oracle: (table, voxels, visible slots, soup)"""
    if not _oracle:
        ses = T.Session(oracle, SC)
        m = Mesh(ses.scene)
        for k in range(SC.frames):
            ses.frame(k)
            m.MeshScene()
            _oracle[k] = (table_of(ses), ses.scene.download(capi.BUF_VOXEL_BLOCKS), visible(ses), m.triangles())
        m.close(); ses.close()
    return _oracle


def test_dirty_set_covers_every_run_that_differs(oracle):
    frames = oracle_frames(oracle)
    prev_runs = MU.runs(*[frames[0][i] for i in (0, 1, 3)])[0]
    for k in range(1, SC.frames):
        table, voxels, vis, tri = frames[k]
        runs = MU.runs(table, voxels, tri)[0]
        out, dirty, changed, removed = MU.terms(frames[k - 1][0], table, vis)
        differs = [s for s in runs if prev_runs.get(s) != runs[s]]
        outside_visible = len(set(differs) - set(vis.tolist()))
        print(f"frame {k}: allocated {out['allocated']}, visible {len(vis)}, |D| {len(dirty)}, triangles {len(tri)}, runs that differ {len(differs)} "
              f"({outside_visible} outside the visible list), appeared {out['appeared']}")
        assert set(differs) <= set(dirty.tolist())
        assert out["vanished"] == 0 and len(removed) == 0
        prev_runs = runs
    assert out["allocated"] == 5934 and len(vis) == 2386 and len(dirty) == 2463          # the figures of the issue, frame 5
    assert len(dirty) <= out["allocated"] / 2


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def fresh(ses, max_triangles=0):
    m = Mesh(ses.scene, max_triangles)
    m.MeshScene()
    tri = m.triangles()
    m.close()
    return tri


def assert_update(m, ses, table0, marks, max_triangles=0, before=None, **kw):
    """Update, then: statistics and delta equal the restatement, the buffer equals a fresh MeshScene.  Returns (stats, the table now)."""
    stats = m.Update()
    delta = m.update_delta()
    table1 = table_of(ses)
    want, dirty, changed, removed = MU.terms(table0, table1, marks, **kw)
    print(stats)
    assert {k: stats[k] for k in MU.STAT_NAMES} == want
    assert np.array_equal(delta["changed"]["slot"], changed["slot"]) and np.array_equal(delta["changed"]["pos"], changed["pos"])
    assert not delta["changed"]["reserved"].any() and delta["removed"].tobytes() == removed.tobytes()
    tri, want_tri = m.triangles(), fresh(ses, max_triangles)
    assert tri.shape == want_tri.shape, f"{len(tri)} triangles, a fresh MeshScene has {len(want_tri)}"
    bad = np.nonzero(np.any(bits(tri).reshape(len(tri), 9) != bits(want_tri).reshape(len(tri), 9), axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(tri)} triangles differ from a fresh MeshScene, first {bad[:3]}"
    assert stats["trianglesAfter"] == len(tri) == m.info()[0]
    assert int(delta["changed"]["noTriangles"].sum()) == stats["trianglesGenerated"]
    if before is not None:
        assert stats["trianglesBefore"] == before
    if not stats["full"]:
        assert stats["trianglesCopied"] + stats["trianglesGenerated"] == len(tri)
        first = delta["changed"]["firstTriangle"].astype(np.int64)
        assert np.all(np.diff(first) >= 0) and (len(first) == 0 or first[-1] + int(delta["changed"]["noTriangles"][-1]) <= len(tri))
    else:
        assert stats["trianglesCopied"] == 0
    return stats, table1


@pytest.mark.gpu
def test_hip_frame_by_frame(hip):
    ses = T.Session(hip, SC)
    ses.frame(0)
    m = Mesh(ses.scene)
    m.MeshScene()
    table, n = table_of(ses), m.info()[0]
    for k in range(1, SC.frames):
        ses.frame(k)
        m.Touch(ses.rs)
        stats, table = assert_update(m, ses, table, visible(ses), before=n)
        n = stats["trianglesAfter"]
        assert stats["full"] == 0 and stats["trianglesCopied"] > 0
        if k >= 2:
            assert stats["remeshed"] < stats["allocated"]
    # the delta's runs are the runs of the blocks: counts per block from the voxels
    a, cnt = MU.block_counts(table, ses.scene.download(capi.BUF_VOXEL_BLOCKS))
    start = np.cumsum(cnt) - cnt
    ch = m.update_delta()["changed"]
    at = np.searchsorted(a, ch["slot"])
    assert np.array_equal(ch["firstTriangle"], start[at]) and np.array_equal(ch["noTriangles"], cnt[at])
    # products computed from the buffer are stale after an update, and are served again once recomputed
    m.Index()
    ses.frame(SC.frames)
    m.Touch(ses.rs)
    m.Update()
    with raises_invalid():
        m.index_info()
    m.Index(); m.ComputeAttributes(capi.MESH_NORMALS)
    assert m.normals().shape == m.triangles().shape
    m.close(); ses.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mesh_micro", "mesh_f_rgb", "mesh_s_rgb_yaw", "mesh_f"])
def test_hip_every_voxel_type(hip, name):
    sc = replace(MC.SCENES[name], frames=2)
    ses = T.Session(hip, sc)
    ses.frame(0)
    m = Mesh(ses.scene)
    m.MeshScene()
    table = table_of(ses)
    ses.frame(1)
    m.Touch(ses.rs)
    stats, _ = assert_update(m, ses, table, visible(ses))
    assert stats["full"] == 0
    m.close(); ses.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, "four"])
def test_hip_every_frame_form(hip, fused):
    ses = T.Session(hip, SC)
    ses.frame(0, fused=fused)
    m = Mesh(ses.scene)
    m.MeshScene()
    table = table_of(ses)
    for k in (1, 2):
        if fused is True:
            ses.frame(k, fused=True)
            m.Touch(ses.rs)
        else:
            # three calls recorded, none launched: the touch must launch them first, the visible list is final only then
            v = ses.view(k)
            ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
            ses.scene.reco.IntegrateIntoScene(v, ses.rs)
            ses.scene.vis.CreateExpectedDepths(v.M_d, v.intr_d, ses.rs)
            m.Touch(ses.rs)
            ses.scene.vis.CreateICPMaps(v, ses.rs, ses.points, ses.normals)
        stats, table = assert_update(m, ses, table, visible(ses))
        assert stats["full"] == 0 and stats["marked"] > 0
    m.close(); ses.close()


@pytest.mark.gpu
def test_hip_accumulated_marks_and_a_missing_one(hip):
    ses = T.Session(hip, SC)
    ses.frame(0)
    m, lazy = Mesh(ses.scene), Mesh(ses.scene)
    m.MeshScene(); lazy.MeshScene()
    table, marks = table_of(ses), []
    for k in (1, 2, 3):
        ses.frame(k)
        m.Touch(ses.rs)
        marks.append(visible(ses))
        if k != 1:
            lazy.Touch(ses.rs)
    stats, _ = assert_update(m, ses, table, np.concatenate(marks))
    assert stats["full"] == 0
    # the same three frames with the touch of frame 1 missing: the blocks that left the view after it keep their old runs (58 of them on
    # the CPU oracle; without frame 2's or frame 3's touch the other two cover every rewritten block)
    lazy_stats = lazy.Update()
    want = m.triangles()
    got = lazy.triangles()
    assert lazy_stats["full"] == 0 and lazy_stats["remeshed"] < stats["remeshed"]
    assert got.shape != want.shape or not np.array_equal(bits(got), bits(want))
    m.close(); lazy.close(); ses.close()


@pytest.mark.gpu
def test_hip_neighbour_rule(hip):
    sc = replace(SC, frames=2)
    ses = MC.fuse(hip, sc)
    m = Mesh(ses.scene)
    m.MeshScene()
    table, voxels = table_of(ses), ses.scene.download(capi.BUF_VOXEL_BLOCKS)
    before = MU.runs(table, voxels, m.triangles())[0]
    a, cnt = MU.block_counts(table, voxels)
    pos = table["pos"][a].astype(np.int64)
    has = dict(zip(MU.keys(pos).tolist(), cnt.tolist()))
    left = np.array([has.get(int(k), 0) for k in MU.keys(pos - np.array([1, 0, 0]))])
    candidates = np.nonzero((cnt > 0) & (left > 0))[0]
    b = candidates[np.argmax(cnt[candidates])]
    slot, ptr = int(a[b]), int(table["ptr"][a[b]])
    voxels = voxels.reshape(-1, 512)
    voxels[ptr] = MD.default_voxels(512, sc.voxelType)
    ses.scene.upload(capi.BUF_VOXEL_BLOCKS, voxels.reshape(-1))
    m.Touch(slots=[slot])
    stats, _ = assert_update(m, ses, table, [slot])
    assert stats["full"] == 0 and stats["marked"] == 1 and 1 < stats["remeshed"] <= 8
    after = MU.runs(table, ses.scene.download(capi.BUF_VOXEL_BLOCKS), m.triangles())[0]
    others = [s for s in after if s != slot and after[s] != before[s]]
    print(f"block {slot} at {table['pos'][slot]} emptied: {len(others)} other blocks changed their run")
    assert len(others) >= 1 and len(after[slot]) == 0
    m.close(); ses.close()


@pytest.mark.gpu
def test_hip_presence_changes_need_no_touch(hip):
    sc = replace(SC, frames=3)
    ses = MC.fuse(hip, sc)
    m = Mesh(ses.scene)
    m.MeshScene()
    table = table_of(ses)
    pos = table["pos"][MU.listed(table)].astype(np.int64)
    centre = pos[np.argmin(np.abs(pos - np.median(pos, axis=0)).sum(axis=1))]          # a block of the surface (the medians alone may lie off it)
    cfg = ses.scene.prune_config(classes=capi.PRUNE_BOX, boxMin=tuple(int(c) - 3 for c in centre), boxMax=tuple(int(c) + 3 for c in centre))
    dropped = ses.scene.prune(cfg)["dropped"]
    assert dropped > 0
    stats, table = assert_update(m, ses, table, [])
    assert stats["full"] == 0 and stats["appeared"] == 0 and stats["vanished"] == dropped and stats["noRemoved"] == dropped
    # the next frame allocates some of them again, maybe in other slots: still no touch for presence, the frame's own touch for its voxels
    ses.frame(3)
    m.Touch(ses.rs)
    stats, _ = assert_update(m, ses, table, visible(ses))
    assert stats["full"] == 0 and stats["appeared"] > 0
    m.close(); ses.close()


@pytest.mark.gpu
def test_hip_full_paths(hip):
    sc = replace(SC, frames=2)
    ses = MC.fuse(hip, sc)
    m = Mesh(ses.scene)
    table = table_of(ses)
    assert_update(m, ses, None, [], run_current=False)                    # never meshed
    assert m.Update()["remeshed"] == 0                                    # and now nothing is left to do
    m.Index()
    m.Smooth(steps=1)
    assert assert_update(m, ses, None, [], run_current=False)[0]["full"] == capi.MESH_UPDATE_NO_RUN_TABLE
    m.Index(); m.Components()
    m.FilterComponents(100)
    assert assert_update(m, ses, None, [], run_current=False)[0]["full"] == capi.MESH_UPDATE_NO_RUN_TABLE
    m.Touch(everything=True)
    m.Touch(slots=[5, 6])
    assert assert_update(m, ses, table, [5, 6], everything=True)[0]["full"] == capi.MESH_UPDATE_ALL_MARKED
    assert m.Update()["full"] == 0                                        # the word is consumed
    # a buffer that the first frames fit and the later ones do not
    n2 = m.info()[0]
    small = Mesh(ses.scene, n2 + 2)
    small.MeshScene()
    assert small.info() == (n2, n2 + 2)
    marks = []
    for k in (2, 3, 4, 5):
        ses.frame(k)
        small.Touch(ses.rs)
        marks.append(visible(ses))
    stats, table5 = assert_update(small, ses, table, np.concatenate(marks), max_triangles=n2 + 2, overflow=True)
    assert stats["full"] == capi.MESH_UPDATE_OVERFLOW and stats["trianglesGenerated"] > n2 + 1 and small.info() == (n2 + 1, n2 + 2)
    # a buffer that is full holds no run table: the next update is a full one again
    assert assert_update(small, ses, None, [], max_triangles=n2 + 2, run_current=False)[0]["full"] == capi.MESH_UPDATE_NO_RUN_TABLE
    small.close(); m.close(); ses.close()


@pytest.mark.gpu
def test_hip_other_cases(hip):
    sc = replace(SC, frames=2)
    ses = MC.fuse(hip, sc)
    m = Mesh(ses.scene)
    m.MeshScene()
    table = table_of(ses)
    n = len(table)
    with raises_invalid():
        m.update_delta()                                                  # no update yet
    m.Touch(slots=[])
    stats, _ = assert_update(m, ses, table, [])
    assert stats["full"] == 0 and stats["remeshed"] == 0 and stats["kept"] == stats["allocated"] and stats["trianglesGenerated"] == 0
    inside = MU.listed(table)[:3].tolist()
    marks = inside + [-1, n, n + 7, 2 ** 31 - 1, inside[0]]
    m.Touch(slots=marks)
    stats, _ = assert_update(m, ses, table, marks)
    assert stats["ignoredMarks"] == 4 and stats["marked"] == 3 and stats["remeshed"] >= 3
    assert m.Update()["ignoredMarks"] == 0
    # refusals: a foreign scene, a dense scene, a render state of another scene, a list without a count
    other = T.Session(hip, replace(sc, frames=1))
    for call in (lambda: hip.fn["mesh_touch"](m.h, other.scene.h, None, None, -1, None), lambda: hip.fn["mesh_update"](other.scene.h, m.h, None, None),
                 lambda: hip.fn["mesh_touch"](m.h, ses.scene.h, other.rs.h, None, 0, None), lambda: hip.fn["mesh_touch"](m.h, ses.scene.h, None, None, 0, None)):
        assert call() == -1 and hip.fn["last_error"]()
    other.close()
    dense = MC.fuse(hip, MC.DENSE)
    dm = Mesh(dense.scene)
    dm.MeshVolume()
    tri = dm.triangles()
    with raises_invalid():
        dm.Touch(everything=True)
    with raises_invalid():
        dm.Update()
    assert np.array_equal(bits(dm.triangles()), bits(tri)) and len(tri) > 0
    assert_update(m, ses, table, [])                                      # the refusals changed nothing
    dm.close(); dense.close(); m.close(); ses.close()


# ---- the adapters ---------------------------------------------------------------------------------------------------------------------

DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "mesh_update_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "mesh_update_demo")


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_demo_and_main_engine_live_mesh_compile(tmp_path):
    assert os.path.exists(build_demo())
    assert "tests/cpp/mesh_update_demo\n" in open(os.path.join(T.ROOT, ".gitignore")).read()
    src = tmp_path / "live_mesh.cpp"
    src.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template class ITMMainEngine_HIP<ITMVoxel_f_rgb, ITMVoxelBlockHash>;\n'
                   'template class ITMMainEngine_HIP<ITMVoxel_s, ITMPlainVoxelArray>;\n'
                   'int f(ITMLibSettings& st) { st.liveMeshEveryNFrames = 4; return st.pruneEveryNFrames; }\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_demo_gives_the_bindings_bytes(hip, tmp_path):
    exe = build_demo()
    path, mine, scratch = str(tmp_path / "demo.stl"), str(tmp_path / "python.stl"), str(tmp_path / "fresh.stl")
    got = json.loads(subprocess.run([exe, "adapter", path], check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])
    W, H, P = 160, 120, 160 * 120
    s = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.01))
    s.reco.ResetScene()
    rs = s.vis.CreateRenderState((W, H))
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    depth = (F(1.5) + F(0.002) * ((x * 7 + y * 13) % 50).astype(F)).astype(F)
    d_depth = hip.to_backend(depth)
    pts = capi.DevBuffer(hip, P * 16, F, (P, 4)); nrm = capi.DevBuffer(hip, P * 16, F, (P, 4))
    m = Mesh(s)
    for k in range(3):
        M = np.eye(4, dtype=F); M[0, 3] = F(-0.2) * F(k)
        v = capi.View(d_depth, W, H, M_d=np.ascontiguousarray(M.T).reshape(16), intr_d=(145.0, 145.0, 80.0, 60.0))
        s.process_frame(v, rs, pts, nrm)
        if k == 0:
            m.MeshScene()
            continue
        m.Touch(rs)
        stats = m.Update()
    assert got == stats and stats["full"] == 0 and stats["trianglesCopied"] > 0 and stats["appeared"] > 0
    m.WriteSTL(mine)
    again = Mesh(s)
    again.MeshScene()
    again.WriteSTL(scratch)
    assert open(path, "rb").read() == open(mine, "rb").read() == open(scratch, "rb").read() and os.path.getsize(path) == 84 + 50 * stats["trianglesAfter"]


@pytest.mark.gpu
def test_main_engine_live_mesh_equals_the_export(hip, tmp_path):
    exe = build_demo()
    live, exported = str(tmp_path / "live.stl"), str(tmp_path / "export.stl")
    got = json.loads(subprocess.run([exe, "engine", live, exported], check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1])
    print(got)
    assert got["full"] == 0 and 0 < got["remeshed"] < got["allocated"] and got["trianglesCopied"] > 0
    assert open(live, "rb").read() == open(exported, "rb").read() and os.path.getsize(live) == 84 + 50 * got["trianglesAfter"] > 84 + 50 * 1000
