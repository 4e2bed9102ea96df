"""Everything the library allocates goes through csrc/device_memory.h (DeviceBuffer / PinnedBuffer over one pair of functions):

  1. no other file of csrc calls the runtime's allocation functions (the four raw entry points of scene.hip excepted);
  2. every owner gives back exactly what it took (itm_debug_memory: live allocations and live bytes);
  3. every single allocation of every listed path may fail (ITM_DEBUG_FAIL_ALLOCATION): the call reports ITM_ERR_DEVICE -- or, where
     the allocation is documented as optional, succeeds without that form --, leaves nothing behind, and the same call then succeeds
     with the result of a clean run.

The scene used throughout: 1024 buckets, 256 excess entries, 512 blocks, ITMVoxel_s, a 64 x 48 render state, the paged mirror with a
pool of two pages.  Frames are those of a 64 x 48 Scenario at 2 cm voxels (about 200 blocks: they fit the pool)."""
import ctypes as C
import gc
import os
import re

import numpy as np
import pytest

import colour_cases as CC
import itm_testlib as T
from infinitam_amd import capi
from infinitam_amd.capi import TrackerConfig

CSRC = os.path.join(T.ROOT, "infinitam_amd", "csrc")
DEBUG_FAIL_ALLOCATION = 28           # include/itm_debug.h
W, H = 64, 48
TABLE = dict(bucketNum=1024, excessNum=256, localBlockNum=512)
SC = T.Scenario(name="memory", w=W, h=H, voxelSize=0.02, mu=0.06, frames=1, **TABLE)


# ---- 1. the source ----------------------------------------------------------------------------------------------------------------
def test_no_allocation_call_outside_device_memory_h():
    calls = re.compile(r"\b(hipMalloc|hipHostMalloc|hipFree|hipHostFree)\(")
    raw_entry_points = {"itm_dev_malloc": "hipMalloc", "itm_dev_free": "hipFree", "itm_host_malloc": "hipHostMalloc", "itm_host_free": "hipHostFree"}
    found = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h", ".hpp", ".cpp")) or name == "device_memory.h":
            continue
        text = open(os.path.join(CSRC, name), errors="replace").read()
        if name == "scene.hip":
            # the bodies of the four entry points that hand raw memory to the host: each holds exactly its one call
            for fn, call in raw_entry_points.items():
                m = re.search(r"^int %s\(.*?\}[ \t]*$" % fn, text, re.S | re.M)
                assert m, fn
                assert calls.findall(m.group(0)) == [call], fn
                text = text.replace(m.group(0), "")
        found += [(name, c) for c in calls.findall(text)]
    assert not found, f"allocation calls outside device_memory.h: {found}"
    assert "device_memory.h" in open(os.path.join(CSRC, "Makefile")).read()
    assert f"#define ITM_DEBUG_FAIL_ALLOCATION {DEBUG_FAIL_ALLOCATION} " in open(os.path.join(T.ROOT, "include", "itm_debug.h")).read()


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def memory(be):
    """(live allocations, live bytes, allocations attempted since load)"""
    out = (C.c_int64 * 3)()
    be.check(be.fn["debug_memory"](out), "debug_memory")
    return tuple(out)


def live(be):
    return memory(be)[:2]


def fail_allocation(be, n):
    be.check(be.fn["debug_set"](DEBUG_FAIL_ALLOCATION, n), "debug_set")


def rc_of(call):
    """The return code of a call made through the binding's checking wrappers."""
    try:
        call()
        return 0
    except capi.ItmError as e:
        return int(re.search(r"failed \((-?\d+)\)", str(e)).group(1))


def fp(a):
    a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


@pytest.fixture
def hipm(hip, monkeypatch):
    """The backend with the mirror form of this file set for every scene the test creates, and the caches that live as long as the
    process warm: the calling thread's handle-less tracker and the image-map slots of the stream used (the null stream)."""
    monkeypatch.setenv("ITM_MIRROR", "paged")
    monkeypatch.setenv("ITM_MIRROR_PAGES", "2")
    for var in ("ITM_MIRROR_BITS", "ITM_NO_ACCELERATION_CUBES"):
        monkeypatch.delenv(var, raising=False)
    fail_allocation(hip, 0)
    ses = fused_session(hip)
    cfg = icp_config()
    view = capi.View(ses._depth, W, H, M_d=SC.pose(0), intr_d=SC.intr()).struct()
    out = (C.c_float * 16)()
    hip.check(hip.fn["track_camera"](C.byref(cfg), C.byref(view), ses.points.ptr, ses.normals.ptr, fp(SC.pose(0))[1], out, None), "track_camera")
    img = capi.DevBuffer(hip, W * H * 4, np.uint8, (H, W, 4))
    ses.scene.vis.DepthToUchar4(img, ses._depth, (W, H))
    hip.sync()
    img.close()
    ses.close()
    # a Scene and its two engines refer to each other: one that an earlier test left unclosed holds its device memory until the cycle
    # collector runs -- now, not between two readings of live()
    gc.collect()
    yield hip
    fail_allocation(hip, 0)


def icp_config():
    cfg = TrackerConfig.default()
    cfg.noHierarchyLevels = 2          # 64 x 48 and 32 x 24
    cfg.trackingRegime[:2] = [3, 1]
    return cfg


def fused_session(be, sc=SC, frames=1):
    ses = T.Session(be, sc)
    for k in range(frames):
        ses.frame(k, fused=True)
    be.sync()
    return ses


def create_scene(be, **kw):
    return be.create_scene(capi.VOXEL_S, capi.INDEX_HASH, SC.params(), **TABLE, **kw)


def scene_forms(scene):
    info = scene.accel_info()
    return (info["directory_bytes"], info["slot_directory_bytes"], info["mirror_bytes"], info["mirror_pages"])


# ---- 2. balanced lifetimes ------------------------------------------------------------------------------------------------------
class IcpHandle:
    def __init__(self, be):
        self.be, self.h = be, C.c_void_p()
        be.check(be.fn["tracker_create"](C.byref(self.h)), "tracker_create")

    def track(self, ses):
        cfg = icp_config()
        view = capi.View(ses._depth, W, H, M_d=SC.pose(0), intr_d=SC.intr()).struct()
        out = (C.c_float * 16)()
        self.be.check(self.be.fn["tracker_track_camera"](self.h, C.byref(cfg), C.byref(view), ses.points.ptr, ses.normals.ptr, fp(SC.pose(0))[1], out, None),
                      "tracker_track_camera")
        return np.array(out[:], np.float32).tobytes()

    def track_weighted(self, ses, sigma):
        cfg = icp_config()
        view = capi.View(ses._depth, W, H, M_d=SC.pose(0), intr_d=SC.intr()).struct()
        out = (C.c_float * 16)()
        self.be.check(self.be.fn["tracker_weighted_track_camera"](self.h, C.byref(cfg), C.byref(view), sigma.ptr, ses.points.ptr, ses.normals.ptr,
                                                                  fp(SC.pose(0))[1], out, None), "tracker_weighted_track_camera")
        return np.array(out[:], np.float32).tobytes()

    def close(self):
        if self.h:
            self.be.check(self.be.fn["tracker_destroy"](self.h), "tracker_destroy")
            self.h = C.c_void_p()


class ColourHandle:
    """The colour tracker on the suite's colour case (colour_cases.py: a 320 x 240 cloud, a VGA frame)."""
    _inputs = None

    def __init__(self, be):
        self.be, self.h = be, C.c_void_p()
        be.check(be.fn["colour_tracker_create"](C.byref(self.h)), "colour_tracker_create")

    @classmethod
    def inputs(cls, be):
        if cls._inputs is None:
            loc, col = CC.cloud()
            M = CC.motions()["both"][0]
            cls._inputs = (be.to_backend(loc), be.to_backend(col), loc.shape[0], be.to_backend(np.ascontiguousarray(CC.frame(M))),
                           be.to_backend(np.zeros((CC.H, CC.W), np.float32)), np.asarray(M, np.float32))
        return cls._inputs

    def track(self):
        loc, col, n, rgb, dummy, M = self.inputs(self.be)
        v = capi.View(dummy, CC.W, CC.H, M_d=M, intr_d=CC.INTR, rgb=rgb, w_rgb=CC.W, h_rgb=CC.H, intr_rgb=CC.INTR)
        cfg = TrackerConfig.default()
        cfg.noHierarchyLevels = CC.LEVELS
        cfg.trackingRegime[:CC.LEVELS] = CC.REGIME
        out = (C.c_float * 16)()
        self.be.check(self.be.fn["colour_tracker_track_camera"](self.h, C.byref(cfg), C.byref(v.struct()), None, loc.ptr, col.ptr, n, out, None),
                      "colour_tracker_track_camera")
        return np.array(out[:], np.float32).tobytes()

    def close(self):
        if self.h:
            self.be.check(self.be.fn["colour_tracker_destroy"](self.h), "colour_tracker_destroy")
            self.h = C.c_void_p()


class RenHandle:
    def __init__(self, be):
        self.be, self.h = be, C.c_void_p()
        be.check(be.fn["ren_tracker_create"](C.byref(self.h)), "ren_tracker_create")

    def track(self, ses):
        v = capi.View(ses._depth, W, H, M_d=SC.pose(0), intr_d=SC.intr())
        out, n = (C.c_float * 16)(), C.c_int()
        self.be.check(self.be.fn["ren_tracker_track_camera"](self.h, C.c_void_p(ses.scene.h), C.byref(v.struct()), out, C.byref(n), None),
                      "ren_tracker_track_camera")
        return np.array(out[:], np.float32).tobytes() + bytes([n.value & 255])

    def close(self):
        if self.h:
            self.be.check(self.be.fn["ren_tracker_destroy"](self.h), "ren_tracker_destroy")
            self.h = C.c_void_p()


class Stager:
    def __init__(self, be):
        self.be, self.h = be, C.c_void_p()
        be.check(be.fn["depth_stager_create"](W, H, 3, C.byref(self.h)), "depth_stager_create")

    def close(self):
        if self.h:
            self.be.check(self.be.fn["depth_stager_destroy"](self.h), "depth_stager_destroy")
            self.h = C.c_void_p()


def sigma_image(be):
    return be.to_backend(np.full((H, W), 0.01, np.float32))


def source_scene(be):
    """A second scene of the same table with frame 1 of the scenario fused: what itm_scene_merge merges into the first."""
    ses = T.Session(be, SC)
    ses.frame(1, fused=True)
    be.sync()
    return ses


@pytest.mark.gpu
def test_every_owner_gives_back_what_it_took(hipm):
    be = hipm
    base = live(be)

    def balanced(what):
        assert live(be) == base, what

    for order in ("scene first", "render state first"):
        s = create_scene(be)
        rs = s.vis.CreateRenderState((W, H))
        assert live(be)[0] > base[0]
        (s, rs)[order != "scene first"].close()
        (rs, s)[order != "scene first"].close()
        balanced(order)

    ses = fused_session(be)
    m = capi.Mesh(ses.scene)
    m.MeshScene(); m.ComputeAttributes(capi.MESH_NORMALS); m.Index()
    assert m.info()[0] > 0 and m.index_info()[0] > 0
    held = live(be)
    m.close()
    assert live(be)[0] < held[0]
    sigma = sigma_image(be)
    for make, run in ((IcpHandle, lambda t: t.track(ses)), (IcpHandle, lambda t: t.track_weighted(ses, sigma)), (ColourHandle, lambda t: t.track()),
                      (RenHandle, lambda t: t.track(ses))):
        before = live(be)
        t = make(be)
        run(t)
        assert live(be)[0] > before[0], make.__name__
        t.close()
        assert live(be) == before, make.__name__
    r = capi.Relocaliser(be, W, H)
    r.process_frame(ses._depth, M_d=SC.pose(0))
    r.close()
    src = source_scene(be)
    before = live(be)
    dst = create_scene(be)
    dst.reco.ResetScene()
    assert dst.merge_from(src.scene)["considered"] > 0
    dst.close()
    assert live(be) == before, "destination of a merge"
    src.close()
    ses.close()
    balanced("mesh, trackers, relocaliser, merge")

    s = create_scene(be, useSwapping=True, transferBlockNum=64)
    s.close()
    balanced("swapping scene")
    g = Stager(be)
    be.check(be.fn["depth_stager_set_conversion"](g.h, 1, 0.001, 0.0, 0.0), "depth_stager_set_conversion")
    g.close()
    balanced("depth stager")


def half_view(be, ses):
    """Frame 0 with the right half of the image invalid: a smaller surface than the whole frame's."""
    d = SC.depth(0).copy()
    d[:, W // 2:] = 0.0
    ses._half = be.to_backend(d)
    return capi.View(ses._half, W, H, M_d=SC.pose(0), intr_d=SC.intr())


@pytest.mark.gpu
def test_reserve_grows_only(hipm):
    """itm_mesh_index sizes its buffers from the mesh: a larger mesh grows them, the smaller one again allocates nothing."""
    be = hipm
    ses = T.Session(be, SC)
    m = capi.Mesh(ses.scene)

    def fuse_and_index(view):
        ses.scene.process_frame(view, ses.rs, ses.points, ses.normals)
        m.MeshScene()
        n = m.info()[0]
        a0 = memory(be)[2]
        m.Index()
        return n, memory(be)[2] - a0, m.index_info()

    try:
        n1, grew1, idx1 = fuse_and_index(half_view(be, ses))
        n2, grew2, idx2 = fuse_and_index(ses.view(0))
        assert 0 < n1 < n2 and grew1 > 0 and grew2 > 0
        ses.scene.reco.ResetScene()
        n3, grew3, idx3 = fuse_and_index(half_view(be, ses))
        assert (n3, idx3) == (n1, idx1) and grew3 == 0
    finally:
        m.close()
        ses.close()


# ---- 3. every allocation may fail ------------------------------------------------------------------------------------------------
class Path:
    """One call whose allocations are failed one by one.  prepare() makes what the call needs (the "handle alone"); run() makes the
    call and returns nothing (it raises ItmError on a non-zero return code); result() is what a clean run and the retry must agree
    on; undo() takes back what a successful run() created (create functions only); close() destroys what prepare() made.
    degraded(): the call succeeded although an allocation failed -- true where what is now missing is documented as optional."""
    name = ""
    creates = False          # a create function: undo() destroys what run() made

    def prepare(self, be): pass
    def run(self, be): raise NotImplementedError
    def result(self, be): return None
    def undo(self, be): pass
    def close(self, be): pass
    def degraded(self, be, clean): return False


class CreateScene(Path):
    name = "itm_scene_create"
    creates = True
    kw = {}

    def run(self, be): self.s = create_scene(be, **self.kw)
    def result(self, be): return scene_forms(self.s)
    def undo(self, be): self.s.close()

    def degraded(self, be, clean):
        # optional: both directories and the mirror's three buffers (the scene then reports that form as absent) and the status word
        # (not reported anywhere: the scene then simply holds one allocation less)
        forms = scene_forms(self.s)
        absent = [a == 0 and b != 0 for a, b in zip(forms[:3], clean[:3])]
        return any(absent) or forms == clean


class CreateSwappingScene(CreateScene):
    name = "itm_scene_create (swapping)"
    kw = dict(useSwapping=True, transferBlockNum=64)


class CreateRenderState(Path):
    name = "itm_render_state_create"
    creates = True

    def prepare(self, be): self.s = create_scene(be)
    def run(self, be): self.rs = self.s.vis.CreateRenderState((W, H))
    def undo(self, be): self.rs.close()
    def close(self, be): self.s.close()


class CreateMesh(CreateRenderState):
    name = "itm_mesh_create"

    def run(self, be): self.rs = capi.Mesh(self.s)


class CreateHandle(Path):
    creates = True

    def __init__(self, cls): self.cls, self.name = cls, cls.__name__ + " create"
    def run(self, be): self.t = self.cls(be)
    def undo(self, be): self.t.close()


class CreateRelocaliser(Path):
    name = "itm_reloc_create"
    creates = True

    def run(self, be): self.r = capi.Relocaliser(be, W, H)
    def undo(self, be): self.r.close()


class WithSession(Path):
    def prepare(self, be): self.ses = fused_session(be)
    def close(self, be): self.ses.close()


class FindVisible(WithSession):
    """n = 2 of its two is the half-allocated state: flags without chunk counts, with which the next call used to launch."""
    name = "itm_find_visible_blocks"

    def run(self, be): self.ses.scene.vis.FindVisibleBlocks(SC.pose(0), SC.intr(), self.ses.rs)

    def result(self, be):
        n = self.ses.scene.counters(self.ses.rs)["noVisibleEntries"]
        return n, self.ses.scene.download(T.BUF_VISIBLE_IDS, self.ses.rs)[:n].tobytes()


class MeshPath(WithSession):
    def prepare(self, be):
        super().prepare(be)
        self.m = capi.Mesh(self.ses.scene)
        self.m.MeshScene()

    def close(self, be):
        self.m.close()
        super().close(be)


class MeshAttributes(MeshPath):
    name = "itm_mesh_attributes"

    def run(self, be): self.m.ComputeAttributes(capi.MESH_NORMALS)
    def result(self, be): return self.m.info(), self.m.normals().tobytes()


class MeshIndex(MeshPath):
    name = "itm_mesh_index"

    def run(self, be): self.m.Index()
    def result(self, be): return self.m.index_info(), self.m.faces().tobytes(), self.m.vertices().tobytes()


class MeshVolumeDense(Path):
    name = "itm_mesh_volume (dense)"

    def prepare(self, be):
        self.s = be.create_scene(capi.VOXEL_S, capi.INDEX_DENSE, SC.params(), denseSize=(16, 16, 16), denseOffset=(-8, -8, 40))
        self.s.reco.ResetScene()
        self.m = capi.Mesh(self.s, 4096)

    def run(self, be): self.m.MeshVolume()
    def result(self, be): return self.m.info()

    def close(self, be):
        self.m.close()
        self.s.close()


class Track(WithSession):
    def __init__(self, cls, how, name): self.cls, self.how, self.name = cls, how, name

    def prepare(self, be):
        super().prepare(be)
        self.sigma = sigma_image(be)
        self.t = self.cls(be)

    def run(self, be): self.out = self.how(self)
    def result(self, be): return self.out

    def degraded(self, be, clean):
        # optional: the command granules in BAR-mapped device memory (tracker.hip, session_reserve: pinned host memory otherwise); the
        # pose is the same bit for bit
        return self.cls is IcpHandle and self.out == clean

    def close(self, be):
        self.t.close()
        self.sigma.close()
        super().close(be)


class Merge(Path):
    name = "itm_scene_merge"

    def prepare(self, be):
        self.src = source_scene(be)
        self.dst = fused_session(be)

    def run(self, be): self.stats = self.dst.scene.merge_from(self.src.scene)
    def result(self, be): return self.stats

    def close(self, be):
        self.dst.close()
        self.src.close()


PATHS = [CreateScene(), CreateSwappingScene(), CreateRenderState(), CreateMesh(), CreateHandle(IcpHandle), CreateHandle(ColourHandle), CreateHandle(RenHandle),
         CreateHandle(Stager), CreateRelocaliser(), FindVisible(), MeshVolumeDense(), MeshAttributes(), MeshIndex(),
         Track(IcpHandle, lambda p: p.t.track(p.ses), "itm_tracker_track_camera"),
         Track(IcpHandle, lambda p: p.t.track_weighted(p.ses, p.sigma), "itm_tracker_weighted_track_camera"),
         Track(ColourHandle, lambda p: p.t.track(), "itm_colour_tracker_track_camera"),
         Track(RenHandle, lambda p: p.t.track(p.ses), "itm_ren_tracker_track_camera"), Merge()]


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS, ids=[p.name for p in PATHS])
def test_every_allocation_may_fail(hipm, path):
    be = hipm
    # the clean run: how many allocations the call attempts, and what it gives
    path.prepare(be)
    a0 = memory(be)[2]
    path.run(be)
    N = memory(be)[2] - a0
    clean = path.result(be)
    path.undo(be)
    path.close(be)
    print(f"{path.name}: {N} allocations")
    for n in range(1, N + 1):
        path.prepare(be)
        alone = live(be)
        fail_allocation(be, n)
        rc = rc_of(lambda: path.run(be))
        fail_allocation(be, 0)          # (it has cleared itself: the n-th attempt was made)
        if rc == 0:
            # only where what is now missing is documented as optional; what the call made is taken back before the retry (a first-use
            # path keeps what it allocated: its retry is then no first call any more, and still has to give the clean result)
            assert path.degraded(be, clean), f"{path.name}: allocation {n} of {N} failed and the call succeeded"
            path.undo(be)
            if path.creates:
                assert live(be) == alone, f"{path.name}: allocation {n} of {N}"
        else:
            assert rc == capi.ERR_DEVICE, (path.name, n, rc)
            assert live(be) == alone, f"{path.name}: allocation {n} of {N} failed and something stayed behind"
        path.run(be)                    # the same call with the key off
        assert path.result(be) == clean, (path.name, n)
        path.undo(be)
        path.close(be)
