"""The sdf mirror is PAGED (infinitam_amd/csrc/accel_device.h): a 16 KB table over the mirror's cube of 256^3 blocks says which
16 x 16 x 16-block pages hold blocks; pages (4 MB of int16 sdf) come from a pool as blocks are allocated.  The reference's footprint is O(pool)
(ITMLib/Objects/ITMLocalVBA.h:18-59); the mirror's now is too (rounds 2-3: 17 GB per scene whatever it held).

Here: (the dense cube remains the default while the device has 3 x 17 GB to spare: it is the faster form, ray cast 38.3 us against 42.8-43.4.)  The footprint on the bench scene, a pool too small for the scene (pages that could not be mapped say nothing: their rays use
the block directory, same results), and pages returning to the pool when the cube moves or the scene is reset."""
import numpy as np
import pytest

import itm_testlib as T
from infinitam_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def paged(monkeypatch):
    """The paged form is what these tests are about (a device with 3 x 17 GB to spare would pick the dense cube)."""
    monkeypatch.setenv("ITM_MIRROR", "paged")

PAGE = 16          # blocks per side of a page (ITM_MIRROR_PAGE_BITS = 4)


def pages_wanted(scene):
    """Distinct pages of the mirror's cube that hold an allocated block, from the table and the cube's origin."""
    info = scene.accel_info()
    e = scene.download(capi.BUF_HASH_ENTRIES)
    c = e["pos"][e["ptr"] >= 0].astype(np.int64) - np.asarray(info["origin_mirror"], np.int64)
    c = c[((c >= 0) & (c < 256)).all(axis=1)] // PAGE
    return len(np.unique(c[:, 0] + 16 * c[:, 1] + 256 * c[:, 2]))


def test_mirror_memory_follows_the_scene_not_the_cube(hip, oracle):
    sc = T.Scenario(name="paged_bench", voxelSize=0.004, localBlockNum=0x40000, frames=6, trajectory="bench")
    ses = T.Session(hip, sc)
    for k in range(sc.frames):
        ses.frame(k, fused="four")
    info = ses.scene.accel_info()
    blocks = int(np.count_nonzero(ses.scene.download(capi.BUF_HASH_ENTRIES)["ptr"] >= 0))
    assert 0 < info["mirror_bytes"] < (1 << 30), info                     # 768 MB pool + 16 KB table (rounds 2-3: 17.18 GB)
    want = pages_wanted(ses.scene)
    assert info["mirror_pages"] == 192 and info["mirror_pages_mapped"] == want and 20 < want < 192, (info, want, blocks)
    a = ses.snapshot(); a.counters = [ses.scene.counters(ses.rs)]
    ref = T.Session(oracle, sc)
    for k in range(sc.frames):
        ref.frame(k)
    b = ref.snapshot(); b.counters = [ref.scene.counters(ref.rs)]
    T.compare_results(a, b, sc, what="paged mirror")
    ses.scene.reco.ResetScene()
    assert ses.scene.accel_info()["mirror_pages_mapped"] == 0, "pages after ResetScene"
    ses.close(); ref.close()


@pytest.mark.parametrize("pages", [1, 5, 12])
def test_a_pool_that_runs_dry_costs_speed_not_results(hip, oracle, monkeypatch, pages):
    """ITM_MIRROR_PAGES (read when the scene is created): with 1, 5 or 12 pages most, many or some of the scene's pages cannot be
    mapped; their table entries say "unmappable", rays through them read the block directory.  Five frames of a turning camera, the
    free-view entry points from another pose, then a cube move (everything unmapped and mapped again at the new origin)."""
    monkeypatch.setenv("ITM_MIRROR_PAGES", str(pages))
    sc = T.Scenario(name="paged_dry_%d" % pages, voxelSize=0.005, w=320, h=240, frames=5, trajectory="yaw")
    a = T.run_scenario(hip, sc, fused="four")
    b = T.run_scenario(oracle, sc)
    T.compare_results(a, b, sc, what=sc.name)
    ses = T.Session(hip, sc)
    for k in range(2):
        ses.frame(k, fused=True)
    info = ses.scene.accel_info()
    want = pages_wanted(ses.scene)
    assert info["mirror_pages"] == pages and info["mirror_pages_mapped"] == pages and want > 12, (info, want)
    ses.close()


def test_pages_return_to_the_pool_when_the_cube_moves(hip, oracle):
    from test_accel_origin import walk_poses
    poses = walk_poses()
    sc = T.Scenario(name="paged_walk", w=160, h=120, voxelSize=0.005, localBlockNum=0x40000, frames=len(poses))
    res, mapped = [], []
    for be in (hip, oracle):
        ses = T.Session(be, sc)
        depth = [be.to_backend(sc.depth(k)) for k in range(sc.frames)]
        for k in range(sc.frames):
            v = capi.View(depth[k], sc.w, sc.h, M_d=poses[k], intr_d=sc.intr())
            ses.scene.process_frame(v, ses.rs, ses.points, ses.normals)
            if be is hip:
                mapped.append(ses.scene.accel_info()["mirror_pages_mapped"])
        r = ses.snapshot(); r.counters = [ses.scene.counters(ses.rs)]
        res.append(r)
        if be is hip:
            assert ses.scene.accel_info()["moves"] >= 3
        ses.close()
    T.compare_results(res[0], res[1], sc, what="paged mirror across cube moves")
    assert max(mapped) <= 192 and min(mapped) > 0
