"""The block directory, the slot directory and the sdf mirror audited DIRECTLY (tests/accel_terms.py against the read-only probe and
census of include/itm_debug.h) after every step of every operation that writes them, in every form the mirror can take:

    (a) default (the dense cube sized from the frustum)      (e) ITM_MIRROR=paged, ITM_MIRROR_PAGES=1
    (b) ITM_MIRROR=dense, ITM_MIRROR_BITS=6                  (f) ITM_MIRROR=paged, ITM_MIRROR_PAGES=5
    (c) ITM_MIRROR=dense, ITM_MIRROR_BITS=5 (smaller than    (g) ITM_MIRROR=off
        the frustum ball: it moves on every frame)           (h) VOXEL_F_RGB: directories only
    (d) ITM_MIRROR=paged, default pool

The behavioural tests (ray cast / ICP maps against the oracle) see a stale cell only if a ray of their poses steps through it; here a
cell left behind at an old origin, a mirror block that is not "absent" after a swap-out or a page that stays mapped after an unfill is
a finding wherever it lies.  Where the oracle can run the same sequence the bit-exact comparison of the maps is kept."""
import numpy as np
import pytest

import accel_terms as A
import itm_testlib as T
import test_scene_merge as TM
import test_swapping
from infinitam_amd import capi, synth
from test_accel_origin import walk_poses

pytestmark = pytest.mark.gpu

W, H = 160, 120
POOL = 0x4000
FORMS = {
    "a": {},
    "b": {"ITM_MIRROR": "dense", "ITM_MIRROR_BITS": "6"},
    "c": {"ITM_MIRROR": "dense", "ITM_MIRROR_BITS": "5"},
    "d": {"ITM_MIRROR": "paged"},
    "e": {"ITM_MIRROR": "paged", "ITM_MIRROR_PAGES": "1"},
    "f": {"ITM_MIRROR": "paged", "ITM_MIRROR_PAGES": "5"},
    "g": {"ITM_MIRROR": "off"},
    "h": {},
}


@pytest.fixture
def form(request, monkeypatch):
    """The variables are read when a scene is created: set for the whole test."""
    name = request.param
    for var in ("ITM_MIRROR", "ITM_MIRROR_BITS", "ITM_MIRROR_PAGES", "ITM_NO_ACCELERATION_CUBES"):
        monkeypatch.delenv(var, raising=False)
    for var, value in FORMS[name].items():
        monkeypatch.setenv(var, value)
    return name


def forms(letters):
    return pytest.mark.parametrize("form", list(letters), indirect=True)


def voxel_kw(form):
    return dict(voxelType=capi.VOXEL_F_RGB, colour=True) if form == "h" else {}


def check_form(scene, form):
    """The scene got the form the test asked for (1 cm voxels: the frustum reaches 39.5 blocks, the default dense cube is 64 per side)."""
    info = scene.accel_info()
    geo = A.geometry(info, scene.cfg.voxelType)
    assert geo["dir"] and geo["slot"], (form, info)
    want = {"a": ("dense", 64, 0), "b": ("dense", 64, 0), "c": ("dense", 32, 0), "d": ("paged", 256, 192), "e": ("paged", 256, 1), "f": ("paged", 256, 5),
            "g": ("none", 0, 0), "h": ("none", 0, 0)}[form]
    assert (geo["form"], geo["side"], geo["pages"]) == want, "form (%s): wanted %s, accel_info says %s" % (form, want, info)


def check_situation(form, facts):
    """What the form is for, from the table and accel_info (not from the probe): unmappable pages in (e) and (f)."""
    if form in ("e", "f"):
        assert max(f["in_unmappable_pages"] for f in facts) > 0, "form (%s): no block lies in an unmappable page" % form


_oracle_results = {}


def oracle_once(key, fn):
    """A reference is computed once and shared by the forms."""
    if key not in _oracle_results:
        _oracle_results[key] = fn()
    return _oracle_results[key]


# ---- 1. frames --------------------------------------------------------------------------------------------------------------------

def run_frames(be, sc, audit):
    ses = T.Session(be, sc)
    facts = []
    ses.frame(0, fused=False); audit(ses, facts, "frame 0, four launched calls")
    ses.frame(1, fused=True); audit(ses, facts, "frame 1, process_frame")
    v = ses.view(2)
    ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
    ses.scene.reco.IntegrateIntoScene(v, ses.rs)
    ses.scene.vis.CreateExpectedDepths(v.M_d, v.intr_d, ses.rs)
    audit(ses, facts, "frame 2, three calls recorded and not flushed")          # the hook launches them
    ses.scene.vis.CreateICPMaps(v, ses.rs, ses.points, ses.normals)
    audit(ses, facts, "frame 2, after the ICP maps")
    ses.frame(3, fused="four"); audit(ses, facts, "frame 3, four recorded calls")
    res = ses.snapshot()
    res.counters = [ses.scene.counters(ses.rs)]
    return ses, res, facts


def do_audit(ses, facts, what):
    facts.append(A.audit(ses.scene, ses.rs, what=what))


def no_audit(ses, facts, what):
    ses.scene.flush(ses.rs)              # (the oracle launches every call at once; this keeps the two runs call for call alike)


@forms("abcdefgh")
def test_frames_in_every_form(hip, oracle, form):
    sc = T.Scenario(name="accel_frames_" + ("rgb" if form == "h" else "s"), w=W, h=H, voxelSize=0.01, frames=4, trajectory="yaw", yaw_rate=0.05, localBlockNum=POOL, **voxel_kw(form))
    ses, got, facts = run_frames(hip, sc, do_audit)
    check_form(ses.scene, form)
    check_situation(form, facts)
    assert facts[-1]["resident"] > 500 and facts[-1]["probed"] > facts[-1]["resident"], facts[-1]["resident"]
    if form == "c":
        assert facts[-1]["moves"] > facts[0]["moves"] >= 0 and facts[-1]["moves"] >= 3, [f["moves"] for f in facts]
        assert facts[-1]["outside_mirror"] > 0, "the small cube holds the whole scene"
    ses.close()

    def ref():
        s, r, _ = run_frames(oracle, sc, no_audit)
        s.close()
        return r
    T.compare_results(got, oracle_once(sc.name, ref), sc, what="frames, form (%s)" % form)


# ---- 2. a camera that walks out of the cubes ----------------------------------------------------------------------------------------

def run_walk(be, sc, audit):
    ses = T.Session(be, sc)
    intr = sc.intr()
    facts, maps = [], []
    for k, M in enumerate(walk_poses()):
        depth = be.to_backend(synth.depth_frame(sc.w, sc.h, synth.parity_position(k), intr))
        v = capi.View(depth, sc.w, sc.h, M_d=M, intr_d=intr)
        if k % 2:
            ses.scene.process_frame(v, ses.rs, ses.points, ses.normals)
        else:
            ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
            ses.scene.reco.IntegrateIntoScene(v, ses.rs)
            ses.scene.vis.CreateExpectedDepths(v.M_d, v.intr_d, ses.rs)
            ses.scene.vis.CreateICPMaps(v, ses.rs, ses.points, ses.normals)
        audit(ses, facts, "walk, frame %d" % k)
        maps.append((ses.scene.download(capi.BUF_RAYCAST_RESULT, ses.rs).copy(), ses.points.numpy().copy()))
    return ses, facts, maps


@forms("acde")
def test_walk_audited_after_every_frame(hip, oracle, form):
    """The old origin's cells must be gone after every move: the census counts the whole cube, the exact-pages rule every page."""
    sc = T.Scenario(name="accel_walk", w=W, h=H, voxelSize=0.01, localBlockNum=POOL)
    ses, facts, maps = run_walk(hip, sc, do_audit)
    check_form(ses.scene, form)
    check_situation(form, facts)
    moves = [f["moves"] for f in facts]
    assert moves[-1] >= 1 and moves[-1] > moves[0], moves
    if form == "c":
        assert all(b > a for a, b in zip(moves, moves[1:])), moves          # smaller than the frustum ball: re-placed on every frame
    if form in ("a", "c"):
        assert facts[-1]["outside_mirror"] > 0, "every block is still inside the dense mirror cube after the walk"
    ses.close()

    def ref():
        s, _, m = run_walk(oracle, sc, no_audit)
        s.close()
        return m
    for k, ((ra, pa), (rb, pb)) in enumerate(zip(maps, oracle_once("walk", ref))):
        assert np.array_equal(ra[..., 3], rb[..., 3]), "frame %d: hit mask" % k
        hit = ra[..., 3] > 0
        assert np.array_equal(ra[hit], rb[hit]) and np.array_equal(pa, pb), "frame %d: ray cast / ICP points" % k


def run_jump(be, audit):
    """Two frames here, two frames 45 m away, one frame here again: at 1 cm voxels further than the DIRECTORY cube reaches (512 blocks of
    8 cm), which the walk above never leaves."""
    here = T.Scenario(name="jump_here", w=W, h=H, voxelSize=0.01, frames=2, localBlockNum=POOL)
    there = T.Scenario(name="jump_there", w=W, h=H, voxelSize=0.01, frames=2, origin=(25.0, -22.0, 30.0), trajectory="yaw", yaw_rate=0.1, localBlockNum=POOL)
    ses = T.Session(be, here)
    facts, maps = [], []
    for sc, k, fused in ((here, 0, True), (here, 1, "four"), (there, 0, True), (there, 1, "four"), (here, 2, True)):
        ses.sc = sc
        ses.frame(k, fused=fused)
        audit(ses, facts, "jump, %s frame %d" % (sc.name, k))
        maps.append((ses.scene.download(capi.BUF_RAYCAST_RESULT, ses.rs).copy(), ses.points.numpy().copy()))
    res = ses.snapshot()
    res.counters = [ses.scene.counters(ses.rs)]
    return ses, here, res, facts, maps


@forms("acde")
def test_jump_that_moves_the_directory_cube_too(hip, oracle, form):
    ses, sc, got, facts, maps = run_jump(hip, do_audit)
    check_form(ses.scene, form)
    check_situation(form, facts)
    dir_origins = [tuple(f["info"]["origin_directory"]) for f in facts]
    mir_origins = [tuple(f["info"]["origin_mirror"]) for f in facts]
    assert dir_origins[1] != dir_origins[2] != dir_origins[4] and mir_origins[1] != mir_origins[2] != mir_origins[4], (dir_origins, mir_origins)
    assert facts[4]["moves"] >= facts[1]["moves"] + 2, [f["moves"] for f in facts]
    for i in (2, 3, 4):          # the blocks of the other place are outside both cubes, by the table and the origins
        assert facts[i]["outside_directory"] > 500 and facts[i]["outside_mirror"] > 500, (i, facts[i]["outside_directory"], facts[i]["outside_mirror"])
    ses.close()

    def ref():
        s, _, r, _, m = run_jump(oracle, no_audit)
        s.close()
        return r, m
    want, want_maps = oracle_once("jump", ref)
    for k, ((ra, pa), (rb, pb)) in enumerate(zip(maps, want_maps)):
        assert np.array_equal(ra[..., 3], rb[..., 3]), "frame %d: hit mask" % k
        hit = ra[..., 3] > 0
        assert np.array_equal(ra[hit], rb[hit]) and np.array_equal(pa, pb), "frame %d: ray cast / ICP points" % k
    T.compare_results(got, want, sc, what="after the jump and back, form (%s)" % form)


# ---- 3. two lives -------------------------------------------------------------------------------------------------------------------

def run_lives(be, audit, after_reset):
    sc1 = T.Scenario(name="life1", w=W, h=H, voxelSize=0.01, frames=2, localBlockNum=POOL)
    sc2 = T.Scenario(name="life2", w=W, h=H, voxelSize=0.01, frames=2, origin=(0.3, 0.1, -0.4), localBlockNum=POOL)      # overlapping the first life's blocks
    ses = T.Session(be, sc1)
    facts = []
    for k in range(2):
        ses.frame(k, fused=True); audit(ses, facts, "first life, frame %d" % k)
    ses.scene.reco.ResetScene()
    after_reset(ses)
    ses.sc = sc2
    for k in range(2):
        ses.frame(k, fused=True); audit(ses, facts, "second life, frame %d" % k)
    res = ses.snapshot()
    res.counters = [ses.scene.counters(ses.rs)]
    return ses, sc2, res, facts


@forms("acdf")
def test_two_lives_across_reset_scene(hip, oracle, form):
    def after_reset(ses):
        f = A.audit(ses.scene, ses.rs, pages_exact=True, what="straight after ResetScene")
        c = f["census"]
        assert (f["resident"], f["swapped_out"], c["directory_cells"], c["slot_directory_cells"], c["mirror_blocks"], c["page_counter"]) == (0, 0, 0, 0, 0, 0), (f["resident"], c)
        assert np.all(c["page_table"] == -1) and f["info"]["mirror_pages_mapped"] == 0 and not f["placed"]
    ses, sc2, got, facts = run_lives(hip, do_audit, after_reset)
    check_form(ses.scene, form)
    check_situation(form, facts)
    if form == "c":
        assert facts[-1]["moves"] > facts[0]["moves"], [f["moves"] for f in facts]
    ses.close()

    def ref():
        s, _, r, _ = run_lives(oracle, no_audit, lambda s: None)
        s.close()
        return r
    T.compare_results(got, oracle_once("lives", ref), sc2, what="second life, form (%s)" % form)


# ---- 4. upload ----------------------------------------------------------------------------------------------------------------------

@forms("adf")
def test_upload_into_a_scene_that_holds_something(hip, oracle, form):
    sc = T.Scenario(name="accel_copy", w=W, h=H, voxelSize=0.01, frames=3, origin=(-30.0, 25.0, 5.0), localBlockNum=POOL)
    src = T.Session(hip, sc)
    for k in range(2):
        v = src.frame(k, fused=True)
    dst = T.Session(hip, T.Scenario(name="accel_dst", w=W, h=H, voxelSize=0.01, localBlockNum=POOL))
    check_form(dst.scene, form)
    dst.frame(0, fused=True)
    facts = [A.audit(dst.scene, dst.rs, what="dst before the upload")]
    old_origin = facts[0]["info"]["origin_directory"]
    for which, name in ((capi.BUF_HASH_ENTRIES, "table"), (capi.BUF_EXCESS_LIST, "excess list"), (capi.BUF_ALLOCATION_LIST, "allocation list"), (capi.BUF_VOXEL_BLOCKS, "voxels")):
        dst.scene.upload(which, src.scene.download(which))
        facts.append(A.audit(dst.scene, dst.rs, what="after the upload of the " + name))
    c = src.scene.counters(src.rs)
    dst.scene.set_counters(dst.rs, c["lastFreeBlockId"], c["lastFreeExcessListId"], 0)
    assert facts[-1]["info"]["origin_directory"] != old_origin and facts[-1]["resident"] == A.audit(src.scene, src.rs, what="src")["resident"] > 500
    check_situation(form, facts[1:])
    def build_ref():
        r = T.Session(oracle, sc)
        for k in range(2):
            r.frame(k, fused=True)
        return r
    ref = oracle_once("copy", build_ref)
    for ses in (dst, ref):
        ses.scene.vis.FindVisibleBlocks(v.M_d, sc.intr(), ses.rs)
        ses.scene.vis.CreateExpectedDepths(v.M_d, sc.intr(), ses.rs)
        ses.scene.vis.FindSurface(v.M_d, sc.intr(), ses.rs)
    ra, rb = dst.scene.download(capi.BUF_RAYCAST_RESULT, dst.rs), ref.scene.download(capi.BUF_RAYCAST_RESULT, ref.rs)
    assert np.array_equal(ra[..., 3], rb[..., 3]) and np.array_equal(ra[ra[..., 3] > 0], rb[rb[..., 3] > 0]) and np.count_nonzero(ra[..., 3] > 0) > 3000
    dst.sc = sc
    dst.frame(2, fused=True)                    # and the scene goes on
    A.audit(dst.scene, dst.rs, what="a further frame after the upload")
    src.close(); dst.close()


# ---- 5. swapping --------------------------------------------------------------------------------------------------------------------

SW, SH = test_swapping.W, test_swapping.H


def run_swapping(be, pool, audit=None, before_swap_out=None):
    """test_swapping's sequence at 1 cm voxels, 0x200 blocks per transfer; audit(scene, rs, what) after each of the four calls."""
    intr, seq = test_swapping.poses_and_depths()
    s = be.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=0.01), useSwapping=True, localBlockNum=pool, transferBlockNum=0x200)
    s.reco.ResetScene()
    rs = s.vis.CreateRenderState((SW, SH))
    pts = capi.DevBuffer(be, SW * SH * 16, np.float32, (SH, SW, 4)); nrm = capi.DevBuffer(be, SW * SH * 16, np.float32, (SH, SW, 4))
    out = []
    for k, (M, depth) in enumerate(seq):
        v = capi.View(be.to_backend(depth), SW, SH, M_d=M, intr_d=intr)
        steps = (("AllocateSceneFromDepth", lambda: s.reco.AllocateSceneFromDepth(v, rs)), ("IntegrateIntoScene", lambda: s.reco.IntegrateIntoScene(v, rs)),
                 ("IntegrateGlobalIntoLocal", lambda: s.swap_integrate_global_into_local(rs)), ("SaveToGlobalMemory", lambda: s.swap_save_to_global_memory(rs)))
        for name, call in steps:
            if name == "SaveToGlobalMemory" and before_swap_out:
                before_swap_out(s, rs)
            call()
            if audit:
                audit(s, rs, "swapping, frame %d after %s" % (k, name))
        s.vis.CreateExpectedDepths(v.M_d, v.intr_d, rs)
        s.vis.CreateICPMaps(v, rs, pts, nrm)
        out.append(dict(hash=s.download(capi.BUF_HASH_ENTRIES), swap=s.download(capi.BUF_SWAP_STATES), raycast=s.download(capi.BUF_RAYCAST_RESULT, rs), points=pts.numpy().copy()))
    return s, rs, out


@forms("acdeg")
@pytest.mark.parametrize("pool", [POOL, 0x200], ids=["pool", "small_pool"])
def test_swapping_audited_after_every_call(hip, oracle, form, pool):
    facts, held = [], {}

    def audit(s, rs, what):
        facts.append(A.audit(s, rs, what=what))

    def before_swap_out(s, rs):
        # what the probe reads for every resident entry before the call: the proof below that it reads live memory
        f = facts[-1]
        slots = np.nonzero(f["hash"]["ptr"] >= 0)[0]
        held.update(slots=slots, probe=s.accel_probe(f["hash"]["pos"][slots]), ptr=f["hash"]["ptr"][slots], sdf=A.raw_sdf(f["voxels"]).reshape(-1, 512))

    shown = []

    def audit_and_show(s, rs, what):
        audit(s, rs, what)
        if what.endswith("SaveToGlobalMemory") and not shown and held:
            now = facts[-1]["hash"]["ptr"][held["slots"]]
            went = np.nonzero((now == -1) & ~held["probe"]["no_place"])[0]
            if len(went):
                before = held["probe"]["values"][went]
                assert np.array_equal(before, held["sdf"][held["ptr"][went]]) and not np.any(before == -32768), "the probe did not read the blocks' sdf values before the swap-out"
                after = s.accel_probe(facts[-1]["hash"]["pos"][held["slots"][went]])
                assert not np.any(after["no_place"]) and np.all(after["values"] == -32768), "%s: the swapped-out entries' mirror blocks are not absent" % what
                shown.append(len(went))

    s, rs, got = run_swapping(hip, pool, audit_and_show, before_swap_out)
    check_form(s, form)
    # the situations, from the downloaded tables alone
    out_counts = [f["swapped_out"] for f in facts]
    assert max(out_counts) > 0, "no block was ever out"
    was_out = np.zeros(len(facts[0]["hash"]), bool)
    came_back = np.zeros(len(was_out), bool)
    for f in facts:
        came_back |= was_out & (f["hash"]["ptr"] >= 0)
        was_out |= f["hash"]["ptr"] == -1
    assert np.count_nonzero(came_back) > 0, "no block came back"
    if pool == 0x200:
        assert max(f["resident"] for f in facts) == pool, "the small pool never ran dry"
    if form != "g":
        assert shown and shown[0] > 0, "no swapped-out entry with a place in the mirror was seen going from its sdf values to absent"
    if form == "e":
        last = facts[-1]
        geo = A.geometry(last["info"], capi.VOXEL_S)
        back = np.nonzero(came_back & (last["hash"]["ptr"] >= 0))[0]
        cells = A.expected_cells(last["hash"], last["voxels"], geo, last["hash"]["pos"][back], last["census"]["page_table"])
        assert np.count_nonzero(cells["page"] == A.PAGE_UNMAPPABLE) > 0, "no swapped-in block lies in an unmappable page"
    if form == "c":
        assert facts[-1]["moves"] > facts[0]["moves"]
    rs.close(); s.close()

    def ref():
        so, ro, res = run_swapping(oracle, pool)
        ro.close(); so.close()
        return res
    for k, (x, y) in enumerate(zip(got, oracle_once("swapping %#x" % pool, ref))):
        T.assert_fields_equal(x["hash"], y["hash"], "frame %d: hash" % k)
        assert np.array_equal(x["swap"], y["swap"]), "frame %d: swap states" % k
        assert np.array_equal(x["raycast"][..., 3], y["raycast"][..., 3]), "frame %d: hit mask" % k
        hit = x["raycast"][..., 3] > 0
        assert np.array_equal(x["raycast"][hit], y["raycast"][hit]) and np.array_equal(x["points"], y["points"]), "frame %d: ray cast / ICP points" % k


# ---- 6. merge -----------------------------------------------------------------------------------------------------------------------

@forms("acde")
@pytest.mark.parametrize("origin", [(0.05, 0.02, -0.1), (25.0, -22.0, 30.0)], ids=["overlapping", "shifted"])
@pytest.mark.parametrize("dst_kind", ["fresh", "swapping"])
def test_merge_audited(hip, form, origin, dst_kind):
    shifted = origin[0] > 1
    b = TM.build(hip, TM.scenario_b(origin=origin))
    facts = []
    if dst_kind == "fresh":
        # a destination that has never seen a frame: A's blocks arrive by a merge too (and place the cubes), then B's
        a = TM.build(hip, TM.scenario_a())
        ses = T.Session(hip, TM.scenario_a())
        dst, rs = ses.scene, ses.rs
        assert not dst.accel_info()["placed"]
        assert dst.merge_from(a.scene)["allocated"] > 500
        facts.append(A.audit(dst, rs, what="fresh dst after the merge of A"))
        A.audit(a.scene, a.rs, what="A after being merged from")
        a.close()
    else:
        dst, rs = TM.swapping_scene(hip, 2)
        facts.append(A.audit(dst, rs, what="swapping dst before the merge"))
        assert facts[0]["swapped_out"] > 100 and facts[0]["resident"] > 100
    check_form(dst, form)
    src_before = A.audit(b.scene, b.rs, what="src before the merge")
    stats = dst.merge_from(b.scene)
    assert stats["allocated"] > 0, stats
    facts.append(A.audit(dst, rs, what="%s dst after the merge of B (%s)" % (dst_kind, "shifted" if shifted else "overlapping")))
    src_after = A.audit(b.scene, b.rs, what="src after the merge")
    T.assert_fields_equal(src_after["hash"], src_before["hash"], "src table")
    T.assert_fields_equal(src_after["voxels"], src_before["voxels"], "src voxels")
    assert src_after["info"] == src_before["info"] and np.array_equal(src_after["census"]["page_table"], src_before["census"]["page_table"])
    if shifted:
        assert facts[-1]["outside_mirror"] > 0 or facts[-1]["outside_directory"] > 0, "every block of the shifted scene lies inside dst's cubes"
    check_situation(form, facts)
    # one further frame on the destination
    if dst_kind == "fresh":
        ses.frame(3, fused=True)
        facts.append(A.audit(dst, rs, what="fresh dst, a frame after the merge"))
        ses.close()
    else:
        intr, seq = test_swapping.poses_and_depths()
        M, depth = seq[7]
        v = capi.View(hip.to_backend(depth), TM.W, TM.H, M_d=M, intr_d=intr)
        for name, call in (("AllocateSceneFromDepth", lambda: dst.reco.AllocateSceneFromDepth(v, rs)), ("IntegrateIntoScene", lambda: dst.reco.IntegrateIntoScene(v, rs)),
                           ("IntegrateGlobalIntoLocal", lambda: dst.swap_integrate_global_into_local(rs)), ("SaveToGlobalMemory", lambda: dst.swap_save_to_global_memory(rs))):
            call()
            facts.append(A.audit(dst, rs, what="swapping dst, a frame after the merge: " + name))
        rs.close(); dst.close()
    if form == "c":
        assert facts[-1]["moves"] > facts[0]["moves"]
    b.close()


# ---- 7. checkpoint ------------------------------------------------------------------------------------------------------------------

@forms("ad")
def test_checkpoint_load_into_a_scene_that_held_something_else(hip, form, tmp_path):
    sc = T.Scenario(name="accel_ckpt", w=W, h=H, voxelSize=0.01, frames=5, localBlockNum=POOL)
    ses = T.Session(hip, sc)
    for k in range(3):
        ses.frame(k, fused=(k % 2 == 0))
    ses.scene.save(str(tmp_path), ses.rs)
    saved = A.audit(ses.scene, ses.rs, what="the scene that was saved")
    other = T.Session(hip, T.Scenario(name="accel_ckpt_other", w=W, h=H, voxelSize=0.01, frames=2, origin=(4.0, -3.0, 2.5), localBlockNum=POOL))
    check_form(other.scene, form)
    for k in range(2):
        other.frame(k, fused=True)
    before = A.audit(other.scene, other.rs, what="the other scene before the load")
    other.scene.load(str(tmp_path), other.rs)
    after = A.audit(other.scene, other.rs, what="after the load")
    assert before["info"]["origin_mirror"] != after["info"]["origin_mirror"] or before["info"]["origin_directory"] != after["info"]["origin_directory"]
    T.assert_fields_equal(after["hash"], saved["hash"], "loaded table")
    other.sc = sc
    for k in range(3, 5):
        ses.frame(k, fused=True); other.frame(k, fused=True)
        A.audit(other.scene, other.rs, what="resumed, frame %d" % k)
    a, b = ses.snapshot(), other.snapshot()
    T.compare_results(a, b, sc, what="resumed in a scene that held something else")
    ses.close(); other.close()
