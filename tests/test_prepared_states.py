"""Integration from prepared voxel states: every weight 0 .. 255 (also above maxW), every stored sdf edge, colour weights decorrelated
from the depth weights -- the full product of tests/prepared_state_cases.py uploaded into hash and dense scenes and then integrated.

Three witnesses, compared bit for bit (no tolerance anywhere): the numpy restatement (tests/fusion_terms.py), the oracle, and -- for
the hash cases on the host -- the reference; on the GPU the product against the oracle in every launch form of the hash and of the
dense integration, with the maps of every frame and an audit of directories and sdf mirror after the last one.  Every test asserts the
coverage conditions of its case, evaluated with the restatement alone (prepared_state_cases.assert_coverage).

The sentinel words (-32768 / 0xffffffff, "no block here" in the sdf mirror): a hash scene refuses foreign voxel bytes that hold one,
a dense scene takes them as the values they are for the reference.
"""
import ctypes as C
import os

import numpy as np
import pytest

import accel_terms as A
import fusion_terms as FT
import itm_testlib as T
import prepared_state_cases as P
from infinitam_amd import capi

# every type at maxW 100; the other maxW / stop combinations on ITMVoxel_s and ITMVoxel_f_rgb
COMBOS = [(k, 100, False) for k in P.TYPES] + [(k, m, s) for k in ("s", "f_rgb") for m, s in ((1, False), (1, True), (100, True), (255, False), (255, True))]
combo_id = lambda c: "%s-maxW%d%s" % (c[0], c[1], "-stop" if c[2] else "")


def scenario(index, kind, maxW, stop, **kw):
    return (P.hash_scenario if index == "hash" else P.dense_scenario)(kind, maxW, stop, **kw)


def compare_frames(got, want, sc, what):
    assert len(got) == len(want) == sc.frames
    for k, (a, b) in enumerate(zip(got, want)):
        T.compare_results(a, b, sc, what="%s frame %d" % (what, k))


# ---- host -------------------------------------------------------------------------------------------------------------------------
def test_tables_hold_what_they_promise():
    s, f = P.SHORT_TABLE.astype(int), P.FLOAT_TABLE
    assert len(np.unique(s)) == P.N_SDF and -32768 not in s
    for lo, hi in ((-32767, -32727), (-40, 40), (32727, 32767)):
        assert np.isin(np.arange(lo, hi + 1), s).all()
    bits = f.view(np.uint32)
    assert len(np.unique(bits)) == P.N_SDF and not np.isnan(f).any() and 0xffffffff not in bits
    for v in (1.0, -1.0, 1.5, -3.0, 1e-30, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))):
        assert np.float32(v) in f
    assert 0x80000000 in bits and 0 in bits and np.any((bits & 0x7f800000 == 0) & (bits & 0x7fffff != 0))          # -0, +0, a denormal
    assert np.isin(P.SHORT_TABLE[np.abs(s) >= 32727].astype(np.float32) / np.float32(32767), f).all()
    v = P.states(capi.VOXEL_F_RGB, P.ORDER)
    assert len(np.unique(v["w_depth"].astype(int) * 256 + v["w_color"])) == 65536                                   # the two weights in every combination
    for c in (0, 1, 2, 127, 128, 254, 255):
        assert (v["clr"] == c).any(axis=0).all()


@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
@pytest.mark.parametrize("index", ["hash", "dense"])
def test_restatement_equals_oracle(oracle, index, combo):
    """Field for field after every frame; a difference is reported with the old (sdf, weight) state of the voxels that differ."""
    sc = scenario(index, *combo)
    p = P.placement(oracle, sc)
    cov = P.restate(oracle, p)
    runs = P.oracle_run(oracle, p)
    before = p.voxels
    for k in range(sc.frames):
        want, got = cov.per_frame[k], runs[k].voxels
        same = all(np.array_equal(want[n].view(np.uint32) if want[n].dtype == np.float32 else want[n], got[n].view(np.uint32) if got[n].dtype == np.float32 else got[n])
                   for n in want.dtype.names)
        assert same, "%s frame %d: %s" % (sc.name, k, FT.describe(before, want, got))
        before = want
    P.assert_coverage(cov, sc)
    print("%s: %d blocks, %.4f of the pairs covered, clamped %d + %d at the initial sdf, %d skipped, %d above maxW"
          % (sc.name, cov.blocks, cov.share, cov.clamped_other, cov.clamped_initial, cov.skipped, cov.above_maxW))


def test_odd_dense_volume_restatement_equals_oracle(oracle):
    sc = P.dense_scenario("s", size=P.DENSE_ODD_SIZE)
    p = P.placement(oracle, sc)
    cov, runs = P.restate(oracle, p), P.oracle_run(oracle, p)
    for k in range(sc.frames):
        assert np.array_equal(cov.per_frame[k], runs[k].voxels), "%s frame %d: %s" % (sc.name, k, FT.describe(p.voxels, cov.per_frame[k], runs[k].voxels))
    P.assert_coverage(cov, sc)


@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_oracle_equals_reference_on_hash_cases(oracle, ref, combo):
    """In the reference's own pool size (a compile-time constant of it).  No dense case: its shim keeps a 512^3 volume
    (tests/test_random_stress.py)."""
    sc = P.hash_scenario(*combo, pool=0)
    p = P.placement(oracle, sc)
    P.assert_coverage(P.restate(oracle, p, keep=False), sc)
    a = P.run(oracle, p)
    if ref.backend is not None:
        compare_frames(a, P.run(ref.backend, p), sc, sc.name + " oracle vs reference")
    ref.check("frames", a)
    P.forget(sc)


# ---- GPU: hash ------------------------------------------------------------------------------------------------------------------------
def hip_equals_oracle(hip, oracle, sc, fused=False, deferred=True, audit=True):
    p = P.placement(oracle, sc)
    P.assert_coverage(P.restate(oracle, p), sc)
    want = P.oracle_run(oracle, p)
    facts = {}

    def after_last(ses):
        if audit and ses.scene.is_hash:
            facts.update(A.audit(ses.scene, ses.rs, what=sc.name))
    got = P.run(hip, p, fused=fused, deferred=deferred, after_last=after_last)
    compare_frames(got, want, sc, "%s fused=%s deferred=%s" % (sc.name, fused, deferred))
    return facts


FORMS = [False, "four", True]
form_id = lambda f: {False: "separate", "four": "four", True: "process_frame"}[f]


@pytest.mark.gpu
@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "immediate"])
@pytest.mark.parametrize("fused", FORMS, ids=form_id)
@pytest.mark.parametrize("kind", list(P.TYPES))
def test_hash_forms_equal_the_oracle(hip, oracle, kind, fused, deferred):
    """integrate_hash_kernel, integrate_project_kernel and itm_process_frame, with deferred fusion on and off."""
    hip_equals_oracle(hip, oracle, P.hash_scenario(kind), fused, deferred)


@pytest.mark.gpu
@pytest.mark.parametrize("combo", [c for c in COMBOS if c[1:] != (100, False)], ids=combo_id)
def test_hash_other_maxW_and_stop_equal_the_oracle(hip, oracle, combo):
    """Weights above maxW, maxW & 0xff at 255, the stopIntegratingAtMaxW skips."""
    hip_equals_oracle(hip, oracle, P.hash_scenario(*combo), fused=True)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", FORMS, ids=form_id)
@pytest.mark.parametrize("kind", ["s", "s_rgb"])
def test_hash_short_types_with_the_paged_mirror(hip, oracle, kind, fused, monkeypatch):
    monkeypatch.setenv("ITM_MIRROR", "paged")
    facts = hip_equals_oracle(hip, oracle, P.hash_scenario(kind), fused)
    assert facts["form"] == "paged", facts["form"]


@pytest.mark.gpu
@pytest.mark.parametrize("key", [5, 12], ids=["no_directory", "no_sdf_mirror"])
def test_hash_without_directory_or_mirror(hip, oracle, key):
    """ITM_DEBUG_NO_DIRECTORY / ITM_DEBUG_NO_SDF_MIRROR (set before the scene is created: no mirror is allocated)."""
    hip.check(hip.fn["debug_set"](key, 1), "debug_set")
    try:
        hip_equals_oracle(hip, oracle, P.hash_scenario("s"), fused=True)
    finally:
        hip.check(hip.fn["debug_set"](key, 0), "debug_set")


# ---- GPU: dense -----------------------------------------------------------------------------------------------------------------------
DENSE_FORMS = {"default": {}, "unclassified": {16: 1}, "classified_after_fetch": {16: 2}, "no_strips": {17: 1}, "group_cull": {9: 1}}


def with_keys(hip, keys, fn):
    for k, v in keys.items():
        hip.check(hip.fn["debug_set"](k, v), "debug_set")
    try:
        return fn()
    finally:
        for k in keys:
            hip.check(hip.fn["debug_set"](k, 0), "debug_set")


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(DENSE_FORMS))
@pytest.mark.parametrize("maxW,stop", [(100, False), (100, True)], ids=["maxW100", "maxW100-stop"])
def test_dense_short_forms_equal_the_oracle(hip, oracle, form, maxW, stop):
    with_keys(hip, DENSE_FORMS[form], lambda: hip_equals_oracle(hip, oracle, P.dense_scenario("s", maxW, stop)))


@pytest.mark.gpu
@pytest.mark.parametrize("stop", [False, True], ids=["", "stop"])
def test_dense_check_mode_counts_no_violation(hip, oracle, stop):
    """ITM_DEBUG_DENSE_CLASSIFY 3: every classified group is also run through the exact path and compared."""
    c = (C.c_int32 * 4)()
    hip.check(hip.fn["debug_dense_classify_check"](c, 1), "classify_check")
    with_keys(hip, {16: 3}, lambda: hip_equals_oracle(hip, oracle, P.dense_scenario("s", 100, stop)))
    hip.check(hip.fn["debug_dense_classify_check"](c, 1), "classify_check")
    free, shadow, mixed, bad = list(c)
    assert bad == 0 and free > 0 and shadow > 0, list(c)


@pytest.mark.gpu
def test_dense_odd_row_length_equals_the_oracle(hip, oracle):
    """sx % 4 != 0: the generic one-voxel-per-lane kernel."""
    hip_equals_oracle(hip, oracle, P.dense_scenario("s", size=P.DENSE_ODD_SIZE))


@pytest.mark.gpu
@pytest.mark.parametrize("combo", [c for c in COMBOS if c[0] != "s" or c[1] != 100], ids=combo_id)
def test_dense_other_types_and_maxW_equal_the_oracle(hip, oracle, combo):
    hip_equals_oracle(hip, oracle, P.dense_scenario(*combo))


# ---- the sentinel words ---------------------------------------------------------------------------------------------------------------
def everything(ses):
    s, rs = ses.scene, ses.rs
    out = {w: s.download(w, rs if w in (capi.BUF_VISIBLE_IDS, capi.BUF_VISIBLE_TYPE) else None)
           for w in (capi.BUF_HASH_ENTRIES, capi.BUF_EXCESS_LIST, capi.BUF_VOXEL_BLOCKS, capi.BUF_ALLOCATION_LIST, capi.BUF_VISIBLE_IDS, capi.BUF_VISIBLE_TYPE)}
    out["counters"] = s.counters(rs)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def compare_frames_nan_aware(got, want, sc, what):
    """compare_frames where a voxel holds a NaN: NaN payloads are not specified, so a NaN equals a NaN; everything else bit for bit."""
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.counters == b.counters, (what, k)
        for n in a.voxels.dtype.names:
            assert np.array_equal(a.voxels[n], b.voxels[n], equal_nan=a.voxels[n].dtype == np.float32), (what, k, "voxels", n)
        for n in ("raycast", "points", "normals"):
            assert np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True), (what, k, n)
        assert np.array_equal(T.range_region(a.range_image, sc.w, sc.h), T.range_region(b.range_image, sc.w, sc.h)) and np.array_equal(a.image, b.image), (what, k)


def assert_unchanged(before, after, what):
    for k in before:
        if isinstance(before[k], dict):
            assert before[k] == after[k], (what, k)
        elif before[k].dtype.names:
            for n in before[k].dtype.names:
                assert np.array_equal(bits(before[k][n]), bits(after[k][n])), (what, k, n)
        else:
            assert np.array_equal(before[k], after[k]), (what, k)


def refused(call, voxel):
    with pytest.raises(capi.ItmError) as e:
        call()
    msg = str(e.value)
    assert "(-1)" in msg and ("voxel %d " % voxel) in msg, msg          # ITM_ERR_INVALID, naming the first such voxel


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(P.TYPES))
def test_hash_scene_refuses_sentinel_words(hip, oracle, kind, tmp_path):
    """Buffer upload and checkpoint load: refused with ITM_ERR_INVALID, the scene as it was; the same pool with -32767 / 0xfffffffe in
    those voxels is accepted and integrates like the oracle."""
    sc = P.hash_scenario(kind, sentinel=True)
    p = P.placement(oracle, sc)
    first = int(p.sentinel_voxels.min())
    ses = T.Session(hip, sc)
    try:
        good = p.voxels.copy()
        good["sdf"][p.sentinel_voxels] = P.sentinel_word(sc.voxelType, harmless=True)
        P.upload(ses, p, voxels=good)
        ses.frame(0, fused=True)
        before = everything(ses)
        A.audit(ses.scene, ses.rs, what="before")
        refused(lambda: ses.scene.upload(capi.BUF_VOXEL_BLOCKS, p.voxels), first)
        assert_unchanged(before, everything(ses), "refused upload")
        # a checkpoint of this scene whose voxel.dat holds the words
        d = str(tmp_path)
        ses.scene.save(d, ses.rs)
        raw = np.fromfile(os.path.join(d, "voxel.dat"), np.uint8)
        bad = before[capi.BUF_VOXEL_BLOCKS].copy()
        bad["sdf"][p.sentinel_voxels] = P.sentinel_word(sc.voxelType)
        raw[4:] = bad.view(np.uint8)
        raw.tofile(os.path.join(d, "voxel.dat"))
        refused(lambda: ses.scene.load(d, ses.rs), first)
        assert_unchanged(before, everything(ses), "refused checkpoint")
        A.audit(ses.scene, ses.rs, what="after the refusals")
    finally:
        ses.close()
    if kind in ("s", "s_rgb"):          # (0xfffffffe is a NaN: accepted above, but what a NaN's payload becomes is not specified)
        q = P.Placement(sc, good, p.pair_of, p.hash, p.excess, p.alloc_list, p.visible_ids, p.visible_type, p.counters, p.blocks)
        compare_frames(P.run(hip, q, fused=True), P.run(oracle, q), sc, sc.name + " harmless words")


@pytest.mark.gpu
def test_swapping_scene_refuses_sentinel_words_in_cached_blocks(hip, tmp_path):
    """cache_blocks.dat of a checkpoint: the host cache of a swapping scene is replaced from it, and its blocks reach the pool later."""
    import swapped_cases as SC
    run = SC.build(hip, 1)                       # the half-swapped scene: 512 blocks live in the host cache alone
    try:
        s, rs, d = run.scene, run.rs, str(tmp_path)
        s.save(d, rs)
        path = os.path.join(d, "cache_blocks.dat")
        raw = np.fromfile(path, np.uint8)
        cached = raw[4:].view(capi.VOXEL_DTYPES[capi.VOXEL_S]).copy()
        assert len(cached) >= 512 * 512, "no block was swapped out: the case is empty"
        before = run.snapshot()
        for word in (-32768, -32767):
            cached["sdf"][700] = word
            raw[4:] = cached.view(np.uint8)
            raw.tofile(path)
            if word == -32768:
                refused(lambda: s.load(d, rs), 700)
                SC.compare(run.snapshot(), before, "refused checkpoint")
            else:
                s.load(d, rs)
                e = int(np.nonzero(s.global_cache_flags())[0][700 // 512])
                assert s.global_cache_block(e)["sdf"][700 % 512] == -32767
    finally:
        run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["s", "f"])
def test_dense_scene_takes_sentinel_words_as_values(hip, oracle, kind):
    """No mirror, no contract: -32768 is the value -32768 / 32767 and 0xffffffff a NaN, as for the reference; a ray of frame 0 crosses them."""
    sc = P.dense_scenario(kind, sentinel=True)
    p = P.placement(oracle, sc)
    assert np.array_equal(p.voxels["sdf"][p.sentinel_voxels].view(np.uint16 if kind == "s" else np.uint32), np.full(4, 0x8000 if kind == "s" else 0xffffffff))
    (compare_frames if kind == "s" else compare_frames_nan_aware)(P.run(hip, p), P.run(oracle, p), sc, sc.name)
