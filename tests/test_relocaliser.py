"""Keyframe relocaliser (include/itm_hip.h, itm_reloc_*; infinitam_amd/csrc/reloc.hip): fern codes of a small, smoothed depth image, a
database of keyframe codes and the nearest-code search, against the float32 numpy restatement of the sequential definition
(tests/reloc_terms.py) -- bit for bit: the image is IEEE float work in a fixed order, the rest is integer work.

CPU: the host-only defaults (configuration, taps, splitmix64 ferns), the struct layout, the restatement itself pinned on the synthetic
scene (orderings only), and recovery on the oracle: the nearest keyframe's pose, ray-cast from there, ICP -- the translation error
falls below half of the keyframe's.  GPU: image and code, search, harvesting, handles, recovery against the oracle, and the C++
engine (tests/cpp/relocaliser_demo.cpp) against the same calls through the Python binding."""
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import itm_testlib as T
import reloc_terms as R
from infinitam_amd import capi, synth
from infinitam_amd.capi import DevBuffer, Relocaliser, RelocConfig, TrackerConfig
from itm_testlib import Scenario

F32 = np.float32
SC = Scenario(name="reloc", w=160, h=120, voxelSize=0.01, frames=40, stream=3)
_cache = {}


def depth_of(sc, k):
    key = ("depth", sc.w, sc.h, sc.stream, k)
    if key not in _cache:
        _cache[key] = sc.depth(k)
    return _cache[key]


def default_setup(be, w, h, seed=1, **kw):
    """(config, pixel, threshold) as the library gives them"""
    cfg = Relocaliser.default_config(be, w, h)
    for n, v in kw.items():
        setattr(cfg, n, v)
    pixel, threshold = Relocaliser.default_ferns(be, cfg, seed)
    return cfg, pixel, threshold


def restated_code(cfg, pixel, threshold, depth):
    taps = np.array(cfg.blurTaps[:], F32)
    S = R.small_image(depth, cfg.levels, cfg.blurRadius, taps)
    return R.encode(S, pixel, threshold, cfg.numFerns, cfg.numDecisions)


def scene_codes(be, sc, frames):
    """restated codes of the scenario's frames under the default configuration (taps and ferns read back from the library)"""
    cfg, pixel, threshold = default_setup(be, sc.w, sc.h)
    out = {}
    for k in frames:
        key = ("code", sc.w, sc.h, sc.stream, k)
        if key not in _cache:
            _cache[key] = restated_code(cfg, pixel, threshold, depth_of(sc, k))
        out[k] = _cache[key]
    return out


# ---- CPU: defaults ------------------------------------------------------------------------------------------------------------------

def test_default_config(hip_host):
    c = Relocaliser.default_config(hip_host, 640, 480)
    assert (c.w, c.h, c.levels, c.w >> c.levels, c.h >> c.levels) == (640, 480, 4, 40, 30)
    assert (c.blurRadius, c.numFerns, c.numDecisions, c.capacity) == (6, 500, 4, 65536)
    c2 = Relocaliser.default_config(hip_host, 160, 120)
    assert c2.levels == 2 == R.default_levels(160) and R.default_levels(640) == 4
    assert Relocaliser.default_config(hip_host, 40, 30).levels == 0 and Relocaliser.default_config(hip_host, 41, 30).levels == 1
    got, want = np.array(c.blurTaps[:7], F32), R.default_taps()
    assert got[0] == 1.0 and np.all(np.diff(got) < 0)
    assert np.all(np.abs(got.view(np.int32) - want.view(np.int32)) <= 1), (got, want)      # exp of the C library against numpy's: 1 ulp
    assert list(c.blurTaps[7:]) == [0.0, 0.0]
    with pytest.raises(capi.ItmError):
        Relocaliser.default_config(hip_host, 0, 480)


@pytest.mark.parametrize("seed", [1, 12345])
def test_default_ferns_are_the_splitmix64_restatement(hip_host, seed):
    for (w, h, kw) in ((640, 480, {}), (160, 120, {"numFerns": 37, "numDecisions": 8})):
        cfg, pixel, threshold = default_setup(hip_host, w, h, seed, **kw)
        ws, hs = cfg.w >> cfg.levels, cfg.h >> cfg.levels
        p, t = R.default_ferns(ws, hs, cfg.numFerns, cfg.numDecisions, seed)
        assert np.array_equal(pixel, p)
        assert np.array_equal(threshold.view(np.uint32), t.view(np.uint32))
        assert pixel.min() >= 0 and pixel.max() < ws * hs and threshold.min() >= F32(0.2) and threshold.max() <= F32(3.0)
    a = Relocaliser.default_ferns(hip_host, Relocaliser.default_config(hip_host, 640, 480), 1)
    b = Relocaliser.default_ferns(hip_host, Relocaliser.default_config(hip_host, 640, 480), 12345)
    assert not np.array_equal(a[0], b[0])
    # other bounds
    cfg = Relocaliser.default_config(hip_host, 640, 480)
    pixel, threshold = Relocaliser.default_ferns(hip_host, cfg, 7, lo=0.5, hi=1.25)
    p, t = R.default_ferns(40, 30, 500, 4, 7, 0.5, 1.25)
    assert np.array_equal(pixel, p) and np.array_equal(threshold.view(np.uint32), t.view(np.uint32))


def test_bad_configurations_are_refused_on_the_host(hip_host):
    cfg = Relocaliser.default_config(hip_host, 640, 480)
    buf_p, buf_t = np.zeros(8192, np.int32), np.zeros(8192, F32)

    def ferns(c):
        return hip_host.fn["reloc_default_ferns"](C.byref(c), 1, 0.2, 3.0, buf_p.ctypes.data_as(C.c_void_p), buf_t.ctypes.data_as(C.c_void_p))

    for name, v in (("numFerns", 0), ("numFerns", 1025), ("numDecisions", 0), ("numDecisions", 9), ("levels", 9), ("blurRadius", 9), ("capacity", 0)):
        c = RelocConfig.from_buffer_copy(cfg)
        setattr(c, name, v)
        assert ferns(c) == capi.ERR_INVALID, name
        assert b"reloc" in hip_host.fn["last_error"]()
        h = C.c_void_p()
        assert hip_host.fn["reloc_create"](C.byref(c), buf_p.ctypes.data_as(C.c_void_p), buf_t.ctypes.data_as(C.c_void_p), C.byref(h)) == capi.ERR_INVALID, name
        assert not h.value
    # a pixel index outside the small image
    h = C.c_void_p()
    bad = buf_p.copy(); bad[17] = 40 * 30
    assert hip_host.fn["reloc_create"](C.byref(cfg), bad.ctypes.data_as(C.c_void_p), buf_t.ctypes.data_as(C.c_void_p), C.byref(h)) == capi.ERR_INVALID
    assert b"pixel" in hip_host.fn["last_error"]()


def test_reloc_symbols_are_host_io_and_exported(hip_host):
    declared = capi.declared_functions()
    names = [n for n in declared if n.startswith("reloc_")]
    assert len(names) == 14
    for n in names:
        assert n in capi._HOST_IO_SIGS and n not in capi._SIGS and n in hip_host.fn
    import infinitam_amd
    assert infinitam_amd.Relocaliser is Relocaliser
    assert (capi.RELOC_MAX_K, capi.RELOC_MAX_FERNS) == (8, 1024) == (R.MAX_K, 1024)


def test_config_layout_matches_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "itm_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d %d\\n",'
                   'sizeof(itm_reloc_config), offsetof(itm_reloc_config, levels), offsetof(itm_reloc_config, blurTaps), offsetof(itm_reloc_config, numFerns),'
                   'offsetof(itm_reloc_config, numDecisions), offsetof(itm_reloc_config, capacity), ITM_RELOC_MAX_K, ITM_RELOC_MAX_FERNS); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(RelocConfig), RelocConfig.levels.offset, RelocConfig.blurTaps.offset, RelocConfig.numFerns.offset, RelocConfig.numDecisions.offset,
            RelocConfig.capacity.offset, capi.RELOC_MAX_K, capi.RELOC_MAX_FERNS]
    assert got == want and got[0] == 64


# ---- CPU: the restatement ------------------------------------------------------------------------------------------------------------

def holes(img):
    """the pattern of test_tracker.holes_image on an image of any size"""
    img = img.copy()
    img[::5, ::3] = -1.0
    img[7:20, 30:60] = 0.0
    return img


def test_restated_subsampling_is_the_oracles(oracle):
    for w, h in ((160, 120), (150, 110), (75, 55)):
        img = holes(synth.depth_frame(w, h, SC.position(1), synth.intrinsics_for(w, h)))
        src = oracle.to_backend(img)
        dst = DevBuffer(oracle, (w // 2) * (h // 2) * 4, F32, (h // 2, w // 2))
        oracle.check(oracle.fn["filter_subsample_with_holes"](src.ptr, w, h, dst.ptr, None), "subsample")
        assert np.array_equal(dst.numpy().view(np.uint32), R.subsample(img).view(np.uint32)), (w, h)


def test_restated_blur_on_known_answers():
    taps = np.array([1.0, 0.5, 0.25], F32)
    img = np.array([[1.0, 0.0, 3.0, 2.0]], F32)
    out = R.blur_pass(img, taps, 1, axis=1)
    # holes take no part: pixel 1 is the mean of its neighbours, the others keep their share
    assert np.array_equal(out, np.array([[1.0, F32(F32(0.5) + F32(1.5)) / F32(1.0), F32(F32(3.0) + F32(1.0)) / F32(1.5), F32(F32(1.5) + F32(2.0)) / F32(1.5)]], F32))
    assert np.array_equal(R.blur_pass(np.zeros((3, 4), F32), taps, 2, axis=0), np.zeros((3, 4), F32))
    assert np.array_equal(R.small_image(img, 0, 0, taps), img)
    # a constant image stays constant up to the rounding of s / n
    const = np.full((9, 11), F32(1.75))
    assert np.abs(R.small_image(const, 0, 2, taps) - const).max() <= 2e-7
    ids, dist = R.search(np.array([[1, 2, 3, 4], [1, 2, 0, 0], [1, 2, 3, 4]], np.uint8), np.array([1, 2, 3, 4], np.uint8), 5)
    assert ids.tolist() == [0, 2, 1, -1, -1] and dist.tolist() == [0.0, 0.0, 0.5, 1.0, 1.0]


def test_dissimilarity_grows_with_camera_distance(hip_host):
    sc = Scenario(name="reloc_mono", w=160, h=120, voxelSize=0.01, frames=61)
    frames = list(range(0, 61, 4))
    codes = scene_codes(hip_host, sc, frames)
    differing = [int((codes[k] != codes[0]).sum()) for k in frames]
    print("ferns of 500 that differ from frame 0, frames 0, 4 .. 60:", differing)
    assert differing[0] == 0 and differing[1] > 0
    assert all(b >= a for a, b in zip(differing, differing[1:])), differing
    # the nearest database row of a frame between two keyframes is one of its two neighbours
    keyframes = frames[::2]                                     # 0, 8, 16 ..
    db = np.stack([codes[k] for k in keyframes])
    for j, q in enumerate(frames[1::2]):                        # 4, 12, 20 ..: between keyframes j and j + 1
        ids, _ = R.search(db, codes[q], 1)
        assert ids[0] in (j, min(j + 1, len(keyframes) - 1)), (q, ids)


# ---- recovery (CPU on the oracle with restated codes, GPU on the product) -----------------------------------------------------------

def recovery_config():
    cfg = TrackerConfig.default()
    cfg.noHierarchyLevels = 3
    cfg.trackingRegime[:3] = [3, 3, 1]      # both, both, rotation only on the coarsest: five levels leave < 100 points there at 160 x 120
    return cfg


QUERIES = (7, 18, 29)


def recover(be, process, nearest, pose_of):
    """Fuses SC's 40 frames harvesting at 0.05 through process(k, depth_dev, pose) -> added; then for the query frames takes the
    nearest keyframe's pose, rebuilds the visible list and the maps from there and tracks.  [(keyframe id, keyframe pose, tracked pose)]"""
    ses = T.Session(be, SC)
    added = []
    for k in range(SC.frames):
        ses.frame(k, fused=True)
        added.append(process(k, ses._depth, SC.pose(k)))
    cfg = recovery_config()
    out = []
    for q in QUERIES:
        d = be.to_backend(depth_of(SC, q))
        kf = nearest(q, d)
        pose = pose_of(kf)
        s, rs = ses.scene, ses.rs
        s.vis.FindVisibleBlocks(pose, SC.intr(), rs)
        s.vis.CreateExpectedDepths(pose, SC.intr(), rs)
        view = capi.View(d, SC.w, SC.h, M_d=pose, intr_d=SC.intr())
        s.vis.CreateICPMaps(view, rs, ses.points, ses.normals)
        vs = view.struct()
        res = (C.c_float * 16)()
        sp = np.ascontiguousarray(pose, F32).ctypes.data_as(C.POINTER(C.c_float))
        be.check(be.fn["track_camera"](C.byref(cfg), C.byref(vs), ses.points.ptr, ses.normals.ptr, sp, res, None), "track_camera")
        out.append((int(kf), np.array(pose, F32), np.array(res[:], F32)))
    ses.close()
    return added, out


def oracle_recovery(oracle, lib):
    """the sequence on the oracle, codes and database from the restatement (`lib`: the product library, for the defaults alone)"""
    if "oracle_recovery" not in _cache:
        codes = scene_codes(lib, SC, range(SC.frames))
        db = R.Database(500, 65536)
        _cache["oracle_recovery"] = recover(oracle, lambda k, d, pose: db.process(codes[k], pose, True, 0.05, 1)[2],
                                            lambda q, d: R.search(db.rows(), codes[q], 1)[0][0], lambda i: db.poses[i])
    return _cache["oracle_recovery"]


def check_recovered(out):
    seen = 0
    for (kf, kf_pose, pose), q in zip(out, QUERIES):
        truth = SC.pose(q)
        before = float(np.linalg.norm(kf_pose[12:15] - truth[12:15]))
        after = float(np.linalg.norm(pose[12:15] - truth[12:15]))
        print(f"query frame {q}: keyframe {kf}, translation error {before:.3e} m before, {after:.3e} m after")
        assert np.all(np.isfinite(pose))
        if before >= 0.01:
            seen += 1
            assert after < 0.5 * before, (q, kf, before, after)
    assert seen >= 2, "the query frames lie between keyframes"


def test_recovery_on_the_oracle(oracle, hip_host):
    added, out = oracle_recovery(oracle, hip_host)
    keyframes = [k for k, a in enumerate(added) if a >= 0]
    assert added[0] == 0 and 4 <= len(keyframes) <= 20, keyframes
    assert [added[k] for k in keyframes] == list(range(len(keyframes)))
    check_recovered(out)


# ---- GPU: image and code --------------------------------------------------------------------------------------------------------------

def frame_inputs(w, h):
    clean = synth.depth_frame(w, h, SC.position(1), synth.intrinsics_for(w, h))
    return {"clean": clean, "holes": holes(clean), "all_holes": np.zeros((h, w), F32)}


def explicit_ferns(S, F, D, rng):
    """pixel 0 and the last pixel, thresholds equal to a pixel's exact value (strict >: bit clear), one ulp below it (bit set)"""
    n = F * D
    flat = S.reshape(-1)
    pixel = rng.integers(0, flat.size, n).astype(np.int32)
    pixel[0] = 0
    pixel[-1] = flat.size - 1
    if n > 2:
        pixel[n // 2] = flat.size - 1
        pixel[n // 2 - 1] = 0
    threshold = rng.uniform(0.2, 3.0, n).astype(F32)
    if not (flat > 0).any():
        return pixel, threshold                              # all holes: positive thresholds, the code is all zero
    kind = np.arange(n) % 3
    threshold[kind == 0] = flat[pixel[kind == 0]]
    below = np.nextafter(flat[pixel[kind == 1]], F32(-np.inf)).astype(F32)
    threshold[kind == 1] = below
    return pixel, threshold


@pytest.mark.gpu
@pytest.mark.parametrize("R_", [0, 1, 6])
@pytest.mark.parametrize("w,h,levels", [(160, 120, 2), (150, 110, 1), (64, 48, 0)])
def test_image_and_code_equal_the_restatement(hip, w, h, levels, R_):
    rng = np.random.default_rng(1000 * w + 10 * levels + R_)
    taps = np.array(Relocaliser.default_config(hip, w, h).blurTaps[:], F32)
    for name, img in frame_inputs(w, h).items():
        S = R.small_image(img, levels, R_, taps)
        assert S.shape == (h >> levels, w >> levels)
        dev = hip.to_backend(img)
        for D in (1, 4, 8):
            for F in (1, 63, 64, 65, 500, 1024):
                pixel, threshold = explicit_ferns(S, F, D, rng)
                r = Relocaliser(hip, w, h, numFerns=F, numDecisions=D, capacity=2, levels=levels, blurRadius=R_, pixel=pixel, threshold=threshold)
                r.encode(dev)
                got_img, got_code = r.read()
                want = R.encode(S, pixel, threshold, F, D)
                what = (name, D, F)
                assert np.array_equal(got_img.view(np.uint32), S.view(np.uint32)), what
                assert np.array_equal(got_code, want), what
                if name == "all_holes":
                    assert not S.any() and not got_code.any(), what
                elif F >= 63:
                    assert want.any() and (want < (1 << D) - 1).any(), what      # the planted thresholds cut both ways
                r.close()
        dev.close()


# ---- GPU: search ----------------------------------------------------------------------------------------------------------------------

def planted_database(rng, N, F, alphabet):
    db = rng.integers(0, alphabet, (N, F)).astype(np.uint8)
    q = rng.integers(0, alphabet, F).astype(np.uint8)
    if N:
        dup = db[N // 2].copy()
        db[0] = dup; db[N - 1] = dup                       # duplicate rows at both ends and in the middle
        for i in {1 % N, N // 3, (N - 2) % N}:
            if i not in (0, N - 1, N // 2) or N < 4:
                db[i] = q                                  # the exact query at several ids
        near = q.copy(); near[: max(F // 7, 1)] ^= 1     # and near misses that tie with each other
        for i in {N // 5, (2 * N) // 3}:
            if i not in (0, N - 1, N // 2):
                db[i] = near
    else:
        dup = q.copy()
    return db, q, dup


@pytest.mark.gpu
@pytest.mark.parametrize("alphabet", [256, 4])
@pytest.mark.parametrize("F", [1, 63, 65, 500, 512, 1024])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1000, 70001])
def test_search_equals_the_restatement(hip, N, F, alphabet):
    rng = np.random.default_rng(N * 2048 + F * 2 + (alphabet == 4))
    db, q, dup = planted_database(rng, N, F, alphabet)
    r = Relocaliser(hip, 16, 12, numFerns=F, numDecisions=1, capacity=max(N, 1), levels=0, blurRadius=0)
    r.upload(db, np.zeros((N, 16), F32))
    assert r.count == N
    for query in (q, dup):
        for k in (1, 3, 8):                                 # k > N for the small databases
            ids, dist = r.find(query, k)
            want_ids, want_dist = R.search(db, query, k)
            assert np.array_equal(ids, want_ids), (k, ids, want_ids, dist, want_dist)
            assert np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32)), (k, dist, want_dist)
    if N >= 63:
        ids, dist = r.find(dup, 3)
        assert ids.tolist()[:1] == [0] and dist[0] == 0.0 and (F == 1 or alphabet == 4 or ids.tolist() == [0, N // 2, N - 1])
    for k in (0, 9):
        with pytest.raises(capi.ItmError):
            r.find(q, k)
    r.close()


# ---- GPU: harvest ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0.05, 0.2])
def test_harvest_equals_the_restatement(hip, threshold):
    codes = scene_codes(hip, SC, range(SC.frames))
    r = Relocaliser(hip, SC.w, SC.h)
    db = R.Database(500, 65536)
    for k in range(SC.frames):
        d = hip.to_backend(depth_of(SC, k))
        got = r.process_frame(d, SC.pose(k), True, threshold, 3)
        want = db.process(codes[k], SC.pose(k), True, threshold, 3)
        assert np.array_equal(r.read()[1], codes[k]), k
        assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (k, got, want)
        d.close()
    assert 2 <= r.count == len(db.codes) < SC.frames
    got_codes, got_poses = r.codes()
    assert np.array_equal(got_codes, db.rows()) and np.array_equal(got_poses, np.array(db.poses))
    for i in range(r.count):
        assert np.array_equal(r.pose(i), db.poses[i])
    with pytest.raises(capi.ItmError):
        r.pose(r.count)
    with pytest.raises(capi.ItmError):
        r.pose(-1)
    # find(NULL) after encode is process_frame without harvesting, and neither changes the database
    d = hip.to_backend(depth_of(SC, 13))
    a = r.process_frame(d, None, False, threshold, 8)
    r.encode(d)
    b = r.find(None, 8)
    assert a[2] == -1 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    want = R.search(db.rows(), codes[13], 8)
    assert np.array_equal(a[0], want[0]) and np.array_equal(a[1].view(np.uint32), want[1].view(np.uint32))
    assert r.count == len(db.codes)
    r.close()


@pytest.mark.gpu
def test_a_full_database_refuses_the_next_keyframe(hip):
    codes = scene_codes(hip, SC, range(SC.frames))
    r = Relocaliser(hip, SC.w, SC.h, capacity=3)
    db = R.Database(500, 3)
    refused = 0
    for k in range(SC.frames):
        d = hip.to_backend(depth_of(SC, k))
        before = r.codes()
        got = r.process_frame(d, SC.pose(k), True, 0.05, 2)
        want = db.process(codes[k], SC.pose(k), True, 0.05, 2)
        assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k
        if got[2] == -2:
            refused += 1
            after = r.codes()
            assert r.count == 3 and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        d.close()
    assert refused >= 1 and r.count == 3
    with pytest.raises(capi.ItmError):
        r.upload(np.zeros((4, 500), np.uint8), np.zeros((4, 16), F32))
    assert r.count == 3
    r.close()


# ---- GPU: handles ---------------------------------------------------------------------------------------------------------------------

def filled(hip, seed=1, frames=range(0, 40, 3)):
    r = Relocaliser(hip, SC.w, SC.h, seed=seed)
    for k in frames:
        d = hip.to_backend(depth_of(SC, k))
        r.process_frame(d, SC.pose(k), True, 0.0, 1)      # every frame whose code differs from its nearest row
        d.close()
    return r


@pytest.mark.gpu
def test_upload_download_save_and_load(hip, tmp_path):
    r = filled(hip)
    codes, poses = r.codes()
    assert len(codes) >= 10
    queries = [scene_codes(hip, SC, [k])[k] for k in (5, 20, 38)]
    want = [r.find(q, 8) for q in queries]
    r.upload(codes, poses)                                   # the identity
    again = r.codes()
    assert np.array_equal(again[0], codes) and np.array_equal(again[1], poses)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(want, [r.find(q, 8) for q in queries]))
    r.save(str(tmp_path))
    assert os.path.exists(tmp_path / "relocaliser.dat")
    fresh = Relocaliser(hip, SC.w, SC.h, capacity=64)        # another capacity is the handle's own business
    fresh.load(str(tmp_path))
    assert fresh.count == len(codes)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(want, [fresh.find(q, 8) for q in queries]))
    assert np.array_equal(fresh.pose(3), poses[3])
    other = Relocaliser(hip, SC.w, SC.h, seed=2)
    rc = hip.fn["reloc_load"](C.c_void_p(other.h), str(tmp_path).encode())
    assert rc == capi.ERR_INVALID and b"other ferns" in hip.fn["last_error"]() and other.count == 0
    small = Relocaliser(hip, SC.w, SC.h, capacity=4)
    assert hip.fn["reloc_load"](C.c_void_p(small.h), str(tmp_path).encode()) == capi.ERR_INVALID and small.count == 0
    coarse = Relocaliser(hip, SC.w, SC.h, blurRadius=2)
    assert hip.fn["reloc_load"](C.c_void_p(coarse.h), str(tmp_path).encode()) == capi.ERR_INVALID
    assert hip.fn["reloc_load"](C.c_void_p(fresh.h), str(tmp_path / "absent").encode()) == capi.ERR_INVALID and fresh.count == len(codes)
    r.upload(np.zeros((0, 500), np.uint8), np.zeros((0, 16), F32))
    assert r.count == 0 and r.find(queries[0], 2)[0].tolist() == [-1, -1]
    for h in (r, fresh, other, small, coarse):
        h.close()


@pytest.mark.gpu
def test_two_handles_on_two_streams_from_two_threads(hip):
    frames = {0: list(range(0, 40, 2)), 1: list(range(39, 0, -3))}
    want = {}
    for i in (0, 1):
        r = Relocaliser(hip, SC.w, SC.h, seed=10 + i)
        want[i] = []
        for k in frames[i]:
            d = hip.to_backend(depth_of(SC, k))
            want[i].append(r.process_frame(d, SC.pose(k), True, 0.1, 4))
            d.close()
        want[i].append(r.codes())
        r.close()
    depths = {k: hip.to_backend(depth_of(SC, k)) for k in set(frames[0]) | set(frames[1])}
    handles = [Relocaliser(hip, SC.w, SC.h, seed=10 + i) for i in (0, 1)]
    streams = []
    for _ in (0, 1):
        st = C.c_void_p(); hip.check(hip.fn["stream_create"](C.byref(st)), "stream_create"); streams.append(st)
    got, errors = {0: [], 1: []}, []
    start = threading.Barrier(2)

    def work(i):
        try:
            start.wait()
            for rep in range(3):                            # the same frames three times over: only the first pass harvests
                for k in frames[i]:
                    res = handles[i].process_frame(depths[k], SC.pose(k), rep == 0, 0.1, 4, stream=streams[i].value)
                    if rep == 0:
                        got[i].append(res)
            got[i].append(handles[i].codes())
        except Exception as e:      # noqa: BLE001 -- reported below, in the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        assert not errors, errors
        for i in (0, 1):
            assert len(got[i]) == len(want[i])
            for a, b in zip(got[i][:-1], want[i][:-1]):
                assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i
            assert np.array_equal(got[i][-1][0], want[i][-1][0]) and np.array_equal(got[i][-1][1], want[i][-1][1])
    finally:
        hip.sync()
        for h in handles:
            h.close()
        for st in streams:
            hip.fn["stream_destroy"](st)


# ---- GPU: recovery ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_recovery_on_hip_follows_the_oracle(hip, oracle):
    r = Relocaliser(hip, SC.w, SC.h)
    added, out = recover(hip, lambda k, d, pose: r.process_frame(d, pose, True, 0.05, 1)[2],
                         lambda q, d: r.process_frame(d, None, False, 0.05, 1)[0][0], lambda i: r.pose(i))
    r.close()
    want_added, want = oracle_recovery(oracle, hip)
    assert added == want_added
    for (kf, kf_pose, pose), (wkf, wkf_pose, wpose) in zip(out, want):
        assert kf == wkf and np.array_equal(kf_pose, wkf_pose)
        assert np.abs(pose[12:15] - wpose[12:15]).max() < 2e-4, (kf, pose[12:15], wpose[12:15])
    check_recovered(out)


# ---- the C++ engine ---------------------------------------------------------------------------------------------------------------------

DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "relocaliser_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "relocaliser_demo")
DEMO_FRAMES, DEMO_QUERY = 24, 10


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_demo_and_engine_members_compile(tmp_path):
    assert os.path.exists(build_demo())
    src = tmp_path / "reloc.cpp"
    src.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template int ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>::Relocalise(const uint8_t*, const int16_t*);\n'
                   'template int ITMMainEngine_HIP<ITMVoxel_f_rgb, ITMPlainVoxelArray>::Relocalise(const uint8_t*, const int16_t*);\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_s_rgb, ITMVoxelBlockHash>::SetKeyframeHarvesting(bool);\n'
                   'int f(ITMRelocaliser_HIP* r, const float* d, const ITMPose* p) { int n[2]; float q[2]; return r->ProcessFrame(d, p, 2, n, q, true); }\n'
                   'ITMLibSettings s; static_assert(sizeof(s.relocCapacity) == 4, ""); bool off = s.useRelocalisation; float t = s.relocHarvestingThreshold;\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)
    assert ITMLibSettings_defaults(tmp_path) == [0, 0.2, 65536]


def ITMLibSettings_defaults(tmp_path):
    src = tmp_path / "defaults.cpp"
    src.write_text('#include <cstdio>\n#include "itm_hip_engines.hpp"\nint main() { itmhip::ITMLibSettings s; '
                   'printf("[%d, %.9g, %d]\\n", s.useRelocalisation ? 1 : 0, (double)s.relocHarvestingThreshold, s.relocCapacity); return 0; }\n')
    exe = tmp_path / "defaults"
    lib = os.path.dirname(__import__("infinitam_amd").lib_path())
    subprocess.run(["g++", "-std=c++14", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(exe), "-L", lib, "-l:libitmhip.so",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    got = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    return [got[0], round(got[1], 6), got[2]]


def demo_raw(k):
    return synth.raw_depth_mm(SC.w, SC.h, SC.position(k), SC.intr()).astype(np.int16)


@pytest.mark.gpu
def test_engine_relocalises_like_the_same_calls_through_the_binding(hip, tmp_path):
    """relocaliser_demo: ITMMainEngine_HIP with useRelocalisation tracks (ICP) and fuses SC's first frames, pose_d is overwritten with a
    pose 30 cm off, Relocalise on a frame of the sequence.  The same calls through the Python binding give the same keyframes, the same
    nearest keyframe, the same refined pose and the same maps, bit for bit."""
    path = tmp_path / "frames.bin"
    raws = [demo_raw(k) for k in range(DEMO_FRAMES)]
    with open(path, "wb") as f:
        f.write(np.array([SC.w, SC.h, DEMO_FRAMES, DEMO_QUERY], np.int32).tobytes())
        f.write(np.array(SC.intr(), F32).tobytes())
        f.write(np.stack(raws).tobytes())
        f.write(np.stack([SC.pose(k) for k in range(DEMO_FRAMES)]).astype(F32).tobytes())
    res = subprocess.run([build_demo(), str(path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])

    # the same through the binding: ITMMainEngine::ProcessFrame as tests/test_tracker.py's closed_loop writes it, plus the harvest
    P = SC.w * SC.h
    sc = Scenario(name="reloc_demo", w=SC.w, h=SC.h, voxelSize=0.01, frames=DEMO_FRAMES, stream=SC.stream)
    ses = T.Session(hip, sc, deferred_fusion=False)
    r = Relocaliser(hip, SC.w, SC.h, capacity=256, lo=0.35, hi=3.0)      # the engine draws the thresholds from the view frustum
    depth = DevBuffer(hip, P * 4, F32, (SC.h, SC.w))
    cfg = recovery_config()

    def view_of(raw, pose):
        d = hip.to_backend(raw)
        hip.check(hip.fn["convert_depth_affine"](d.ptr, depth.ptr, SC.w, SC.h, 0.001, 0.0, None), "convert")
        hip.sync()
        d.close()
        return capi.View(depth, SC.w, SC.h, M_d=pose, intr_d=SC.intr())

    def track(v, pose):
        vs = v.struct()
        out = (C.c_float * 16)()
        sp = np.ascontiguousarray(pose, F32).ctypes.data_as(C.POINTER(C.c_float))
        hip.check(hip.fn["track_camera"](C.byref(cfg), C.byref(vs), ses.points.ptr, ses.normals.ptr, sp, out, None), "track_camera")
        return np.array(out[:], F32)

    pose = SC.pose(0).astype(F32)
    added = []
    for k in range(DEMO_FRAMES):
        v = view_of(raws[k], pose)
        if k > 0:
            pose = track(v, pose)
            v.M_d = pose
        ses.scene.process_frame(v, ses.rs, ses.points, ses.normals)
        added.append(r.process_frame(depth, pose, True, 0.05, 1)[2])
    v = view_of(raws[DEMO_QUERY], pose)
    ids, dist, _ = r.process_frame(depth, None, False, 0.05, 1)
    kf_pose = r.pose(int(ids[0]))
    s, rs = ses.scene, ses.rs
    s.vis.FindVisibleBlocks(kf_pose, SC.intr(), rs)
    v.M_d = kf_pose
    s.vis.CreateExpectedDepths(kf_pose, SC.intr(), rs)
    s.vis.CreateICPMaps(v, rs, ses.points, ses.normals)
    tracked = track(v, kf_pose)
    v.M_d = tracked
    s.vis.CreateExpectedDepths(tracked, SC.intr(), rs)
    s.vis.CreateICPMaps(v, rs, ses.points, ses.normals)
    bits = ses.points.numpy().view(np.uint32).reshape(-1)
    digest = [int(bits.astype(np.uint64).sum()), int(np.bitwise_xor.reduce(bits))]

    assert (got["none"], got["kept"]) == (-1, 1), "an empty database: -1 and the pose stays"
    assert got["added"] == [max(a, -1) for a in added] and sum(a >= 0 for a in added) >= 3
    assert got["count"] == r.count
    assert got["keyframe"] == got["nearest"] == int(ids[0]) and F32(got["dist"]) == dist[0]
    assert np.array_equal(np.array(got["keyframe_pose"], F32), kf_pose)
    assert np.array_equal(np.array(got["pose"], F32), tracked), (got["pose"], tracked.tolist())
    assert got["points"] == digest and got["age"] == 0
    # and it is a recovery: from 30 cm off to the keyframe's pose to (well) within half of the keyframe's distance to the truth
    truth = SC.pose(DEMO_QUERY)
    before, after = np.linalg.norm(kf_pose[12:15] - truth[12:15]), np.linalg.norm(tracked[12:15] - truth[12:15])
    print(f"keyframe {int(ids[0])}: translation error {before:.3e} m before, {after:.3e} m after")
    assert before < 0.1 and (before < 0.01 or after < 0.5 * before), (before, after)
    r.close()
    ses.close()
