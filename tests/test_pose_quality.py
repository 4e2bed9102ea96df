"""Pose quality and the tracking verdict (include/itm_hip.h, itm_pose_quality_*; infinitam_amd/csrc/pose_quality.hip): a depth image under
a pose judged against the fused TSDF, against the float32 numpy restatement of the sequential definition (tests/pose_quality_terms.py,
built on tests/scene_query_terms.py) -- counts and residual image bit for bit, the two double sums within the rounding bound of their
additions.

CPU: the host-only defaults, refusals and verdict, the struct layouts, the restatement pinned on the synthetic scene fused by the
oracle (true pose GOOD, shifted and turned poses not), the engine's settings and members.  GPU: the kernel in both wave shapes, on
every voxel access path, on the image shapes where its indexing can go wrong; handles on two threads; recorded frames; and the C++
engine (tests/cpp/tracking_verdict_demo.cpp) acting on the verdict.

The poses.  "+3 cm along z" adds 0.03 to the pose's translation z (world -> camera): every point lands 3 cm nearer than the surface
that was fused, in voxels that hold free space -- KNOWN, and further than inlierDistance = 1 cm from the surface, so not one inlier.
The yaw turns the camera by 0.17 rad about y in place; the lateral shifts move along the wall."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import itm_testlib as T
import pose_quality_terms as PQ
import scene_query_terms as SQ
from infinitam_amd import capi, synth
from infinitam_amd.capi import DevBuffer, PoseQuality, PoseQualityConfig, PoseQualityStats
from itm_testlib import Scenario

F32 = np.float32
BASE = dict(w=160, h=120, voxelSize=0.01, frames=5, stream=3)
SC = Scenario(name="pq_hash_s", **BASE)
SCENES = {
    "hash_s": SC,
    "hash_f_rgb": Scenario(name="pq_hash_f_rgb", voxelType=T.VOXEL_F_RGB, colour=True, **BASE),
    "dense_s": Scenario(name="pq_dense_s", indexType=T.INDEX_DENSE, denseSize=(64, 64, 64), denseOffset=(-32, -32, 95), **BASE),
    "hash_far": Scenario(name="pq_hash_far", origin=(40.0, -30.0, 20.0), **BASE),
}
JUDGED = 2                # the frame whose depth image is judged
COUNTS = ("noPixels", "noValid", "noKnown", "noInliers")


def poses_of(sc):
    """the four poses the kernel is judged at, for the depth image of frame JUDGED: the truth and the three kinds of error of the header"""
    true = sc.pose(JUDGED)
    return {"true": true, "z+3cm": PQ.shifted(true, tz=0.03), "yaw": PQ.yawed(true, 0.17), "x+10cm": PQ.shifted(true, tx=0.1)}


# ---- CPU: defaults, refusals, layouts, verdict ------------------------------------------------------------------------------------------

def test_default_config(hip_host):
    c = PoseQuality.default_config(hip_host, 0.02)
    want = PQ.default_config(0.02)
    assert F32(c.inlierDistance) == want["inlierDistance"] == F32(F32(0.5) * F32(0.02)) and c.minWeight == 1
    for n in ("minValidFraction", "failOverlap", "poorOverlap", "failInliers", "goodInliers"):
        assert F32(getattr(c, n)) == want[n], n
    assert [round(float(getattr(c, n)), 6) for n in ("minValidFraction", "failOverlap", "poorOverlap", "failInliers", "goodInliers")] == [0.05, 0.1, 0.3, 0.5, 0.9]
    assert PQ.config_of(c) == {k: v for k, v in want.items()}
    assert F32(PoseQuality.default_config(hip_host, 0.04).inlierDistance) == F32(0.02)
    for mu in (0.0, -1.0, float("nan")):
        with pytest.raises(capi.ItmError):
            PoseQuality.default_config(hip_host, mu)
    assert hip_host.fn["pose_quality_default_config"](0.02, None) == capi.ERR_INVALID


BAD_CONFIGS = [("inlierDistance", 0.0), ("inlierDistance", -0.01), ("inlierDistance", float("nan")), ("minWeight", 0), ("minWeight", -3),
               ("minValidFraction", -0.01), ("minValidFraction", 1.01), ("failOverlap", -0.5), ("poorOverlap", 1.5), ("failInliers", float("nan")),
               ("goodInliers", 2.0), ("failOverlap", 0.31), ("failInliers", 0.91), ("poorOverlap", 0.09), ("goodInliers", 0.49)]


def test_bad_configurations_are_refused_on_the_host(hip_host):
    good = PoseQuality.default_config(hip_host, 0.02)
    stats = PoseQualityStats(100, 100, 100, 100, 0.0, 0.0)
    assert PoseQuality.verdict(hip_host, stats, good) == capi.TRACKING_GOOD
    h = PoseQuality(hip_host)                                  # creating a handle touches no device
    view = capi.View(1, 4, 4).struct()                         # never dereferenced: the configuration is refused first
    for name, v in BAD_CONFIGS:
        c = PoseQualityConfig.from_buffer_copy(good)
        setattr(c, name, v)
        assert PQ.config_refused(PQ.config_of(c)), (name, v)
        out = C.c_int32(7)
        assert hip_host.fn["pose_quality_verdict"](C.byref(stats), C.byref(c), C.byref(out)) == capi.ERR_INVALID, (name, v)
        assert b"pose quality" in hip_host.fn["last_error"]() and out.value == 7
        got = PoseQualityStats()
        assert hip_host.fn["pose_quality_evaluate"](C.c_void_p(h.h), C.c_void_p(1), C.byref(view), C.byref(c), C.byref(got), None, None) == capi.ERR_INVALID, (name, v)
    # the limits themselves are allowed
    for name, v in (("minValidFraction", 0.0), ("goodInliers", 1.0), ("failOverlap", 0.3), ("failInliers", 0.9), ("minWeight", 300)):
        c = PoseQualityConfig.from_buffer_copy(good)
        setattr(c, name, v)
        assert not PQ.config_refused(PQ.config_of(c))
        PoseQuality.verdict(hip_host, stats, c)
    # null arguments and empty images
    got = PoseQualityStats()
    for w, hgt in ((0, 4), (4, 0), (-1, -1)):
        v = capi.View(1, w, hgt).struct()
        assert hip_host.fn["pose_quality_evaluate"](C.c_void_p(h.h), C.c_void_p(1), C.byref(v), C.byref(good), C.byref(got), None, None) == capi.ERR_INVALID
    for args in ((None, C.c_void_p(1), C.byref(view), C.byref(good), C.byref(got)), (C.c_void_p(h.h), None, C.byref(view), C.byref(good), C.byref(got)),
                 (C.c_void_p(h.h), C.c_void_p(1), None, C.byref(good), C.byref(got)), (C.c_void_p(h.h), C.c_void_p(1), C.byref(view), None, C.byref(got)),
                 (C.c_void_p(h.h), C.c_void_p(1), C.byref(view), C.byref(good), None)):
        assert hip_host.fn["pose_quality_evaluate"](*args, None, None) == capi.ERR_INVALID
    assert hip_host.fn["pose_quality_verdict"](None, C.byref(good), C.byref(C.c_int32())) == capi.ERR_INVALID
    assert hip_host.fn["pose_quality_create"](None) == capi.ERR_INVALID
    assert hip_host.fn["pose_quality_destroy"](None) == 0
    h.close()


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    fields_c = ["inlierDistance", "minWeight", "minValidFraction", "failOverlap", "poorOverlap", "failInliers", "goodInliers"]
    fields_s = ["noPixels", "noValid", "noKnown", "noInliers", "sumSqKnown", "sumSqInliers"]
    body = ['printf("%zu %zu ", sizeof(itm_pose_quality_config), sizeof(itm_pose_quality));']
    body += [f'printf("%zu ", offsetof(itm_pose_quality_config, {n}));' for n in fields_c]
    body += [f'printf("%zu ", offsetof(itm_pose_quality, {n}));' for n in fields_s]
    body += ['printf("%d %d %d %.9g %.9g\\n", ITM_TRACKING_FAILED, ITM_TRACKING_POOR, ITM_TRACKING_GOOD, (double)ITM_POSE_QUALITY_UNKNOWN, (double)ITM_POSE_QUALITY_NONE);']
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "itm_hip.h"\nint main(void){' + "".join(body) + "return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    want = [C.sizeof(PoseQualityConfig), C.sizeof(PoseQualityStats)] + [getattr(PoseQualityConfig, n).offset for n in fields_c] + [getattr(PoseQualityStats, n).offset for n in fields_s]
    assert [int(x) for x in got[:len(want)]] == want and want[:2] == [28, 32]
    assert [int(x) for x in got[len(want):len(want) + 3]] == [capi.TRACKING_FAILED, capi.TRACKING_POOR, capi.TRACKING_GOOD] == [PQ.FAILED, PQ.POOR, PQ.GOOD] == [0, 1, 2]
    assert [F32(x) for x in got[-2:]] == [capi.POSE_QUALITY_UNKNOWN, capi.POSE_QUALITY_NONE] == [PQ.UNKNOWN, PQ.NONE]


# thresholds that are exact in binary, so that "equal" can be hit: of 1600 pixels 100 must be valid; of 800 valid 100 / 200 known; of 400
# known 200 / 350 inliers
EXACT = dict(inlierDistance=0.01, minWeight=1, minValidFraction=0.0625, failOverlap=0.125, poorOverlap=0.25, failInliers=0.5, goodInliers=0.875)
VERDICT_TABLE = [
    # (noPixels, noValid, noKnown, noInliers), overrides, result
    ((1600, 99, 99, 99), {}, PQ.FAILED), ((1600, 100, 100, 100), {}, PQ.GOOD),                                   # noValid < minValidFraction * noPixels
    ((1600, 800, 99, 99), {}, PQ.FAILED), ((1600, 800, 100, 100), {}, PQ.POOR),                                  # noKnown < failOverlap * noValid
    ((1600, 800, 199, 199), {}, PQ.POOR), ((1600, 800, 200, 200), {}, PQ.GOOD),                                  # noKnown < poorOverlap * noValid
    ((1600, 800, 400, 199), {}, PQ.FAILED), ((1600, 800, 400, 200), {}, PQ.POOR),                                # noInliers < failInliers * noKnown
    ((1600, 800, 400, 349), {}, PQ.POOR), ((1600, 800, 400, 350), {}, PQ.GOOD),                                  # noInliers < goodInliers * noKnown
    ((1600, 800, 0, 0), {}, PQ.FAILED),                                                                          # noKnown == 0 ...
    ((1600, 800, 0, 0), {"failOverlap": 0.0, "poorOverlap": 0.0, "failInliers": 0.0, "goodInliers": 0.0}, PQ.FAILED),   # ... by its own rule alone
    ((1600, 800, 1, 0), {"failOverlap": 0.0, "poorOverlap": 0.0, "failInliers": 0.0, "goodInliers": 0.0}, PQ.GOOD),
    ((1600, 0, 0, 0), {}, PQ.FAILED),                                                                            # noValid == 0 ...
    ((1600, 0, 0, 0), {"minValidFraction": 0.0, "failOverlap": 0.0, "poorOverlap": 0.0, "failInliers": 0.0, "goodInliers": 0.0}, PQ.FAILED),   # ... is noKnown == 0 too
    ((0, 0, 0, 0), {"minValidFraction": 0.0}, PQ.FAILED),
]


def test_verdict_on_a_table_of_counts(hip_host):
    for counts, over, want in VERDICT_TABLE:
        cfg = PoseQualityConfig(**{**EXACT, **over})
        stats = PoseQualityStats(*counts, 0.0, 0.0)
        got = PoseQuality.verdict(hip_host, stats, cfg)
        assert got == want == PQ.verdict(stats.as_dict(), PQ.config_of(cfg)), (counts, over, got, want)
    # the defaults are float32 values compared in double: 0.05f is a little more than 0.05, so 50 valid pixels of 1000 are too few
    dflt = PoseQuality.default_config(hip_host, 0.02)
    assert float(F32(0.05)) * 1000 > 50
    assert PoseQuality.verdict(hip_host, PoseQualityStats(1000, 50, 50, 50, 0.0, 0.0), dflt) == PQ.FAILED
    assert PoseQuality.verdict(hip_host, PoseQualityStats(1000, 51, 51, 51, 0.0, 0.0), dflt) == PQ.GOOD
    # and the library agrees with the restatement on counts drawn at random around the thresholds
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(3000):
        P = int(rng.integers(1, 2000))
        V = int(rng.integers(0, min(P, 4 * max(int(0.05 * P), 1)) + 1)) if rng.random() < 0.3 else int(rng.integers(0, P + 1))
        K = int(rng.integers(0, V + 1)) if rng.random() < 0.5 else int(min(V, rng.integers(0, int(0.35 * V) + 2)))
        I = int(rng.integers(0, K + 1)) if rng.random() < 0.5 else int(rng.integers(int(0.45 * K), K + 1))
        stats = PoseQualityStats(P, V, K, I, 0.0, 0.0)
        got = PoseQuality.verdict(hip_host, stats, dflt)
        assert got == PQ.verdict(stats.as_dict(), PQ.config_of(dflt)), (P, V, K, I)
        seen.add(got)
    assert seen == {0, 1, 2}


def test_symbols_are_declared_exported_and_host_callable(hip_host):
    declared = capi.declared_functions()
    names = sorted(n for n in declared if n.startswith("pose_quality_"))
    assert names == ["pose_quality_create", "pose_quality_default_config", "pose_quality_destroy", "pose_quality_evaluate", "pose_quality_verdict"]
    for n in names:
        assert n in capi._HOST_IO_SIGS and n not in capi._SIGS and n in hip_host.fn
    import infinitam_amd
    assert infinitam_amd.PoseQuality is PoseQuality and infinitam_amd.PoseQualityConfig is PoseQualityConfig and infinitam_amd.PoseQualityStats is PoseQualityStats
    out = subprocess.run(["nm", "-D", "--defined-only", infinitam_amd.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert all("itm_" + n in exported for n in names)


# ---- CPU: the restatement on the oracle's scene ---------------------------------------------------------------------------------------------

_oracle = {}


def oracle_scene(oracle):
    if "reader" not in _oracle:
        ses = T.Session(oracle, SC)
        for k in range(SC.frames):
            ses.frame(k, fused=True)
        _oracle["reader"] = PQ.reader_of(ses.scene)
        ses.close()
    return _oracle["reader"]


def restated(reader, sc, depth, pose, cfg=None):
    return PQ.evaluate(reader, depth, pose, sc.intr(), sc.voxelSize, sc.mu, cfg or PQ.default_config(sc.mu))


def test_restatement_separates_the_classes_on_the_oracle(oracle):
    reader = oracle_scene(oracle)
    cfg = PQ.default_config(SC.mu)
    depth, poses = SC.depth(JUDGED), poses_of(SC)
    shown = {}

    def judge(name, d, pose):
        s, img = restated(reader, SC, d, pose)
        overlap, ratio = s["noKnown"] / max(s["noValid"], 1), s["noInliers"] / max(s["noKnown"], 1)
        shown[name] = (round(overlap, 3), round(ratio, 3), PQ.verdict(s, cfg))
        # the image and the counts say the same
        known = np.abs(img) < F32(1e29)
        assert s["noKnown"] == int(known.sum()) and s["noValid"] == int((img != PQ.NONE).sum()) and s["noInliers"] == int((np.abs(img[known]) <= cfg["inlierDistance"]).sum())
        assert np.all(np.abs(img[known]) <= F32(SC.mu))
        return s, overlap, ratio, PQ.verdict(s, cfg)

    s, overlap, ratio, v = judge("true", depth, poses["true"])
    assert v == PQ.GOOD and overlap > 0.9 and ratio > 0.99 and s["noValid"] == s["noPixels"] == SC.w * SC.h
    s, overlap, ratio, v = judge("true, 20 frames on", SC.depth(JUDGED + 20), SC.pose(JUDGED + 20))
    assert v == PQ.GOOD and overlap > 0.8 and ratio > 0.98
    s, overlap, ratio, v = judge("z+3cm", depth, poses["z+3cm"])
    assert v == PQ.FAILED and s["noInliers"] == 0 and s["sumSqInliers"] == 0.0
    s, overlap, ratio, v = judge("yaw", depth, poses["yaw"])
    assert v == PQ.FAILED and overlap < 0.2 and ratio < 0.4
    for tx in (0.02, 0.05, 0.1, 0.2, 0.3, -0.02, -0.1, -0.3):
        s, overlap, ratio, v = judge(f"x{tx:+.2f}", depth, PQ.shifted(poses["true"], tx=tx))
        assert v != PQ.FAILED and overlap >= 0.4 and 0.7 <= ratio < 0.9, (tx, overlap, ratio)
    print("pose: (overlap, inlier ratio, verdict)", shown)
    # holes count as NONE and nothing else changes class
    holes = depth.copy(); holes[::5, ::3] = -1.0; holes[7:20, 30:60] = 0.0; holes[50, 50] = np.nan
    sh, imgh = restated(reader, SC, holes, poses["true"])
    s0, img0 = restated(reader, SC, depth, poses["true"])
    gone = ~(holes > 0)
    assert sh["noValid"] == s0["noValid"] - int(gone.sum()) and np.all(imgh[gone] == PQ.NONE) and np.array_equal(imgh[~gone].view(np.uint32), img0[~gone].view(np.uint32))


# ---- CPU: the engine's settings and members ------------------------------------------------------------------------------------------------

DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "tracking_verdict_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "tracking_verdict_demo")


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
    src = tmp_path / "verdict.cpp"
    src.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template class ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>;\n'
                   'template class ITMMainEngine_HIP<ITMVoxel_f_rgb, ITMPlainVoxelArray>;\n'
                   'typedef ITMMainEngine_HIP<ITMVoxel_s_rgb, ITMVoxelBlockHash> E;\n'
                   'int f(E* e) { const itm_pose_quality& q = e->GetPoseQuality(); return (int)e->GetTrackingResult() + q.noKnown + e->GetRelocalisationCount() + (e->LastFrameFused() ? 1 : 0); }\n'
                   'itm_pose_quality g(ITMPoseQuality_HIP* p, const ITMScene<ITMVoxel_f, ITMPlainVoxelArray>* s, const ITMView* v, const ITMTrackingState* t, float* r) '
                   '{ itm_pose_quality q = p->Evaluate(s, v, t, r); return p->Verdict(q) == ITMPoseQuality_HIP::TRACKING_GOOD ? q : p->Evaluate(s, v, t); }\n'
                   'ITMLibSettings s; static_assert(sizeof(s.poseQuality) == sizeof(itm_pose_quality_config), "");\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)
    src = tmp_path / "defaults.cpp"
    src.write_text('#include <cstdio>\n#include "itm_hip_engines.hpp"\nint main() { itmhip::ITMLibSettings s; '
                   'printf("[%d, %d, %.9g, %d]\\n", s.useTrackingVerdict ? 1 : 0, s.relocFusionDelay, (double)s.poseQuality.inlierDistance, s.useRelocalisation ? 1 : 0); return 0; }\n')
    exe = tmp_path / "defaults"
    lib = os.path.dirname(__import__("infinitam_amd").lib_path())
    subprocess.run(["g++", "-std=c++14", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(exe), "-L", lib, "-l:libitmhip.so",
                    "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    assert json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == [0, 10, 0, 0]


# ---- GPU: the kernel against the restatement --------------------------------------------------------------------------------------------------

# the forms of the sdf mirror a hash scene can be created with (read from the environment at creation)
FORMS = {"paged": {"ITM_MIRROR": "paged"}, "paged_few": {"ITM_MIRROR": "paged", "ITM_MIRROR_PAGES": "5"}, "mirror_off": {"ITM_MIRROR": "off"}}


@contextlib.contextmanager
def environment(values):
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
    """A scene fused from the scenario's frames on the product, the restatement's reader of it, and a handle."""

    def __init__(self, be, sc, env=None, moved_away=False):
        self.be, self.sc = be, sc
        with environment(env or {}):
            self.ses = T.Session(be, sc)
        for k in range(sc.frames):
            self.ses.frame(k, fused=True)
        if moved_away:      # one frame 40 m away: both cubes are re-placed around the new camera, every block fused so far lies outside them
            self.ses.sc = Scenario(**{**sc.__dict__, "origin": (40.0, -30.0, 20.0)})
            self.ses.frame(0, fused=True)
            self.ses.sc = sc
        self.scene = self.ses.scene
        self.reader = PQ.reader_of(self.scene)
        self.handle = PoseQuality(be)
        self.depth = sc.depth(JUDGED)
        self.depth_dev = be.to_backend(self.depth)

    def view(self, pose, depth_dev=None, w=None, h=None):
        return capi.View(depth_dev or self.depth_dev, w or self.sc.w, h or self.sc.h, M_d=pose, intr_d=self.sc.intr())

    def close(self):
        self.handle.close()
        self.depth_dev.close()
        self.ses.close()


_built = {}


def built(be, name, **kw):
    key = (id(be), name, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _built:
        _built[key] = Built(be, SCENES[name], **kw)
    return _built[key]


@pytest.fixture(scope="module", autouse=True)
def close_scenes():
    yield
    for b in _built.values():
        b.close()
    _built.clear()


@pytest.fixture(params=[0, 1], ids=["tiles", "rows"])
def shape(request, hip):
    """both wave shapes of the kernel: 8 x 8 tiles (the default) and 64 consecutive pixels"""
    hip.check(hip.fn["debug_set"](capi.DEBUG_POSE_QUALITY_ROWS, request.param), "debug_set")
    yield request.param
    hip.check(hip.fn["debug_set"](capi.DEBUG_POSE_QUALITY_ROWS, 0), "debug_set")


def check_against_restatement(b, depth, pose, what, depth_dev=None, cfg=None):
    """counts exactly, the image bit for bit, each sum within n * 2^-53 * sum of math.fsum's (n additions of non-negative doubles),
    and a second call with the same bits"""
    h, w = depth.shape
    want, want_img = restated(b.reader, b.sc, depth, pose, PQ.config_of(cfg) if cfg is not None else None)
    own = depth_dev is None
    dev = b.be.to_backend(depth) if own else depth_dev
    view = b.view(pose, dev, w, h)
    got, img = b.handle.evaluate(b.scene, view, cfg, residuals=True)
    again, img2 = b.handle.evaluate(b.scene, view, cfg, residuals=True)
    bare = b.handle.evaluate(b.scene, view, cfg)                     # residuals_dev == NULL
    if own:
        dev.close()
    got = got.as_dict()
    print(what, got, "restated sums", want["sumSqKnown"], want["sumSqInliers"])
    assert {n: got[n] for n in COUNTS} == {n: want[n] for n in COUNTS}, (what, got, want)
    if not np.array_equal(img.view(np.uint32), want_img.view(np.uint32)):
        bad = np.argwhere(img.view(np.uint32) != want_img.view(np.uint32))
        raise AssertionError(f"{what}: {len(bad)} residuals differ, first at {bad[:5].tolist()}: {img[tuple(bad[0])]} vs {want_img[tuple(bad[0])]}")
    for name, n in (("sumSqKnown", want["noKnown"]), ("sumSqInliers", want["noInliers"])):
        assert abs(got[name] - want[name]) <= n * 2.0 ** -53 * want[name], (what, name, got[name], want[name])
    for other in (again.as_dict(), bare.as_dict()):
        assert other == got, (what, other, got)                     # the doubles compare by value: the same bits (no NaN, no -0)
    assert np.array_equal(img2.view(np.uint32), img.view(np.uint32))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_counts_and_residuals_equal_the_restatement(hip, shape, name):
    b = built(hip, name)
    cfg = PoseQuality.default_config(hip, b.sc.mu)
    seen = {}
    for pose_name, pose in poses_of(b.sc).items():
        got = check_against_restatement(b, b.depth, pose, f"{name}, {pose_name}", b.depth_dev)
        seen[pose_name] = (got, PoseQuality.verdict(hip, PoseQualityStats(**got), cfg))
    assert seen["z+3cm"][0]["noInliers"] == 0 and seen["z+3cm"][1] == PQ.FAILED and seen["yaw"][1] == PQ.FAILED
    assert seen["true"][0]["noKnown"] > 1000 and seen["true"][0]["noInliers"] > 0.99 * seen["true"][0]["noKnown"]
    if name != "dense_s":                 # the 64^3 volume holds the sphere's front alone
        assert seen["true"][1] == PQ.GOOD and seen["x+10cm"][1] == PQ.POOR
    # another configuration: a voxel needs three observations, the band is a voxel wide
    strict = PoseQualityConfig.from_buffer_copy(cfg)
    strict.minWeight, strict.inlierDistance = 3, 0.004
    got = check_against_restatement(b, b.depth, poses_of(b.sc)["true"], f"{name}, strict", b.depth_dev, strict)
    assert 0 < got["noInliers"] < got["noKnown"] < seen["true"][0]["noKnown"]


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["paged", "paged_few", "mirror_off", "directory_off", "table_walk"])
def test_every_voxel_access_path(hip, path):
    if path == "directory_off":
        b = built(hip, "hash_s")
        hip.check(hip.fn["debug_set"](5, 1), "debug_set")              # ITM_DEBUG_NO_DIRECTORY
    else:
        b = built(hip, "hash_s", env=FORMS.get(path), moved_away=path == "table_walk")
    try:
        info = b.scene.accel_info()
        if path.startswith("paged"):
            assert info["mirror_pages"] > 0, info
        elif path == "mirror_off":
            assert info["mirror_bytes"] == 0, info
        elif path == "table_walk":
            assert info["moves"] >= 1, info
        for pose_name, pose in poses_of(b.sc).items():
            check_against_restatement(b, b.depth, pose, f"{path}, {pose_name}", b.depth_dev)
    finally:
        hip.check(hip.fn["debug_set"](5, 0), "debug_set")


@pytest.mark.gpu
def test_image_shapes_where_the_indexing_can_go_wrong(hip, shape):
    b = built(hip, "hash_s")
    cfg = PoseQuality.default_config(hip, SC.mu)
    true = poses_of(SC)["true"]
    full = b.depth
    for name, d in (("157 x 113", full[:113, :157]), ("1 x 1", full[60:61, 80:81]), ("7 x 3", full[:3, :7]), ("65 x 9", full[40:49, 30:95]), ("8 x 8", full[:8, :8])):
        for pose_name in ("true", "x+10cm"):
            check_against_restatement(b, np.ascontiguousarray(d), poses_of(SC)[pose_name], f"{name}, {pose_name}")
    got = check_against_restatement(b, np.full((SC.h, SC.w), F32(-1.0)), true, "all -1")
    assert got["noValid"] == 0 and got["noKnown"] == 0 and PoseQuality.verdict(hip, PoseQualityStats(**got), cfg) == PQ.FAILED
    hole = full.copy(); hole[45:75, 60:100] = 0.0; hole[3, 5] = np.nan
    got = check_against_restatement(b, hole, true, "40 x 30 hole")
    assert got["noValid"] == SC.w * SC.h - 40 * 30 - 1
    # an empty scene straight after ResetScene
    ses = T.Session(hip, SC)
    empty = Built.__new__(Built)
    empty.be, empty.sc, empty.ses, empty.scene, empty.handle, empty.depth_dev = hip, SC, ses, ses.scene, b.handle, b.depth_dev
    empty.reader = PQ.reader_of(ses.scene)
    got = check_against_restatement(empty, full, true, "empty scene", b.depth_dev)
    assert got["noKnown"] == 0 and got["noValid"] == SC.w * SC.h and PoseQuality.verdict(hip, PoseQualityStats(**got), cfg) == PQ.FAILED
    ses.close()


@pytest.mark.gpu
def test_two_handles_on_two_threads_answer_like_one(hip):
    b = built(hip, "hash_s")
    poses = list(poses_of(SC).values())
    want = [b.handle.evaluate(b.scene, b.view(p), residuals=True) for p in poses]
    handles = [PoseQuality(hip) for _ in (0, 1)]
    streams = []
    for _ in (0, 1):
        st = C.c_void_p(); hip.check(hip.fn["stream_create"](C.byref(st)), "stream_create"); streams.append(st)
    got, errors = {0: [], 1: []}, []
    start = threading.Barrier(2)

    def work(i):
        try:
            start.wait()
            for rep in range(5):
                order = poses if i == 0 else poses[::-1]
                for p in order:
                    res = handles[i].evaluate(b.scene, b.view(p), residuals=(rep == 0), stream=streams[i].value)
                    if rep == 0:
                        got[i].append(res)
                    else:
                        got[i].append((res, None))
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
            assert len(got[i]) == 5 * len(poses)
            for j, (st, img) in enumerate(got[i]):
                k = j % len(poses)
                k = k if i == 0 else len(poses) - 1 - k
                assert st.as_dict() == want[k][0].as_dict(), (i, j)
                assert img is None or np.array_equal(img.view(np.uint32), want[k][1].view(np.uint32))
    finally:
        hip.sync()
        for h in handles:
            h.close()
        for st in streams:
            hip.fn["stream_destroy"](st)


@pytest.mark.gpu
def test_evaluate_launches_recorded_frames_first(hip):
    b = built(hip, "hash_s")                                   # frames 0 .. 4, each launched
    pose = poses_of(SC)["true"]
    ses = T.Session(hip, SC, deferred_fusion=True)
    for k in range(SC.frames - 1):
        ses.frame(k, fused="four")
    before = b.handle.evaluate(ses.scene, b.view(pose))
    view = ses.view(SC.frames - 1)
    ses.scene.reco.AllocateSceneFromDepth(view, ses.rs)        # recorded, not launched
    ses.scene.reco.IntegrateIntoScene(view, ses.rs)
    ses.scene.vis.CreateExpectedDepths(view.M_d, view.intr_d, ses.rs)
    got, img = b.handle.evaluate(ses.scene, b.view(pose), residuals=True)
    want, want_img = b.handle.evaluate(b.scene, b.view(pose), residuals=True)
    assert got.as_dict() == want.as_dict() and np.array_equal(img.view(np.uint32), want_img.view(np.uint32))
    assert before.as_dict() != want.as_dict(), "the fifth frame changes what the pose is judged against"
    ses.close()


# ---- GPU: the engine --------------------------------------------------------------------------------------------------------------------------

ENGINE_FRAMES, BAD = 12, 6
ENGINE_SC = Scenario(name="pq_engine", w=160, h=120, voxelSize=0.01, frames=ENGINE_FRAMES, stream=3, localBlockNum=0x2000)


def demo_raw(k):
    return synth.raw_depth_mm(SC.w, SC.h, SC.position(k), SC.intr()).astype(np.int16)


def write_frames(path, raws, poses):
    with open(path, "wb") as f:
        f.write(np.array([SC.w, SC.h, len(raws)], np.int32).tobytes())
        f.write(np.array(SC.intr(), F32).tobytes())
        f.write(np.stack(raws).astype(np.int16).tobytes())
        f.write(np.stack(poses).astype(F32).tobytes())


def run_demo(path, **args):
    res = subprocess.run([build_demo(), str(path)] + [f"{k}={v}" for k, v in args.items()], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def engine_inputs(bad=None):
    raws = [demo_raw(k) for k in range(ENGINE_FRAMES)]
    poses = [SC.pose(k).astype(F32) for k in range(ENGINE_FRAMES)]
    if bad is not None:
        poses[bad] = PQ.shifted(poses[bad], tz=0.1)
    return raws, poses


@pytest.mark.gpu
def test_engine_is_unchanged_while_every_pose_is_good(hip, tmp_path):
    raws, poses = engine_inputs()
    write_frames(tmp_path / "frames.bin", raws, poses)
    on = run_demo(tmp_path / "frames.bin", verdict=1)
    off = run_demo(tmp_path / "frames.bin", verdict=0)
    assert [f["result"] for f in on["frames"]] == [PQ.GOOD] * ENGINE_FRAMES and all(f["fused"] for f in on["frames"])
    assert on["frames"][0]["stats"] == [0, 0, 0, 0, 0.0, 0.0] and all(f["stats"][2] > 10000 for f in on["frames"][1:])
    assert on["digest"] == off["digest"]
    assert all(f["stats"] == [0, 0, 0, 0, 0.0, 0.0] and f["result"] == PQ.GOOD and not f["fused"] and f["recoveries"] == 0 for f in off["frames"])
    assert [f["pose"] for f in on["frames"]] == [f["pose"] for f in off["frames"]]


@pytest.mark.gpu
def test_engine_refuses_a_bad_pose_from_outside(hip, tmp_path):
    raws, poses = engine_inputs(bad=BAD)
    write_frames(tmp_path / "frames.bin", raws, poses)
    got = run_demo(tmp_path / "frames.bin", verdict=1)
    skipped = run_demo(tmp_path / "frames.bin", verdict=1, skip=BAD)
    frames = got["frames"]
    assert [f["result"] for f in frames] == [PQ.GOOD] * BAD + [PQ.FAILED] + [PQ.GOOD] * (ENGINE_FRAMES - BAD - 1)
    assert [f["fused"] for f in frames] == [1] * BAD + [0] + [1] * (ENGINE_FRAMES - BAD - 1)
    assert np.array_equal(np.array(frames[BAD]["pose"], F32), poses[BAD - 1]) and frames[BAD]["recoveries"] == 0
    assert got["digest"] == skipped["digest"] and len(skipped["frames"]) == ENGINE_FRAMES - 1
    # and the bad pose does damage without the verdict
    assert run_demo(tmp_path / "frames.bin", verdict=0)["digest"] != got["digest"]


@pytest.mark.gpu
def test_engine_recovers_from_a_keyframe_and_delays_fusion(hip, tmp_path):
    raws, poses = engine_inputs(bad=BAD)
    write_frames(tmp_path / "frames.bin", raws, poses)
    got = run_demo(tmp_path / "frames.bin", verdict=1, reloc=1, delay=2)
    frames = got["frames"]
    keyframes = [np.array(p, F32) for p in got["keyframe_poses"]]
    assert len(keyframes) >= 1 and frames[BAD]["recoveries"] == 1 and frames[-1]["recoveries"] == 1
    assert frames[BAD]["result"] != PQ.FAILED and any(np.array_equal(np.array(frames[BAD]["pose"], F32), kf) for kf in keyframes)
    assert [f["result"] for f in frames[:BAD] + frames[BAD + 1:]] == [PQ.GOOD] * (ENGINE_FRAMES - 1)
    assert [f["fused"] for f in frames] == [1] * BAD + [0, 0, 0] + [1] * (ENGINE_FRAMES - BAD - 3)
    assert frames[BAD + 2]["keyframes"] == frames[BAD - 1]["keyframes"], "no keyframe is harvested while fusion is delayed"

    # the same frames through the binding: fed and fused as the engine says it did, judged at the pose the engine judged
    ses = T.Session(hip, ENGINE_SC, deferred_fusion=False)
    q = PoseQuality(hip)
    depth = DevBuffer(hip, SC.w * SC.h * 4, F32, (SC.h, SC.w))
    for k, f in enumerate(frames):
        d = hip.to_backend(raws[k])
        hip.check(hip.fn["convert_depth_affine"](d.ptr, depth.ptr, SC.w, SC.h, 0.001, 0.0, None), "convert")
        hip.sync()
        d.close()
        pose = np.array(f["pose"], F32) if k == BAD else poses[k]      # after the recovery: the second evaluation, at the recovered pose
        view = capi.View(depth, SC.w, SC.h, M_d=pose, intr_d=SC.intr())
        if k > 0:
            st = q.evaluate(ses.scene, view).as_dict()
            assert f["stats"] == [st[n] for n in COUNTS] + [st["sumSqKnown"], st["sumSqInliers"]], (k, f["stats"], st)
            assert f["result"] == PoseQuality.verdict(hip, PoseQualityStats(**st), PoseQuality.default_config(hip, SC.mu)), k
        if k == BAD:
            ses.scene.vis.FindVisibleBlocks(pose, SC.intr(), ses.rs)      # the recovery rebuilds the live visible list at the keyframe's pose
        if f["fused"]:
            ses.scene.process_frame(view, ses.rs, ses.points, ses.normals)
    q.close()
    depth.close()
    ses.close()


@pytest.mark.gpu
def test_engine_survives_a_covered_sensor(hip, tmp_path):
    order = [0, 1, 2, 3, 4, 5, None, None, None, 5, 6]
    raws = [demo_raw(k) if k is not None else np.zeros((SC.h, SC.w), np.int16) for k in order]
    poses = [SC.pose(k if k is not None else 5).astype(F32) for k in order]       # the ICP tracker reads poses[0] alone
    write_frames(tmp_path / "frames.bin", raws, poses)
    got = run_demo(tmp_path / "frames.bin", tracker="icp", verdict=1, reloc=1, delay=0, digests=1)
    frames = got["frames"]
    last = frames[5]
    assert [f["result"] for f in frames[:6]] == [PQ.GOOD] * 6 and all(f["fused"] for f in frames[:6])
    for f in frames[6:9]:
        assert f["result"] == PQ.FAILED and not f["fused"] and f["stats"][1] == 0
        assert f["pose"] == last["pose"] and f["digest"] == last["digest"] and f["keyframes"] == last["keyframes"] and f["recoveries"] == 0
    assert frames[9]["result"] == PQ.GOOD and frames[9]["fused"] and frames[9]["digest"] != last["digest"]
    assert np.abs(np.array(frames[9]["pose"], F32)[12:15] - SC.pose(5)[12:15]).max() < 5e-3
    assert frames[10]["result"] == PQ.GOOD
