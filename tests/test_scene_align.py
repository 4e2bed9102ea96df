"""Scene alignment (include/itm_hip.h: itm_scene_band_samples, itm_aligner_evaluate / _align; restatement: tests/scene_align_terms.py).

  * CPU: the two host steps (itm_align_step, itm_align_apply_step) against numpy float64, the defaults, the refusals, the struct
    layouts, the symbols, the adapters; the restated loop on the analytic scenes -- it recovers the exact ground truth on the room
    corner from both starts, with conditioning >= 1e-2, and reports conditioning < 1e-3 on the sphere in front of a wall.  Its own
    error e_ref is the yardstick for the GPU.
  * GPU: band samples bit for bit; an evaluation's valid count exact and every sum within ulp32(sum64) + n 2^-52 sum|term| (the ICP
    bound of tests/test_tracker_terms.py: no transcendental is involved); the loop ends CONVERGED within e_ref + 4 minStep of the truth
    -- with the step size as the only stopping rule the GPU loop and the restated loop each stop within about two steps of the same
    minimum, whatever accept and reject branches rounding makes them take -- DEGENERATE where the geometry is, TOO_FEW_SAMPLES
    with the input pose where it is; the adapters give the same pose; a fusion under the refined pose is closer than under the start."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import mesh_attr_cases as MC
import mesh_dense_cases as MD
import scene_align_terms as A
import scene_query_terms as Q
import test_scene_query as TQ
from infinitam_amd import capi
from infinitam_amd.capi import AlignConfig, AlignEval, AlignResult, SceneAligner, _P      # (none of them exists without the feature)

F = np.float32
EPS52 = 2.0 ** -52
SIZE3 = (A.N, A.N, A.N)
MIN_STEP = 1e-5
VOXEL_TYPES = {"s": capi.VOXEL_S, "f": capi.VOXEL_F, "s_rgb": capi.VOXEL_S_RGB, "f_rgb": capi.VOXEL_F_RGB}
NEW_SYMBOLS = ("align_default_config", "align_step", "align_apply_step", "scene_band_samples", "aligner_create", "aligner_destroy", "aligner_set_samples",
               "aligner_evaluate", "aligner_align")


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64).astype(F))).astype(np.float64)


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def default_cfg(be, **kw):
    return capi.align_default_config(A.VOXEL_SIZE, A.MU, be).replace(**kw)


# ---- the restated loop on the analytic scenes: computed once, the yardstick of the GPU tests ---------------------------------------------

_reference = {}


def reference(voxel, corner, start):
    """(pose, result, (rotation error, translation error)) of the restated loop on the analytic pair"""
    key = (voxel, corner, start)
    if key not in _reference:
        dst, src = A.analytic_pair(VOXEL_TYPES[voxel], corner)
        reader = A.dense_reader(dst)
        samples = A.band_samples(src, A.VOXEL_SIZE, A.MU, dense=(SIZE3, (0, 0, 0)))
        M, res = A.align(lambda P: A.evaluate(reader, samples, P, A.VOXEL_SIZE, A.MU, F(A.MU) / F(4)), A.STARTS[start], min_step=MIN_STEP)
        _reference[key] = (M, res, A.pose_error(M, A.TRUTH))
    return _reference[key]


# ---- CPU: the host steps -----------------------------------------------------------------------------------------------------------------

def random_eval(rng):
    J = rng.normal(size=(200, 6)) * np.array([1, 1, 1, 0.3, 0.3, 0.3])
    e = capi.AlignEval()
    H = (J.T @ J).astype(F)
    H = ((H + H.T) * F(0.5)).astype(F)
    e.f, e.noValid = 1.0, 200
    e.nabla[:] = [float(v) for v in (J.T @ rng.normal(size=200)).astype(F)]
    e.hessian[:] = [float(H[r, c]) for c in range(6) for r in range(6)]
    return e, H.astype(np.float64), np.array(e.nabla[:], np.float64)


def test_align_step_equals_numpy_float64(hip_host):
    rng = np.random.default_rng(3)
    for lam in (0.0, 1e-3, 1.0, 1e4):
        e, H, g = random_eval(rng)
        step = np.zeros(6, F)
        assert hip_host.fn["align_step"](C.byref(e), lam, fptr(step)) == 0
        want = A.step_of(g, H, lam)
        assert np.all(np.abs(step.astype(np.float64) - want) <= ulp32(want)), (lam, step, want)
    # a diagonal entry below 1e-15 is replaced by lambda * 1e-10, as ren_step does
    e, H, g = random_eval(rng)
    for k in range(6):
        e.hessian[5 + 6 * k] = e.hessian[k + 6 * 5] = 0.0
    H[5, :] = H[:, 5] = 0.0
    assert hip_host.fn["align_step"](C.byref(e), 2.0, fptr(step)) == 0
    want = A.step_of(g, H, 2.0)
    assert abs(want[5] + g[5] / 2e-10) <= 1e-9 * abs(want[5])
    assert np.all(np.abs(step.astype(np.float64) - want) <= ulp32(want))
    # not positive definite: no step
    e, H, g = random_eval(rng)
    e.hessian[0] = -1.0
    assert hip_host.fn["align_step"](C.byref(e), 1.0, fptr(step)) == 0 and not step.any()
    assert hip_host.fn["align_step"](None, 1.0, fptr(step)) == capi.ERR_INVALID


def test_align_apply_step_equals_numpy_float64(hip_host):
    rng = np.random.default_rng(4)
    for scale in (1e-6, 1e-3, 0.3, 2.0):
        pose = A.rigid(A.rotation(rng.normal(size=3), rng.uniform(0, 3)), rng.normal(size=3)).astype(F)
        step = (rng.normal(size=6) * scale).astype(F)
        out = np.zeros(16, F)
        flat = np.ascontiguousarray(pose.T).reshape(16)
        assert hip_host.fn["align_apply_step"](fptr(flat), fptr(step), fptr(out)) == 0
        want = A.se3_exp(step.astype(np.float64)) @ pose.astype(np.float64)
        got = out.reshape(4, 4).T.astype(np.float64)
        assert np.all(np.abs(got - want) <= ulp32(want) + 1e-15), (scale, got - want)
        assert np.array_equal(got[3], [0, 0, 0, 1])
    assert hip_host.fn["align_apply_step"](None, fptr(step), fptr(out)) == capi.ERR_INVALID


def test_default_config(hip_host):
    c = capi.align_default_config(0.01, 0.04, hip_host)
    assert (c.minWeight, c.stride, c.maxEvaluations, c.minValid) == (1, 1, 60, 100)
    assert c.maxAbsSdf == 1.0 and c.huberDelta == F(0.04) / F(4) and c.minStep == F(1e-5) and c.minConditioning == F(1e-3)
    assert capi.align_default_config(0.005, 0.02, hip_host).huberDelta == F(0.02) / F(4)
    for vs, mu in ((0.0, 0.04), (0.01, -1.0), (np.nan, 0.04), (0.01, np.inf)):
        with pytest.raises(capi.ItmError, match=r"\(-1\)"):
            capi.align_default_config(vs, mu, hip_host)
    # the header says what the conditioning threshold is: policy between the two analytic scenes, not tuned on sensor data
    text = open(capi.header_path()).read()
    assert re.search(r"minConditioning is POLICY chosen on analytic scenes", text) and "nobody has tuned it on sensor data" in text


def test_refusals_on_the_host(hip_host):
    """the matrix and the configuration are checked before anything else is looked at: no scene and no GPU are needed to be refused"""
    be = hip_host
    h = _P()
    be.check(be.fn["aligner_create"](C.byref(h)), "aligner_create")
    good = default_cfg(be)
    truth = np.ascontiguousarray(A.TRUTH.astype(F).T).reshape(16)

    def refused(matrix, cfg, why, align=True, evaluate=True):
        out, res, ev = np.full(16, 7, F), capi.AlignResult(), capi.AlignEval()
        m = np.ascontiguousarray(matrix, F).reshape(16)
        ok = True
        if align:
            rc = be.fn["aligner_align"](h, None, fptr(m), C.byref(cfg), fptr(out), C.byref(res), None)
            ok &= rc == capi.ERR_INVALID and why in (be.fn["last_error"]() or b"") and np.all(out == 7)
        if evaluate:
            rc = be.fn["aligner_evaluate"](h, None, fptr(m), C.byref(cfg), C.byref(ev), None)
            ok &= rc == capi.ERR_INVALID and why in (be.fn["last_error"]() or b"")
        return ok

    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 5, 13, 15):
            m = truth.copy()
            m[at] = bad
            assert refused(m, good, b"not finite"), (bad, at)
    m = truth.copy()
    m[0] += 2e-3
    assert refused(m, good, b"orthonormal")
    m = truth.copy()
    m[1] += 4e-4                                  # within 1e-3: passes this check (and is refused further on, for the scene it lacks)
    assert not refused(m, good, b"orthonormal") and refused(m, good, b"no samples", evaluate=False)
    assert refused(truth * np.array([1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, 1, 1, 1, 1, 1], F), good, b"reflection")
    assert refused(truth, good.replace(huberDelta=0.0), b"huberDelta") and refused(truth, good.replace(huberDelta=-1.0), b"huberDelta")
    assert refused(truth, good.replace(huberDelta=float("nan")), b"huberDelta")
    assert refused(truth, good.replace(minStep=0.0), b"minStep") and refused(truth, good.replace(minStep=-1e-5), b"minStep")
    assert refused(truth, good, b"no samples", evaluate=False), "no samples set"
    assert be.fn["aligner_align"](h, None, None, C.byref(good), None, None, None) == capi.ERR_INVALID
    assert be.fn["aligner_set_samples"](h, None, 5, None) == capi.ERR_INVALID and be.fn["aligner_set_samples"](h, _P(16), -1, None) == capi.ERR_INVALID
    assert be.fn["aligner_set_samples"](h, _P(24), 5, None) == capi.ERR_INVALID, "alignment of the samples"
    assert be.fn["scene_band_samples"](None, None, 0, C.byref(good), None, 0, C.byref(C.c_int32()), None) == capi.ERR_INVALID
    assert be.fn["aligner_destroy"](h) == 0 and be.fn["aligner_destroy"](None) == 0


def header_struct(name):
    """[(type, field, array length)] of `typedef struct NAME { ... } NAME;` in include/itm_hip.h"""
    text = open(capi.header_path()).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            fields.append((typ, m.group(1), int(m.group(2) or 0)))
    return fields


def test_struct_layouts_match_the_header():
    ctype = {"int32_t": C.c_int32, "float": C.c_float, "double": C.c_double}
    for name, cls, size in (("itm_align_config", capi.AlignConfig, 32), ("itm_align_eval", capi.AlignEval, 176), ("itm_align_result", capi.AlignResult, 40)):
        want = [(f, ctype[t] * n if n else ctype[t]) for t, f, n in header_struct(name)]
        assert [(f, t) for f, t in cls._fields_] == want, name
        assert C.sizeof(cls) == size, name
    text = open(capi.header_path()).read()
    for k, n in enumerate(("CONVERGED", "MAX_EVALUATIONS", "STALLED", "TOO_FEW_SAMPLES", "DEGENERATE")):
        assert re.search(r"#define ITM_ALIGN_%s %d\b" % (n, k), text) and getattr(capi, "ALIGN_" + n) == k
    assert re.search(r"#define ITM_COUNTER_ALIGN_SEQ %d\b" % capi.COUNTER_ALIGN_SEQ, open(os.path.join(os.path.dirname(capi.header_path()), "itm_debug.h")).read())


def test_scene_align_is_declared_and_bound(hip_host):
    declared = capi.declared_functions()
    for name in NEW_SYMBOLS:
        assert name in declared and name in capi._HOST_IO_SIGS and name not in capi._SIGS and name in hip_host.fn, name
    for name in ("band_samples", "align_from", "align_config"):
        assert callable(getattr(capi.Scene, name))
    for name in ("set_samples", "evaluate", "align"):
        assert callable(getattr(capi.SceneAligner, name))


DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "scene_align_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "scene_align_demo")


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_adapters_compile_and_link(tmp_path):
    assert os.path.exists(build_demo())
    src = tmp_path / "align.cpp"
    src.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template class ITMSceneAlignEngine_HIP<ITMVoxel_f_rgb, ITMPlainVoxelArray>;\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>::AlignSceneFrom(const ITMMainEngine_HIP&, Matrix4f&, itm_align_result*);\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_f, ITMPlainVoxelArray>::AlignSceneFrom(const ITMMainEngine_HIP&, Matrix4f&, itm_align_result*);\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(src)], check=True, capture_output=True)


# ---- CPU: the restated loop ---------------------------------------------------------------------------------------------------------------

# "Recovers the truth": the analytic pair differs from a continuous sdf by its 1 cm sampling, by the truncation of the stored value and
# by the band's edge, so the minimum of the discrete cost is not exactly the truth; a hundredth of a voxel (1e-4 m) is the resolution
# asked of it, and the same displacement at the volume's half diagonal (0.55 m) as an angle: 1.8e-4 rad.
RECOVERED = (1.8e-4, 1e-4)


@pytest.mark.parametrize("start", list(A.STARTS))
@pytest.mark.parametrize("voxel", ["s", "f"])
def test_restated_loop_recovers_the_truth_on_the_corner(voxel, start):
    M, res, (rot, trans) = reference(voxel, True, start)
    rot0, trans0 = A.pose_error(A.STARTS[start], A.TRUTH)
    print(f"restated loop, corner, {voxel}, {start}: {res}; e_ref = {rot:.3e} rad, {trans:.3e} m (start {rot0:.3e} rad, {trans0:.3e} m)")
    assert res["status"] == capi.ALIGN_CONVERGED and res["evaluations"] <= 30
    assert rot <= RECOVERED[0] and trans <= RECOVERED[1]
    assert res["conditioning"] >= 1e-2 and res["finalCost"] < res["initialCost"]


def test_restated_loop_reports_the_degenerate_scene():
    M, res, (rot, trans) = reference("s", False, "3deg_15mm")
    print(f"restated loop, wall + sphere: {res}; error {rot:.3e} rad, {trans:.3e} m")
    assert res["status"] == capi.ALIGN_DEGENERATE and 0 <= res["conditioning"] < 1e-3
    assert res["finalCost"] <= res["initialCost"]
    assert rot > 100 * RECOVERED[0], "the confident wrong answer the status is there for"


def test_restated_pieces():
    rng = np.random.default_rng(0)
    J = rng.normal(size=(50, 6))
    H = J.T @ J
    assert 0 < A.conditioning(H) <= 1 and abs(A.conditioning(np.diag([1, 2, 3, 4, 5, 6.0])) - 1 / 3) < 1e-12
    # the value does not change when the metre or the radian is rescaled
    u = np.array([1e3, 1e3, 1e3, 0.01, 0.01, 0.01])
    assert A.conditioning(H * u[:, None] * u[None, :]) == pytest.approx(A.conditioning(H), rel=1e-9)
    # a free coordinate axis: seen; scaling every parameter by its own diagonal entry turns its noise into a 1
    free = np.diag([3.0, 2.0, 4.0, 5.0, 6.0, 6e-4])
    assert A.conditioning(free) == pytest.approx(1e-4) and A.conditioning_per_parameter(free) == pytest.approx(1.0)
    H[:, 3:] = H[3:, :] = 0
    assert A.conditioning(H) == 0.0
    w = rng.normal(size=6) * 0.4
    E = A.se3_exp(w)
    assert np.allclose(E[:3, :3].T @ E[:3, :3], np.eye(3), atol=1e-14) and np.allclose(A.se3_exp(-w) @ E, np.eye(4), atol=1e-14)
    assert A.pose_error(A.se3_exp([0, 0, 0, 0, 0, 1e-3]) @ A.TRUTH, A.TRUTH)[0] == pytest.approx(1e-3, rel=1e-9)
    # the band samples of the dense array and of the same voxels as blocks are the same set
    dst, _ = A.analytic_pair(capi.VOXEL_S)
    table, blocks, _ = MD.dense_as_hash(dst, SIZE3, (0, 0, 0), capi.VOXEL_S)
    a = A.band_samples(dst, A.VOXEL_SIZE, A.MU, stride=2, dense=(SIZE3, (0, 0, 0)))
    b = A.band_samples(blocks, A.VOXEL_SIZE, A.MU, stride=2, entries=table)
    assert len(a) == len(b) > 5000 and {r.tobytes() for r in a} == {r.tobytes() for r in b}


# ---- GPU: scenes ------------------------------------------------------------------------------------------------------------------------

def analytic_scene(be, voxel, index, voxels, pool=0x1000):
    """a scene holding the 64^3 analytic voxels: the dense array, or the same voxels as blocks of a hash scene"""
    vt, prm = VOXEL_TYPES[voxel], capi.default_params(voxelSize=A.VOXEL_SIZE, mu=A.MU)
    if index == "dense":
        s = be.create_scene(vt, capi.INDEX_DENSE, prm, denseSize=SIZE3, denseOffset=(0, 0, 0))
        s.reco.ResetScene()
        if voxels is not None:
            s.upload(capi.BUF_VOXEL_BLOCKS, voxels)
        return s
    s = be.create_scene(vt, capi.INDEX_HASH, prm, localBlockNum=pool)
    s.reco.ResetScene()
    if voxels is not None:
        table, blocks, _ = MD.dense_as_hash(voxels, SIZE3, (0, 0, 0), vt)
        s.upload(capi.BUF_HASH_ENTRIES, table)
        s.upload(capi.BUF_VOXEL_BLOCKS, blocks)
    return s


class Pair:
    def __init__(self, be, voxel, index, corner=True):
        self.dst_voxels, self.src_voxels = A.analytic_pair(VOXEL_TYPES[voxel], corner)
        self.dst, self.src = analytic_scene(be, voxel, index, self.dst_voxels), analytic_scene(be, voxel, index, self.src_voxels)

    def close(self):
        self.dst.close(); self.src.close()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def device_samples(scene, cfg, slots=None, capacity=None):
    buf, count = scene.band_samples(cfg, slots, capacity)
    got = buf.numpy() if buf.shape[0] else np.zeros((0, 4), F)
    buf.close()
    return got, count


# ---- GPU: band samples --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("index", ["hash", "dense"])
@pytest.mark.parametrize("voxel", list(VOXEL_TYPES))
def test_band_samples_equal_the_restatement(hip, voxel, index):
    voxels = A.analytic_voxels(VOXEL_TYPES[voxel], A.TRUTH)
    voxels["w_depth"][::7] = 3                                    # two weights in the band: minWeight is a real test
    s = analytic_scene(hip, voxel, index, voxels)
    try:
        cases = [dict(), dict(stride=2), dict(stride=3, maxAbsSdf=0.5), dict(minWeight=2), dict(minWeight=4)]
        for kw in cases:
            cfg = default_cfg(hip, **kw)
            want = A.band_samples_of(s, cfg)
            got, count = device_samples(s, cfg)
            assert count == len(want) and np.array_equal(bits(got), bits(want)), (voxel, index, kw, count, len(want))
        assert len(A.band_samples_of(s, default_cfg(hip, minWeight=4))) == 0 and len(A.band_samples_of(s, default_cfg(hip))) > 40000
        # a capacity below the count: the full count, the first samples
        cfg = default_cfg(hip, stride=2)
        want = A.band_samples_of(s, cfg)
        got, count = device_samples(s, cfg, capacity=1001)
        assert count == len(want) > 1001 and np.array_equal(bits(got), bits(want[:1001]))
        got, count = device_samples(s, cfg, capacity=len(want) + 50)
        assert count == len(want) and np.array_equal(bits(got), bits(want))
        if index == "hash":
            entries = s.download(capi.BUF_HASH_ENTRIES)
            live = np.nonzero(entries["ptr"] >= 0)[0]
            for slots in (live[::3], np.concatenate([live[5:9], live[5:9], [0, len(entries) - 1]]), np.zeros(0, np.int64)):
                want = A.band_samples_of(s, cfg, slots=slots)
                got, count = device_samples(s, cfg, slots=np.asarray(slots, np.int32))
                assert count == len(want) and np.array_equal(bits(got), bits(want))
            with pytest.raises(capi.ItmError, match=r"\(-1\).*slot"):
                s.band_samples(cfg, np.array([3, len(entries)], np.int32))
        else:
            with pytest.raises(capi.ItmError, match=r"\(-1\).*slot list"):
                s.band_samples(cfg, np.array([0], np.int32))
        for bad in (dict(maxAbsSdf=0.0), dict(maxAbsSdf=1.5), dict(stride=0)):
            with pytest.raises(capi.ItmError, match=r"\(-1\)"):
                s.band_samples(default_cfg(hip, **bad))
    finally:
        s.close()


@pytest.mark.gpu
def test_band_samples_of_fused_and_half_swapped_scenes(hip):
    import swapped_cases
    scene, rs = swapped_cases.swapping_scene(hip, 1)
    try:
        entries = scene.download(capi.BUF_HASH_ENTRIES)
        assert np.count_nonzero(entries["ptr"] == -1) > 100 and np.count_nonzero(entries["ptr"] >= 0) > 100
        for kw in (dict(), dict(stride=2, minWeight=2)):
            cfg = scene.align_config(**kw)
            want = A.band_samples_of(scene, cfg)
            got, count = device_samples(scene, cfg)
            assert count == len(want) > 1000 and np.array_equal(bits(got), bits(want))
    finally:
        rs.close(); scene.close()
    ses = MC.fuse(hip, MC.DENSE)
    try:
        cfg = ses.scene.align_config()
        want = A.band_samples_of(ses.scene, cfg)
        got, count = device_samples(ses.scene, cfg)
        assert count == len(want) > 1000 and np.array_equal(bits(got), bits(want))
    finally:
        ses.close()


@pytest.mark.gpu
def test_band_samples_launch_recorded_frames_first(hip):
    sc = MC.SCENES["mesh_micro"]
    results = []
    for deferred in (True, False):
        ses = T.Session(hip, sc, deferred_fusion=deferred)
        ses.frame(0, fused="four" if deferred else False)
        view = ses.view(1)
        ses.scene.reco.AllocateSceneFromDepth(view, ses.rs)          # deferred: recorded, not launched
        ses.scene.reco.IntegrateIntoScene(view, ses.rs)
        ses.scene.vis.CreateExpectedDepths(view.M_d, view.intr_d, ses.rs)
        results.append(device_samples(ses.scene, ses.scene.align_config(minWeight=2)))
        ses.close()
    (a, na), (b, nb) = results
    assert na == nb > 1000 and np.array_equal(bits(a), bits(b)), "voxels of weight 2 exist once the second frame is fused"


# ---- GPU: evaluation ------------------------------------------------------------------------------------------------------------------------

def bound_check(ev, sums, what):
    """the valid count exact, every sum within ulp32(sum64) + n 2^-52 sum|term|; returns the worst ratio to the bound"""
    assert ev.noValid == sums.n, (what, ev.noValid, sums.n)
    got = A.pack(ev.f, ev.nabla[:], ev.hessian[:])
    H = np.asarray(ev.hessian[:], F).reshape(6, 6)
    assert np.array_equal(H, H.T), what
    worst = 0.0
    for k in range(A.KV):
        bound = ulp32(sums.sum64[k]) + sums.n * EPS52 * sums.A[k]
        err = abs(got[k] - sums.sum64[k])
        assert err <= bound, (what, k, got[k], sums.sum64[k], err, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    return worst


def same_eval(a, b):
    return bytes(a) == bytes(b)


PERTURBED = A.rigid(A.rotation((2, -1, 1), np.radians(2.5)), (0.018, 0.012, -0.016)) @ A.TRUTH      # a good share out of the band and in the Huber tail


@pytest.mark.gpu
@pytest.mark.parametrize("voxel,index", [("s", "hash"), ("s", "dense"), ("f", "hash"), ("f", "dense"), ("s_rgb", "hash"), ("f_rgb", "dense")])
def test_evaluation_on_the_corner_scene(hip, voxel, index):
    pair = Pair(hip, voxel, index)
    aligner = capi.SceneAligner(hip)
    try:
        cfg = default_cfg(hip)
        reader = Q.reader_of(pair.dst)
        samples = A.band_samples_of(pair.src, cfg)
        assert len(samples) > 70001
        worst = {}
        for name, M in (("truth", A.TRUTH), ("perturbed", PERTURBED)):
            for n in (0, 1, 63, 64, 65, 257, 20011, 70001):
                sub = samples[:: max(1, len(samples) // max(n, 1))][:n] if n < 20011 else samples[:n]
                assert len(sub) == n
                aligner.set_samples(sub)
                ev = aligner.evaluate(pair.dst, M, cfg)
                if n == 0:
                    assert bytes(ev) == bytes(capi.AlignEval()), "n == 0: zeros"
                    continue
                t, valid, huber = A.sample_terms(reader, sub, M, A.VOXEL_SIZE, A.MU, cfg.huberDelta)
                worst[(name, n)] = bound_check(ev, A.Sums(t, valid), f"{voxel} {index} {name} n={n}")
                assert same_eval(ev, aligner.evaluate(pair.dst, M, cfg)), "two evaluations give identical bits"
                if name == "perturbed" and n >= 20011:
                    assert 0.05 * n < valid.sum() < 0.95 * n and huber.sum() > 0.05 * n, (valid.sum(), huber.sum(), n)      # both shares are there
                if name == "truth" and n >= 20011:
                    assert valid.sum() > 0.7 * n and huber.sum() < 0.01 * n
        print(f"evaluation, corner scene, {voxel} {index}: worst ratio to the bound {max(worst.values()):.3f} over {len(worst)} evaluations")
        # an invalid position contributes nothing: samples far outside, not finite, and at the limit of the position rule
        sub = samples[:257].copy()
        aligner.set_samples(sub)
        base = aligner.evaluate(pair.dst, A.TRUTH, cfg)
        junk = np.array([[np.nan, 0, 0, 0], [0, np.inf, 0, 0], [0, 0, 2621.36, 0], [-3000, 0, 0, 0], [1e30, 1e30, 1e30, 0], [0.3, 0.3, 0.3, np.nan]], F)
        mixed = np.concatenate([sub[:100], junk[:5], sub[100:]])
        aligner.set_samples(mixed)
        assert aligner.evaluate(pair.dst, A.TRUTH, cfg).noValid == base.noValid
        t, valid, _ = A.sample_terms(reader, mixed, A.TRUTH, A.VOXEL_SIZE, A.MU, cfg.huberDelta)
        assert not valid[100:105].any()
        bound_check(aligner.evaluate(pair.dst, A.TRUTH, cfg), A.Sums(t, valid), "invalid positions")
        # the sequence numbers of the handle's records roll over: same bits on either side
        aligner.set_samples(sub)
        hip.debug_counter(capi.COUNTER_ALIGN_SEQ, aligner, 0xfffffffc)
        for _ in range(6):
            assert same_eval(aligner.evaluate(pair.dst, A.TRUTH, cfg), base)
        assert hip.debug_counter(capi.COUNTER_ALIGN_SEQ, aligner) < 16
    finally:
        aligner.close()
        pair.close()


class Fused:
    """a fused Session scene under one access path, closed by the test"""

    def __init__(self, be, path):
        self.be, self.path = be, path
        if path == "dense":
            self.ses = MC.fuse(be, MC.DENSE)
        else:
            with TQ.environment(TQ.FORMS.get(path, {})):
                self.ses = MC.fuse(be, MC.SCENES["mesh_micro"])
        self.scene = self.ses.scene

    def __enter__(self):
        if self.path == "directory_off":
            self.be.check(self.be.fn["debug_set"](TQ.DEBUG_NO_DIRECTORY, 1), "debug_set")
        return self

    def __exit__(self, *exc):
        if self.path == "directory_off":
            self.be.check(self.be.fn["debug_set"](TQ.DEBUG_NO_DIRECTORY, 0), "debug_set")
        self.ses.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["default", "paged", "paged_few", "mirror_off", "directory_off", "dense"])
def test_evaluation_under_every_access_path(hip, path):
    with Fused(hip, path) as b:
        scene = b.scene
        info = scene.accel_info() if scene.is_hash else None
        if path.startswith("paged"):
            assert info["mirror_pages"] == (5 if path == "paged_few" else info["mirror_pages"]) > 0, info
        elif path == "mirror_off":
            assert info["mirror_bytes"] == 0 and info["directory_bytes"] > 0, info
        cfg = scene.align_config()
        vs, mu = float(scene.params.voxelSize), float(scene.params.mu)
        reader = Q.reader_of(scene)
        samples = A.band_samples_of(scene, cfg)
        assert len(samples) > 5000
        aligner = capi.SceneAligner(hip)
        try:
            centre = samples[:, :3].astype(np.float64).mean(0)
            shift = A.rigid(np.eye(3), centre)
            M = shift @ A.rigid(A.rotation((1, 1, 0), np.radians(1.0)), (0.004, -0.003, 0.005)) @ np.linalg.inv(shift)
            worst = 0.0
            for n in (65, min(20011, len(samples))):
                sub = samples[:: len(samples) // n][:n]
                aligner.set_samples(sub)
                ev = aligner.evaluate(scene, M, cfg)
                t, valid, huber = A.sample_terms(reader, sub, M, vs, mu, cfg.huberDelta)
                worst = max(worst, bound_check(ev, A.Sums(t, valid), f"{path} n={n}"))
                assert same_eval(ev, aligner.evaluate(scene, M, cfg))
            assert 0.05 * n < valid.sum() < n, (path, valid.sum())
            print(f"evaluation, fused scene, {path}: worst ratio to the bound {worst:.3f}, {valid.sum()} of {n} valid, {huber.sum()} in the Huber tail")
        finally:
            aligner.close()


# ---- GPU: alignment -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("index", ["hash", "dense"])
@pytest.mark.parametrize("voxel", ["s", "f"])
def test_alignment_recovers_the_corner_scene(hip, voxel, index):
    """Measured on the MI355X (profiles/scene_align_notes.md has the table): the GPU errors equal e_ref to four digits."""
    pair = Pair(hip, voxel, index)
    try:
        for start, init in A.STARTS.items():
            _, ref, (rot_ref, trans_ref) = reference(voxel, True, start)
            M, res = pair.dst.align_from(pair.src, init, default_cfg(hip, minStep=MIN_STEP))
            rot, trans = A.pose_error(M, A.TRUTH)
            print(f"alignment, corner, {voxel} {index} {start}: {res.as_dict()}; error {rot:.4e} rad {trans:.4e} m; e_ref {rot_ref:.4e} rad {trans_ref:.4e} m "
                  f"({ref['evaluations']} evaluations)")
            assert res.status == capi.ALIGN_CONVERGED, capi.ALIGN_STATUS_NAMES[res.status]
            assert res.finalCost <= res.initialCost and res.conditioning >= 1e-2 and res.noValid > 50000
            assert rot <= rot_ref + 4 * MIN_STEP and trans <= trans_ref + 4 * MIN_STEP
    finally:
        pair.close()


@pytest.mark.gpu
@pytest.mark.parametrize("index", ["hash", "dense"])
def test_alignment_reports_the_degenerate_scene(hip, index):
    pair = Pair(hip, "s", index, corner=False)
    try:
        cfg = default_cfg(hip)
        M, res = pair.dst.align_from(pair.src, A.STARTS["3deg_15mm"], cfg)
        print(f"alignment, wall + sphere, {index}: {res.as_dict()}; error {A.pose_error(M, A.TRUTH)}")
        assert res.status == capi.ALIGN_DEGENERATE and 0 <= res.conditioning < cfg.minConditioning
        assert res.finalCost <= res.initialCost
    finally:
        pair.close()


@pytest.mark.gpu
def test_alignment_reports_a_fused_sphere_and_wall_scene(hip):
    """a fused Session scene (the sphere in front of a wall of every fused test) aligned to its twin"""
    a, b = MC.fuse(hip, MC.SCENES["mesh_micro"]), MC.fuse(hip, MC.SCENES["mesh_micro"])
    try:
        cfg = a.scene.align_config()
        samples = A.band_samples_of(b.scene, cfg)
        centre = samples[:, :3].astype(np.float64).mean(0)
        shift = A.rigid(np.eye(3), centre)
        init = shift @ A.rigid(A.rotation((0, 0, 1), np.radians(2.0)), (0.004, -0.003, 0.003)) @ np.linalg.inv(shift)
        M, res = a.scene.align_from(b.scene, init, cfg)
        print(f"alignment, fused sphere and wall: {res.as_dict()}; left over {A.pose_error(M, np.eye(4))}")
        assert res.status == capi.ALIGN_DEGENERATE and 0 <= res.conditioning < cfg.minConditioning
        assert res.finalCost <= res.initialCost and res.noValid > 1000
    finally:
        a.close(); b.close()


@pytest.mark.gpu
def test_too_few_samples_return_the_input_pose(hip):
    pair = Pair(hip, "s", "hash")
    aligner = capi.SceneAligner(hip)
    try:
        cfg = default_cfg(hip)
        samples = A.band_samples_of(pair.src, cfg)
        init = A.STARTS["3deg_15mm"].astype(F)
        aligner.set_samples(samples[::1000][:60])                          # fewer than minValid samples at all
        M, res = aligner.align(pair.dst, init, cfg)
        assert res.status == capi.ALIGN_TOO_FEW_SAMPLES and res.evaluations == 1 and res.noValid < cfg.minValid
        assert np.array_equal(bits(M), bits(init))
        far = A.rigid(np.eye(3), (5.0, 0, 0)) @ A.TRUTH                    # many samples, none valid where they land
        aligner.set_samples(samples)
        M, res = aligner.align(pair.dst, far, cfg)
        assert res.status == capi.ALIGN_TOO_FEW_SAMPLES and res.noValid == 0 and np.array_equal(bits(M), bits(far.astype(F)))
        M, res = aligner.align(pair.dst, init, cfg.replace(maxEvaluations=2))
        assert res.status == capi.ALIGN_MAX_EVALUATIONS and res.evaluations == 2 and res.finalCost < res.initialCost
        aligner.set_samples(np.zeros((0, 4), F))
        with pytest.raises(capi.ItmError, match=r"\(-1\).*no samples"):
            aligner.align(pair.dst, init, cfg)
    finally:
        aligner.close()
        pair.close()


def words(a):
    return [int(v) for v in bits(a).reshape(-1)]


@pytest.mark.gpu
def test_adapters_give_the_pose_of_the_aligner(hip, tmp_path):
    pair = Pair(hip, "s", "hash")
    aligner = capi.SceneAligner(hip)
    try:
        cfg = default_cfg(hip)
        init = A.STARTS["3deg_15mm"]
        buf, count = pair.src.band_samples(cfg)
        aligner.set_samples(buf, count)
        M, res = aligner.align(pair.dst, init, cfg)
        ev = aligner.evaluate(pair.dst, M, cfg)
        M2, res2 = pair.dst.align_from(pair.src, init, cfg)
        assert np.array_equal(bits(M), bits(M2)) and res.as_dict() == res2.as_dict()
        files = []
        for name, voxels in (("dst", pair.dst_voxels), ("src", pair.src_voxels)):
            table, blocks, _ = MD.dense_as_hash(voxels, SIZE3, (0, 0, 0), capi.VOXEL_S)
            for kind, arr in (("table", table), ("blocks", blocks)):
                path = tmp_path / f"{name}_{kind}.bin"
                arr.tofile(path)
                files.append(str(path))
        flat = np.ascontiguousarray(init.astype(F).T).reshape(16)
        out = subprocess.run([build_demo()] + files + ["%.9g" % v for v in flat], check=True, capture_output=True, text=True).stdout
        got = json.loads(out.strip().splitlines()[-1])
        assert got["samples"] == count
        assert got["pose_bits"] == words(np.ascontiguousarray(M.T).reshape(16))
        assert (got["status"], got["evaluations"], got["noValid"]) == (res.status, res.evaluations, res.noValid)
        assert got["finalCost"] == res.finalCost and got["conditioning"] == res.conditioning and got["initialCost"] == res.initialCost
        assert got["eval_noValid"] == ev.noValid and got["eval_f_bits"] == words([ev.f]) and got["eval_nabla_bits"] == words(ev.nabla[:])
    finally:
        aligner.close()
        pair.close()


def band_differences(d, t, step):
    """d, t: the voxels of dst and of the twin at the same positions -> (voxels of dst's band that the twin has observed, how many of them
    differ by more than `step`, their mean |difference|)"""
    band = (d["w_depth"] > 0) & (np.abs(A.to_float(d["sdf"])) < 1) & (t["w_depth"] > 0)
    diff = np.abs(A.to_float(t["sdf"]).astype(np.float64) - A.to_float(d["sdf"]).astype(np.float64))[band]
    return int(band.sum()), int((diff > step).sum()), float(diff.mean())


@pytest.mark.gpu
@pytest.mark.parametrize("index", ["hash", "dense"])
def test_fusion_under_the_refined_pose_is_closer(hip, index):
    pair = Pair(hip, "s", index)
    try:
        init = A.STARTS["3deg_15mm"]
        M, res = pair.dst.align_from(pair.src, init)
        assert res.status == capi.ALIGN_CONVERGED
        step = 1.0 / 32767.0
        counts = {}
        for name, pose in (("start", init), ("refined", M)):
            twin = analytic_scene(hip, "s", index, None)
            try:
                twin.resample_from(pair.src, pose)
                if index == "dense":
                    t = twin.download(capi.BUF_VOXEL_BLOCKS)
                    d = pair.dst_voxels
                else:
                    # the twin's voxels at dst's positions, through the restatement's reader
                    reader = Q.reader_of(twin)
                    z, y, x = np.meshgrid(np.arange(A.N), np.arange(A.N), np.arange(A.N), indexing="ij")
                    lin, found = reader.locate(x.reshape(-1), y.reshape(-1), z.reshape(-1))
                    vox = twin.download(capi.BUF_VOXEL_BLOCKS)
                    t = vox[lin].copy()
                    t["w_depth"][~found] = 0
                    d = pair.dst_voxels
                counts[name] = band_differences(d, t, step)
            finally:
                twin.close()
        print(f"fusion, {index}: (band voxels observed, beyond one short sdf step, mean |difference|) {counts}")
        assert counts["start"][0] > 20000 and counts["refined"][0] > 20000
        assert counts["refined"][1] / counts["refined"][0] < counts["start"][1] / counts["start"][0]
        # the start is 15 mm off, 0.375 of the band's half width; what is left under a refined pose is the resampling's own interpolation
        assert counts["refined"][2] < 0.5 * counts["start"][2]
    finally:
        pair.close()
