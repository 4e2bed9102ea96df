"""The view builder against its restatements (tests/viewbuilder_terms.py) on the cases of tests/viewbuilder_cases.py: ragged image
sizes around the filter's 16 x 16 tile and 2-pixel halo, holes, exact zeros, isolated pixels, kilometre depths, a periodic image.

On the CPU the float32 restatement (`seq32`) is pinned to the oracle, and through it to the reference, bit for bit -- filter,
normals / uncertainty and the whole UpdateView sequence on every case -- so that what judges the kernels is itself judged first.

On the GPU:
  * seam invariance: on an image of period 5 x 7 the filter gives the same bits 5 pixels to the right and 7 pixels down, wherever
    both pixels are interior -- the same 25 values through the same operations, at every position of the window in a tile;
  * structure, exact: holes, zero border, -1 outputs, isolated centres; normals bit for bit on images prefilled with a sentinel
    (the never-written border and the kept xyz of rejected pixels count); inf / NaN classes of the uncertainty of a zero centre;
  * filter accuracy: |hip - ref64| and |oracle - ref64| within the proof bound E of viewbuilder_terms (C_A = 20 roundings in an
    exponent), and a tripwire |hip - oracle| <= 2 D ulp, D = what exchanging libm's expf for numpy's float32 exp does to seq32;
  * uncertainty accuracy: |hip - ref64| and |oracle - ref64| within the first-order bound of viewbuilder_terms, for both kinds of
    intrinsics (focal lengths as the reference hands them over: normal.z stays next to 1; their reciprocals: real tilts);
  * itm_update_view against the library's own single steps, bit for bit, both calibrations, all four (filter, noise) combinations;
  * the conversions on every int16 value.

Constants and measurements (the tests print them):
  C_A    = 20   counted in viewbuilder_terms' docstring
  K_EXP  = 1    the oracle (glibc expf) passes the filter bound with 0; plus one for the device library
  K_ACOS = 2    the oracle (glibc acosf) passes the uncertainty bound with 1, not with 0; plus one
  D      = 4 ulp (x86-64 glibc expf against numpy's float32 exp, one pass, worst over the cases), so the tripwire is 8 ulp;
           MI355X: |hip - oracle| is at most 4 ulp, and the two differ at all on 5.8 % of the 77 403 filtered pixels
  worst |got - ref64| / E, filter:       CPU oracle 0.161 (0.161 with K_EXP = 0 too: the bound is carried by its rounding terms);
                                         MI355X 0.161, both on sphere_wall_163x125
  worst |got - ref64| / E, uncertainty:  CPU oracle 0.779 (0.785 with K_ACOS = 1); MI355X 0.779, sphere_wall_163x125 with reciprocal
                                         focal lengths; no pixel of any case is excluded (pi/2 - theta < 64 ulp)
"""
import ctypes as C

import numpy as np
import pytest

import viewbuilder_cases as VC
import viewbuilder_terms as VT
from infinitam_amd.capi import DevBuffer

F = np.float32
K_EXP = 1
K_ACOS = 2
SENTINEL = F(7.25)           # neither 0 nor -1: what a kernel must leave alone stays recognisable
DISPARITY = (0, 1135.09, 0.0819141)
ALL_CASES = pytest.mark.parametrize("name", VC.NAMES)


# ---- one call each, on any backend --------------------------------------------------------------------------------------------
def intr_arg(intr):
    return (C.c_float * 4)(*intr)


def run_filter(be, img):
    h, w = img.shape
    src = be.to_backend(np.asarray(img, F))
    dst = be.to_backend(np.full((h, w), SENTINEL, F))
    be.check(be.fn["filter_depth"](src.ptr, dst.ptr, w, h, None), "filter_depth")
    return dst.numpy()


def run_normals(be, img, intr):
    h, w = img.shape
    src = be.to_backend(np.asarray(img, F))
    nrm = be.to_backend(np.full((h, w, 4), SENTINEL, F))
    sig = be.to_backend(np.full((h, w), SENTINEL, F))
    be.check(be.fn["compute_normal_and_weights"](src.ptr, nrm.ptr, sig.ptr, w, h, intr_arg(intr), None), "normals")
    return nrm.numpy(), sig.numpy()


def run_update(be, raw, calib, intr, bilateral, noise, fill=SENTINEL):
    """-> (depth, scratch, normals, sigmaZ), every output prefilled with the sentinel"""
    h, w = raw.shape
    src = be.to_backend(np.asarray(raw, np.int16))
    depth, scratch, sig = (be.to_backend(np.full((h, w), fill, F)) for _ in range(3))
    nrm = be.to_backend(np.full((h, w, 4), fill, F))
    be.check(be.fn["update_view"](src.ptr, w, h, calib[0], calib[1], calib[2], intr_arg(intr), int(bilateral), int(noise), depth.ptr,
                                  scratch.ptr, nrm.ptr, sig.ptr, None), "update_view")
    return depth.numpy(), scratch.numpy(), nrm.numpy(), sig.numpy()


def sentinels(h, w):
    return np.full((h, w, 4), SENTINEL, F), np.full((h, w), SENTINEL, F)


def assert_same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    bad = np.argwhere(VT.bits(a) != VT.bits(b))
    assert bad.size == 0, f"{what}: {len(bad)} value(s) differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]!r} != {b[tuple(bad[0])]!r}"


# ---- shared, computed once ----------------------------------------------------------------------------------------------------
_memo = {}


def memo(key, make):
    if key not in _memo:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _memo[key] = v
    return _memo[key]


def oracle_filter(oracle, name):
    return memo(("filter", name), lambda: run_filter(oracle, VC.case(name).depth))


def oracle_normals(oracle, name, kind):
    c = VC.case(name)
    return memo(("normals", name, kind), lambda: run_normals(oracle, c.depth, getattr(c, kind)))


def seq32_filter(name):
    return memo(("seq32", name), lambda: VT.filter_seq32(VC.case(name).depth))


def ref64_filter(name):
    return memo(("ref64", name), lambda: VT.filter_ref64(VC.case(name).depth))


def has_interior(c):
    return c.w > 2 * VT.RADIUS and c.h > 2 * VT.RADIUS


def tripwire_d():
    """D: the worst ulp difference of seq32's output between libm's expf and numpy's float32 exp, over the cases"""
    def make():
        worst = 0
        for name in VC.NAMES:
            other = VT.filter_seq32(VC.case(name).depth, VT.exp_numpy)
            worst = max(worst, int(VT.ulp_distance(seq32_filter(name), other).max()))
        return worst
    return memo("D", make)


def filter_ratio(got, name, k_exp):
    """worst |got - ref64| / E over the filtered pixels of a case (0 where there is none), and the pixel count"""
    c = VC.case(name)
    if not has_interior(c):
        return 0.0, 0
    r = ref64_filter(name)
    if not r.live.any():
        return 0.0, 0
    err = np.abs(got[2:-2, 2:-2].astype(np.float64) - r.out)[r.live]
    E = r.bound(k_exp)[r.live]
    assert (E > 0).all() or (err[E == 0] == 0).all()
    return float(np.max(np.where(E > 0, err / np.where(E > 0, E, 1.0), 0.0))), int(r.live.sum())


def sigma_ratio(sig, depth, normals, k_acos):
    """worst |sig - ref64| / E over the valid, not excluded pixels; the count of valid and of excluded pixels"""
    r = VT.sigma_ref64(depth, normals)
    m = r.valid & ~r.excluded
    if not m.any():
        return 0.0, int(r.valid.sum()), int(r.excluded.sum())
    err = np.abs(sig.astype(np.float64) - r.out)[m]
    return float((err / r.bound(k_acos)[m]).max()), int(r.valid.sum()), int(r.excluded.sum())


# ---- CPU: the restatement is the oracle, the cases are what they claim -----------------------------------------------------------
def test_the_160x120_case_is_the_image_of_test_viewbuilder():
    import test_viewbuilder
    assert_same_bits(VC.case("sphere_wall_160x120").depth, test_viewbuilder.noisy_depth(), "sphere_wall_160x120")


def test_the_cases_hold_what_they_are_for():
    sizes = {(VC.case(n).w, VC.case(n).h) for n in VC.NAMES}
    assert sizes == {(1, 1), (4, 7), (7, 4), (5, 5), (16, 16), (17, 17), (18, 21), (19, 21), (20, 20), (33, 47), (35, 19), (83, 61),
                     (160, 120), (163, 125)}
    for w, h in VC.MANDATORY_SIZES:
        assert f"sphere_wall_{w}x{h}" in VC.NAMES
    for name in VC.NAMES:
        d = VC.case(name).depth
        if name.startswith("isolated"):
            valid = np.argwhere(d >= 0)
            assert len(valid) > 0
            for y, x in valid:
                win = d[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3]
                assert (win >= 0).sum() == 1
        if name.startswith("planted_zeros") or name.startswith("periodic"):
            zero = (d == 0) & ~np.signbit(d)
            assert zero.any()
            inner = zero[1:-1, 1:-1]
            centres = inner & (d[1:-1, 2:] > 0) & (d[1:-1, :-2] > 0) & (d[2:, 1:-1] > 0) & (d[:-2, 1:-1] > 0)
            beside = (d[1:-1, 1:-1] > 0) & (zero[1:-1, 2:] | zero[1:-1, :-2] | zero[2:, 1:-1] | zero[:-2, 1:-1])
            assert centres[1:-1, 1:-1].any() and (beside[1:-1, 1:-1].any() or min(d.shape) <= 5), name
        if name.startswith("kilometres"):
            assert (d > 1000).sum() > d.size // 20 and ((d > 0) & (d < 10)).any()
        if name.startswith("periodic"):
            assert_same_bits(d[:-VC.PERIOD_Y, :-VC.PERIOD_X], d[VC.PERIOD_Y:, VC.PERIOD_X:], name)
            v = d[d > 0]
            assert v.min() >= 0.8 and v.max() <= 2.5 and (d == -1).any()


@ALL_CASES
def test_seq32_is_the_oracles_filter(oracle, ref, name):
    c = VC.case(name)
    a = oracle_filter(oracle, name)
    if ref.backend is not None:
        assert_same_bits(a, run_filter(ref.backend, c.depth), "oracle, reference")
    ref.check("filter", a)
    assert_same_bits(seq32_filter(name), a, "seq32, oracle")


@ALL_CASES
def test_seq32_is_the_oracles_normals_and_uncertainty(oracle, ref, name):
    c = VC.case(name)
    for kind in ("intr", "intr_inverse"):
        na, sa = oracle_normals(oracle, name, kind)
        if ref.backend is not None:
            nb, sb = run_normals(ref.backend, c.depth, getattr(c, kind))
            assert_same_bits(na, nb, "normals: oracle, reference")
            assert_same_bits(sa, sb, "sigmaZ: oracle, reference")
        ref.check(kind, (na, sa))
        ns, ss = VT.normals_seq32(c.depth, getattr(c, kind), *sentinels(c.h, c.w))
        assert_same_bits(ns, na, f"normals ({kind}): seq32, oracle")
        assert_same_bits(ss, sa, f"sigmaZ ({kind}): seq32, oracle")


@ALL_CASES
def test_seq32_is_the_oracles_update_view(oracle, ref, name):
    """conversion, five passes, normals: the four (filter, noise) combinations of the case's raw frame"""
    c = VC.case(name)
    nrm0, sig0 = sentinels(c.h, c.w)
    conv, _, _, _ = VT.update_view_seq32(c.raw, *c.calib, c.intr, False, False, nrm0, sig0)
    filt, _, _, passes = VT.update_view_seq32(c.raw, *c.calib, c.intr, True, False, nrm0, sig0)
    want = {(False, False): (conv, sig0, nrm0, sig0),
            (True, False): (filt, passes[4], nrm0, sig0),
            (False, True): (conv, sig0) + VT.normals_seq32(conv, c.intr, nrm0, sig0),
            (True, True): (filt, passes[4]) + VT.normals_seq32(filt, c.intr, nrm0, sig0)}
    certified = {}
    for (bilateral, noise), w in want.items():
        a = run_update(oracle, c.raw, c.calib, c.intr, bilateral, noise)
        if ref.backend is not None:
            # the reference builds a view of its own, whose images start at 0, and keeps its five passes there: zero-filled outputs
            # on both sides, and the scratch image is this library's
            a0, b = (run_update(be, c.raw, c.calib, c.intr, bilateral, noise, fill=F(0)) for be in (oracle, ref.backend))
            for i, what in ((0, "depth"), (2, "normals"), (3, "sigmaZ")):
                assert_same_bits(a0[i], b[i], f"{what} ({bilateral}, {noise}): oracle, reference")
        certified[f"filter{int(bilateral)}_noise{int(noise)}"] = (a[0], a[2], a[3])
        for i, what in enumerate(("depth", "scratch", "normals", "sigmaZ")):
            assert_same_bits(w[i], a[i], f"{what} ({bilateral}, {noise}): seq32, oracle")
    ref.check("update_view", certified)


def test_the_oracle_is_seam_invariant_on_the_periodic_image(oracle):
    """the premise of the GPU test: equal windows give equal bits"""
    out = oracle_filter(oracle, "periodic_83x61")
    assert_same_bits(out[2:-2, 2:-2 - VC.PERIOD_X], out[2:-2, 2 + VC.PERIOD_X:-2], "5 to the right")
    assert_same_bits(out[2:-2 - VC.PERIOD_Y, 2:-2], out[2 + VC.PERIOD_Y:-2, 2:-2], "7 down")
    # and not trivially so: most valid pixels are a blend of their window, not their own centre, so a misplaced tap would show
    d = VC.case("periodic_83x61").depth[2:-2, 2:-2]
    assert len(np.unique(out[2:-2, 2:-2])) > 20 and (out[2:-2, 2:-2] != d)[d > 0].mean() > 0.9


def test_the_oracle_meets_the_filter_bound_without_an_exp_allowance(oracle):
    """K_EXP is the smallest integer with which the oracle passes (0), plus one"""
    worst = {k: 0.0 for k in (K_EXP - 1, K_EXP)}
    pixels = 0
    for name in VC.NAMES:
        for k in worst:
            ratio, n = filter_ratio(oracle_filter(oracle, name), name, k)
            worst[k] = max(worst[k], ratio)
        pixels += n
    print(f"filter, oracle on the CPU: worst |oracle - ref64| / E = {worst[K_EXP]:.3f} with K_EXP = {K_EXP}, {worst[K_EXP - 1]:.3f} with "
          f"{K_EXP - 1}, over {pixels} pixels; D = {tripwire_d()} ulp")
    assert K_EXP - 1 == 0 and worst[K_EXP - 1] <= 1.0 and pixels > 40000
    assert tripwire_d() >= 1          # the two exp implementations do differ: the tripwire is not an equality in disguise


def test_the_oracle_meets_the_uncertainty_bound_with_one_ulp_of_acos(oracle):
    """K_ACOS is the smallest integer with which the oracle passes (1), plus one; and the excluded pixels are few"""
    worst = {k: 0.0 for k in (K_ACOS - 1, K_ACOS)}
    pixels = 0
    for name in VC.NAMES:
        c = VC.case(name)
        for kind in ("intr", "intr_inverse"):
            nrm, sig = oracle_normals(oracle, name, kind)
            for k in worst:
                ratio, valid, excluded = sigma_ratio(sig, c.depth, nrm, k)
                worst[k] = max(worst[k], ratio)
            assert excluded <= 0.001 * valid, (name, kind, excluded, valid)
            pixels += valid
    print(f"sigmaZ, oracle on the CPU: worst |oracle - ref64| / E = {worst[K_ACOS]:.3f} with K_ACOS = {K_ACOS}, {worst[K_ACOS - 1]:.3f} "
          f"with {K_ACOS - 1}, over {pixels} pixels")
    assert worst[K_ACOS - 1] <= 1.0 and pixels > 80000


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_filter_is_seam_invariant_on_the_periodic_image(hip):
    out = run_filter(hip, VC.case("periodic_83x61").depth)
    assert_same_bits(out[2:-2, 2:-2 - VC.PERIOD_X], out[2:-2, 2 + VC.PERIOD_X:-2], "5 to the right")
    assert_same_bits(out[2:-2 - VC.PERIOD_Y, 2:-2], out[2 + VC.PERIOD_Y:-2, 2:-2], "7 down")


@pytest.mark.gpu
@ALL_CASES
def test_filter_structure_is_the_oracles(hip, oracle, name):
    c = VC.case(name)
    a, b = run_filter(hip, c.depth), oracle_filter(oracle, name)
    assert np.array_equal(a <= 0, b <= 0)
    for v in (F(0), F(-1)):          # the zero border (+0.0, every pixel of an image without interior) and the invalid centres
        at = VT.bits(b) == VT.bits(v)
        assert np.array_equal(VT.bits(a) == VT.bits(v), at)
    border = np.ones((c.h, c.w), bool)
    border[2:-2, 2:-2] = False
    assert (VT.bits(a)[border] == 0).all()
    if name.startswith("isolated"):
        inner = np.zeros((c.h, c.w), bool)
        inner[2:-2, 2:-2] = c.depth[2:-2, 2:-2] >= 0
        assert inner.any()
        assert_same_bits(a[inner], c.depth[inner], "a lone centre is its own mean")


@pytest.mark.gpu
@ALL_CASES
def test_normals_are_the_oracles_and_the_uncertainty_is_of_its_class(hip, oracle, name):
    c = VC.case(name)
    for kind in ("intr", "intr_inverse"):
        na, sa = run_normals(hip, c.depth, getattr(c, kind))
        nb, sb = oracle_normals(oracle, name, kind)
        assert_same_bits(na, nb, f"normals ({kind})")          # border and rejected xyz: the sentinel on both sides
        for v in (SENTINEL, F(-1)):
            assert np.array_equal(VT.bits(sa) == VT.bits(v), VT.bits(sb) == VT.bits(v)), (kind, v)
        assert np.array_equal(np.isnan(sa), np.isnan(sb)), kind
        assert np.array_equal(np.isposinf(sa), np.isposinf(sb)) and not np.isneginf(sa).any(), kind


@pytest.mark.gpu
@ALL_CASES
def test_filter_is_within_the_proof_bound_and_the_tripwire(hip, oracle, name):
    c = VC.case(name)
    a, b = run_filter(hip, c.depth), oracle_filter(oracle, name)
    ra, n = filter_ratio(a, name, K_EXP)
    rb, _ = filter_ratio(b, name, K_EXP)
    d = tripwire_d()
    m = b > 0
    assert np.array_equal(a > 0, m)
    ulps = VT.ulp_distance(a[m], b[m]) if m.any() else np.zeros(1, np.int64)
    print(f"{name}: |hip - ref64| / E = {ra:.3f}, |oracle - ref64| / E = {rb:.3f} over {n} pixels (K_EXP = {K_EXP}); "
          f"|hip - oracle| <= {int(ulps.max())} ulp, D = {d}; hip != oracle at {np.count_nonzero(ulps) / max(ulps.size, 1):.4f} of the pixels")
    assert ra <= 1.0 and rb <= 1.0
    assert ulps.max() <= 2 * d


@pytest.mark.gpu
@ALL_CASES
def test_uncertainty_is_within_the_first_order_bound(hip, oracle, name):
    c = VC.case(name)
    for kind in ("intr", "intr_inverse"):
        na, sa = run_normals(hip, c.depth, getattr(c, kind))
        nb, sb = oracle_normals(oracle, name, kind)
        assert_same_bits(na, nb, f"normals ({kind})")
        ra, valid, excluded = sigma_ratio(sa, c.depth, nb, K_ACOS)
        rb, _, _ = sigma_ratio(sb, c.depth, nb, K_ACOS)
        print(f"{name} ({kind}): |hip - ref64| / E = {ra:.3f}, |oracle - ref64| / E = {rb:.3f} over {valid} pixels, {excluded} excluded "
              f"(K_ACOS = {K_ACOS})")
        assert excluded <= 0.001 * valid
        assert ra <= 1.0 and rb <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("size", VC.MANDATORY_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bilateral,noise", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("calib", [VC.AFFINE_MM, DISPARITY], ids=["affine", "disparity"])
def test_update_view_is_its_own_single_steps(hip, calib, bilateral, noise, size):
    """itm_update_view == conversion, five itm_filter_depth calls, itm_compute_normal_and_weights: depth, scratch, normals and -- compared
    nowhere else -- sigmaZ, bit for bit; what a combination does not write keeps the sentinel"""
    w, h = size
    c = VC.case(f"sphere_wall_{w}x{h}")
    raw = VC.raw_for(c.depth, calib, c.intr[0])
    depth, scratch, nrm, sig = run_update(hip, raw, calib, c.intr, bilateral, noise)
    src = hip.to_backend(raw)
    conv = DevBuffer(hip, w * h * 4, F, (h, w))
    if calib[0] == 0:
        hip.check(hip.fn["convert_disparity"](src.ptr, conv.ptr, w, h, calib[1], calib[2], c.intr[0], None), "convert_disparity")
    else:
        hip.check(hip.fn["convert_depth_affine"](src.ptr, conv.ptr, w, h, calib[1], calib[2], None), "convert_depth_affine")
    want = conv.numpy()
    assert (want > 0).sum() > w * h // 2
    want_scratch = np.full((h, w), SENTINEL, F)
    if bilateral:
        for _ in range(5):
            want = run_filter(hip, want)
        want_scratch = want
    want_nrm, want_sig = run_normals(hip, want, c.intr) if noise else sentinels(h, w)
    assert_same_bits(depth, want, "depth")
    assert_same_bits(scratch, want_scratch, "scratch")
    assert_same_bits(nrm, want_nrm, "normals")
    assert_same_bits(sig, want_sig, "sigmaZ")
    if noise:
        assert (want_sig > 0).sum() > w * h // 4


def every_int16(w, h):
    if w * h >= 65536:
        return (np.arange(w * h, dtype=np.int64) - 32768).astype(np.int16).reshape(h, w)
    special = [-32768, -32767, -2, -1, 0, 1, 2, 1134, 1135, 1136, 31999, 32000, 32001, 32766, 32767]
    rest = (np.arange(w * h - len(special), dtype=np.int64) * 77 - 32768).astype(np.int16)
    return np.concatenate([np.array(special, np.int16), rest]).reshape(h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(256, 256), (37, 23)], ids=["256x256", "37x23"])
@pytest.mark.parametrize("calib", [(1, 0.001, 0.0), (1, 0.0005, 0.01), DISPARITY, VC.DISPARITY_INT],
                         ids=["affine mm", "affine with offset", "kinect disparity", "disparity with an integer origin"])
def test_conversions_of_every_int16_value_are_the_oracles(hip, oracle, calib, size):
    w, h = size
    raw = every_int16(w, h)
    intr = (232.0, 232.0, w / 2.0, h / 2.0)
    a = run_update(hip, raw, calib, intr, False, False)
    b = run_update(oracle, raw, calib, intr, False, False)
    assert_same_bits(a[0], b[0], "depth")
    assert_same_bits(b[0], VT.convert(raw, *calib, intr[0]), "oracle, restatement")
    if calib == VC.DISPARITY_INT:
        assert (a[0][raw == 1135] == -1).all()          # t == 0: depth 0, which is not > 0
    for i in (1, 2, 3):
        assert (a[i] == SENTINEL).all()
