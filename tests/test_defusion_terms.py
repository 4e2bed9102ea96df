"""Pins tests/defusion_terms.py, the numpy restatement of itm_deintegrate_from_scene (include/itm_hip.h): against a literal per-voxel
loop, rule by rule, and as the inverse of fusion_terms.integrate.  No GPU, no oracle.

Round trip, fusion_terms.integrate then defusion_terms.deintegrate of the same frame, maxW = 255, weights 1 .. 254 x the 2048-entry
sdf tables of prepared_state_cases.  With W the old weight, F the old value, o the observation (|F|, |o| <= 1):
  weights   W -> W + 1 -> W, exactly: integers.
  short     the stored average A' = trunc(32767 A) / 32767 is off A = (W F + o) / (W + 1) by less than one step s = 1 / 32767; the
            inverse scales that error by (W + 1) / W <= 2, and storing again truncates once more: |F' - F| < 2 s + s, plus the float
            roundings (each below 2^-23 relative to W + 1 <= 255, i.e. far below s).  In steps of the stored integer: at most 3 from the
            three terms, asserted as <= 4.  Seen here: 3.
  float     four rounded operations (W F, + o, (W + 1) A', - o) of magnitude at most W + 1, each off by at most 2^-24 (W + 1), then
            the two quotients' roundings of a value <= 1: after the division by W, (4 (W + 1) / W + 2) 2^-24 <= 10 x 2^-24 < 2^-20.
            Seen here: 0.19 x 2^-20.
  clamp     the bounds above allow |F'| up to 1 + 2^-20, so they do not exclude a clamp; it is asserted over the whole table instead: no
            round trip of a value in [-1, 1] leaves [-1, 1].
The four entries of the float table outside [-1, 1] (1.5, -3, 2, -1.25: values no integration produces, there to test the integration's
arithmetic) are not in the TSDF's range; the definition's own clamp brings their round trip to +-1.  They are asserted to do exactly
that (test_round_trip_of_out_of_range_floats_clamps) and are left out of the bounds above, which are derived for |F| <= 1.
"""
import numpy as np
import pytest

import defusion_terms as DT
import fusion_terms as FT
import prepared_state_cases as P

F = np.float32
KINDS = list(P.TYPES)


def frame(kind, maxW=100):
    sc = P.dense_scenario(kind, maxW)
    return sc, sc.frame_inputs(0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.array_equal(bits(a[n]), bits(b[n])) for n in a.dtype.names)


def random_voxels(kind, n, seed):
    """n voxels of the dense case's volume (positions and prepared states drawn independently)."""
    sc, fr = frame(kind)
    rng = np.random.default_rng(seed)
    ix, iy, iz = FT.dense_coordinates(sc.denseSize, sc.denseOffset)
    at = rng.integers(0, len(ix), n)
    old = P.states(sc.voxelType, rng.integers(0, P.N_PAIRS, n))
    return sc, fr, old, ix[at], iy[at], iz[at]


# ---- the literal loop -------------------------------------------------------------------------------------------------------------------
def one_voxel(voxel_type, old, ix, iy, iz, fr, keep):
    """The definition of include/itm_hip.h for ONE voxel, in scalar float32 steps.  Returns (new voxel, set of fact names)."""
    short, colour = voxel_type in FT.SHORT_TYPES, voxel_type in FT.COLOUR_TYPES
    new, facts = old.copy(), set()
    M = np.asarray(fr.M_d, F)
    vs, mu = F(fr.voxelSize), F(fr.mu)
    m = (F(ix) * vs, F(iy) * vs, F(iz) * vs)
    row = lambda Mx, r: F(F(F(F(Mx[r] * m[0]) + F(Mx[4 + r] * m[1])) + F(Mx[8 + r] * m[2])) + F(Mx[12 + r] * F(1.0)))
    pcx, pcy, pcz = row(M, 0), row(M, 1), row(M, 2)
    fx, fy, cx, cy = (F(x) for x in fr.intr_d)
    h, w = fr.depth.shape
    eta = F(-1.0)
    kept = bool(keep) and int(old["w_depth"]) != 0 and int(old["w_depth"]) >= int(fr.maxW)
    if not pcz <= 0:
        u, v = F(F(F(fx * pcx) / pcz) + cx), F(F(F(fy * pcy) / pcz) + cy)
        if not (u < 1 or u > F(w - 2) or v < 1 or v > F(h - 2)):
            dm = fr.depth[int(F(v + F(0.5))), int(F(u + F(0.5)))]
            if not dm <= 0:
                eta = F(dm - pcz)
                if not eta < -mu:
                    W = int(old["w_depth"])
                    if W == 0:
                        facts.add("unobserved")
                    elif kept:
                        facts.add("saturated")
                    elif W == 1:
                        new["sdf"], new["w_depth"] = (32767 if short else F(1.0)), 0
                        facts |= {"touched", "reset"}
                    else:
                        oldF = F(F(old["sdf"]) / F(32767.0)) if short else F(old["sdf"])
                        obs = min(F(1.0), F(eta / mu))
                        f = F(F(F(F(W) * oldF) - obs) / F(W - 1))
                        g = f
                        if F(1.0) < g:
                            g = F(1.0)
                        if not F(-1.0) < g:
                            g = F(-1.0)
                        if g != f:
                            facts.add("clamped")
                        new["sdf"] = np.int16(int(np.trunc(F(g * F(32767.0))))) if short else g
                        new["w_depth"] = W - 1
                        facts.add("touched")
    if colour and not kept and not (eta > mu or abs(F(eta / mu)) > F(0.25)):
        Mr = FT.matmul4(fr.rgb_to_depth_inv if fr.rgb_to_depth_inv is not None else np.eye(4, dtype=F).reshape(16), fr.M_d)
        qx, qy, qz = row(Mr, 0), row(Mr, 1), row(Mr, 2)
        fxc, fyc, cxc, cyc = (F(x) for x in (fr.intr_rgb or fr.intr_d))
        hc, wc = fr.rgb.shape[:2]
        u, v = F(F(F(fxc * qx) / qz) + cxc), F(F(F(fyc * qy) / qz) + cyc)
        Wc = int(old["w_color"])
        if not (u < 1 or u > F(wc - 2) or v < 1 or v > F(hc - 2)) and Wc != 0 and not (keep and Wc >= (int(fr.maxW) & 0xff)):
            facts.add("coloured")
            if Wc == 1:
                new["clr"], new["w_color"] = 0, 0
                facts.add("colour_reset")
            else:
                px, py = int(np.floor(u)), int(np.floor(v))
                dx, dy = F(u - F(px)), F(v - F(py))
                ox, oy = F(F(1.0) - dx), F(F(1.0) - dy)
                for c in range(3):
                    a, b, cc, d = (F(fr.rgb[py + j, px + i, c]) for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)))
                    b, cc, d = (b if dx != 0 else F(0)), (cc if dy != 0 else F(0)), (d if dx != 0 and dy != 0 else F(0))
                    meas = F(F(F(F(F(a * ox) * oy) + F(F(b * dx) * oy)) + F(F(cc * ox) * dy)) + F(F(d * dx) * dy))
                    meas = F(meas / F(255.0))
                    x = F(F(F(F(F(old["clr"][c]) / F(255.0)) * F(Wc)) - meas) / F(Wc - 1))
                    x = F(x * F(255.0))
                    vi = int(F(x - F(0.5))) if x < 0 else int(F(x + F(0.5)))
                    new["clr"][c] = min(max(vi, 0), 255)
                new["w_color"] = Wc - 1
    return new, facts


@pytest.mark.parametrize("keep", [False, True], ids=["all", "keep_saturated"])
@pytest.mark.parametrize("kind", KINDS)
def test_vectorised_form_equals_the_literal_loop(kind, keep):
    sc, fr, old, ix, iy, iz = random_voxels(kind, 3000, 7)
    new, facts = DT.deintegrate(sc.voxelType, old, ix, iy, iz, fr, keep)
    seen = set()
    with np.errstate(all="ignore"):
        for i in range(len(old)):
            want, f = one_voxel(sc.voxelType, old[i], int(ix[i]), int(iy[i]), int(iz[i]), fr, keep)
            assert same(new[i:i + 1], np.array([want], old.dtype)), (i, old[i], want, new[i])
            assert f == {n for n in DT.FACTS if facts[n][i]}, (i, old[i], f)
            seen |= f
    assert seen >= {"touched", "reset", "unobserved", "clamped"} | ({"saturated"} if keep else set()) | ({"coloured"} if sc.colour else set()), seen


# ---- the rules, one at a time -----------------------------------------------------------------------------------------------------------
def gated(kind, n=400, colour_gate=True):
    """n voxel positions of the dense case whose depth part the integration writes (and, for colour types with colour_gate, whose colour
    part too)."""
    sc, fr = frame(kind)
    ix, iy, iz = FT.dense_coordinates(sc.denseSize, sc.denseOffset)
    probe = P.fresh_pool(sc.voxelType, len(ix))
    _, facts = FT.integrate(sc.voxelType, probe, ix, iy, iz, fr)
    k = np.nonzero(facts["coloured"] if sc.colour and colour_gate else facts["touched"])[0]
    assert len(k) >= n
    k = k[:: len(k) // n][:n]
    return sc, fr, ix[k], iy[k], iz[k], facts["eta"][k]


def untouched_but(old, new, fields):
    for n in old.dtype.names:
        if n not in fields:
            assert np.array_equal(bits(old[n]), bits(new[n])), n


@pytest.mark.parametrize("kind", KINDS)
def test_case_rules(kind):
    sc, fr, ix, iy, iz, eta = gated(kind)
    n = len(ix)
    short = sc.voxelType in FT.SHORT_TYPES
    base = P.states(sc.voxelType, P.ORDER[:n])
    base["sdf"] = P.SHORT_TABLE[1000] if short else F(0.25)
    if sc.colour:
        base["w_color"] = 7
    init = 32767 if short else F(1.0)

    def run(w, keep, **fields):
        old = base.copy()
        old["w_depth"] = w
        for k, v in fields.items():
            old[k] = v
        new, facts = DT.deintegrate(sc.voxelType, old, ix, iy, iz, fr, keep)
        return old, new, facts

    # weight 0: nothing of the depth part changes
    old, new, facts = run(0, False)
    assert facts["unobserved"].all() and not facts["touched"].any()
    untouched_but(old, new, ("clr", "w_color"))
    # weight 1: the initial value and weight 0
    old, new, facts = run(1, False)
    assert facts["reset"].all() and facts["touched"].all() and not facts["clamped"].any()
    assert (new["sdf"] == init).all() and (new["w_depth"] == 0).all()
    untouched_but(old, new, ("sdf", "w_depth", "clr", "w_color"))
    # saturated (at and above maxW), kept: not a byte changes, colour included
    for w in (sc.maxW, sc.maxW + 50):
        old, new, facts = run(w, True)
        assert facts["saturated"].all() and not facts["touched"].any() and not facts["coloured"].any()
        assert same(old, new)
        # ... and not kept: a count of w
        old, new, facts = run(w, False)
        assert facts["touched"].all() and not facts["saturated"].any() and (new["w_depth"] == w - 1).all()
    # clamp: an observation of free space (obs = 1 where eta >= mu, else > -1) taken out of a voxel that holds -1
    old, new, facts = run(2, False, sdf=(-32767 if short else F(-1.0)))
    assert facts["clamped"].sum() >= n // 2 and (facts["clamped"] <= facts["touched"]).all()
    assert (new["sdf"][facts["clamped"]] == (-32767 if short else F(-1.0))).all() and (new["w_depth"] == 1).all()
    if sc.colour:
        old, new, facts = run(5, False, w_color=0)
        assert not facts["coloured"].any() and np.array_equal(old["clr"], new["clr"]) and (new["w_color"] == 0).all()
        old, new, facts = run(5, False, w_color=1)
        assert facts["colour_reset"].all() and (new["clr"] == 0).all() and (new["w_color"] == 0).all()
        old, new, facts = run(5, True, w_color=sc.maxW)
        assert not facts["coloured"].any() and np.array_equal(old["clr"], new["clr"]) and (new["w_color"] == sc.maxW).all() and facts["touched"].all()
        old, new, facts = run(5, False, w_color=sc.maxW)
        assert facts["coloured"].all() and (new["w_color"] == sc.maxW - 1).all()


@pytest.mark.parametrize("kind", KINDS)
def test_voxels_the_integration_would_not_write_are_not_touched(kind):
    sc, fr, old, ix, iy, iz = random_voxels(kind, 20000, 11)
    _, fused = FT.integrate(sc.voxelType, old, ix, iy, iz, fr)
    for keep in (False, True):
        new, facts = DT.deintegrate(sc.voxelType, old, ix, iy, iz, fr, keep)
        quiet = ~fused["touched"] & ~fused["coloured"]
        assert quiet.sum() > 1000 and same(old[quiet], new[quiet])
        assert not (facts["touched"] & ~fused["touched"]).any() and not (facts["coloured"] & ~fused["coloured"]).any()
        assert np.array_equal(facts["eta"], fused["eta"], equal_nan=True)


# ---- the round trip -----------------------------------------------------------------------------------------------------------------------
_round_trips = {}


def round_trip(kind):
    """Weights 1 .. 254 x the whole sdf table at positions the integration writes, maxW 255: (old, after integrate + deintegrate, facts)."""
    if kind not in _round_trips:
        sc, fr, ix, iy, iz, _ = gated(kind, 1021, colour_gate=False)          # (a prime number of positions: no weight or table entry is tied to one)
        fr.maxW = 255
        pairs = np.arange(P.N_SDF, 255 * P.N_SDF)
        at = np.arange(len(pairs)) % len(ix)
        old = P.states(sc.voxelType, pairs)
        if sc.colour:
            old["w_color"] = np.minimum(old["w_color"], 254)
        mid, fused = FT.integrate(sc.voxelType, old, ix[at], iy[at], iz[at], fr)
        assert fused["touched"].all() and (not sc.colour or fused["coloured"].sum() > 1000)
        new, facts = DT.deintegrate(sc.voxelType, mid, ix[at], iy[at], iz[at], fr, False)
        _round_trips[kind] = (sc, old, new, facts)
    return _round_trips[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_returns_the_weights_and_the_sdf_within_the_bounds(kind):
    sc, old, new, facts = round_trip(kind)
    assert len(np.unique(old["w_depth"])) == 254 and old["w_depth"].min() == 1 and old["w_depth"].max() == 254
    assert np.array_equal(new["w_depth"], old["w_depth"])
    assert facts["touched"].all() and not facts["reset"].any() and not facts["unobserved"].any() and not facts["saturated"].any()
    if sc.colour:
        assert np.array_equal(new["w_color"], old["w_color"])
    if sc.voxelType in FT.SHORT_TYPES:
        steps = np.abs(new["sdf"].astype(np.int64) - old["sdf"].astype(np.int64))
        print("%s: worst short round trip %d steps" % (kind, steps.max()))
        assert steps.max() <= 4, steps.max()
        assert not facts["clamped"].any()
    else:
        inside = np.abs(old["sdf"]) <= 1.0
        assert np.count_nonzero(~inside) == 4 * 254          # 1.5, -3, 2, -1.25: see the module's docstring and the next test
        err = np.abs(new["sdf"].astype(np.float64) - old["sdf"].astype(np.float64))[inside]
        print("%s: worst float round trip %.3f x 2^-20" % (kind, err.max() * 2.0 ** 20))
        assert err.max() <= 2.0 ** -20, err.max() * 2.0 ** 20
        assert not facts["clamped"][inside].any()


@pytest.mark.parametrize("kind", ["f", "f_rgb"])
def test_round_trip_of_out_of_range_floats_clamps(kind):
    """A float sdf outside [-1, 1] is no value of a TSDF; the average that comes back lies outside too (it is the stored value up to
    rounding: the observation moves it by at most 2 / W towards [-1, 1]) unless the weight is so low that the observation brought it
    inside, and the definition's clamp sets what lies outside to +-1."""
    sc, old, new, facts = round_trip(kind)
    out = np.abs(old["sdf"]) > 1.0
    assert np.array_equal(new["w_depth"][out], old["w_depth"][out])
    assert (np.abs(new["sdf"][out]) <= 1.0).all()
    assert facts["clamped"][out].all() and (new["sdf"][out] == np.sign(old["sdf"][out])).all()


def test_keep_saturated_changes_nothing_below_saturation():
    """keepSaturated only acts at weight >= maxW: below it both settings give the same voxels."""
    sc, fr, old, ix, iy, iz = random_voxels("s_rgb", 20000, 13)
    low = (old["w_depth"] < sc.maxW) & (old["w_color"] < sc.maxW)
    a, _ = DT.deintegrate(sc.voxelType, old[low], ix[low], iy[low], iz[low], fr, False)
    b, _ = DT.deintegrate(sc.voxelType, old[low], ix[low], iy[low], iz[low], fr, True)
    assert low.sum() > 1000 and same(a, b)
