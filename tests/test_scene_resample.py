"""itm_rigid_quantise / itm_scene_resample (include/itm_hip.h): one TSDF scene resampled into another's frame under a rigid transform and
fused there on the GPU.

The product is compared, as whole arrays and bit for bit, with the restatement in tests/scene_resample_terms.py applied to the downloads
taken before the call; there is no tolerance anywhere in those comparisons.  The restatement itself is anchored without a GPU: identity
and whole-voxel transforms against copies, the 24 axis rotations against permuted voxels, affine fields against their exact values, a
plane against its analytic distance within a derived bound, hand cases for the arithmetic, a hand-written candidate list and table."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import itm_testlib as T
import scene_coarsen_terms as K
import scene_merge_terms as M
import scene_resample_terms as R
import test_scene_coarsen as TC
import test_scene_merge as TM
from infinitam_amd import capi
from infinitam_amd.capi import Mesh

W, H = TM.W, TM.H
SIZE, MU = 0.01, 0.04
POOL = TM.POOL
_P = C.c_void_p
ONE = R.ONE


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def rigid(axis, angle, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rotation(axis, angle), t
    return m.astype(np.float32)


# dstFromSrc of the GPU cases: 0.3 rad about (1, 2, 3), a fractional translation; the literals of tests/cpp/scene_resample_demo.cpp
SKEW = np.array([0.958526731, 0.243323788, -0.148391441, 0, -0.230562791, 0.968097508, 0.0981226042, 0,
                 0.167532951, -0.0598395914, 0.984048724, 0, 0.123400003, -0.0566999987, 0.0891000032, 1], np.float32).reshape(4, 4).T
YAW45 = rigid((0, 0, 1), np.pi / 4, (0.0, 0.0, 0.0))


def axis_rotations():
    """The 24 rotations that map the axes onto the axes: signed permutation matrices of determinant +1."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            m = np.zeros((3, 3), np.int64)
            for i in range(3):
                m[i, perm[i]] = signs[i]
            if round(np.linalg.det(m)) == 1:
                out.append(m)
    assert len(out) == 24
    return out


def fine_a(**kw):
    return TM.scenario_a(mu=MU, **kw)


def fine_b(**kw):
    return TM.scenario_b(mu=MU, **kw)


def dense_arg(dst, src):
    if dst.is_hash:
        return None
    return (tuple(src.cfg.denseSize), tuple(src.cfg.denseOffset), tuple(dst.cfg.denseSize), tuple(dst.cfg.denseOffset))


def as_q(q):
    return q if isinstance(q, dict) else q.as_dict()


def resample_and_compare(dst, src, q, slots=None, what="resample"):
    """dst.resample_from(src, q) against the restatement on the downloads taken before the call; src must come out untouched."""
    d0, s0 = TM.snapshot(dst), TM.snapshot(src)
    want, wstats, where = R.resample(d0, s0, as_q(q), slots, dense_arg(dst, src))
    stats = dst.resample_from(src, capi.RigidQ.from_dict(as_q(q)), slots)
    got, s1 = TM.snapshot(dst), TM.snapshot(src)
    print(what, "stats", stats, "restatement", wstats)
    assert stats == wstats, "%s: stats %s vs restatement %s" % (what, stats, wstats)
    if dst.is_hash:
        M.assert_state_equal(got, want, what, T.assert_fields_equal)
        M.assert_state_equal(s1, s0, what + " (src untouched)", T.assert_fields_equal)
        assert np.array_equal(s1["alloc"], s0["alloc"]) and np.array_equal(s1["excess"], s0["excess"])
    else:
        T.assert_fields_equal(got["voxels"], want["voxels"], what + ": voxels")
        T.assert_fields_equal(s1["voxels"], s0["voxels"], what + ": src voxels")
    if "swap" in d0:
        assert np.array_equal(got["swap"], d0["swap"]), what + ": swap states of dst changed"
    return stats, got, d0, where


# ---- CPU: the restatement's voxel arithmetic -----------------------------------------------------------------------------------------

def random_blocks(voxelType, lo, hi, seed):
    """Blocks lo .. hi - 1 per axis, every voxel observed (weights >= 1), random content."""
    rng = np.random.default_rng(seed)
    out = {}
    for bz in range(lo, hi):
        for by in range(lo, hi):
            for bx in range(lo, hi):
                v = K.default_voxels((8, 8, 8), voxelType)
                v["sdf"] = rng.integers(-32767, 32768, (8, 8, 8)) if K.is_short(voxelType) else rng.uniform(-1, 1, (8, 8, 8)).astype(np.float32)
                v["w_depth"] = rng.integers(1, 101, (8, 8, 8))
                if K.has_colour(voxelType):
                    v["clr"], v["w_color"] = rng.integers(0, 256, (8, 8, 8, 3)), rng.integers(1, 101, (8, 8, 8))
                out[(bx, by, bz)] = v
    return out


def grid_of(blocks, lo, hi, voxelType):
    """The voxels of `blocks` as one array [z, y, x] over the voxel coordinates 8 lo .. 8 hi - 1."""
    n = 8 * (hi - lo)
    g = K.default_voxels((n, n, n), voxelType)
    for (bx, by, bz), v in blocks.items():
        g[8 * (bz - lo):8 * (bz - lo) + 8, 8 * (by - lo):8 * (by - lo) + 8, 8 * (bx - lo):8 * (bx - lo) + 8] = v
    return g


def lookup(grid, lo, p):
    """(grid at the voxel coordinates p [..., 3], which of them lie inside it)."""
    n = grid.shape[0]
    i = p - 8 * lo
    inside = np.all((i >= 0) & (i < n), axis=-1)
    return grid[np.where(inside, i[..., 2], 0), np.where(inside, i[..., 1], 0), np.where(inside, i[..., 0], 0)].copy(), inside


def voxel_coordinates(positions):
    l = np.arange(512)
    local = np.stack([l & 7, (l >> 3) & 7, l >> 6], axis=-1)
    return 8 * np.asarray(positions, np.int64)[:, None, :] + local[None, :, :]


def candidate_blocks(q, blocks):
    C, _, outOfRange = R.candidates(q, sorted(blocks))
    assert outOfRange == 0
    return np.unique(C, axis=0)


def expect_copied(src_blocks, voxelType, q, source_of):
    """r over every candidate block equals the src voxel at source_of(dst voxel), TVoxel() where src stores none."""
    src = TC.hand_src(voxelType, src_blocks)
    grid = grid_of(src_blocks, -1, 2, voxelType)
    positions = candidate_blocks(q, src_blocks)
    got = R.resampled_blocks(src, positions, q)
    v = voxel_coordinates(positions)
    want, inside = lookup(grid, -1, source_of(v))
    want[~inside] = K.default_voxels((), voxelType)
    assert np.count_nonzero(inside) == 27 * 512, "the candidate blocks do not hold the whole image"
    T.assert_fields_equal(got.reshape(-1), want.reshape(-1), "copied voxels")
    return positions


@pytest.mark.parametrize("shift", [(0, 0, 0), (3, 8, 21), (-11, -5, -16), (-1, 64, -13)])
def test_a_whole_voxel_translation_copies_the_voxels(shift):
    """inv the identity, invT whole voxels: u = 0 everywhere and r is src's voxel at q - shift.  The stored cube is voxels -8 .. 15, so
    the negative shifts carry blocks across the origin: the Q30 and Q6 values that are shifted arithmetically are negative."""
    q = R.identity(shift)
    s = np.asarray(shift, np.int64)
    f, u = R.position(q, np.array([[-8, 0, 15], [0, 0, 0]]) + s)
    assert np.all(u == 0) and np.array_equal(f, [[-8, 0, 15], [0, 0, 0]])
    for vt in (capi.VOXEL_S_RGB, capi.VOXEL_F):
        positions = expect_copied(random_blocks(vt, -1, 2, 3), vt, q, lambda v: v - s)
        if min(shift) < 0:
            assert positions.min() < -1


def test_the_24_axis_rotations_permute_the_voxels():
    """q = Rm p + shift with a signed permutation Rm: r at dst voxel q is src's voxel at Rm^T (q - shift), exactly."""
    vs = 0.0078125                      # 2^-7 m: shift * vs and t / vs are exact in float32
    shift = np.array([3, -7, 12], np.int64)
    blocks = random_blocks(capi.VOXEL_S_RGB, -1, 2, 5)
    for rm in axis_rotations():
        m = np.eye(4, dtype=np.float32)
        m[:3, :3], m[:3, 3] = rm, shift * vs
        q = R.quantise(m, vs)
        assert sorted(set(abs(v) for v in q["inv"] + q["fwd"])) == [0, ONE] and q["fwdT"] == [int(s) * ONE for s in shift]
        expect_copied(blocks, capi.VOXEL_S_RGB, q, lambda v: (v - shift) @ rm)      # row vector times Rm = Rm^T times the column


SKEW_FRACTIONAL = rigid((1, 2, 3), 0.3, (0.0234, -0.0167, 0.0091))


@pytest.mark.parametrize("voxelType", [capi.VOXEL_S, capi.VOXEL_F])
def test_affine_sdf_and_constant_weight_are_reproduced_exactly(voxelType):
    """Trilinear interpolation reproduces an affine field: where the eight taps are stored, sdf' is the field at P / 64 rounded to the
    nearest (halves away from zero; exact for the float type, whose values n / 2048 need no rounding) and w' = w."""
    def f(x, y, z):
        v = 3 * x - 5 * y + 7 * z + 11
        return v if voxelType == capi.VOXEL_S else v.astype(np.float32) * np.float32(0.03125)
    blocks = TC.ramp_blocks(voxelType, -1, 2, f, 37)
    q = R.quantise(SKEW_FRACTIONAL, SIZE)
    positions = candidate_blocks(q, blocks)
    got = R.resampled_blocks(TC.hand_src(voxelType, blocks), positions, q)
    cell, u = R.position(q, voxel_coordinates(positions))
    assert len(np.unique(u)) == 64, "the fractions do not cover 0 .. 63"
    stored = np.all((cell >= -8) & (cell + 1 <= 15), axis=-1)
    P = 64 * cell + u
    num = 3 * P[..., 0] - 5 * P[..., 1] + 7 * P[..., 2] + 11 * 64                     # 64 f(P / 64)
    if voxelType == capi.VOXEL_S:
        want = np.sign(num) * ((2 * np.abs(num) + 64) // 128)
        assert np.count_nonzero(np.abs(num) % 64 == 32) > 0, "no half to round"
    else:
        want = (num.astype(np.float64) / 2048.0).astype(np.float32)
    assert np.count_nonzero(stored) > 5000
    assert np.array_equal(got["sdf"][stored], want[stored].astype(got["sdf"].dtype)) and np.all(got["w_depth"][stored] == 37)
    edge = ~stored & (got["w_depth"] > 0)
    assert np.count_nonzero(edge) > 0 and np.all(got["w_depth"][edge] <= 37)


def test_a_plane_is_resampled_within_the_derived_bound():
    """A plane with a float normal through 3^3 blocks, stored as short sdf.  At voxels whose eight taps are stored and unclipped:
    |sdf' - analytic| <= 2 + 32767 (voxelSize / mu) sqrt(3) / 128 short units -- 0.5 storage rounding of the taps, 0.5 rounding of the
    result, the position rounded to 1/64 voxel (at most 1/128 voxel per axis, sqrt(3) / 128 along a unit normal), and 1 of slack for
    Q30 and the float32 matrix (a Q30 entry is worth 2^-30 voxel per voxel of coordinate: nothing at these coordinates).  The bound is
    derived, not tuned; with voxelSize / mu = 1/4 it is 112.8 units, the measured maximum 94.2."""
    n = np.array([0.36, -0.48, 0.8])
    d = 0.013                                                     # metres: the plane n . x = d
    scale = 32767.0 * SIZE / MU
    def f(x, y, z):
        return np.rint(np.clip(scale * (n[0] * x + n[1] * y + n[2] * z - d / SIZE), -32767, 32767)).astype(np.int64)
    blocks = TC.ramp_blocks(capi.VOXEL_S, -1, 2, f, 50)
    m = SKEW_FRACTIONAL
    q = R.quantise(m, SIZE)
    positions = candidate_blocks(q, blocks)
    got = R.resampled_blocks(TC.hand_src(capi.VOXEL_S, blocks), positions, q)
    v = voxel_coordinates(positions)
    cell, _ = R.position(q, v)
    m64 = m.astype(np.float64)
    p = ((v * float(np.float32(SIZE)) - m64[:3, 3]) @ m64[:3, :3]) / float(np.float32(SIZE))       # R^T (x - t) in voxels
    analytic = scale * (p @ n - d / SIZE)
    ok = np.all((cell >= -8) & (cell + 1 <= 15), axis=-1) & (np.abs(analytic) < 32767 - 2 * scale)          # no tap is clipped
    bound = 2 + 32767 * (SIZE / MU) * np.sqrt(3) / 128
    err = np.abs(got["sdf"][ok].astype(np.float64) - analytic[ok])
    print("plane: voxels checked", np.count_nonzero(ok), "max |error|", err.max(), "bound", bound)
    assert np.count_nonzero(ok) > 2000 and err.max() <= bound


def fractional(u):
    """q whose src position of dst voxel v is v + u / 64 per axis."""
    q = R.identity()
    q["invT"] = [int(c) * (ONE >> 6) for c in u]
    q["fwdT"] = [-t for t in q["invT"]]
    return q


def one_block(voxelType, voxels):
    """r of dst block 0 from a src whose block 0 holds `voxels` ({(x, y, z): fields})."""
    v = K.default_voxels((8, 8, 8), voxelType)
    for (x, y, z), fields in voxels.items():
        for name, value in fields.items():
            v[name][z, y, x] = value
    return lambda q: R.resampled_blocks(TC.hand_src(voxelType, {(0, 0, 0): v}), np.array([(0, 0, 0)]), q).reshape(8, 8, 8)


def test_single_tap_gives_the_trilinear_weights():
    """One observed voxel (3, 3, 3) of weight 64 and u = (16, 32, 48): dst voxel (3, 3, 3) - k sees it as tap k with
    c_k = (kx ? 16 : 48)(ky ? 32 : 32)(kz ? 48 : 16), w' = (64 c_k + 2^17) >> 18 = (c_k + 2048) >> 12."""
    blk = one_block(capi.VOXEL_S, {(3, 3, 3): dict(sdf=-1234, w_depth=64)})(fractional((16, 32, 48)))
    want = {(0, 0, 0): 48 * 32 * 16, (1, 0, 0): 16 * 32 * 16, (0, 1, 0): 48 * 32 * 16, (1, 1, 0): 16 * 32 * 16,
            (0, 0, 1): 48 * 32 * 48, (1, 0, 1): 16 * 32 * 48, (0, 1, 1): 48 * 32 * 48, (1, 1, 1): 16 * 32 * 48}
    assert sum(want.values()) == 1 << 18
    for k, c in want.items():
        got = blk[3 - k[2], 3 - k[1], 3 - k[0]]
        assert got["w_depth"] == (c + 2048) >> 12 and got["sdf"] == -1234, (k, got)
    assert [(c + 2048) >> 12 for c in want.values()] == [6, 2, 6, 2, 18, 6, 18, 6]
    assert np.count_nonzero(blk["w_depth"]) == 8
    # u = 0: the voxel reaches its own dst voxel only, with its own weight
    blk = one_block(capi.VOXEL_S, {(3, 3, 3): dict(sdf=-1234, w_depth=64)})(R.identity())
    assert np.count_nonzero(blk["w_depth"]) == 1 and (blk[3, 3, 3]["sdf"], blk[3, 3, 3]["w_depth"]) == (-1234, 64) and blk["sdf"][0, 0, 0] == 32767


def two_taps(s0, w0, s1, w1, u=32):
    """dst voxel (2, 2, 2) between src voxels (2, 2, 2) and (3, 2, 2): c = 64^2 (64 - u) and 64^2 u."""
    return one_block(capi.VOXEL_S, {(2, 2, 2): dict(sdf=s0, w_depth=w0), (3, 2, 2): dict(sdf=s1, w_depth=w1)})(fractional((u, 0, 0)))[2, 2, 2]


def test_rounding_is_to_nearest_with_halves_away_from_zero():
    mean_of = lambda a, b: int(two_taps(a, 1, b, 1)["sdf"])                       # u = 32: S / A = (a + b) / 2
    assert [mean_of(1, 2), mean_of(-1, -2), mean_of(0, 1), mean_of(0, -1), mean_of(2, 2), mean_of(-7, 2)] == [2, -2, 1, -1, 2, -3]
    assert mean_of(32767, 32767) == 32767 and mean_of(-32767, -32767) == -32767
    third = lambda a, b: int(two_taps(a, 1, b, 1, u=16)["sdf"])                   # (3 a + b) / 4
    assert [third(0, 1), third(0, 2), third(0, 3), third(0, -1), third(0, -2), third(0, -3)] == [0, 1, 1, 0, -1, -1]
    assert int(two_taps(100, 3, 0, 1)["sdf"]) == 75                               # weighted by the observation weights too


def test_weight_is_rounded_and_clamped():
    assert two_taps(5, 255, 5, 255)["w_depth"] == 255                             # A = 255 * 2^18
    assert two_taps(5, 1, 5, 0)["w_depth"] == 1 and two_taps(5, 1, 5, 0)["sdf"] == 5          # A = 2^17: (2^17 + 2^17) >> 18 = 1
    assert two_taps(5, 1, 5, 0, u=48)["w_depth"] == 1                             # A = 2^16: rounds to 0, never below 1
    assert two_taps(5, 3, 5, 0)["w_depth"] == 2 and two_taps(5, 2, 5, 1)["w_depth"] == 2      # 1.5 -> 2 (halves up)
    assert two_taps(5, 0, 5, 0)["w_depth"] == 0 and two_taps(5, 0, 5, 0)["sdf"] == 32767      # A = 0: r carries no depth
    # dst's maxW clamps in the combine; a voxel without observation leaves dst's as it is
    dst = TM.hand_state({0: ((0, 0, 0), 0, 0)}, 1, -1, 3, 0)
    dst["maxW"] = 20
    v = K.default_voxels((8, 8, 8), capi.VOXEL_S)
    v[2, 2, 2] = (900, 200)
    src = TC.hand_src(capi.VOXEL_S, {(0, 0, 0): v})
    h = np.zeros(8, capi.HASH_ENTRY_DTYPE); h["ptr"] = -2; h[0] = src["hash"][0]
    src.update(hash=h)
    out, stats, _ = R.resample(dst, src, R.identity(), slots=[0])
    assert out["voxels"]["w_depth"][2 + 8 * 2 + 64 * 2] == 20
    keep = np.ones(512, bool); keep[2 + 8 * 2 + 64 * 2] = False
    T.assert_fields_equal(out["voxels"][:512][keep], dst["voxels"][:512][keep], "voxels without observation")


def test_colour_without_colour_weight_stays_zero():
    blk = one_block(capi.VOXEL_S_RGB, {(2, 2, 2): dict(sdf=100, w_depth=50, w_color=0, clr=(200, 100, 50))})(R.identity())
    v = blk[2, 2, 2]
    assert v["w_depth"] == 50 and v["sdf"] == 100 and tuple(v["clr"]) == (0, 0, 0) and v["w_color"] == 0
    blk = one_block(capi.VOXEL_F_RGB, {(2, 2, 2): dict(sdf=0.5, w_depth=50, w_color=16, clr=(200, 100, 51)),
                                       (3, 2, 2): dict(sdf=0.25, w_depth=50, w_color=0, clr=(9, 9, 9))})(fractional((32, 0, 0)))
    v = blk[2, 2, 2]
    assert v["sdf"] == np.float32(0.375) and tuple(v["clr"]) == (200, 100, 51) and v["w_color"] == 8      # Bc = 16 * 2^17
    # depth and colour are independent: colour observed where depth is not
    blk = one_block(capi.VOXEL_S_RGB, {(2, 2, 2): dict(w_depth=0, w_color=7, clr=(1, 2, 3))})(R.identity())
    assert tuple(blk[2, 2, 2]["clr"]) == (1, 2, 3) and blk[2, 2, 2]["w_color"] == 7 and blk[2, 2, 2]["w_depth"] == 0 and blk[2, 2, 2]["sdf"] == 32767


# ---- CPU: the candidate list and the table --------------------------------------------------------------------------------------------

def test_candidate_list_of_one_block_under_a_45_degree_yaw():
    """Block (2, 0, 0) = voxels 16 .. 23 x 0 .. 7 under a yaw of 45 degrees about the origin: the dilated cube [15, 24] x [-1, 8] maps to
    x' in [4.9, 17.7], y' in [9.9, 22.6] (voxels) and z stays.  With the margins the voxel ranges are [3, 19], [8, 24] and [-2, 10]: blocks
    x' 0 .. 2, y' 1 .. 3, z -1 .. 1.  The inverse test drops two of the nine per layer: the cube of (0, 3) maps back to y in [12.0, 21.9]
    and that of (2, 3) to x in [28.3, 38.2], which miss the block's 0 .. 7 and 16 .. 23 by more than the margins; (1, 3) maps to
    x in [22.6, 32.5], y in [6.4, 16.3] and stays, as the other six do."""
    q = R.quantise(YAW45, SIZE)
    C, per, outOfRange = R.candidates(q, [(2, 0, 0)])
    xy = [(0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3)]
    kept = [c for c in xy if c in HAND_YAW_XY]
    want = [(x, y, z) for z in (-1, 0, 1) for (x, y) in kept]
    assert [tuple(c) for c in C.tolist()] == want and per.tolist() == [len(want)] and outOfRange == 0
    # the same from real geometry: a dst block is needed iff its cube, widened by the footprint, meets the rotated cube (a superset test
    # on axis-aligned boxes can only add blocks, never lose one)
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    needed = set()
    for x in np.arange(16, 24.01, 0.25):
        for y in np.arange(0, 8.01, 0.25):
            needed.add((int(np.floor((c * x - s * y) / 8)), int(np.floor((s * x + c * y) / 8))))
    assert needed <= set(kept)


HAND_YAW_XY = {(0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (2, 2), (1, 3)}


def test_restated_allocation_known_answers():
    """bucketNum = 8, four excess entries, as test_scene_merge's hand tables.  q shifts by 3 voxels: the participant at block 0 has the
    eight candidates {0, 1}^3, in the order x innermost; they hash to 0 5 5 0 7 2 2 7.  Round 1: the higher index wins each head
    (indices 3, 2, 7, 6), the sweep serves slots 0, 2, 5, 7 in ascending order; round 2: the other four on the tails, again ascending;
    round 3 finds no request."""
    q = R.identity((3, 3, 3))
    C, per, _ = R.candidates(q, [(0, 0, 0)])
    assert [tuple(c) for c in C.tolist()] == [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
    assert [M.hash_index(c, 7) for c in C.tolist()] == [0, 5, 5, 0, 7, 2, 2, 7]
    dst = TM.hand_state({}, 8, 7, 3, 0)
    src = TM.hand_state({0: ((0, 0, 0), 0, 0), 1: ((0, 0, 0), 0, 1), 5: ((9, 9, 9), 0, -1)}, 2, -1, 3, 1)      # two participants at one position: C holds every candidate twice
    table = {0: ((1, 1, 0), 4, 7), 2: ((0, 1, 1), 3, 6), 5: ((0, 1, 0), 2, 5), 7: ((1, 1, 1), 1, 4),
             11: ((0, 0, 0), 0, 3), 10: ((1, 0, 1), 0, 2), 9: ((1, 0, 0), 0, 1), 8: ((0, 0, 1), 0, 0)}
    for every in (False, True):
        out, stats, where = R.resample(dst, src, q, every_candidate=every)
        assert TM.table_of(out) == table
        assert (out["lastFreeBlockId"], out["lastFreeExcessListId"]) == (-1, -1)
        assert stats == dict(rounds=3, considered=2, candidates=16, alreadyPresent=0, allocated=8, resampled=8, unserved=0, srcWithoutBlock=1, dstSwappedOut=0, outOfRange=0)
        assert where == {pos: slot for slot, (pos, _, _) in table.items()}
        # the voxels: r combined into what the block held (the pool is random); block (0, 0, 0) of dst reads src voxels -3 .. 4: only 0 .. 4 are stored
        r = R.resampled_blocks(src, np.array([(0, 0, 0)]), q)
        T.assert_fields_equal(out["voxels"][3 * 512:4 * 512], M.combine_voxels(r[0], dst["voxels"][3 * 512:4 * 512], capi.VOXEL_S, 100), "dst block (0, 0, 0)")
        assert np.count_nonzero(r[0]["w_depth"]) <= 125
    # one position present and swapped out, one present; the excess list runs dry after one entry: found ones are counted per candidate
    dst = TM.hand_state({0: ((1, 1, 0), 0, -1), 5: ((0, 1, 0), 0, 6)}, 8, 5, 0, 0)
    for every in (False, True):
        out, stats, where = R.resample(dst, src, q, slots=[1, 5, 1], every_candidate=every)
        # round 1: heads 7 and 2 are empty -> indices 7, 6 win; tails 0 and 5 -> indices 0, 1 ask on the tails: slot 0 takes the one excess entry, slot 5 finds none left
        assert TM.table_of(out) == {0: ((1, 1, 0), 1, -1), 5: ((0, 1, 0), 0, 6), 8: ((0, 0, 0), 0, 5), 2: ((0, 1, 1), 0, 4), 7: ((1, 1, 1), 0, 3)}
        # round 2: the three losers ask on the tails 2, 5 and 7, the excess list is empty, none is served: the rounds end
        assert stats == dict(rounds=2, considered=1, candidates=8, alreadyPresent=2, allocated=3, resampled=4, unserved=3, srcWithoutBlock=1, dstSwappedOut=1, outOfRange=0)
        assert (out["lastFreeBlockId"], out["lastFreeExcessListId"]) == (2, -1)
    # blocks at the rim of the short range: candidates beyond it are dropped and counted
    far = TM.hand_state({0: ((32767, 0, -32768), 0, 0)}, 1, -1, 3, 1)
    C, per, outOfRange = R.candidates(R.identity(), far["hash"]["pos"][:1].astype(np.int64))
    assert len(C) == 12 and outOfRange == 15 and C[:, 0].max() == 32767 and C[:, 2].min() == -32768


# ---- CPU: oracle scenes ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_states(oracle):
    """A and B on the oracle (computed once, read only)."""
    out = {}
    for name, sc in (("A", fine_a()), ("B", fine_b())):
        ses = TM.build(oracle, sc)
        out[name] = M.state_of(ses.scene)
        ses.close()
    return out


def subset_of(state, count):
    """The scene reduced to the first `count` entries of its table that hold a block (taps read the whole of src, whatever a slot list
    selects: a smaller src keeps the numpy voxel rule quick)."""
    h = state["hash"].copy()
    h["ptr"][np.nonzero(h["ptr"] >= 0)[0][count:]] = -2
    return dict(state, hash=h)


def blocks_by_position(state):
    h = state["hash"]
    vox = state["voxels"].reshape(-1, 512)
    return {tuple(int(c) for c in h["pos"][s]): vox[h["ptr"][s]] for s in np.nonzero(h["ptr"] >= 0)[0]}


def assert_equals_merge(resampled, merged, before, what):
    """Identity q against itm_scene_merge: every block the merge holds is in the resampled scene with the same 512 voxels; the blocks
    the resample holds beyond those (candidates around the participants: the definition over-allocates) hold what they held as free
    blocks -- nothing was observed for them."""
    got, want, pool = blocks_by_position(resampled), blocks_by_position(merged), before["voxels"].reshape(-1, 512)
    assert set(want) <= set(got), what + ": a block of the merge is missing"
    for pos, blk in want.items():
        T.assert_fields_equal(got[pos], blk, "%s: block %s" % (what, (pos,)))
    extra = sorted(set(got) - set(want))
    h = resampled["hash"]
    ptr_of = {tuple(int(c) for c in h["pos"][s]): int(h["ptr"][s]) for s in np.nonzero(h["ptr"] >= 0)[0]}
    for pos in extra:
        T.assert_fields_equal(got[pos], pool[ptr_of[pos]], "%s: over-allocated block %s" % (what, (pos,)))
    return len(extra)


def test_identity_equals_the_merge_on_oracle_scenes(oracle_states):
    """B, reduced to 300 blocks, into A with identity q."""
    a, b = oracle_states["A"], subset_of(oracle_states["B"], 300)
    merged, ms, _ = M.merge(a, b)
    out, stats, _ = R.resample(a, b, R.identity())
    assert ms["alreadyPresent"] > 0 and ms["allocated"] > 0
    extra = assert_equals_merge(out, merged, a, "identity")
    print("identity: merge", ms, "resample", stats, "over-allocated blocks", extra)
    assert stats["considered"] == ms["considered"] == 300 and stats["candidates"] == 27 * 300 and stats["unserved"] == 0
    assert stats["allocated"] == ms["allocated"] + extra and stats["resampled"] >= ms["combined"]


def test_restatement_invariants_on_oracle_scenes(oracle_states):
    """A into an empty table under the skew transform: positions once each, chains end, counters move by what was allocated; the blocks
    that observed something are the image of A."""
    a = subset_of(oracle_states["A"], 400)
    slots = np.nonzero(a["hash"]["ptr"] >= 0)[0]
    empty = dict(a)
    h = a["hash"].copy(); h["ptr"], h["offset"], h["pos"] = -2, 0, 0
    n = len(a["voxels"]) // 512
    empty.update(hash=h, voxels=K.default_voxels(len(a["voxels"]), a["voxelType"]), alloc=np.arange(n, dtype=np.int32), lastFreeBlockId=n - 1,
                 excess=np.arange(len(a["excess"]), dtype=np.int32), lastFreeExcessListId=len(a["excess"]) - 1)
    q = R.quantise(SKEW, SIZE)
    out, stats, where = R.resample(empty, a, q)
    # (check_invariants wants src's positions for the union it compares with: the candidates are the result's own)
    TM.check_invariants(empty, out, dict(hash=out["hash"]), dict(stats, unserved=0))
    assert stats["allocated"] == stats["resampled"] == len(set(where.values())) and stats["unserved"] == 0 and stats["alreadyPresent"] == 0
    per = stats["candidates"] / stats["considered"]
    observed = np.count_nonzero(out["voxels"]["w_depth"].reshape(-1, 512).any(axis=1))
    print("skew: stats", stats, "candidates per participant %.1f" % per, "blocks that observed something", observed)
    assert 8 <= per <= 64 and 0 < observed <= stats["resampled"]
    w_src = a["voxels"]["w_depth"].reshape(-1, 512)[a["hash"]["ptr"][slots]]
    assert 0.5 < np.count_nonzero(out["voxels"]["w_depth"]) / np.count_nonzero(w_src) < 2.0, "the image holds about as many observed voxels as the blocks it came from"


# ---- CPU: the quantiser and the bindings -----------------------------------------------------------------------------------------------

def test_rigid_quantise(hip_host):
    q = capi.rigid_quantise(np.eye(4), SIZE, hip_host).as_dict()
    assert q == R.identity() == R.quantise(np.eye(4), SIZE)
    for rm in axis_rotations():
        m = np.eye(4, dtype=np.float32); m[:3, :3] = rm
        q = capi.rigid_quantise(m, SIZE, hip_host).as_dict()
        assert q["fwd"] == [int(v) * ONE for v in rm.reshape(-1)] and q["inv"] == [int(v) * ONE for v in rm.T.reshape(-1)] and q["invT"] == q["fwdT"] == [0, 0, 0]
    # a skew rotation: within 1 of numpy's rint of the same double expressions (the host compiler may contract where numpy does not)
    for m in (SKEW, SKEW_FRACTIONAL, rigid((-2, 1, 0.5), 2.9, (-20.0, 3.5, 11.25))):
        q, want = capi.rigid_quantise(m, SIZE, hip_host).as_dict(), R.quantise(m, SIZE)
        assert all(abs(a - b) <= 1 for k in want for a, b in zip(q[k], want[k])), (q, want)
        assert R.within_bounds(q)
        inv, fwd = np.array(q["inv"], object).reshape(3, 3), np.array(q["fwd"], object).reshape(3, 3)
        prod = inv.dot(fwd)
        assert all(abs(int(prod[i, j]) - (ONE * ONE if i == j else 0)) <= 8 * ONE for i in range(3) for j in range(3)), "inv fwd is not within 8 * 2^-30 of the identity"
    # the flat column-major form is the same matrix
    assert capi.rigid_quantise(np.ascontiguousarray(SKEW.T).reshape(16), SIZE, hip_host).as_dict() == capi.rigid_quantise(SKEW, SIZE, hip_host).as_dict()

    def refused(m, size=SIZE):
        out = capi.RigidQ()
        flat = np.ascontiguousarray(np.asarray(m, np.float32).T).reshape(16)
        rc = hip_host.fn["rigid_quantise"](flat.ctypes.data_as(C.POINTER(C.c_float)), float(size), C.byref(out))
        return rc == capi.ERR_INVALID and len(hip_host.fn["last_error"]() or b"") > 0
    ok = SKEW.copy()
    assert not refused(ok)
    for i, j in ((0, 0), (1, 3), (3, 3)):
        for bad in (np.nan, np.inf):
            m = ok.copy(); m[i, j] = bad
            assert refused(m), "a non-finite entry"
    m = ok.copy(); m[3, 1] = 1e-6
    assert refused(m), "a bottom row other than (0, 0, 0, 1)"
    m = ok.copy(); m[3, 3] = 2.0
    assert refused(m), "a bottom row other than (0, 0, 0, 1)"
    m = ok.copy(); m[:3, :3] *= np.float32(1.001)
    assert refused(m), "scaled: R^T R - I above 1e-4"
    m = ok.copy(); m[0, 1] += np.float32(0.001)
    assert refused(m), "sheared: R^T R - I above 1e-4"
    m = ok.copy(); m[:3, 0] = -m[:3, 0]
    assert refused(m), "a reflection"
    m = ok.copy(); m[1, 3] = np.float32(-SIZE * 2 ** 18)
    assert refused(m), "|t| / voxelSize >= 2^18"
    m = ok.copy(); m[1, 3] = np.float32(SIZE * (2 ** 18 - 64))
    assert not refused(m)
    assert refused(ok, 0.0) and refused(ok, -1.0) and refused(ok, float("nan")), "a voxelSize that is not positive and finite"
    with pytest.raises(capi.ItmError):
        capi.rigid_quantise(np.zeros((4, 4)), SIZE, hip_host)


def test_scene_resample_is_declared_and_bound(hip_host):
    for name in ("scene_resample", "rigid_quantise"):
        assert name in capi.declared_functions() and name in capi._HOST_IO_SIGS and name in hip_host.fn
    assert C.sizeof(capi.ResampleStats) == 40 and C.sizeof(capi.RigidQ) == 128
    assert "resample.hip" in open(os.path.join(T.ROOT, "infinitam_amd", "csrc", "Makefile")).read()


def test_record_layouts_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "itm_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(itm_rigid_q), '
                   'offsetof(itm_rigid_q, invT), offsetof(itm_rigid_q, fwd), offsetof(itm_rigid_q, fwdT), sizeof(itm_resample_stats), offsetof(itm_resample_stats, outOfRange));return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    Q = capi.RigidQ
    assert got == [C.sizeof(Q), Q.invT.offset, Q.fwd.offset, Q.fwdT.offset, C.sizeof(capi.ResampleStats), capi.ResampleStats.outOfRange.offset]


DEMO_SRC = os.path.join(T.ROOT, "tests", "cpp", "scene_resample_demo.cpp")
DEMO_EXE = os.path.join(T.ROOT, "tests", "cpp", "scene_resample_demo")


def build_demo():
    import infinitam_amd
    lib = infinitam_amd.lib_path()
    if not os.path.exists(lib):
        infinitam_amd.build()
    cmd = ["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-I", os.path.join(T.ROOT, "include"), DEMO_SRC, "-o", DEMO_EXE,
           "-L", os.path.dirname(lib), "-l:libitmhip.so", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True)
    return DEMO_EXE


def test_resample_adapters_compile_and_link():
    assert os.path.exists(build_demo())


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def empty(be, sc):
    return T.Session(be, sc)


def skew_q(be):
    return capi.rigid_quantise(SKEW, SIZE, be).as_dict()


@pytest.mark.gpu
@pytest.mark.parametrize("voxel", [capi.VOXEL_S, capi.VOXEL_F, capi.VOXEL_S_RGB, capi.VOXEL_F_RGB])
def test_resampling_into_an_empty_scene_equals_the_restatement(hip, voxel):
    """Case a: A under the skew transform."""
    colour = voxel in (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB)
    sc = fine_a(voxelType=voxel, colour=colour)
    a, d = TM.build(hip, sc), empty(hip, sc)
    stats, got, _, _ = resample_and_compare(d.scene, a.scene, skew_q(hip), what="case a, voxel type %d" % voxel)
    assert stats["allocated"] == stats["resampled"] > 100 and stats["rounds"] >= 2 and stats["unserved"] == 0 and stats["alreadyPresent"] == 0
    assert 8 <= stats["candidates"] / stats["considered"] <= 64
    assert np.count_nonzero(got["voxels"]["w_depth"]) > 10000
    if colour:
        assert np.count_nonzero(got["voxels"]["w_color"]) > 10000 and np.count_nonzero(got["voxels"]["clr"]) > 10000
    a.close(); d.close()


@pytest.mark.gpu
def test_resampling_the_whole_scene_into_one_that_holds_another(hip):
    """Case b: every block of A into a dst that holds B, so the combine runs against real content and most candidates are present."""
    a, d = TM.build(hip, fine_a()), TM.build(hip, fine_b())
    stats, got, before, _ = resample_and_compare(d.scene, a.scene, skew_q(hip), what="case b")
    assert stats["alreadyPresent"] > 1000 and stats["allocated"] > 100 and stats["unserved"] == 0
    assert stats["considered"] == int(np.count_nonzero(TM.snapshot(a.scene)["hash"]["ptr"] >= 0))
    both = (before["voxels"]["w_depth"] > 0) & (got["voxels"]["w_depth"] > before["voxels"]["w_depth"])
    assert np.count_nonzero(both) > 10000, "few voxels were combined with content of dst"
    a.close(); d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bucketNum,excessNum,runs_dry", [(0x800, 0x1800, False), (0x400, 0x100, True)])
def test_resampling_into_tiny_tables_equals_the_restatement(hip, bucketNum, excessNum, runs_dry):
    """Case c: the tables of test_scene_coarsen's case b; the second cannot hold the candidates of 300 blocks (1024 heads, 256 excess
    entries), so its excess list runs dry."""
    a = TM.build(hip, fine_a())
    d = empty(hip, fine_a(bucketNum=bucketNum, excessNum=excessNum))
    held = np.nonzero(a.scene.download(capi.BUF_HASH_ENTRIES)["ptr"] >= 0)[0]
    stats, got, before, where = resample_and_compare(d.scene, a.scene, skew_q(hip), held[:300].astype(np.int32), what="case c, %#x + %#x" % (bucketNum, excessNum))
    assert stats["rounds"] >= 3, "no chain grew by more than one entry"
    if runs_dry:
        assert stats["unserved"] > 0 and got["lastFreeExcessListId"] == -1 and got["lastFreeBlockId"] >= 0
        TC.assert_only_D_changed(before, got, where, "case c")
    else:
        assert stats["unserved"] == 0
    a.close(); d.close()


@pytest.mark.gpu
def test_resampling_with_an_exhausted_voxel_pool_equals_the_restatement(hip):
    """Case d: 100 voxel blocks for the candidates of 300 participants."""
    a, d = TM.build(hip, fine_a()), empty(hip, fine_a(localBlockNum=100))
    held = np.nonzero(a.scene.download(capi.BUF_HASH_ENTRIES)["ptr"] >= 0)[0]
    stats, got, _, _ = resample_and_compare(d.scene, a.scene, skew_q(hip), held[:300].astype(np.int32), what="case d")
    assert stats["allocated"] == 100 == stats["resampled"] and stats["unserved"] > 0 and got["lastFreeBlockId"] == -1
    a.close(); d.close()


@pytest.mark.gpu
def test_resampling_a_visible_list_equals_the_restatement(hip):
    """Case e: a third of A's visible list, permuted, with duplicates, into a dst that holds B; from a host array and a device buffer."""
    a = TM.build(hip, fine_a())
    n = a.scene.counters(a.rs)["noVisibleEntries"]
    ids = a.scene.download(capi.BUF_VISIBLE_IDS, a.rs)[:n].copy()
    ids = ids[: n // 3]
    slots = np.random.default_rng(7).permutation(np.concatenate([ids, ids[:17], ids[5:9]])).astype(np.int32)
    d = TM.build(hip, fine_b())
    q = skew_q(hip)
    stats, got, before, where = resample_and_compare(d.scene, a.scene, q, slots, what="case e")
    assert stats["considered"] == len(ids) and stats["allocated"] > 0 and stats["alreadyPresent"] > 0
    assert 0 < stats["resampled"] < np.count_nonzero(got["hash"]["ptr"] >= 0)
    TC.assert_only_D_changed(before, got, where, "case e")
    d2 = TM.build(hip, fine_b())
    dev = hip.to_backend(slots)
    assert d2.scene.resample_from(a.scene, capi.RigidQ.from_dict(q), dev) == stats
    T.assert_fields_equal(d2.scene.download(capi.BUF_HASH_ENTRIES), got["hash"], "device list vs host list: hash")
    T.assert_fields_equal(d2.scene.download(capi.BUF_VOXEL_BLOCKS), got["voxels"], "device list vs host list: voxels")
    # a matrix in the place of q: quantised with dst's voxel size
    d3 = TM.build(hip, fine_b())
    assert d3.scene.resample_from(a.scene, SKEW, slots) == stats
    T.assert_fields_equal(d3.scene.download(capi.BUF_VOXEL_BLOCKS), got["voxels"], "matrix vs q: voxels")
    a.close(); d.close(); d2.close(); d3.close()


@pytest.mark.gpu
def test_resampling_between_swapping_scenes_equals_the_restatement(hip):
    """Case f: test_scene_merge's swapping scenes: entries of src and of dst are swapped out."""
    (src, rs_s), (dst, rs_d) = TM.swapping_scene(hip, 1), TM.swapping_scene(hip, 2)
    sp, dp = src.download(capi.BUF_HASH_ENTRIES)["ptr"], dst.download(capi.BUF_HASH_ENTRIES)["ptr"]
    assert np.count_nonzero(sp == -1) > 100 and np.count_nonzero(dp == -1) > 100
    q = capi.rigid_quantise(rigid((1, 2, 3), 0.05, (0.0234, -0.0167, 0.0091)), SIZE, hip).as_dict()
    # (mu of these scenes is the default of both; the small turn keeps src's blocks over dst's, swapped-out ones among them)
    stats, _, _, _ = resample_and_compare(dst, src, q, what="case f")
    assert stats["srcWithoutBlock"] == int(np.count_nonzero(sp == -1)) and stats["dstSwappedOut"] > 0 and stats["resampled"] > 100
    rs_s.close(); rs_d.close(); src.close(); dst.close()


@pytest.mark.gpu
def test_resampling_dense_scenes_equals_the_restatement(hip):
    """Case g: 64^3 cells each at different offsets, so taps leave src's array; dst holds B: the combine runs against content."""
    a = TM.build(hip, fine_a(indexType=capi.INDEX_DENSE, denseSize=(64, 64, 64), denseOffset=(-32, -32, 95), localBlockNum=0))
    d = TM.build(hip, fine_b(indexType=capi.INDEX_DENSE, denseSize=(64, 64, 64), denseOffset=(-40, -20, 90), localBlockNum=0))
    assert np.count_nonzero(a.scene.download(capi.BUF_VOXEL_BLOCKS)["w_depth"]) > 1000
    before = d.scene.download(capi.BUF_VOXEL_BLOCKS)
    q = capi.rigid_quantise(rigid((1, 2, 3), 0.1, (0.0234, -0.0167, 0.0091)), SIZE, hip).as_dict()
    stats, got, _, _ = resample_and_compare(d.scene, a.scene, q, what="case g")
    assert stats == dict(dict.fromkeys(R.STATS, 0), considered=1, resampled=1)
    changed = got["voxels"]["w_depth"] != before["w_depth"]
    assert np.count_nonzero(changed) > 1000 and np.count_nonzero(~changed & (before["w_depth"] > 0)) > 0
    # a slot list is refused, dst untouched
    dev = hip.to_backend(np.zeros(1, np.int32))
    cq = capi.RigidQ.from_dict(q)
    assert hip.fn["scene_resample"](_P(d.scene.h), _P(a.scene.h), C.byref(cq), _P(dev.ptr), 1, None, None) == capi.ERR_INVALID
    T.assert_fields_equal(d.scene.download(capi.BUF_VOXEL_BLOCKS), got["voxels"], "dense dst after a refusal")
    a.close(); d.close()


@pytest.mark.gpu
def test_identity_on_the_gpu_equals_merge_from_on_a_twin(hip):
    """Case h: B into A with identity q, and merge_from on a twin of A: every block of the merged twin is in the resampled scene with the
    same voxels, bit for bit; the blocks beyond (the definition allocates the candidates around every participant) are untouched."""
    b = TM.build(hip, fine_b())
    a, twin = TM.build(hip, fine_a()), TM.build(hip, fine_a())
    before = TM.snapshot(a.scene)
    ms = twin.scene.merge_from(b.scene)
    stats = a.scene.resample_from(b.scene, capi.RigidQ.from_dict(R.identity()))
    extra = assert_equals_merge(TM.snapshot(a.scene), TM.snapshot(twin.scene), before, "case h")
    print("case h: merge", ms, "resample", stats, "over-allocated", extra)
    assert stats["considered"] == ms["considered"] and stats["candidates"] == 27 * ms["considered"] and stats["allocated"] == ms["allocated"] + extra
    assert ms["alreadyPresent"] > 0 and ms["allocated"] > 0
    a.close(); b.close(); twin.close()


@pytest.mark.gpu
def test_resampling_launches_recorded_frames_first(hip):
    """Case i: both scenes hold recorded, unflushed engine calls when resample_from is called; the result is that of the eager run."""
    results = []
    for recorded in (True, False):
        pair = []
        for sc in (fine_b(), fine_a()):
            ses = TM.build(hip, sc, frames=2, deferred=recorded)
            v = ses.view(2)
            ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
            ses.scene.reco.IntegrateIntoScene(v, ses.rs)
            ses.scene.vis.CreateExpectedDepths(v.M_d, v.intr_d, ses.rs)        # recorded: nothing of frame 2 has been launched yet
            pair.append(ses)
        d, a = pair
        q = capi.RigidQ.from_dict(skew_q(hip))
        stats = d.scene.resample_from(a.scene, q)
        results.append((stats, TM.snapshot(d.scene)))
        a.close(); d.close()
    assert results[0][0] == results[1][0] and results[0][0]["allocated"] > 0 and results[0][0]["alreadyPresent"] > 0
    M.assert_state_equal(results[0][1], results[1][1], "case i: recorded vs eager", T.assert_fields_equal)


@pytest.mark.gpu
def test_resample_refusals_leave_dst_untouched(hip):
    """Case j."""
    a = TM.build(hip, fine_a(), frames=1)
    d = empty(hip, fine_a())
    depth = [hip.to_backend(d.sc.depth(k)) for k in range(2)]
    v = [capi.View(depth[k], W, H, M_d=d.sc.pose(k), intr_d=d.sc.intr()) for k in range(2)]
    d.scene.process_frame_ahead(v[0], v[1], d.rs, d.points, d.normals)          # dst holds a frame and the requests of the next
    before = TM.snapshot(d.scene)
    entries = len(TM.snapshot(a.scene)["hash"])
    good = skew_q(hip)

    def refused(dst, src, q=good, slots=None, n=None):
        dev = hip.to_backend(np.asarray(slots, np.int32)) if slots is not None else None
        count = (len(slots) if slots is not None else 0) if n is None else n
        cq = capi.RigidQ.from_dict(q) if q is not None else None
        rc = hip.fn["scene_resample"](_P(dst.h if dst else None), _P(src.h if src else None), C.byref(cq) if cq is not None else None, _P(dev.ptr if dev else None), count,
                                      None, None)
        hip.sync()
        return rc == capi.ERR_INVALID and len(hip.fn["last_error"]() or b"") > 0

    def scene(voxel=capi.VOXEL_S, index=capi.INDEX_HASH, size=SIZE, mu=MU, **kw):
        s = hip.create_scene(voxel, index, capi.default_params(voxelSize=size, mu=mu), localBlockNum=POOL if index == capi.INDEX_HASH else 0, **kw)
        s.reco.ResetScene()
        return s

    def with_entry(name, i, value):
        q = {k: list(v) for k, v in good.items()}
        q[name][i] = value
        return q

    up = lambda x: float(np.nextafter(np.float32(x), np.float32(1)))
    other_type, dense = scene(capi.VOXEL_F), scene(index=capi.INDEX_DENSE, denseSize=(64, 64, 64))
    double_size, off_size, other_mu, ok = scene(size=2 * SIZE), scene(size=up(SIZE)), scene(mu=up(MU)), scene()
    assert refused(d.scene, a.scene), "dst holds the block requests of a frame issued ahead"
    d.scene.cancel_ahead(d.rs)
    assert refused(None, a.scene) and refused(d.scene, None), "null scene"
    assert refused(d.scene, a.scene, q=None), "null transform"
    assert refused(d.scene, d.scene), "dst is src"
    assert refused(d.scene, other_type), "voxel type mismatch"
    assert refused(d.scene, dense), "hash with dense"
    assert refused(d.scene, double_size), "doubled voxel size"
    assert refused(d.scene, off_size), "voxelSize differing in the last bit"
    assert refused(d.scene, other_mu), "mu differing in the last bit"
    assert refused(d.scene, ok, slots=[0, entries, 3]) and refused(d.scene, ok, slots=[-1]), "a slot outside the table"
    assert refused(d.scene, ok, slots=[0, 1], n=-2), "a negative count"
    # a row of inv / fwd that sums to more than 1.75 * 2^30; a translation of 2^48 or beyond
    over = R.ROW_BOUND - sum(abs(x) for x in good["inv"][:3]) + abs(good["inv"][0]) + 1
    assert refused(d.scene, a.scene, q=with_entry("inv", 0, over)) and refused(d.scene, a.scene, q=with_entry("fwd", 8, -ONE - (3 * ONE) // 4)), "a row sum over the bound"
    assert not R.within_bounds(with_entry("inv", 0, over)) and R.within_bounds(with_entry("inv", 0, over - 1))
    assert refused(d.scene, a.scene, q=with_entry("invT", 1, 1 << 48)) and refused(d.scene, a.scene, q=with_entry("fwdT", 2, -(1 << 48))), "|T| >= 2^48"
    after = TM.snapshot(d.scene)
    M.assert_state_equal(after, before, "refusals", T.assert_fields_equal)
    assert np.array_equal(after["alloc"], before["alloc"]) and np.array_equal(after["excess"], before["excess"])
    assert d.scene.resample_from(a.scene, capi.RigidQ.from_dict(with_entry("invT", 1, (1 << 48) - 1)))["candidates"] == 0      # in order, and far from everything
    assert d.scene.resample_from(a.scene, capi.RigidQ.from_dict(good))["allocated"] > 0                     # and the call that is in order goes through
    for s in (other_type, dense, double_size, off_size, other_mu, ok):
        s.close()
    a.close(); d.close()


FAR = (25.0, -22.0, 30.0)      # metres: src lies far outside cubes placed around the origin


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["default", "no directory", "no sdf mirror", "shifted origin"])
def test_derived_structures_after_resampling_are_those_of_an_upload(hip, oracle, form):
    """Case k: the existing audit (tests/accel_terms.py) on dst straight after the call; then the resampled scene and a twin that received
    the same state through itm_upload take one further frame: every buffer stays identical, and the ray cast equals the oracle's."""
    import accel_terms as A
    key = {"no directory": 5, "no sdf mirror": 12}.get(form)
    if key:
        hip.check(hip.fn["debug_set"](key, 1), "debug_set")
    try:
        if form == "shifted origin":      # dst has placed its cubes around a frame of its own; the image of src lies far outside them
            sa = fine_a(origin=FAR)
            a, d = TM.build(hip, sa), TM.build(hip, fine_a(), frames=1)
        else:
            sa = fine_a()
            a, d = TM.build(hip, sa), empty(hip, fine_a())
        stats, state, _, _ = resample_and_compare(d.scene, a.scene, skew_q(hip), what="case k (%s)" % form)
        assert stats["allocated"] > 100
        if form == "shifted origin":
            org = np.array(d.scene.accel_info()["origin_directory"])
            pos = state["hash"]["pos"][state["hash"]["ptr"] >= 0].astype(np.int64)
            assert int(np.count_nonzero(np.any((pos < org) | (pos >= org + 512), axis=1))) > 100, "the image lies inside dst's cubes"
        A.audit(d.scene, d.rs, what="dst after the resample (%s)" % form)
        A.audit(a.scene, a.rs, what="src after the resample (%s)" % form)
        sc = fine_a()
        twin, ref = T.Session(hip, sc), T.Session(oracle, sc)
        TM.upload_state(twin, state, d); TM.upload_state(ref, state, d)
        for ses in (d, twin, ref):
            ses.sc = sc
            ses.frame(3, fused=True)
        rd, rt, ro = d.snapshot(), twin.snapshot(), ref.snapshot()
        T.assert_fields_equal(rd.hash, rt.hash, "hash")
        T.assert_fields_equal(rd.voxels, rt.voxels, "voxels")
        assert np.array_equal(rd.excess, rt.excess) and np.array_equal(rd.alloc_list, rt.alloc_list)
        assert rd.counters[0]["lastFreeBlockId"] == rt.counters[0]["lastFreeBlockId"] and rd.counters[0]["lastFreeExcessListId"] == rt.counters[0]["lastFreeExcessListId"]
        assert np.array_equal(rd.raycast, rt.raycast) and np.array_equal(rd.points, rt.points) and np.array_equal(rd.normals, rt.normals), "maps"
        assert np.array_equal(rd.raycast[..., 3], ro.raycast[..., 3]), "hit mask vs oracle"
        hit = rd.raycast[..., 3] > 0
        assert np.count_nonzero(hit) > 5000
        assert np.array_equal(rd.raycast[hit], ro.raycast[hit]) and np.array_equal(rd.points, ro.points), "ray cast vs oracle"
        A.audit(d.scene, d.rs, what="dst a frame after the resample (%s)" % form)
        a.close(); d.close(); twin.close(); ref.close()
    finally:
        if key:
            hip.check(hip.fn["debug_set"](key, 0), "debug_set")


@pytest.mark.gpu
def test_mesh_of_the_resampled_scene_is_the_mesh_of_the_uploaded_state(hip):
    """Case l: the restated state, uploaded into a twin, meshes to the same triangles, vertices and faces, bit for bit."""
    a, d = TM.build(hip, fine_a()), empty(hip, fine_a())
    d0, s0 = TM.snapshot(d.scene), TM.snapshot(a.scene)
    held = np.nonzero(s0["hash"]["ptr"] >= 0)[0][::2].astype(np.int32)
    q = skew_q(hip)
    d.scene.resample_from(a.scene, capi.RigidQ.from_dict(q), held)
    want, _, _ = R.resample(d0, s0, q, held)
    twin = T.Session(hip, fine_a())
    TM.upload_state(twin, want, d)
    meshes = []
    for ses in (d, twin):
        m = Mesh(ses.scene)
        m.MeshVolume(); m.Index()
        meshes.append((m.triangles(), m.vertices(), m.faces()))
        m.close()
    assert len(meshes[0][0]) > 1000
    for got, exp, what in zip(meshes[0], meshes[1], ("triangles", "vertices", "faces")):
        assert got.shape == exp.shape and np.array_equal(got.view(np.uint32), exp.view(np.uint32)), what
    a.close(); d.close(); twin.close()


# ---- the C++ adapters ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_cpp_resample_demo_equals_the_python_path(hip, tmp_path):
    """Case m."""
    exe = build_demo()
    got = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
    w, h, P = 160, 120, 160 * 120
    scenes = []
    for z, tx0 in ((1.5, 0.0), (1.52, -0.4)):
        s = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=SIZE, mu=MU), localBlockNum=0x2000, bucketNum=0x1000, excessNum=0x400)
        s.reco.ResetScene()
        s.set_deferred_fusion(True)
        rs = s.vis.CreateRenderState((w, h))
        depth = hip.to_backend(np.full((h, w), z, np.float32))
        pts = capi.DevBuffer(hip, P * 16, np.float32, (P, 4)); nrm = capi.DevBuffer(hip, P * 16, np.float32, (P, 4))
        for k in range(2):
            Mk = np.eye(4, dtype=np.float32); Mk[0, 3] = np.float32(tx0) - np.float32(0.01) * np.float32(k)
            v = capi.View(depth, w, h, M_d=np.ascontiguousarray(Mk.T).reshape(16), intr_d=(145.0, 145.0, 80.0, 60.0))
            s.reco.AllocateSceneFromDepth(v, rs)
            s.reco.IntegrateIntoScene(v, rs)
            s.vis.CreateExpectedDepths(v.M_d, v.intr_d, rs)
            s.vis.CreateICPMaps(v, rs, pts, nrm)
        scenes.append((s, rs))
    (a, rs_a), (c, rs_c) = scenes
    n = a.counters(rs_a)["noVisibleEntries"]
    stats = c.resample_from(a, SKEW, a.download(capi.BUF_VISIBLE_IDS, rs_a)[:n].copy())
    cnt = c.counters()
    assert stats["allocated"] > 0 and stats["resampled"] > 0 and stats["considered"] == n
    for k, v in stats.items():
        assert got[k] == v, (k, got, stats)
    assert (got["lastFreeBlockId"], got["lastFreeExcessListId"]) == (cnt["lastFreeBlockId"], cnt["lastFreeExcessListId"])
    assert got["table"] == TM.word_digest(c.download(capi.BUF_HASH_ENTRIES)) and got["voxels"] == TM.word_digest(c.download(capi.BUF_VOXEL_BLOCKS))
    for s, rs in scenes:
        rs.close(); s.close()
    # two main engines: MergeSceneFrom(other, thisFromOther) against the Python path on the scenes their frames left (itm_scene_save)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for p in dirs:
        p.mkdir()
    eng = json.loads(subprocess.run([exe, "--engines", str(dirs[0]), str(dirs[1])], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])
    pair = []
    for p in dirs:
        s = hip.create_scene(capi.VOXEL_S, capi.INDEX_HASH, capi.default_params(voxelSize=SIZE, mu=MU), localBlockNum=0x4000)
        s.reco.ResetScene()
        s.load(str(p))
        pair.append(s)
    stats = pair[0].resample_from(pair[1], SKEW)
    assert stats["allocated"] > 0 and stats["alreadyPresent"] > 0 and stats["unserved"] == 0
    for k, v in stats.items():
        assert eng[k] == v, (k, eng, stats)
    assert eng["table"] == TM.word_digest(pair[0].download(capi.BUF_HASH_ENTRIES)) and eng["voxels"] == TM.word_digest(pair[0].download(capi.BUF_VOXEL_BLOCKS))
    for s in pair:
        s.close()
