"""Hash integration: the decisions a wave makes once for a whole item, against the per-voxel code they replace.

What ships (profiles/integrate_uniform_notes.md): ONE range decision per item -- both ends of every lane's column of pc.z values inside
[1e-4, 1e4] -- after which the projection runs without the pc.z <= 0 exit and without its IEEE-division side.  The host tests restate
that decision in float32 and check it against every voxel of blocks placed at the bounds; they also keep the two identities the
measured-and-dropped steps rested on (the free-space average, the table of weight reciprocals), so that whoever takes those steps up
again starts from a checked statement.  The GPU tests compare voxels, weights, lists and maps bit for bit with the oracle and audit
the sdf mirror against the voxels, on scenes built for the paths: a wall seen head-on again and again (every slice in front of it is
observed free space that is free already), the same wall tilted, both alternating, holes, half-observed blocks, and scenes scaled so
that blocks straddle pc.z = 1e-4, 1e4 and 0.  There are no per-path counters in the product: which path a scene reaches is asserted
by construction, from the final block table and the pose, with the same float32 restatement.
"""
from dataclasses import dataclass
from fractions import Fraction

import numpy as np
import pytest

import accel_terms as A
import itm_testlib as T
from itm_testlib import Scenario
from infinitam_amd import capi, synth

F = np.float32
W, H = 64, 48


# ---- the decision, restated ------------------------------------------------------------------------------------------
def column_z(M, pos, voxelSize, slices=range(8)):
    """pc.z of the 64 lanes x the given slices of block `pos`, in the kernel's operation order: ((m2 x + m6 y) + m10 z) + m14."""
    M = np.asarray(M, F)
    vs = F(voxelSize)
    lane = np.arange(64)
    mx = ((pos[0] * 8 + (lane & 7)).astype(F) * vs)[:, None]
    my = ((pos[1] * 8 + (lane >> 3)).astype(F) * vs)[:, None]
    mz = ((pos[2] * 8 + np.asarray(list(slices))).astype(F) * vs)[None, :]
    with np.errstate(all="ignore"):
        return ((M[2] * mx + M[6] * my) + M[10] * mz) + M[14] * F(1.0)


def in_normal_range(z):
    return (z >= F(1e-4)) & (z <= F(1e4))


def item_in_range(M, pos, voxelSize, z0=0, n=8):
    """The kernel's decision for the item (block `pos`, slices z0 .. z0 + n - 1): both END slices of every lane in range."""
    ends = column_z(M, pos, voxelSize, (z0, z0 + n - 1))
    return bool(in_normal_range(ends).all())


def yaw_pitch(t, yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = -(R @ np.asarray(t, np.float64))
    return np.ascontiguousarray(m.T.astype(F)).reshape(16)


# ---- host-only ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxW", [1, 100, 255])
def test_free_space_average_leaves_32767_and_counts_the_weight(maxW):
    """computeUpdatedVoxelDepthInfo for a voxel holding sdf 32767 and an observation clamped to 1, in float32, every weight 0 .. 255."""
    for w in range(256):
        oldF = F(32767) / F(32767)
        newF = F(w) * oldF + F(1) * F(1.0)
        newW = w + 1
        assert newF == F(newW), w
        newF = newF / F(newW)
        assert newF == F(1.0), w
        assert int(np.int16(newF * F(32767.0))) == 32767, w
        assert min(newW, maxW) == (newW if newW < maxW else maxW)


def test_weight_reciprocals_by_float_division_are_correctly_rounded():
    """The 256 entries 1.0f / (float)w, w = 1 .. 256: each is the float nearest to 1 / w (what refined_rcp gives, test_hip_parity.py)."""
    table = F(1.0) / np.arange(1, 257).astype(F)
    for w in range(1, 257):
        t = table[w - 1]
        exact = Fraction(1, w)
        err = abs(Fraction(float(t)) - exact)
        for other in (np.nextafter(t, F(0)), np.nextafter(t, F(2))):
            assert err <= abs(Fraction(float(other)) - exact), w


def _blocks_at(zc, voxelSize):
    """Block positions around camera-space depth zc on and beside the optical axis (identity rotation, camera at the origin)."""
    bz = int(np.floor(zc / (8 * voxelSize)))
    return [(bx, by, bz + dz) for bx in (-2, -1, 0, 1) for by in (-1, 0) for dz in (-2, -1, 0, 1, 2)]


@pytest.mark.parametrize("bound,voxelSize", [(1e-4, 1e-5), (1e-4, 3e-6), (1e4, 50.0), (1e4, 7.0), (0.0, 0.01), (0.0, 1e-5)])
def test_end_slices_decide_for_every_voxel_of_blocks_at_the_bounds(bound, voxelSize):
    """Exhaustive: for blocks below, across and above a bound, under straight and rotated poses, the decision from the two end
    slices is TRUE exactly when every one of the 512 voxels is in range (so a block across pc.z = 0, 1e-4 or 1e4 takes the per-voxel
    code and a block just inside does not), for whole blocks and for the half blocks of the 8- and 12-byte voxel types."""
    rng = np.random.default_rng(int(voxelSize * 1e7) + int(bound))
    poses = [synth.pose_matrix((0.0, 0.0, 0.0)), synth.pose_matrix((0.0, 0.0, 0.37 * voxelSize)), synth.pose_matrix((3 * voxelSize, -voxelSize, -2.6 * voxelSize))]
    poses += [yaw_pitch(rng.normal(size=3) * voxelSize, rng.uniform(-0.6, 0.6), rng.uniform(-0.6, 0.6)) for _ in range(12)]
    seen = {True: 0, False: 0}
    for M in poses:
        for pos in _blocks_at(bound, voxelSize):
            pos = np.asarray(pos)
            for z0, n in ((0, 8), (0, 4), (4, 4)):
                every = bool(in_normal_range(column_z(M, pos, voxelSize, range(z0, z0 + n))).all())
                decided = item_in_range(M, pos, voxelSize, z0, n)
                assert decided == every, (bound, voxelSize, pos.tolist(), z0, n)
                seen[decided] += 1
    assert seen[True] and seen[False], seen


def test_columns_of_pc_z_are_monotone_under_random_poses():
    """What the decision rests on: along a lane's column the rounded pc.z never leaves the interval of its two end values."""
    rng = np.random.default_rng(7)
    for _ in range(300):
        vs = float(10.0 ** rng.uniform(-5, 1.5))
        M = yaw_pitch(rng.normal(size=3) * vs * 40, rng.uniform(-3.1, 3.1), rng.uniform(-1.5, 1.5))
        pos = rng.integers(-300, 300, size=3)
        z = column_z(M, pos, vs)
        lo, hi = np.minimum(z[:, 0], z[:, 7])[:, None], np.maximum(z[:, 0], z[:, 7])[:, None]
        assert ((z >= lo) & (z <= hi)).all()


# ---- scenes ---------------------------------------------------------------------------------------------------------------
@dataclass
class Wall(Scenario):
    """A plane `dist` in front of the camera, tilted about the image's vertical axis by tilts[k] in frame k (cycled); the camera
    looks along +z from (0, 0, cam_z[k]).  The depth images need not agree with the poses: parity holds for any input."""
    w: int = W
    h: int = H
    voxelSize: float = 0.02
    mu: float = 0.08
    dist: float = 0.8
    tilts: tuple = (0.0,)
    cam_z: tuple = (0.0,)
    holes: bool = False
    half_until: int = 0          # frames before this one see the left half of the image only
    frustum: tuple = (0.35, 3.0)

    def params(self):
        return capi.default_params(self.voxelSize, self.mu, self.maxW, self.frustum[0], self.frustum[1], self.stopIntegratingAtMaxW)

    def pose(self, k):
        return synth.pose_matrix((0.0, 0.0, self.cam_z[k % len(self.cam_z)]))

    def depth(self, k):
        fx, _, cx, _ = self.intr()
        u = np.arange(self.w, dtype=np.float64)[None, :].repeat(self.h, 0)
        d = self.dist / (1.0 - np.tan(self.tilts[k % len(self.tilts)]) * (u - cx) / fx)
        if self.holes:
            d[10:30, 20:44] = 0.0
            d[0:7, :] = -1.0
            d[40:, 50:] = 0.0
        if k < self.half_until:
            d[:, self.w // 2:] = 0.0
        return np.ascontiguousarray(d.astype(F))


def run_and_compare(hip, oracle, sc, fused):
    """fused=False: every engine call launched on its own (integrate_hash_kernel); fused="four": the four calls recorded and
    launched as the fused frame (integrate_project_kernel).  The mirror is audited against the voxels after the last frame."""
    facts = {}

    def hook(k, ses):
        if k == sc.frames - 1:
            facts.update(A.audit(ses.scene, ses.rs, what=sc.name))
    a = T.run_scenario(hip, sc, fused=fused, per_frame_hook=hook)
    b = _oracle_result(oracle, sc)
    T.compare_results(a, b, sc, what="%s/%s" % (sc.name, fused))
    return a, facts


_oracle_cache = {}


def _oracle_result(oracle, sc):
    """One oracle run per scenario, shared by the launch forms and never modified."""
    if sc.name not in _oracle_cache:
        _oracle_cache[sc.name] = T.run_scenario(oracle, sc)
    return _oracle_cache[sc.name]


def items_by_decision(res, sc):
    """(items in range, other items) among the allocated blocks under the LAST frame's pose, by the float32 restatement."""
    M = sc.pose(sc.frames - 1)
    n = 8 if sc.voxelType == T.VOXEL_S else 4
    inr = out = 0
    hsh = res.hash[res.hash["ptr"] >= 0]
    for pos in hsh["pos"]:
        for z0 in range(0, 8, n):
            if item_in_range(M, np.asarray(pos, np.int64), sc.voxelSize, z0, n):
                inr += 1
            else:
                out += 1
    return inr, out


FORMS = [False, "four"]
MAXW = 4
HEAD_ON = Wall(name="wall_head_on", maxW=MAXW, frames=MAXW + 5)
HEAD_ON_STOP = Wall(name="wall_head_on_stop", maxW=MAXW, frames=MAXW + 5, stopIntegratingAtMaxW=True)
TILTED = Wall(name="wall_tilted", tilts=(np.pi / 6,), frames=4)
ALTERNATING = Wall(name="wall_alternating", tilts=(0.0, np.pi / 6, 0.0, -np.pi / 6, 0.0, 0.0), frames=6, maxW=3)
HOLES = Wall(name="wall_with_holes", holes=True, frames=4, maxW=3)
HALF_FIRST = Wall(name="wall_half_first", half_until=2, frames=5)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", FORMS, ids=["separate", "fused"])
@pytest.mark.parametrize("sc", [HEAD_ON, HEAD_ON_STOP, TILTED, ALTERNATING, HOLES, HALF_FIRST], ids=lambda s: s.name)
def test_walls_match_the_oracle(hip, oracle, sc, fused):
    """Free space in front of a wall, observed again and again (weights 1 .. maxW, then saturated, with and without
    stopIntegratingAtMaxW); no slice uniform (tilted); blocks changing between the two from frame to frame; invalid depth over part
    of a block's footprint; half of a block's footprint observed in earlier frames only (unequal weights within a slice)."""
    a, _ = run_and_compare(hip, oracle, sc, fused)
    inr, out = items_by_decision(a, sc)
    assert inr > 20 and out == 0, (inr, out)                 # every block of these scenes is projected without the per-voxel tests
    w = a.voxels["w_depth"].reshape(-1, 512)[a.hash["ptr"][a.hash["ptr"] >= 0]]
    assert w.max() == min(sc.maxW, sc.frames), (int(w.max()), sc.maxW, sc.frames)
    if sc is HALF_FIRST:
        assert len(np.unique(w[w > 0])) >= 2


NEAR = Wall(name="blocks_across_1e-4", voxelSize=1e-5, mu=6e-5, dist=1.5e-4, frustum=(1e-6, 1.0), frames=3)
FAR = Wall(name="blocks_across_1e4", voxelSize=50.0, mu=200.0, dist=1e4, frustum=(1.0, 3e4), frames=3)
ACROSS_ZERO = Wall(name="blocks_across_zero", voxelSize=1e-5, mu=6e-5, dist=1.5e-4, frustum=(1e-6, 1.0), cam_z=(0.0, 6e-5, 1.1e-4), frames=3)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", FORMS, ids=["separate", "fused"])
@pytest.mark.parametrize("sc", [NEAR, FAR, ACROSS_ZERO], ids=lambda s: s.name)
def test_blocks_at_the_range_bounds_match_the_oracle(hip, oracle, sc, fused):
    """Scenes scaled so that allocated blocks lie below, across and above pc.z = 1e-4 / 1e4 / 0: items across a bound run the
    per-voxel code (IEEE divisions, the pc.z <= 0 exit), items inside run the short projection -- both kinds must be present."""
    a, _ = run_and_compare(hip, oracle, sc, fused)
    inr, out = items_by_decision(a, sc)
    assert inr > 0 and out > 0, (inr, out)


TYPES = [(T.VOXEL_S, False), (T.VOXEL_F, False), (T.VOXEL_S_RGB, True), (T.VOXEL_F_RGB, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("fused", FORMS, ids=["separate", "fused"])
@pytest.mark.parametrize("voxel,colour", TYPES, ids=["s", "f", "s_rgb", "f_rgb"])
def test_every_voxel_type(hip, oracle, voxel, colour, fused):
    sc = Wall(name="types_%d" % voxel, voxelType=voxel, colour=colour, tilts=(0.0, np.pi / 6, 0.0), frames=4, maxW=3, holes=True)
    run_and_compare(hip, oracle, sc, fused)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", FORMS, ids=["separate", "fused"])
@pytest.mark.parametrize("voxel,colour", TYPES[0:1] + TYPES[2:3], ids=["s", "s_rgb"])
def test_short_types_with_the_paged_mirror(hip, oracle, voxel, colour, fused, monkeypatch):
    monkeypatch.setenv("ITM_MIRROR", "paged")
    sc = Wall(name="types_%d" % voxel, voxelType=voxel, colour=colour, tilts=(0.0, np.pi / 6, 0.0), frames=4, maxW=3, holes=True)
    _, facts = run_and_compare(hip, oracle, sc, fused)
    assert facts["form"] == "paged", facts["form"]
