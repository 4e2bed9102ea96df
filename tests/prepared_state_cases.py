"""Voxel states that no handful of frames reaches from an empty scene, and their placement in hash and dense scenes.

The tables (all deterministic):
  short sdf   2048 values: every short in [-32767, -32727], [-40, 40] and [32727, 32767], 1245 evenly spaced ones, seeded draws for the
              rest; -32768 is not among them (it is no value of the format: include/itm_hip.h, "sentinel words")
  float sdf   2048 values: 1400 of the short table (all of its three runs, every third of the rest) divided by 32767; +-1, +-0, the
              neighbours of +-1 towards 0, 0.5 +- 1 ulp, 1e-30, a denormal, 1.5, -3, 2, -1.25; seeded uniform draws in [-1, 1]; no NaN
  w_depth     every value 0 .. 255
  w_color     (7 w_depth + j) & 255 for sdf index j: every value, decorrelated from w_depth
  clr         per channel one of 0, 1, 2, 127, 128, 254, 255 (three times in ten) or a seeded draw
The state table is the full product 256 x 2048 = 524 288 (pair id = w_depth * 2048 + sdf index) under a seeded permutation: voxel i of
a prepared pool holds pair ORDER[i mod 524 288], so no field correlates with position.

Coverage is evaluated with the restatement (fusion_terms.py) alone.  A pair counts as covered when a voxel is updated WHILE IT STILL
HOLDS its prepared state, i.e. in the first frame that writes it; a later frame of the same case still finds the prepared state in
every voxel the earlier ones left alone.
"""
from dataclasses import dataclass, field

import numpy as np

import fusion_terms as FT
import itm_testlib as T
from infinitam_amd import capi, synth
from test_integrate_uniform_paths import yaw_pitch

F = np.float32
N_SDF, N_W = 2048, 256
N_PAIRS = N_SDF * N_W
W, H = 160, 120
POOL = 0x2800                  # blocks in the pool of the hash cases (the reference shim's is a compile-time constant: pool=0 there)
TYPES = {"s": capi.VOXEL_S, "f": capi.VOXEL_F, "s_rgb": capi.VOXEL_S_RGB, "f_rgb": capi.VOXEL_F_RGB}


def short_table():
    runs = np.concatenate([np.arange(-32767, -32726), np.arange(-40, 41), np.arange(32727, 32768)])
    even = np.round(np.linspace(-32700, 32700, 1245)).astype(np.int64)
    have = set(runs.tolist()) | set(even.tolist())
    rng = np.random.default_rng(20240)
    while len(have) < N_SDF:
        have.add(int(rng.integers(-32726, 32727)))
    t = np.array(sorted(have), np.int16)
    assert len(t) == N_SDF and t.min() == -32767 and t.max() == 32767
    return t


def float_table():
    s = short_table().astype(np.int64)
    run = (s <= -32727) | (np.abs(s) <= 40) | (s >= 32727)
    rest = s[~run][::3]
    from_short = np.concatenate([s[run], rest])[:1400].astype(F) / F(32767.0)
    one = F(1.0)
    special = np.array([1.0, -1.0, 0.0, -0.0, np.nextafter(one, F(0)), np.nextafter(-one, F(0)), np.nextafter(F(0.5), F(0)), np.nextafter(F(0.5), one),
                        1e-30, 1e-41, 1.5, -3.0, 2.0, -1.25], F)
    rng = np.random.default_rng(20241)
    have = {v.tobytes(): v for v in np.concatenate([from_short, special])}
    while len(have) < N_SDF:
        v = F(rng.uniform(-1.0, 1.0))
        have.setdefault(v.tobytes(), v)
    t = np.array(list(have.values()), F)
    assert len(t) == N_SDF and not np.isnan(t).any()
    return t


SHORT_TABLE, FLOAT_TABLE = short_table(), float_table()
ORDER = np.random.default_rng(20242).permutation(N_PAIRS)
_rng = np.random.default_rng(20243)
_palette = np.array([0, 1, 2, 127, 128, 254, 255], np.uint8)
CLR_TABLE = np.where(_rng.random((N_PAIRS, 3)) < 0.3, _palette[_rng.integers(0, 7, (N_PAIRS, 3))], _rng.integers(0, 256, (N_PAIRS, 3))).astype(np.uint8)


def states(voxel_type, pairs):
    """The voxels holding the given pair ids."""
    pairs = np.asarray(pairs, np.int64)
    w, j = pairs // N_SDF, pairs % N_SDF
    v = np.zeros(len(pairs), capi.VOXEL_DTYPES[voxel_type])
    v["sdf"] = (SHORT_TABLE if voxel_type in FT.SHORT_TYPES else FLOAT_TABLE)[j]
    v["w_depth"] = w
    if voxel_type in FT.COLOUR_TYPES:
        v["w_color"] = (7 * w + j) & 255
        v["clr"] = CLR_TABLE[pairs]
    return v


def fresh_pool(voxel_type, n):
    v = np.zeros(n, capi.VOXEL_DTYPES[voxel_type])
    v["sdf"] = 32767 if voxel_type in FT.SHORT_TYPES else 1.0
    return v


# ---- scenes -----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Shot:
    """One frame: the pose fed to the engines and the wall its depth image shows (a plane `dist` in front of the camera, tilted about
    the image's vertical axis; the images need not agree with the poses: parity holds for any input)."""
    M: tuple
    dist: float
    tilt: float = 0.0
    holes: bool = True


def shot(t, yaw, pitch, dist, tilt=0.0, holes=True):
    return Shot(tuple(float(x) for x in yaw_pitch(t, yaw, pitch)), dist, tilt, holes)


@dataclass
class Prepared(T.Scenario):
    w: int = W
    h: int = H
    mu: float = 0.04
    shots: tuple = ()
    frustum: tuple = (0.2, 5.0)
    sentinel: bool = False          # a few voxels of a block a ray crosses hold the word no short / float sdf may hold in a hash scene

    def params(self):
        return capi.default_params(self.voxelSize, self.mu, self.maxW, self.frustum[0], self.frustum[1], self.stopIntegratingAtMaxW)

    def pose(self, k):
        return np.array(self.shots[k].M, F)

    def depth(self, k):
        s = self.shots[k]
        fx, _, cx, _ = self.intr()
        u = np.arange(self.w, dtype=np.float64)[None, :].repeat(self.h, 0)
        d = s.dist / (1.0 - np.tan(s.tilt) * (u - cx) / fx)
        if s.holes:
            d[30:44, 50:70] = 0.0
            d[0:3, :] = -1.0
            d[100:, 140:] = 0.0
            d[77, 13] = -1.0
        return np.ascontiguousarray(d.astype(F))

    def frame_inputs(self, k):
        return FT.Frame(M_d=self.pose(k), intr_d=self.intr(), depth=self.depth(k), mu=self.mu, maxW=self.maxW, stop=self.stopIntegratingAtMaxW,
                        voxelSize=self.voxelSize, rgb=synth.rgb_frame(self.w, self.h) if self.colour else None, intr_rgb=self.intr())


# hash: a tilted wall 0.8 m away with a band of one block (8 voxels of 3 mm) on each side, then the same wall from a tilted pose
HASH_SHOTS = (shot((0.0, 0.0, 0.0), 0.0, 0.0, 0.8, tilt=0.35), shot((0.05, -0.02, 0.01), 0.12, -0.08, 0.8, tilt=0.2))
# dense: 64 x 64 x 128 voxels of 1 cm from z = 0.5 m.  Frames 0 and 1: the frustum cuts the front of the volume, the wall stands in its
# back part (free space in front of it, shadow behind it); frame 2: from further back, the wall behind the volume (every voxel free).
DENSE_SIZE, DENSE_ODD_SIZE, DENSE_OFFSET = (64, 64, 128), (66, 62, 128), (-32, -32, 50)
DENSE_SHOTS = (shot((0.0, 0.0, 0.0), 0.0, 0.0, 1.5, tilt=0.25), shot((0.03, 0.01, -0.02), 0.05, -0.03, 1.55, tilt=-0.2),
               shot((0.0, 0.0, -0.6), 0.0, 0.0, 3.2, tilt=0.0, holes=False))


def hash_scenario(kind, maxW=100, stop=False, pool=POOL, sentinel=False):
    return Prepared(name="prepared_hash_%s_%d_%d_%x%s" % (kind, maxW, stop, pool, "_sentinel" if sentinel else ""), voxelType=TYPES[kind], colour="rgb" in kind,
                    voxelSize=0.003, mu=0.024, maxW=maxW, stopIntegratingAtMaxW=stop, frames=2, shots=HASH_SHOTS, localBlockNum=pool, sentinel=sentinel)


def dense_scenario(kind, maxW=100, stop=False, size=DENSE_SIZE, sentinel=False):
    return Prepared(name="prepared_dense_%s_%d_%d_%d%s" % (kind, maxW, stop, size[0], "_sentinel" if sentinel else ""), voxelType=TYPES[kind], colour="rgb" in kind,
                    indexType=capi.INDEX_DENSE, denseSize=size, denseOffset=DENSE_OFFSET, voxelSize=0.01, mu=0.04, maxW=maxW, stopIntegratingAtMaxW=stop,
                    frames=3, shots=DENSE_SHOTS, sentinel=sentinel)


# ---- placement ----------------------------------------------------------------------------------------------------------------
@dataclass
class Placement:
    """What is uploaded into a fresh scene before frame 0, and which pair each voxel of the pool holds (-1: not prepared)."""
    sc: Prepared
    voxels: np.ndarray
    pair_of: np.ndarray
    hash: np.ndarray = None
    excess: np.ndarray = None
    alloc_list: np.ndarray = None
    visible_ids: np.ndarray = None
    visible_type: np.ndarray = None
    counters: dict = None
    blocks: int = 0
    sentinel_voxels: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))


_allocations, _placements = {}, {}


def sentinel_word(voxel_type, harmless=False):
    """-32768 / the word 0xffffffff: what the sdf mirror keeps for "no block here"; harmless: the nearest word that is a value."""
    if voxel_type in FT.SHORT_TYPES:
        return np.int16(-32767 if harmless else -32768)
    return np.array([0xfffffffe if harmless else 0xffffffff], np.uint32).view(F)[0]


def _allocation(oracle, sc):
    """Table, lists and counters after the oracle's AllocateSceneFromDepth of frame 0 in an empty scene (the same for every voxel type)."""
    key = (sc.localBlockNum, sc.voxelSize, sc.mu)
    if key not in _allocations:
        ses = T.Session(oracle, sc)
        ses.scene.reco.AllocateSceneFromDepth(ses.view(0), ses.rs)
        s, rs = ses.scene, ses.rs
        _allocations[key] = dict(hash=s.download(capi.BUF_HASH_ENTRIES), excess=s.download(capi.BUF_EXCESS_LIST), alloc_list=s.download(capi.BUF_ALLOCATION_LIST),
                                 visible_ids=s.download(capi.BUF_VISIBLE_IDS, rs), visible_type=s.download(capi.BUF_VISIBLE_TYPE, rs), counters=s.counters(rs),
                                 pool=len(s.download(capi.BUF_VOXEL_BLOCKS)))
        ses.close()
    return _allocations[key]


def placement(oracle, sc) -> Placement:
    if sc.name in _placements:
        return _placements[sc.name]
    if sc.indexType == capi.INDEX_DENSE:
        n = int(np.prod(sc.denseSize))
        pair_of = ORDER[np.arange(n) % N_PAIRS]
        p = Placement(sc, states(sc.voxelType, pair_of), pair_of)
        if sc.sentinel:      # on the optical axis of frame 0, in front of the wall
            sx, sy, _ = sc.denseSize
            p.sentinel_voxels = np.array([(60 * sy + sy // 2) * sx + sx // 2 + d for d in (0, 1, sx, sx * sy)], np.int64)
    else:
        a = _allocation(oracle, sc)
        ptrs = a["hash"]["ptr"][a["hash"]["ptr"] >= 0].astype(np.int64)          # table order
        pair_of = np.full(a["pool"], -1, np.int64)
        idx = (ptrs[:, None] * 512 + np.arange(512)[None, :]).reshape(-1)
        pair_of[idx] = ORDER[np.arange(len(idx)) % N_PAIRS]
        voxels = fresh_pool(sc.voxelType, a["pool"])
        voxels[idx] = states(sc.voxelType, pair_of[idx])
        p = Placement(sc, voxels, pair_of, a["hash"], a["excess"], a["alloc_list"], a["visible_ids"], a["visible_type"], a["counters"], len(ptrs))
        if sc.sentinel:      # the block that holds the point where the optical axis of frame 0 meets the wall
            pos = a["hash"]["pos"].astype(np.int64).reshape(-1, 3)
            at = np.floor(np.array([0.0, 0.0, sc.shots[0].dist]) / (8 * sc.voxelSize)).astype(np.int64)
            e = np.nonzero((a["hash"]["ptr"] >= 0) & np.all(pos == at, axis=1))[0]
            assert len(e) == 1, "no block on the optical axis"
            p.sentinel_voxels = int(a["hash"]["ptr"][e[0]]) * 512 + np.array([0, 73, 292, 511], np.int64)
    if sc.sentinel:
        p.voxels["sdf"][p.sentinel_voxels] = sentinel_word(sc.voxelType)
        p.pair_of = p.pair_of.copy()
        p.pair_of[p.sentinel_voxels] = -1
    _placements[sc.name] = p
    return p


def upload(ses, p: Placement, voxels=None):
    s, rs = ses.scene, ses.rs
    if p.hash is not None:
        s.upload(capi.BUF_HASH_ENTRIES, p.hash)
    s.upload(capi.BUF_VOXEL_BLOCKS, p.voxels if voxels is None else voxels)
    if p.hash is not None:
        s.upload(capi.BUF_EXCESS_LIST, p.excess)
        s.upload(capi.BUF_ALLOCATION_LIST, p.alloc_list)
        s.upload(capi.BUF_VISIBLE_IDS, p.visible_ids, rs)
        s.upload(capi.BUF_VISIBLE_TYPE, p.visible_type, rs)
        s.set_counters(rs, p.counters["lastFreeBlockId"], p.counters["lastFreeExcessListId"], p.counters["noVisibleEntries"])


def run(be, p: Placement, fused=False, deferred=True, after_last=None):
    """The case's frames on a fresh scene of `be` holding the placement: one snapshot (voxels, table, lists, counters, maps) per frame."""
    sc = p.sc
    ses = T.Session(be, sc, deferred_fusion=deferred)
    try:
        upload(ses, p)
        out = []
        for k in range(sc.frames):
            ses.frame(k, fused=fused)
            snap = ses.snapshot()
            snap.counters = [ses.scene.counters(ses.rs)]
            out.append(snap)
        if after_last:
            after_last(ses)
        return out
    finally:
        ses.close()


_oracle_runs = {}


def oracle_run(oracle, p: Placement):
    """One oracle run per case, shared by every launch form and never modified."""
    if p.sc.name not in _oracle_runs:
        _oracle_runs[p.sc.name] = run(oracle, p)
    return _oracle_runs[p.sc.name]


# ---- the restatement over a case, and the coverage it shows ---------------------------------------------------------------------------
@dataclass
class Coverage:
    blocks: int = 0
    pairs: np.ndarray = None            # [256, 2048] bool: the pair sat on a voxel that was updated while it held its prepared state
    w_color: np.ndarray = None          # [256] bool: ... whose colour was updated
    clamped_other: int = 0              # updated voxels with eta >= mu whose old sdf is not the initial value (32767 / 1.0)
    clamped_initial: int = 0            # ... whose old sdf is
    skipped: int = 0                    # kept by stopIntegratingAtMaxW although the depth part would have written them
    above_maxW: int = 0                 # updated voxels whose old weight is above maxW
    per_frame: list = field(default_factory=list)       # the restated pool after every frame

    @property
    def share(self):
        return float(self.pairs.mean())


_coverage = {}


def forget(sc):
    """Drops what is cached for a case (the cases in the reference's pool size are large and used by one test each)."""
    for d in (_placements, _coverage, _oracle_runs):
        d.pop(sc.name, None)


def restate(oracle, p: Placement, keep=True) -> Coverage:
    """Every frame of the case through fusion_terms.integrate.  The oracle is asked only for what the fusion takes as given in a hash
    scene: the table and the visible list after each frame's allocation.  keep: the restated pool after every frame stays in the result."""
    sc = p.sc
    if sc.name in _coverage:
        return _coverage[sc.name]
    cov = Coverage(blocks=p.blocks, pairs=np.zeros(N_PAIRS, bool), w_color=np.zeros(256, bool))
    vox = p.voxels.copy()
    prepared = p.pair_of >= 0
    initial = sentinel_free_initial(sc.voxelType)
    dense = sc.indexType == capi.INDEX_DENSE
    ses = None
    if not dense:
        ses = T.Session(oracle, sc)
        upload(ses, p)
    try:
        for k in range(sc.frames):
            if dense:
                idx = np.arange(len(vox))
                ix, iy, iz = FT.dense_coordinates(sc.denseSize, sc.denseOffset)
            else:
                v = ses.view(k)
                ses.scene.reco.AllocateSceneFromDepth(v, ses.rs)
                n = ses.scene.counters(ses.rs)["noVisibleEntries"]
                idx, ix, iy, iz = FT.hash_coordinates(ses.scene.download(capi.BUF_HASH_ENTRIES), ses.scene.download(capi.BUF_VISIBLE_IDS, ses.rs)[:n])
            fr = sc.frame_inputs(k)
            old = vox[idx]
            new, facts = FT.integrate(sc.voxelType, old, ix, iy, iz, fr)
            t, c = facts["touched"], facts["coloured"]
            held = prepared[idx]
            cov.pairs[p.pair_of[idx[t & held]]] = True
            if sc.colour:
                cov.w_color[old["w_color"][c & held]] = True
            clamped = t & (facts["eta"] >= F(sc.mu))
            cov.clamped_initial += int(np.count_nonzero(clamped & (old["sdf"] == initial)))
            cov.clamped_other += int(np.count_nonzero(clamped & (old["sdf"] != initial)))
            cov.skipped += int(np.count_nonzero(facts["skipped"]))
            cov.above_maxW += int(np.count_nonzero(t & (old["w_depth"] > sc.maxW)))
            prepared[idx[t | c]] = False
            vox[idx] = new
            if keep:
                cov.per_frame.append(vox.copy())
            if not dense:
                ses.scene.upload(capi.BUF_VOXEL_BLOCKS, vox)          # the oracle's next allocation does not read the voxels; kept in step anyway
    finally:
        if ses:
            ses.close()
    cov.pairs = cov.pairs.reshape(N_W, N_SDF)
    _coverage[sc.name] = cov
    return cov


def sentinel_free_initial(voxel_type):
    return np.int16(32767) if voxel_type in FT.SHORT_TYPES else F(1.0)


def assert_coverage(cov: Coverage, sc):
    """The conditions that keep a case from hiding a gap.  With stopIntegratingAtMaxW a voxel of weight maxW is never updated, by
    definition: that weight is then required among the SKIPPED voxels' instead (cov.skipped > 0 below), every other one as always."""
    weights = cov.pairs.any(axis=1)
    if sc.stopIntegratingAtMaxW:
        assert not weights[sc.maxW] and cov.skipped > 0, (sc.name, cov.skipped)
        weights[sc.maxW] = True
    assert weights.all(), (sc.name, "weights never updated", np.nonzero(~weights)[0].tolist())
    assert cov.pairs.any(axis=0).all(), (sc.name, "sdf table entries never updated", np.nonzero(~cov.pairs.any(axis=0))[0].tolist())
    assert cov.share >= 0.95, (sc.name, cov.share)
    if sc.colour:
        assert cov.w_color.all(), (sc.name, "colour weights never updated", np.nonzero(~cov.w_color)[0].tolist())
    if sc.indexType == capi.INDEX_HASH:
        assert 2048 <= cov.blocks <= 8192, (sc.name, cov.blocks)
    else:
        # The table holds the initial sdf once per weight: 256 voxels.  More than those reach the initial value only by being updated
        # (a clamped observation on weight 0 gives exactly 1.0) and are counted when a LATER frame updates them again.  With maxW 1 and
        # stopIntegratingAtMaxW no voxel is ever updated twice, and the one of weight 1 never: 255 voxels is all there can be.
        once = sc.stopIntegratingAtMaxW and sc.maxW == 1
        assert cov.clamped_other >= 20000 and cov.clamped_initial >= (200 if once else 1000), (sc.name, cov.clamped_other, cov.clamped_initial)
        if sc.stopIntegratingAtMaxW:
            assert cov.skipped >= 1000, (sc.name, cov.skipped)
        if sc.maxW < 255:          # (no uchar is above 255)
            assert cov.above_maxW >= 1000, (sc.name, cov.above_maxW)
