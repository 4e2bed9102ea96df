"""Restatement of itm_scene_coarsen (include/itm_hip.h) in plain numpy over the downloaded structured arrays: a transcription of the
header's definition -- blocks placed by the rounds of scene_merge_terms.merge with the participants' positions halved, then every coarse
voxel from its 27 taps in the stated order, int64 for the integer sums and float64 for the float sdf.  No library is involved."""
import numpy as np

import scene_merge_terms as M
from infinitam_amd import capi

TAPS = [(kx, ky, kz) for kz in (-1, 0, 1) for ky in (-1, 0, 1) for kx in (-1, 0, 1)]      # kz outermost, kx innermost, each ascending


def coefficient(k):
    return (2 - abs(k[0])) * (2 - abs(k[1])) * (2 - abs(k[2]))


def coarse_position(pos):
    """b >> 1 per component, arithmetic."""
    return np.asarray(pos, np.int64) >> 1


def is_short(voxelType):
    return voxelType in (capi.VOXEL_S, capi.VOXEL_S_RGB)


def has_colour(voxelType):
    return voxelType in (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB)


def default_voxels(shape, voxelType):
    """TVoxel(): sdf at its initial value, weights and colour 0."""
    v = np.zeros(shape, capi.VOXEL_DTYPES[voxelType])
    v["sdf"] = 32767 if is_short(voxelType) else 1.0
    return v


def weight_of(total, maxW):
    """min(maxW, 255, max(1, (total + 32) div 64))"""
    return np.minimum(np.minimum(np.maximum((total + 32) // 64, 1), 255), maxW)


def coarse_voxels(tap, shape, voxelType, maxW):
    """The coarse voxels of `shape`; tap(k) gives the structured array of that shape holding t_k = readVoxel(src, 2q + k) for every q."""
    short, colour = is_short(voxelType), has_colour(voxelType)
    A = np.zeros(shape, np.int64)
    S = np.zeros(shape, np.int64 if short else np.float64)
    Bc, C = np.zeros(shape, np.int64), np.zeros(tuple(shape) + (3,), np.int64)
    for k in TAPS:
        t, c = tap(k), coefficient(k)
        a = c * t["w_depth"].astype(np.int64)
        A += a
        if short:
            S += a * t["sdf"].astype(np.int64)
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                S = S + a.astype(np.float64) * t["sdf"].astype(np.float64)
        if colour:
            b = c * t["w_color"].astype(np.int64)
            Bc += b
            C += b[..., None] * t["clr"].astype(np.int64)
    out = default_voxels(shape, voxelType)
    on = A != 0
    out["w_depth"] = np.where(on, weight_of(A, maxW) & 0xff, 0)
    if short:
        assert np.abs(S).max(initial=0) < 2 ** 31
        mag = (2 * np.abs(S) + A) // np.where(on, 2 * A, 1)
        out["sdf"] = np.where(on, np.sign(S) * mag, 32767)
    else:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            out["sdf"] = np.where(on, (S / A.astype(np.float64)).astype(np.float32), np.float32(1.0))
    if colour:
        con = Bc != 0
        out["clr"] = np.where(con[..., None], (2 * C + Bc[..., None]) // np.where(con, 2 * Bc, 1)[..., None], 0)
        out["w_color"] = np.where(con, weight_of(Bc, maxW) & 0xff, 0)
    return out


def fine_blocks(src):
    """position -> voxel block of src as readVoxel finds it: entries with ptr >= 0 inside the pool (the first in slot order of a position)."""
    h, nblocks = src["hash"], len(src["voxels"]) // 512
    found = {}
    for s in np.nonzero((h["ptr"] >= 0) & (h["ptr"] < nblocks))[0]:
        found.setdefault(tuple(int(c) for c in h["pos"][s]), int(h["ptr"][s]))
    return found


def coarse_blocks(src, positions, maxW):
    """[len(positions), 512] coarse voxels of the coarse blocks at `positions`, in the block's own order x + 8 y + 64 z."""
    vt = src["voxelType"]
    found, vox = fine_blocks(src), src["voxels"].reshape(-1, 512)
    n = len(positions)
    fine = default_voxels((n, 17, 17, 17), vt)                # [block, z, y, x]: fine voxels 16B - 1 .. 16B + 15 per axis
    ranges = ((slice(0, 1), slice(7, 8)), (slice(1, 9), slice(0, 8)), (slice(9, 17), slice(0, 8)))      # (in the 17, in the fine block) for 2B - 1, 2B, 2B + 1
    for i, B in enumerate(positions):
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    ptr = found.get((2 * int(B[0]) - 1 + dx, 2 * int(B[1]) - 1 + dy, 2 * int(B[2]) - 1 + dz))
                    if ptr is not None:
                        blk = vox[ptr].reshape(8, 8, 8)
                        fine[i, ranges[dz][0], ranges[dy][0], ranges[dx][0]] = blk[ranges[dz][1], ranges[dy][1], ranges[dx][1]]

    def tap(k):      # coarse voxel l of the block: fine voxel 2 l + k is place 2 l + k + 1 of the 17
        return fine[:, 1 + k[2]:17 + k[2]:2, 1 + k[1]:17 + k[1]:2, 1 + k[0]:17 + k[0]:2]
    return coarse_voxels(tap, (n, 8, 8, 8), vt, maxW).reshape(n, 512)


def coarse_dense(src, srcSize, srcOffset, dstSize, dstOffset, voxelType, maxW):
    """Every cell of a dense dst: q = cell + dstOffset, taps through the dense readVoxel of src (absent outside its array)."""
    fine = src["voxels"].reshape(srcSize[2], srcSize[1], srcSize[0])
    q = [np.arange(dstSize[a], dtype=np.int64) + dstOffset[a] for a in range(3)]

    def tap(k):
        p = [2 * q[a] + k[a] - srcOffset[a] for a in range(3)]
        ok = [(p[a] >= 0) & (p[a] < srcSize[a]) for a in range(3)]
        t = fine[np.ix_(np.where(ok[2], p[2], 0), np.where(ok[1], p[1], 0), np.where(ok[0], p[0], 0))].copy()
        inside = ok[2][:, None, None] & ok[1][None, :, None] & ok[0][None, None, :]
        t[~inside] = default_voxels((), voxelType)
        return t
    return coarse_voxels(tap, (dstSize[2], dstSize[1], dstSize[0]), voxelType, maxW).reshape(-1)


def halved(src):
    """src's state with every position halved: what the rounds of the merge are run on."""
    s = dict(src)
    s["hash"] = src["hash"].copy()
    s["hash"]["pos"] = coarse_position(src["hash"]["pos"])
    return s


def coarsen(dst, src, slots=None, dense=None):
    """The sequential definition.  dst / src: dicts as scene_merge_terms.state_of returns.  dense: (srcSize, srcOffset, dstSize,
    dstOffset) for the dense index.  Returns (new dst state, stats, where); the inputs are left unchanged."""
    out = dict(dst)
    if "hash" not in dst:
        out["voxels"] = coarse_dense(src, *dense, dst["voxelType"], dst["maxW"])
        return out, dict(rounds=0, considered=1, alreadyPresent=0, allocated=0, written=1, unserved=0, srcWithoutBlock=0, dstSwappedOut=0), {}
    # steps 1 and 2: the merge's, on the halved positions; only the table, the counters and `where` are kept from it
    placed, ms, where = M.merge(dst, halved(src), slots)
    h = placed["hash"]
    D = sorted(set(where.values()))
    nblocks = len(dst["voxels"]) // 512
    write = [d for d in D if 0 <= h["ptr"][d] < nblocks]
    stats = dict(rounds=ms["rounds"], considered=ms["considered"], alreadyPresent=ms["alreadyPresent"], allocated=ms["allocated"], written=len(write),
                 unserved=ms["unserved"], srcWithoutBlock=ms["srcWithoutBlock"], dstSwappedOut=sum(1 for d in D if h["ptr"][d] == -1))
    vox = dst["voxels"].copy().reshape(-1, 512)
    if write:
        vox[h["ptr"][write]] = coarse_blocks(src, h["pos"][write].astype(np.int64), dst["maxW"])
    out.update(hash=h, voxels=vox.reshape(-1), lastFreeBlockId=placed["lastFreeBlockId"], lastFreeExcessListId=placed["lastFreeExcessListId"])
    return out, stats, where
