"""Restatement of itm_scene_merge (include/itm_hip.h) in plain numpy / Python over the downloaded structured arrays: a sequential
transcription of the definition -- participants in ascending src slot order, rounds of (request, ascending sweep), then the combine of
DeviceAgnostic/ITMSwappingEngine.h:7-69 in float32 in the reference's operation order.  No library is involved."""
import numpy as np

from infinitam_amd import capi

F32 = np.float32


def hash_index(pos, mask):
    """hashIndex (DeviceAgnostic/ITMRepresentationAccess.h:8-10): the coordinates sign-extend to 32 bits, the products wrap."""
    x, y, z = (int(c) & 0xffffffff for c in pos)
    return (((x * 73856093) & 0xffffffff) ^ ((y * 19349669) & 0xffffffff) ^ ((z * 83492791) & 0xffffffff)) & mask


def to_uchar(x):
    """TO_UCHAR3 per component: (int)(x +- 0.5) (truncation), then clamped to 0 .. 255."""
    half = np.where(x < 0, x - F32(0.5), x + F32(0.5)).astype(F32)
    return np.clip(np.trunc(half).astype(np.int64), 0, 255).astype(np.uint8)


def combine_voxels(src, dst, voxelType, maxW):
    """dst' = CombineVoxelInformation(src, dst) with src in the role of the stored block; structured arrays of equal shape."""
    out = dst.copy()
    short = voxelType in (capi.VOXEL_S, capi.VOXEL_S_RGB)
    oldW, newW = src["w_depth"].astype(np.int32), dst["w_depth"].astype(np.int32)
    if short:
        oldF, newF = src["sdf"].astype(F32) / F32(32767.0), dst["sdf"].astype(F32) / F32(32767.0)
    else:
        oldF, newF = src["sdf"].astype(F32), dst["sdf"].astype(F32)
    on = oldW != 0
    sumW = oldW + newW
    with np.errstate(divide="ignore", invalid="ignore"):
        f = (oldW.astype(F32) * oldF + newW.astype(F32) * newF) / sumW.astype(F32)
    if short:
        with np.errstate(invalid="ignore"):
            enc = np.trunc(np.where(on, f, F32(0)) * F32(32767.0)).astype(np.int32).astype(np.int16)      # (short)(f * 32767)
        out["sdf"] = np.where(on, enc, dst["sdf"])
    else:
        out["sdf"] = np.where(on, f, dst["sdf"])
    out["w_depth"] = np.where(on, np.minimum(sumW, maxW) & 0xff, newW).astype(np.uint8)
    if voxelType in (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB):
        oldW, newW = src["w_color"].astype(np.int32), dst["w_color"].astype(np.int32)
        on = oldW != 0
        sumW = oldW + newW
        oldC, newC = src["clr"].astype(F32) / F32(255.0), dst["clr"].astype(F32) / F32(255.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (oldC * oldW.astype(F32)[..., None] + newC * newW.astype(F32)[..., None]) / sumW.astype(F32)[..., None]
            clr = to_uchar(np.where(on[..., None], c, F32(0)) * F32(255.0))
        out["clr"] = np.where(on[..., None], clr, dst["clr"])
        out["w_color"] = np.where(on, np.minimum(sumW, maxW) & 0xff, newW).astype(np.uint8)
    return out


def state_of(scene, rs=None):
    """Everything the merge reads or writes, downloaded: a dict of arrays and the two counters."""
    c = scene.counters(rs)
    st = dict(voxels=scene.download(capi.BUF_VOXEL_BLOCKS), voxelType=int(scene.cfg.voxelType), maxW=int(scene.params.maxW),
              lastFreeBlockId=c["lastFreeBlockId"], lastFreeExcessListId=c["lastFreeExcessListId"], bucketNum=int(scene.cfg.bucketNum))
    if scene.is_hash:
        st.update(hash=scene.download(capi.BUF_HASH_ENTRIES), excess=scene.download(capi.BUF_EXCESS_LIST), alloc=scene.download(capi.BUF_ALLOCATION_LIST))
    return st


def find(pos, hpos, hoff, hptr, bucketNum):
    """(slot of the entry at `pos` or -1, request target, target is a chain tail)."""
    idx = hash_index(pos, bucketNum - 1)
    if hptr[idx] >= -1 and (hpos[idx] == pos).all():
        return idx, -1, False
    if hptr[idx] < -1:
        return -1, idx, False
    while hoff[idx] >= 1:
        idx = bucketNum + int(hoff[idx]) - 1
        if hptr[idx] >= -1 and (hpos[idx] == pos).all():
            return idx, -1, False
    return -1, idx, True


def merge(dst, src, slots=None):
    """The sequential definition.  dst / src: dicts as state_of returns.  Returns (new dst state, stats, where) -- where[src slot] is the
    dst slot of every participant that has one.  The inputs are left unchanged."""
    out = dict(dst)
    if "hash" not in dst:                         # dense index: voxel by voxel
        out["voxels"] = combine_voxels(src["voxels"], dst["voxels"], dst["voxelType"], dst["maxW"])
        return out, dict(rounds=0, considered=1, alreadyPresent=0, allocated=0, combined=1, unserved=0, srcWithoutBlock=0, dstSwappedOut=0), {}
    hpos, hoff, hptr = dst["hash"]["pos"].copy(), dst["hash"]["offset"].copy(), dst["hash"]["ptr"].copy()
    alloc, excess = dst["alloc"], dst["excess"]
    B, E, bucketNum = dst["lastFreeBlockId"], dst["lastFreeExcessListId"], dst["bucketNum"]
    sh = src["hash"]
    selected = np.arange(len(sh)) if slots is None else np.unique(np.asarray(slots, np.int64))
    assert selected.size == 0 or (selected[0] >= 0 and selected[-1] < len(sh)), "slot outside src's table"
    sptr = sh["ptr"][selected]
    participants = [int(s) for s in selected[sptr >= 0]]
    stats = dict(rounds=0, considered=len(participants), alreadyPresent=0, allocated=0, combined=0, unserved=0,
                 srcWithoutBlock=int(np.count_nonzero(sptr == -1)), dstSwappedOut=0)
    where = {}
    pending = participants
    while True:
        stats["rounds"] += 1
        requests, asking = {}, []
        for s in pending:                          # ascending: a later request on the same target overwrites the earlier one
            slot, target, tail = find(sh["pos"][s], hpos, hoff, hptr, bucketNum)
            if slot >= 0:
                where[s] = slot
                if stats["rounds"] == 1:
                    stats["alreadyPresent"] += 1
            else:
                requests[target] = (s, tail)
                asking.append(s)
        if not requests:
            break
        served = 0
        for target in sorted(requests):
            s, tail = requests[target]
            if tail:
                if B >= 0 and E >= 0:
                    ptr, off = int(alloc[B]), int(excess[E]); B -= 1; E -= 1
                    hoff[target] = off + 1
                    new = bucketNum + off
                else:
                    continue
            elif B >= 0:
                ptr = int(alloc[B]); B -= 1
                new = target
            else:
                continue
            hpos[new], hoff[new], hptr[new] = sh["pos"][s], 0, ptr
            where[s] = new
            served += 1
        stats["allocated"] += served
        pending = [s for s in asking if s not in where]
        if served == 0:
            stats["unserved"] = len(asking)
            break
    h = dst["hash"].copy()
    h["pos"], h["offset"], h["ptr"] = hpos, hoff, hptr
    vox = dst["voxels"].copy().reshape(-1, 512)
    svox = src["voxels"].reshape(-1, 512)
    pairs = [(s, d) for s, d in sorted(where.items()) if hptr[d] >= 0]
    stats["dstSwappedOut"] = len(where) - len(pairs)
    stats["combined"] = len(pairs)
    if pairs:
        sp = np.array([sh["ptr"][s] for s, _ in pairs]); dp = np.array([hptr[d] for _, d in pairs])
        vox[dp] = combine_voxels(svox[sp], vox[dp], dst["voxelType"], dst["maxW"])
    out.update(hash=h, voxels=vox.reshape(-1), lastFreeBlockId=B, lastFreeExcessListId=E)
    return out, stats, where


def assert_state_equal(got, want, what, fields_equal):
    """Whole arrays: table, voxels, the allocation list below lastFreeBlockId, the excess list below its counter, the counters."""
    assert (got["lastFreeBlockId"], got["lastFreeExcessListId"]) == (want["lastFreeBlockId"], want["lastFreeExcessListId"]), \
        "%s: counters %s vs %s" % (what, (got["lastFreeBlockId"], got["lastFreeExcessListId"]), (want["lastFreeBlockId"], want["lastFreeExcessListId"]))
    fields_equal(got["hash"], want["hash"], what + ": hash")
    fields_equal(got["voxels"], want["voxels"], what + ": voxels")
    n, m = max(want["lastFreeBlockId"] + 1, 0), max(want["lastFreeExcessListId"] + 1, 0)
    assert np.array_equal(got["alloc"][:n], want["alloc"][:n]), what + ": allocation list"
    assert np.array_equal(got["excess"][:m], want["excess"][:m]), what + ": excess list"
