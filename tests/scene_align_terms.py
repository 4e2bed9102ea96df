"""numpy restatement of the scene alignment (include/itm_hip.h: itm_scene_band_samples, itm_aligner_evaluate, itm_aligner_align):

  band_samples        the kept voxels of a downloaded scene and their float4 samples, in the defined order (bit for bit)
  sample_terms        the 28 per-sample terms (rho, (w r) J, (w J_r) J_c packed lower-triangular) in float32, operation for operation,
                      on scene_query_terms' reader and trilinear
  sums                their sums and absolute sums in float64: what a GPU evaluation is bounded against
  align               the whole Levenberg-Marquardt loop in float64 over such evaluations
  conditioning        smallest eigenvalue of the Hessian scaled per unit (metres, radians)

and the analytic scenes the convergence tests run on: a room corner with a sphere (well posed) and a wall with a sphere (the rotation
about the wall's normal through the sphere's centre is free), as voxel arrays of a dense 64^3 volume and of the same voxels in blocks."""
import numpy as np

import mesh_attr_terms as MT
import scene_query_terms as Q
from infinitam_amd import capi

F = np.float32
KV = 28
SHORT = (capi.VOXEL_S, capi.VOXEL_S_RGB)
LAMBDA_START, LAMBDA_MAX = 1.0, 1e8


# ---- band samples -----------------------------------------------------------------------------------------------------------------------

def to_float(sdf):
    """TVoxel::SDF_valueToFloat"""
    sdf = np.asarray(sdf)
    return (sdf.astype(F) / F(32767)).astype(F) if sdf.dtype == np.int16 else sdf.astype(F)


def band_samples(voxels, voxel_size, mu, min_weight=1, max_abs_sdf=1.0, stride=1, entries=None, dense=None, slots=None):
    """float32 [count, 4] from downloaded voxels: hash (entries: the table; slots: None or the selected table slots) in ascending slot,
    then x + 8 y + 64 z; dense (dense = (size, offset)) in ascending linear index"""
    if dense is None:
        chosen = np.arange(len(entries)) if slots is None else np.unique(np.asarray(slots, np.int64))
        chosen = chosen[(entries["ptr"][chosen] >= 0) & ((entries["ptr"][chosen].astype(np.int64) + 1) * 512 <= len(voxels))]
        lin = (entries["ptr"][chosen].astype(np.int64)[:, None] * 512 + np.arange(512)[None, :]).reshape(-1)
        v = np.arange(512)
        local = np.stack([v & 7, (v >> 3) & 7, v >> 6], -1)
        pos = (entries["pos"][chosen].astype(np.int64)[:, None, :] * 8 + local[None, :, :]).reshape(-1, 3)
    else:
        (sx, sy, sz), off = dense
        lin = np.arange(sx * sy * sz, dtype=np.int64)
        pos = np.stack([lin % sx, (lin // sx) % sy, lin // (sx * sy)], -1) + np.asarray(off, np.int64)
    vox = voxels[lin]
    sdf = to_float(vox["sdf"])
    keep = (vox["w_depth"].astype(np.int64) >= min_weight) & (np.abs(sdf) < F(max_abs_sdf)) & np.all(pos % stride == 0, axis=1)
    out = np.zeros((int(keep.sum()), 4), F)
    out[:, :3] = pos[keep].astype(F) * F(voxel_size)
    out[:, 3] = sdf[keep] * F(mu)
    return out


def band_samples_of(scene, cfg, slots=None):
    """band_samples of a live scene (downloads it) under an AlignConfig"""
    voxels = scene.download(capi.BUF_VOXEL_BLOCKS)
    kw = dict(min_weight=cfg.minWeight, max_abs_sdf=cfg.maxAbsSdf, stride=cfg.stride)
    if scene.is_hash:
        return band_samples(voxels, scene.params.voxelSize, scene.params.mu, entries=scene.download(capi.BUF_HASH_ENTRIES), slots=slots, **kw)
    return band_samples(voxels, scene.params.voxelSize, scene.params.mu, dense=(tuple(scene.cfg.denseSize), tuple(scene.cfg.denseOffset)), **kw)


# ---- one evaluation ---------------------------------------------------------------------------------------------------------------------

def matrix32(M):
    """the float32 4 x 4 matrix the kernel reads (x_dst = M x_src)"""
    return np.asarray(M, np.float64).astype(F).reshape(4, 4)


def sample_terms(reader, samples, M, voxel_size, mu, delta):
    """(t float32 [n, 28], valid bool [n], huber bool [n]): the terms of every sample at dstFromSrc = M, zero rows where the sample is
    not valid; huber: valid samples in the linear part of the cost"""
    s4 = np.asarray(samples, F).reshape(-1, 4)
    M = matrix32(M)
    vs, mu, delta = F(voxel_size), F(mu), F(delta)
    p, d = s4[:, :3], s4[:, 3]
    with np.errstate(all="ignore"):
        x = [((M[k, 0] * p[:, 0] + M[k, 1] * p[:, 1]) + M[k, 2] * p[:, 2]) + M[k, 3] for k in range(3)]
        q = np.stack([x[0] / vs, x[1] / vs, x[2] / vs], -1).astype(F)
        bad = Q.invalid(q)
        q = np.where(bad[:, None], F(0), q).astype(F)
        i, c = MT.split(q)
        cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
        v, ok = [], ~bad
        for k in range(8):
            raw, found = reader.raw(i[:, 0] + (k & 1), i[:, 1] + ((k >> 1) & 1), i[:, 2] + (k >> 2))
            v.append(raw)
            ok &= found & (reader.to_float(raw) != F(1))
        s = Q.trilinear(reader, q)[0]
        one = F(1)
        gx, gy, gz = one - cx, one - cy, one - cz
        g = [reader.to_float(gz * (gy * (v[1] - v[0]) + cy * (v[3] - v[2])) + cz * (gy * (v[5] - v[4]) + cy * (v[7] - v[6]))),
             reader.to_float(gz * (gx * (v[2] - v[0]) + cx * (v[3] - v[1])) + cz * (gx * (v[6] - v[4]) + cx * (v[7] - v[5]))),
             reader.to_float(gy * (gx * (v[4] - v[0]) + cx * (v[5] - v[1])) + cy * (gx * (v[6] - v[2]) + cx * (v[7] - v[3])))]
        r = mu * s - d
        scale = F(mu / vs)
        n = [g[0] * scale, g[1] * scale, g[2] * scale]
        j = n + [x[1] * n[2] - x[2] * n[1], x[2] * n[0] - x[0] * n[2], x[0] * n[1] - x[1] * n[0]]
        a = np.abs(r)
        quad = a <= delta
        w = np.where(quad, one, delta / a).astype(F)
        rho = np.where(quad, (F(0.5) * r) * r, delta * (a - F(0.5) * delta)).astype(F)
        wr = w * r
        t = np.zeros((len(s4), KV), F)
        t[:, 0] = rho
        k = 0
        for rr in range(6):
            t[:, 1 + rr] = wr * j[rr]
            wj = w * j[rr]
            for cc in range(rr + 1):
                t[:, 7 + k] = wj * j[cc]
                k += 1
    t[~ok] = 0
    return t, ok, ok & ~quad


class Sums:
    """float64 sums of the terms, their absolute sums and the valid count"""

    def __init__(self, t, valid):
        t64 = t.astype(np.float64)
        self.n = int(valid.sum())
        self.sum64 = t64.sum(0)
        self.A = np.abs(t64).sum(0)

    @property
    def f(self):
        return self.sum64[0]

    @property
    def nabla(self):
        return self.sum64[1:7].copy()

    @property
    def hessian(self):
        """[6, 6], symmetric"""
        H = np.zeros((6, 6))
        k = 0
        for r in range(6):
            for c in range(r + 1):
                H[r, c] = H[c, r] = self.sum64[7 + k]
                k += 1
        return H


def pack(f, nabla, hessian):
    """the 28 values in the sums' order from f, nabla[6] and hessian[36] (hessian[r + c * 6])"""
    H = np.asarray(hessian, np.float64).reshape(6, 6)
    return np.concatenate([[float(f)], np.asarray(nabla, np.float64), [H[c, r] for r in range(6) for c in range(r + 1)]])


def evaluate(reader, samples, M, voxel_size, mu, delta):
    t, valid, _ = sample_terms(reader, samples, M, voxel_size, mu, delta)
    return Sums(t, valid)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------

def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def se3_exp(step):
    """the 4 x 4 matrix of the twist (v, w): Rodrigues, with series below 1e-3 as se3.h has them"""
    v, w = np.asarray(step[:3], np.float64), np.asarray(step[3:], np.float64)
    th = float(np.sqrt(w @ w))
    t2 = th * th
    if th < 1e-3:
        A = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0)
        B = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0)
        Cc = 1.0 / 6.0 - t2 / 120.0 * (1.0 - t2 / 42.0)
    else:
        A, B, Cc = np.sin(th) / th, (1.0 - np.cos(th)) / t2, (th - np.sin(th)) / (t2 * th)
    K = hat(w)
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + A * K + B * (K @ K)
    E[:3, 3] = v + B * np.cross(w, v) + Cc * np.cross(w, np.cross(w, v))
    return E


def orthonormalise(M):
    M = np.array(M, np.float64).reshape(4, 4)
    R = M[:3, :3]
    for _ in range(3):
        R = 0.5 * R @ (3.0 * np.eye(3) - R.T @ R)
    M[:3, :3] = R
    return M


def step_of(nabla, H, lam):
    """-(H + lam diag(H))^-1 nabla, a diagonal entry below 1e-15 replaced by lam * 1e-10; None when that is not positive definite"""
    A = np.array(H, np.float64)
    d = np.diag(A).copy()
    np.fill_diagonal(A, np.where(np.abs(d) < 1e-15, lam * 1e-10, d + lam * d))
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return -np.linalg.solve(A, np.asarray(nabla, np.float64))


def conditioning(H):
    """smallest eigenvalue of S H S, S = diag(a, a, a, b, b, b): 1 / a^2 the largest translational, 1 / b^2 the largest rotational
    diagonal entry"""
    H = np.asarray(H, np.float64).reshape(6, 6)
    d = np.diag(H)
    top = np.array([d[:3].max()] * 3 + [d[3:].max()] * 3)
    if not np.all(top > 0):
        return 0.0
    s = 1.0 / np.sqrt(top)
    return float(np.linalg.eigvalsh(0.5 * (H + H.T) * s[:, None] * s[None, :])[0])


def conditioning_per_parameter(H):
    """smallest eigenvalue of D^-1/2 H D^-1/2, D = diag(H): what `conditioning` is not (it cannot see a free coordinate axis)"""
    H = np.asarray(H, np.float64).reshape(6, 6)
    s = 1.0 / np.sqrt(np.diag(H))
    return float(np.linalg.eigvalsh(0.5 * (H + H.T) * s[:, None] * s[None, :])[0])


def align(evaluate_at, init, min_step=1e-5, max_evaluations=60, min_valid=100, min_conditioning=1e-3):
    """The loop of itm_aligner_align in float64 over evaluate_at(M) -> Sums.  Returns (matrix [4, 4], dict as itm_align_result)."""
    pose = orthonormalise(init)
    cur = evaluate_at(pose)
    res = dict(evaluations=1, noValid=cur.n, initialCost=cur.f / cur.n if cur.n else 0.0)
    res["finalCost"] = res["initialCost"]
    if cur.n < min_valid or cur.n <= 0:
        res.update(status=capi.ALIGN_TOO_FEW_SAMPLES, conditioning=0.0)
        return np.array(init, np.float64).reshape(4, 4), res
    lam, status = LAMBDA_START, capi.ALIGN_MAX_EVALUATIONS
    while res["evaluations"] < max_evaluations:
        step = step_of(cur.nabla, cur.hessian, lam)
        accepted = False
        if step is not None:
            if np.abs(step).max() < min_step:
                status = capi.ALIGN_CONVERGED
                break
            nxt = se3_exp(step) @ pose
            trial = evaluate_at(nxt)
            res["evaluations"] += 1
            accepted = trial.n >= min_valid and trial.n > 0 and trial.f / trial.n < cur.f / cur.n
            if accepted:
                pose, cur, lam = nxt, trial, lam * 0.1
        if not accepted:
            lam *= 10.0
            if lam > LAMBDA_MAX:
                status = capi.ALIGN_STALLED
                break
    cond = conditioning(cur.hessian)
    if cond < min_conditioning:
        status = capi.ALIGN_DEGENERATE
    res.update(status=status, noValid=cur.n, finalCost=cur.f / cur.n, conditioning=cond)
    return pose, res


def pose_error(M, truth):
    """(rotation in radians, translation in metres) of the motion M truth^-1 that is left over in dst's frame: the twist the aligner's
    steps are made of"""
    E = np.asarray(M, np.float64).reshape(4, 4) @ np.linalg.inv(np.asarray(truth, np.float64).reshape(4, 4))
    R = E[:3, :3]
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(np.sqrt(a @ a), 0.5 * (np.trace(R) - 1.0))), float(np.linalg.norm(E[:3, 3]))


# ---- analytic scenes --------------------------------------------------------------------------------------------------------------------

N, VOXEL_SIZE, MU = 64, 0.01, 0.04
SPHERE_CENTRE, SPHERE_RADIUS = np.array([0.33, 0.30, 0.25]), 0.12
PLANES = (0.06, 0.05, 0.07)                     # x, y, z = ...: the room's corner, seen from inside (the room is the greater side)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    K = hat(a / np.linalg.norm(a))
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def rigid(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M


TRUTH = rigid(rotation((1, 2, 3), np.radians(2.0)), (0.0234, -0.0167, 0.0091))      # x_dst = TRUTH x_src, exactly


def start(angle_deg, shift_mm):
    """TRUTH perturbed on the left by a rotation about (3, -1, 2) and a shift along (1, -1, 1)"""
    return rigid(rotation((3, -1, 2), np.radians(angle_deg)), np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0) * shift_mm / 1000.0) @ TRUTH


STARTS = {"3deg_15mm": start(3.0, 15.0), "10deg_40mm": start(10.0, 40.0)}


def world_sdf(X, corner=True):
    """metres, positive in free space: the minimum over the planes (all three, or z alone) and the sphere"""
    d = X[..., 2] - PLANES[2]
    if corner:
        d = np.minimum(d, np.minimum(X[..., 0] - PLANES[0], X[..., 1] - PLANES[1]))
    return np.minimum(d, np.linalg.norm(X - SPHERE_CENTRE, axis=-1) - SPHERE_RADIUS)


def analytic_voxels(voxel_type, world_from_frame=None, corner=True):
    """The 64^3 voxels (structured, linear index x + 64 (y + 64 z)) of the world seen in a frame with x_world = world_from_frame x_frame:
    behind -mu unobserved (sdf 1, weight 0), in front truncated to 1 with weight 1, in the band encoded as the voxel type encodes"""
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    X = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float64) * VOXEL_SIZE
    if world_from_frame is not None:
        X = X @ world_from_frame[:3, :3].T + world_from_frame[:3, 3]
    f = (world_sdf(X, corner) / MU).astype(F)
    behind, front = f < F(-1), f >= F(1)
    f = np.where(behind | front, F(1), f).astype(F)
    v = np.zeros(N * N * N, capi.VOXEL_DTYPES[voxel_type])
    v["sdf"] = (f * F(32767)).astype(np.int16) if voxel_type in SHORT else f      # (short)(f * 32767): truncation, as the fusion stores
    v["w_depth"] = np.where(behind, 0, 1)
    return v


def analytic_pair(voxel_type, corner=True):
    """(dst voxels, src voxels): dst in the world frame, src in the frame with x_dst = TRUTH x_src"""
    return analytic_voxels(voxel_type, None, corner), analytic_voxels(voxel_type, TRUTH, corner)


def dense_reader(voxels):
    return Q.SceneReader(voxels, dense=((N, N, N), (0, 0, 0)))
