"""numpy restatements of the tracker evaluations: the per-residual float terms of the ICP, weighted ICP and colour kernels, and two
sums of them (tests/test_tracker_terms.py).

Each restatement follows its kernel operation for operation in np.float32 -- the same order of products and sums, no fused
multiply-add (the library and the reference build with -ffp-contract=off) -- and returns a `Terms`:

  * `valid`: the residual mask in the kernel's order (raster order of the depth image, index order of the point cloud);
  * `t[i, k]`: the 28 float terms of valid residual i -- f, nabla[6], the packed lower Hessian[21] -- 0 outside the active block;
  * `sum64`: the exact sum of every column (math.fsum), the target of the kernels' double accumulation;
  * `seq32`: the sequential float32 sum in the reference's loop order (np.add.accumulate), which reproduces the reference (and the
    oracle, its bit-exact restatement) bit for bit -- that pins the restatement itself to the reference before it judges a kernel;
  * `A[k] = sum |t[i, k]|` (exact) and the count `n`.

Kernels: infinitam_amd/csrc/tracker.hip (gh_project, gh_taps, gh_blend, gh_row<MODE, WEIGHTED>, wicp_weight),
infinitam_amd/csrc/colour_tracker.hip (colour_eval_kernel, bilinear) and infinitam_amd/csrc/ren_tracker.hip (ren_eval_kernel).

Ren reads voxels from the scene's downloaded hash entries and voxel blocks (or the dense array) through its own lookup, not
through the library's mirror or block directory, so that those are checked from outside.  Its two exponentials use the host
libm's expf through ctypes: that is the function the reference's recordings were made with, and with it `seq32` reproduces
them bit for bit (tests/test_tracker_terms.py checks it).  numpy's own float32 exp is not used for Ren."""
import ctypes
import ctypes.util
import functools
import math
from dataclasses import dataclass

import numpy as np

F = np.float32
KV = 28                              # f, nabla[6], packed lower-triangular hessian[21]
MY_INF = F(0x7f800000)               # the reference's MY_INF: the integer 0x7f800000 converted to float
WICP_MIN_SIGMA_Z = F(0.0012)


def packed_index(np_):
    """(r, c) of the packed lower-triangular entries of an np_ x np_ block, in the kernels' order (k = 0, 1, ...)."""
    return [(r, c) for r in range(np_) for c in range(r + 1)]


def active(np_):
    """indices of the 28 values that an evaluation with np_ parameters writes"""
    return [0] + [1 + r for r in range(np_)] + [7 + k for k in range(np_ * (np_ + 1) // 2)]


@dataclass
class Terms:
    valid: np.ndarray        # bool, one per residual
    t: np.ndarray            # float32 [n, 28]
    np_: int                 # number of parameters (3 or 6)
    extra: dict = None       # per-residual intermediates of the valid residuals (ICP: `dist`, `u`, `v`)
    count: int = None        # the valid count where it is not the number of rows (Ren: energy rows that fail the Jacobian test)

    @property
    def n(self):
        return int(self.t.shape[0]) if self.count is None else self.count

    @property
    def rows(self):
        return int(self.t.shape[0])

    @functools.cached_property
    def sum64(self):
        return np.array([math.fsum(self.t[:, k].astype(np.float64)) for k in range(KV)])

    @functools.cached_property
    def seq32(self):
        if self.rows == 0:
            return np.zeros(KV, F)
        return np.add.accumulate(self.t, axis=0, dtype=F)[-1]

    @functools.cached_property
    def A(self):
        return np.array([math.fsum(np.abs(self.t[:, k]).astype(np.float64)) for k in range(KV)])


def transform(M, x, y, z):
    """transform_point: Matrix4 (column-major m[16]) times (x, y, z, 1), per row ((m0 x + m4 y) + m8 z) + m12 * 1, each rounded"""
    m = np.asarray(M, F).reshape(16)
    return [((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * F(1) for r in range(3)]


# ---- ICP and weighted ICP -------------------------------------------------------------------------------------------------------
def wicp_weight(sigma):
    """wicp_weight: minSigmaZ / sigma * 0.5 + 0.5 where sigma > 0, else 0"""
    s = np.asarray(sigma, F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = (WICP_MIN_SIGMA_Z / s) * F(0.5) + F(0.5)
    return np.where(s > 0, w, F(0)).astype(F)


def _blend(taps, dx, dy):
    """interpolateBilinear_withHoles on the four taps [n, 4] each: the four weighted taps added left to right"""
    a, b, c, d = taps
    odx, ody = F(1) - dx, F(1) - dy
    return [((a[:, j] * odx * ody + b[:, j] * dx * ody) + c[:, j] * odx * dy) + d[:, j] * dx * dy for j in range(4)]


def icp_terms(depth, points, normals, view_intr, scene_intr, inv_pose, scene_pose, dist_thresh, mode, weight=None):
    """computePerPointGH_Depth_Ab (weight None) or computePerPointGH_wICP (weight = the sigmaZ image of the level) for every pixel
    of `depth` [h, w], against the scene maps `points`, `normals` [sceneH, sceneW, 4]."""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    sh, sw = points.shape[:2]
    P = np.asarray(points, F).reshape(-1, 4)
    N = np.asarray(normals, F).reshape(-1, 4)
    vfx, vfy, vcx, vcy = [F(v) for v in view_intr]
    sfx, sfy, scx, scy = [F(v) for v in scene_intr]
    np_ = 6 if mode == 3 else 3
    ys, xs = np.mgrid[0:h, 0:w]
    x, y, d = xs.reshape(-1).astype(F), ys.reshape(-1).astype(F), depth.reshape(-1)
    with np.errstate(all="ignore"):
        live = ~(d <= F(1e-8))
        cx3 = d * ((x - vcx) / vfx)
        cy3 = d * ((y - vcy) / vfy)
        qx, qy, qz = transform(inv_pose, cx3, cy3, d)
        rx, ry, rz = transform(scene_pose, qx, qy, qz)
        live &= ~(rz <= F(0))
        u = sfx * rx / rz + scx
        v = sfy * ry / rz + scy
        live &= (u >= F(0)) & (u <= F(sw - 2)) & (v >= F(0)) & (v <= F(sh - 2))
        idx = np.nonzero(live)[0]
        u, v, qx, qy, qz = u[idx], v[idx], qx[idx], qy[idx], qz[idx]
        ix = np.floor(u).astype(np.int32).astype(np.int16).astype(np.int64)      # (short)floor(...)
        iy = np.floor(v).astype(np.int32).astype(np.int16).astype(np.int64)
        dx, dy = u - ix.astype(F), v - iy.astype(F)
        tap_idx = [ix + iy * sw, (ix + 1) + iy * sw, ix + (iy + 1) * sw, (ix + 1) + (iy + 1) * sw]
        tp = [P[i] for i in tap_idx]
        tn = [N[i] for i in tap_idx]
        ok = ~((tp[0][:, 3] < 0) | (tp[1][:, 3] < 0) | (tp[2][:, 3] < 0) | (tp[3][:, 3] < 0))
        cp = _blend(tp, dx, dy)
        ok &= ~(cp[3] < F(0))
        ex, ey, ez = cp[0] - qx, cp[1] - qy, cp[2] - qz
        dist = (ex * ex + ey * ey) + ez * ez
        ok &= ~(dist > F(dist_thresh))
        nhole = (tn[0][:, 3] < 0) | (tn[1][:, 3] < 0) | (tn[2][:, 3] < 0) | (tn[3][:, 3] < 0)
        nb = _blend(tn, dx, dy)
        nx, ny, nz = [np.where(nhole, F(0), c).astype(F) for c in nb[:3]]   # a hole in the normals: zero normal, still counts
        b = (nx * ex + ny * ey) + nz * ez
        if weight is not None:
            wg = wicp_weight(np.asarray(weight, F).reshape(-1)[idx])
            nx, ny, nz = nx * wg, ny * wg, nz * wg
        if mode == 2:
            Acols = [nx, ny, nz]
        else:
            Acols = [qz * ny - qy * nz, -qz * nx + qx * nz, qy * nx - qx * ny]
            if mode == 3:
                Acols += [nx, ny, nz]
        keep = np.nonzero(ok)[0]
        t = np.zeros((keep.size, KV), F)
        bb = b * b
        t[:, 0] = ((bb * wg) * wg)[keep] if weight is not None else bb[keep]
        for r in range(np_):
            t[:, 1 + r] = (b * Acols[r])[keep]
        for k, (r, c) in enumerate(packed_index(np_)):
            t[:, 7 + k] = (Acols[r] * Acols[c])[keep]
    valid = np.zeros(h * w, bool)
    valid[idx[keep]] = True
    return Terms(valid, t, np_, {"dist": dist[keep], "u": u[keep], "v": v[keep]})


def icp_f(S0, n):
    """ITMDepthTracker's f from a float sum of the squared residuals: sqrt(S0) / n, 1e5 when n <= 100"""
    return F(np.sqrt(F(S0)) / F(n)) if n > 100 else F(1e5)


def icp_seq32(terms):
    """(n, f, nabla[6], hessian[6, 6]) as the reference's ComputeGandH returns them: sequential float sums"""
    s = terms.seq32
    return terms.n, icp_f(s[0], terms.n), unpack_nabla(s, terms.np_), unpack_hessian(s, terms.np_)


def unpack_nabla(s, np_):
    g = np.zeros(6, s.dtype)
    g[:np_] = s[1:1 + np_]
    return g


def unpack_hessian(s, np_, ld=6):
    """the symmetric np_ x np_ Hessian, column-major with leading dimension ld, from the packed sums"""
    H = np.zeros((ld, ld) if ld == 6 else (np_, np_), s.dtype)
    for k, (r, c) in enumerate(packed_index(np_)):
        H[r, c] = H[c, r] = s[7 + k]
    return H


def pack(nabla, hessian, np_, ld=6):
    """the 27 gradient / packed Hessian values (index 1..27 of the 28) from an evaluation's nabla and column-major hessian"""
    H = np.asarray(hessian).reshape(-1)
    out = np.zeros(KV - 1, np.float64)
    out[:np_] = np.asarray(nabla, np.float64)[:np_]
    for k, (r, c) in enumerate(packed_index(np_)):
        out[6 + k] = H[r + c * ld]
    return out


# ---- colour ---------------------------------------------------------------------------------------------------------------------
def _bilinear_colour(src, u, v):
    """interpolateBilinear of colour_tracker.hip: the right / lower taps only where the position is not on the pixel (else 0)"""
    H, W = src.shape[:2]
    S = src.reshape(-1, 4).astype(F)
    ix, iy = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    dx, dy = u - ix.astype(F), v - iy.astype(F)
    zero = np.zeros((u.size, 4), F)
    a = S[ix + iy * W]
    b = np.where((dx != 0)[:, None], S[np.minimum(ix + 1, W - 1) + iy * W], zero)
    c = np.where((dy != 0)[:, None], S[ix + np.minimum(iy + 1, H - 1) * W], zero)
    d = np.where(((dx != 0) & (dy != 0))[:, None], S[np.minimum(ix + 1, W - 1) + np.minimum(iy + 1, H - 1) * W], zero)
    return _blend((a, b, c, d), dx, dy)


def colour_terms(locations, colours, rgb, gx, gy, intr, M, mode):
    """colour_eval_kernel for the points locations / colours [n, 4] on one level (rgb uint8, gx / gy int16 [H, W, 4]; intr: the
    level's fx, fy, cx, cy) at the world -> rgb camera matrix M (column-major)."""
    loc = np.asarray(locations, F).reshape(-1, 4)
    col = np.asarray(colours, F).reshape(-1, 4)
    H, W = rgb.shape[:2]
    fx, fy, px0, py0 = [F(v) for v in intr]
    np_ = 3 if mode == 1 else 6
    k_start = 3 if np_ == 3 else 0
    m = np.asarray(M, F).reshape(16)
    X, Y, Z, Wc = loc[:, 0], loc[:, 1], loc[:, 2], loc[:, 3]
    with np.errstate(all="ignore"):
        cx, cy, cz, cw = [((m[r] * X + m[4 + r] * Y) + m[8 + r] * Z) + m[12 + r] * Wc for r in range(4)]
        live = ~(cz <= F(0))
        u = fx * cx / cz + px0
        v = fy * cy / cz + py0
        live &= (u >= F(0)) & (u <= F(W - 1)) & (v >= F(0)) & (v <= F(H - 1))
        idx = np.nonzero(live)[0]
        u, v, cx, cy, cz, cw, kn = u[idx], v[idx], cx[idx], cy[idx], cz[idx], cw[idx], col[idx]
        obs = _bilinear_colour(rgb, u, v)
        ok = ~(obs[3] < F(254))
        ex, ey, ez = [obs[j] - F(255) * kn[:, j] for j in range(3)]
        t0 = (ex * ex + ey * ey) + ez * ez
        gxo, gyo = _bilinear_colour(gx, u, v), _bilinear_colour(gy, u, v)
        ddx, ddy, ddz = F(2) * ex, F(2) * ey, F(2) * ez
        z0 = np.zeros_like(cz)
        dcols = []
        for para in range(np_):
            case = para + k_start
            pxx, pyy, pzz = [(cw, z0, z0), (z0, cw, z0), (z0, z0, cw), (z0, -cz, cy), (cz, z0, -cx), (-cy, cx, z0)][case]
            jx = fx * ((cz * pxx - pzz * cx) / (cz * cz))
            jy = fy * ((cz * pyy - pzz * cy) / (cz * cz))
            dcols.append([jx * gxo[j] + jy * gyo[j] for j in range(3)])
        keep = np.nonzero(ok)[0]
        t = np.zeros((keep.size, KV), F)
        t[:, 0] = t0[keep]
        for para in range(np_):
            dp = dcols[para]
            t[:, 1 + para] = ((dp[0] * ddx + dp[1] * ddy) + dp[2] * ddz)[keep]
        for k, (r, c) in enumerate(packed_index(np_)):
            dr, dc = dcols[r], dcols[c]
            t[:, 7 + k] = (F(2) * ((dr[0] * dc[0] + dr[1] * dc[1]) + dr[2] * dc[2]))[keep]
    valid = np.zeros(loc.shape[0], bool)
    valid[idx[keep]] = True
    return Terms(valid, t, np_)


def colour_scale(total, valid):
    """F_oneLevel / G_oneLevel's scaleForOcclusions: noTotalPoints / valid count in float, 1 when nothing is valid"""
    return F(1) if valid == 0 else F(F(total) / F(valid))


def colour_seq32(terms, total):
    """(f, count, nabla[np], hessian[np * np] column-major) as the reference's F_oneLevel / G_oneLevel return them"""
    s = terms.seq32
    sc = colour_scale(total, terms.n)
    f = MY_INF if terms.n == 0 else F(s[0] * sc)
    np_ = terms.np_
    nab = (s[1:1 + np_] * sc).astype(F)
    Hm = unpack_hessian((s * sc).astype(F), np_, ld=np_)
    return f, terms.n, nab, Hm.T.reshape(-1)



# ---- Ren ------------------------------------------------------------------------------------------------------------------------
REN_DTUNE = F(6)
_LIBM = ctypes.CDLL(ctypes.util.find_library("m"))
_LIBM.expf.restype, _LIBM.expf.argtypes = ctypes.c_float, [ctypes.c_float]
_EXPF = np.frompyfunc(lambda v: _LIBM.expf(v), 1, 1)


def expf(x):
    """the host libm's expf, element by element"""
    x = np.asarray(x, F)
    return np.asarray(_EXPF(x), dtype=np.float64).astype(F).reshape(x.shape)


def round_ref(x):
    """(int)(x + copysign(0.5, x)): the reference's ROUND, in float, then truncation"""
    r = x + np.copysign(F(0.5), x).astype(F)
    return np.trunc(r).astype(np.int64)


class VoxelReader:
    """readVoxel at integer voxel positions from downloaded scene buffers: `entries` (HASH_ENTRY_DTYPE, every entry with ptr >= 0
    names an allocated block) and `voxels` (the voxel blocks, 512 per block) for the hash index, or `dense` = (size, offset) with
    `voxels` the dense array in x-fastest order.  Absent voxels read the default sdf (32767 short / 1.0 float), found = False."""

    def __init__(self, voxels, entries=None, dense=None):
        self.sdf = np.asarray(voxels["sdf"]).reshape(-1)
        self.short = self.sdf.dtype == np.int16
        self.dense = dense
        if dense is None:
            e = entries[entries["ptr"] >= 0]
            self.blocks = {tuple(int(c) for c in p): int(q) for p, q in zip(e["pos"], e["ptr"])}

    def raw(self, x, y, z):
        x, y, z = (np.asarray(a, np.int64) for a in (x, y, z))
        if self.dense is not None:
            (sx, sy, sz), (ox, oy, oz) = self.dense
            qx, qy, qz = x - ox, y - oy, z - oz
            found = (qx >= 0) & (qx < sx) & (qy >= 0) & (qy < sy) & (qz >= 0) & (qz < sz)
            lin = np.where(found, qx + qy * sx + qz * sx * sy, 0)
        else:
            b = np.stack([x >> 3, y >> 3, z >> 3], -1)
            uniq, inv = np.unique(b.reshape(-1, 3), axis=0, return_inverse=True)
            ptr = np.array([self.blocks.get(tuple(int(c) for c in u), -1) for u in uniq], np.int64)[inv.reshape(-1)].reshape(x.shape)
            found = ptr >= 0
            lin = np.where(found, ptr * 512 + (x & 7) + (y & 7) * 8 + (z & 7) * 64, 0)
        v = self.sdf[lin].astype(F)
        return np.where(found, v, F(32767) if self.short else F(1)).astype(F), found

    def value(self, x, y, z):
        """VX::to_float of the raw sdf: short / 32767 (IEEE division), float as it is"""
        v, found = self.raw(x, y, z)
        return (v / F(32767) if self.short else v).astype(F), found


def ren_terms(points, invM, voxel_size, reader):
    """ren_eval_kernel (GH) for the unprojected points [n, 4] at the camera -> world matrix invM (column-major).  Row i of `t` is
    every point whose voxel is not 1: its energy in column 0, and -jacobian / jacobian products where the point also passes the
    Jacobian test (found, six found neighbours != 1); the count is the number of those.  f = -sum of column 0."""
    pts = np.asarray(points, F).reshape(-1, 4)
    m = np.asarray(invM, F).reshape(16)
    oov = F(1) / F(voxel_size)
    with np.errstate(all="ignore"):
        pts = pts[pts[:, 3] > F(-1)]
        X, Y, Z, W = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
        cx, cy, cz = [((m[r] * X + m[4 + r] * Y) + m[8 + r] * Z) + m[12 + r] * W for r in range(3)]
        ix, iy, iz = round_ref(cx * oov), round_ref(cy * oov), round_ref(cz * oov)
        dt, found = reader.value(ix, iy, iz)
        rows = np.nonzero(dt != F(1))[0]
        dt, found, ix, iy, iz, cx, cy, cz = dt[rows], found[rows], ix[rows], iy[rows], iz[rows], cx[rows], cy[rows], cz[rows]
        expdt = expf(-dt * REN_DTUNE)
        t = np.zeros((rows.size, KV), F)
        t[:, 0] = (F(4) * expdt) / ((expdt + F(1)) * (expdt + F(1)))
        a = [reader.value(ix + dx_, iy + dy_, iz + dz_) for dx_, dy_, dz_ in
             ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
        ok = found.copy()
        for v, f in a:
            ok &= f & (v != F(1))
        deto = expdt + F(1)
        e2 = expf((-dt * F(2)) * REN_DTUNE)
        prefix = (F(4) * REN_DTUNE) * ((F(2) * e2) / ((deto * deto) * deto) - expdt / (deto * deto))
        dx = ((a[0][0] - a[1][0]) * F(0.5)) * prefix
        dy = ((a[2][0] - a[3][0]) * F(0.5)) * prefix
        dz = ((a[4][0] - a[5][0]) * F(0.5)) * prefix
        j = [dx, dy, dz, F(4) * (dz * cy - dy * cz), F(4) * (dx * cz - dz * cx), F(4) * (dy * cx - dx * cy)]
        for r in range(6):
            t[:, 1 + r] = np.where(ok, -j[r], F(0))
        for k, (r, c) in enumerate(packed_index(6)):
            t[:, 7 + k] = np.where(ok, j[r] * j[c], F(0))
    return Terms(np.asarray(ok), t, 6, count=int(ok.sum()))


def ren_seq32(terms):
    """(f, count, nabla[6], hessian[36]) as the reference's F_oneLevel / G_oneLevel return them: sequential float sums"""
    s = terms.seq32
    return F(-s[0]), terms.n, unpack_nabla(s, 6), unpack_hessian(s, 6).reshape(-1)
