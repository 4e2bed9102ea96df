"""The per-voxel fusion update restated in numpy float32, operation for operation and in the reference's order:

    computeUpdatedVoxelDepthInfo / computeUpdatedVoxelColorInfo / ComputeUpdatedVoxelInfo   DeviceAgnostic/ITMSceneReconstructionEngine.h:9-139
    interpolateBilinear                                                                     DeviceAgnostic/ITMPixelUtils.h:11-39
    Matrix4 * Vector4 (left-to-right sum of four products per row)                          ORUtils/Matrix.h:115-122
    SDF_valueToFloat / SDF_floatToValue of the short and the float encoding                 Utils/ITMLibDefines.h
    the (uchar) stores of both weights, the (uchar) maxW of the colour update, stopIntegratingAtMaxW

Every array is np.float32 and every line below is ONE array operation, so every operation rounds once, division is IEEE and nothing is
contracted.  Nothing here calls the oracle or the product: it is the third witness beside them, and because it works on plain arrays of
(position, old fields) it is also what tells a failing comparison WHICH (sdf, weight) pair went wrong, and what the coverage conditions
of tests/prepared_state_cases.py are evaluated with.
"""
from dataclasses import dataclass

import numpy as np

from infinitam_amd import capi

F = np.float32
SHORT_TYPES = (capi.VOXEL_S, capi.VOXEL_S_RGB)
COLOUR_TYPES = (capi.VOXEL_S_RGB, capi.VOXEL_F_RGB)


@dataclass
class Frame:
    """What one IntegrateIntoScene call reads beside the voxels."""
    M_d: np.ndarray                 # 16 floats, column-major world -> camera
    intr_d: tuple                   # fx, fy, cx, cy
    depth: np.ndarray               # [h, w] float32
    mu: float
    maxW: int
    stop: bool = False              # stopIntegratingAtMaxW
    voxelSize: float = 0.005
    rgb: np.ndarray = None          # [hc, wc, 4] uint8
    intr_rgb: tuple = None
    rgb_to_depth_inv: np.ndarray = None


def matmul4(lhs, rhs):
    """Matrix4 * Matrix4 (ORUtils/Matrix.h:102-108): every element accumulated from zero over k, column-major storage."""
    lhs, rhs = np.asarray(lhs, F).reshape(16), np.asarray(rhs, F).reshape(16)
    out = np.zeros(16, F)
    for col in range(4):
        for row in range(4):
            acc = F(0.0)
            for k in range(4):
                acc = F(acc + F(lhs[k * 4 + row] * rhs[col * 4 + k]))
            out[col * 4 + row] = acc
    return out


def transform(M, mx, my, mz):
    """M * (mx, my, mz, 1): ((m0 x + m4 y) + m8 z) + m12 * 1 per row -- the sum order of column_z (tests/test_integrate_uniform_paths.py)."""
    M = np.asarray(M, F).reshape(16)
    one = F(1.0)
    return tuple(((M[r] * mx + M[4 + r] * my) + M[8 + r] * mz) + M[12 + r] * one for r in range(3))


def sdf_to_float(raw, short):
    """SDF_valueToFloat: (float)(x) / 32767.0f for the short encoding, the value itself for the float one."""
    return raw.astype(F) / F(32767.0) if short else raw.astype(F)


def float_to_sdf(f, short):
    """SDF_floatToValue: (short)(x * 32767.0f) -- the conversion truncates towards zero -- or the value itself."""
    return np.trunc(f * F(32767.0)).astype(np.int32).astype(np.int16) if short else f.astype(F)


def positions(ix, iy, iz, voxelSize):
    """pt_model of integer voxel coordinates: (float)i * voxelSize."""
    vs = F(voxelSize)
    return ix.astype(F) * vs, iy.astype(F) * vs, iz.astype(F) * vs


def bilinear(img, u, v):
    """interpolateBilinear: taps b, c, d are read only where their weight is not zero, and are 0 otherwise.  Returns [n, 3]."""
    h, w = img.shape[:2]
    px, py = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    dx, dy = u - px.astype(F), v - py.astype(F)
    flat = img.reshape(-1, 4)[:, :3].astype(F)
    zero = np.zeros((len(u), 3), F)
    a = flat[px + py * w]
    b = np.where((dx != 0)[:, None], flat[np.minimum(px + 1, w - 1) + py * w], zero)
    c = np.where((dy != 0)[:, None], flat[px + np.minimum(py + 1, h - 1) * w], zero)
    d = np.where(((dx != 0) & (dy != 0))[:, None], flat[np.minimum(px + 1, w - 1) + np.minimum(py + 1, h - 1) * w], zero)
    one = F(1.0)
    ox, oy, dx, dy = (one - dx)[:, None], (one - dy)[:, None], dx[:, None], dy[:, None]
    return ((a * ox * oy + b * dx * oy) + c * ox * dy) + d * dx * dy


def integrate(voxel_type, old, ix, iy, iz, fr: Frame):
    """One ComputeUpdatedVoxelInfo per voxel.  `old` is a structured array of capi.VOXEL_DTYPES[voxel_type], ix / iy / iz the voxels'
    integer coordinates.  Returns (new, facts): `new` a copy of `old` with the updated fields, facts a dict of per-voxel arrays
      touched   the depth part wrote sdf and w_depth         coloured  the colour part wrote clr and w_color
      skipped   stopIntegratingAtMaxW kept a voxel that the depth part would have written
      eta       what computeUpdatedVoxelDepthInfo returned (-1 where it left early; garbage where `skipped`)"""
    short, colour = voxel_type in SHORT_TYPES, voxel_type in COLOUR_TYPES
    n = len(old)
    new = old.copy()
    mu = F(fr.mu)
    with np.errstate(all="ignore"):
        mx, my, mz = positions(ix, iy, iz, fr.voxelSize)
        pcx, pcy, pcz = transform(fr.M_d, mx, my, mz)
        fx, fy, cx, cy = (F(x) for x in fr.intr_d)
        h, w = fr.depth.shape
        front = ~(pcz <= 0)
        u = fx * pcx / pcz + cx
        v = fy * pcy / pcz + cy
        inside = front & ~((u < 1) | (u > F(w - 2)) | (v < 1) | (v > F(h - 2)))
        pix = np.where(inside, (u + F(0.5)).astype(np.int64) + (v + F(0.5)).astype(np.int64) * w, 0)
        dm = fr.depth.reshape(-1)[pix]
        valid = inside & ~(dm <= 0.0)
        eta = np.where(valid, dm - pcz, F(-1.0)).astype(F)
        would = valid & ~(eta < -mu)
        stopped = (old["w_depth"].astype(np.int64) == int(fr.maxW)) if fr.stop else np.zeros(n, bool)
        touched = would & ~stopped
        # ---- the running average
        oldF = sdf_to_float(old["sdf"], short)
        oldW = old["w_depth"].astype(np.int64)
        q = eta / mu
        newF = np.where(F(1.0) < q, F(1.0), q).astype(F)            # MIN(1.0f, eta / mu)
        newF = oldW.astype(F) * oldF + F(1.0) * newF
        newW = oldW + 1
        newF = newF / newW.astype(F)
        newW = np.where(newW < int(fr.maxW), newW, int(fr.maxW))
        new["sdf"] = np.where(touched, float_to_sdf(newF, short), old["sdf"])
        new["w_depth"] = np.where(touched, newW.astype(np.uint8), old["w_depth"])
        facts = dict(touched=touched, skipped=would & stopped, eta=eta, coloured=np.zeros(n, bool))
        if not colour:
            return new, facts
        # ---- the colour part: only inside a quarter of the band, and never where the depth part left with -1 (|-1 / mu| > 0.25 for mu < 4)
        gate = ~stopped & ~((eta > mu) | (np.abs(eta / mu) > F(0.25)))
        M_rgb = matmul4(fr.rgb_to_depth_inv if fr.rgb_to_depth_inv is not None else np.eye(4, dtype=F).reshape(16), fr.M_d)
        qx, qy, qz = transform(M_rgb, mx, my, mz)
        fxc, fyc, cxc, cyc = (F(x) for x in (fr.intr_rgb or fr.intr_d))
        hc, wc = fr.rgb.shape[:2]
        uc = fxc * qx / qz + cxc
        vc = fyc * qy / qz + cyc
        coloured = gate & ~((uc < 1) | (uc > F(wc - 2)) | (vc < 1) | (vc > F(hc - 2)))
        k = np.nonzero(coloured)[0]
        oldWc = old["w_color"][k].astype(F)
        oc = old["clr"][k].astype(F) / F(255.0)
        meas = bilinear(fr.rgb, uc[k], vc[k]) / F(255.0)
        nc = oc * oldWc[:, None] + meas * F(1.0)
        newWc = oldWc + F(1.0)
        nc = nc / newWc[:, None]
        maxWu = F(int(fr.maxW) & 0xff)                               # the parameter is a uchar
        newWc = np.where(newWc < maxWu, newWc, maxWu)
        x = nc * F(255.0)
        vi = np.where(x < 0, x - F(0.5), x + F(0.5)).astype(np.int64)          # TO_UCHAR3: ROUND, then clamp
        clr = new["clr"].copy()
        clr[k] = np.clip(vi, 0, 255).astype(np.uint8)
        new["clr"] = clr
        wcol = new["w_color"].copy()
        wcol[k] = newWc.astype(np.uint8)
        new["w_color"] = wcol
        facts["coloured"] = coloured
    return new, facts


def hash_coordinates(hsh, slots):
    """(pool index, ix, iy, iz) of every voxel of the table entries `slots` that hold a block (ptr >= 0), in list order."""
    e = hsh[np.asarray(slots, np.int64)]
    e = e[e["ptr"] >= 0]
    t = np.arange(512)
    pos = e["pos"].astype(np.int64).reshape(-1, 3)
    ix = (pos[:, 0:1] * 8 + (t & 7)[None, :]).reshape(-1)
    iy = (pos[:, 1:2] * 8 + ((t >> 3) & 7)[None, :]).reshape(-1)
    iz = (pos[:, 2:3] * 8 + (t >> 6)[None, :]).reshape(-1)
    idx = (e["ptr"].astype(np.int64)[:, None] * 512 + t[None, :]).reshape(-1)
    return idx, ix, iy, iz


def dense_coordinates(size, offset):
    """(ix, iy, iz) of every voxel of a dense volume in storage order (x fastest), volume offset included."""
    sx, sy, sz = size
    loc = np.arange(sx * sy * sz, dtype=np.int64)
    z = loc // (sx * sy)
    y = (loc - z * sx * sy) // sx
    x = loc - z * sx * sy - y * sx
    return x + offset[0], y + offset[1], z + offset[2]


def describe(old, new_want, new_got, limit=6):
    """Where two results differ: the old fields (the (sdf, weight) pair that failed), what was expected and what was found."""
    bad = np.zeros(len(old), bool)
    for name in old.dtype.names:
        d = new_want[name] != new_got[name]
        bad |= d.reshape(len(old), -1).any(axis=1)
    i = np.nonzero(bad)[0]
    lines = ["%d voxels differ" % len(i)]
    for j in i[:limit]:
        lines.append("  voxel %d: old %s -> expected %s, found %s" % (j, old[j], new_want[j], new_got[j]))
    return "\n".join(lines)
