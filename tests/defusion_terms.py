"""The per-voxel de-integration (itm_deintegrate_from_scene, include/itm_hip.h) restated in numpy float32 on top of the helpers of
fusion_terms.py: the projection, the depth pixel, eta and the exits are the integration's, line for line; what follows them is the
running average run backwards.

Every array is np.float32 and every line is ONE array operation, so every operation rounds once, division is IEEE and nothing is
contracted.  Nothing here calls the oracle or the product.
"""
import numpy as np

import fusion_terms as FT

F = np.float32
FACTS = ("touched", "reset", "unobserved", "saturated", "clamped", "coloured", "colour_reset")
# the fact behind each count of itm_deintegrate_stats (blocks and visited are the caller's: they are not per-voxel decisions)
STATS = {"touched": "touched", "reset": "reset", "unobserved": "unobserved", "saturated": "saturated", "clamped": "clamped", "coloured": "coloured",
         "colourReset": "colour_reset"}


def deintegrate(voxel_type, old, ix, iy, iz, fr: FT.Frame, keep_saturated):
    """One inverse update per voxel.  `old` is a structured array of capi.VOXEL_DTYPES[voxel_type], ix / iy / iz the voxels' integer
    coordinates, fr.stop is not consulted.  Returns (new, facts): `new` a copy of `old` with the updated fields, facts a dict of
    per-voxel bool arrays
      touched       the depth part wrote sdf and w_depth (reset: ... the initial value and weight 0; clamped: ... a value that had left [-1, 1])
      unobserved    the integration would have written the voxel, its weight is 0: left alone
      saturated     ... its weight is at or above maxW and keep_saturated: left alone, colour included
      coloured      the colour part wrote clr and w_color (colour_reset: ... zeros)
    and `eta`, what the depth part returned (-1 where it left early), `would`, the voxels the integration's depth part would write, and
    `colour_gate`, the voxels that reach the cases on w_color (geometry, and not kept as saturated)."""
    short, colour = voxel_type in FT.SHORT_TYPES, voxel_type in FT.COLOUR_TYPES
    n = len(old)
    new = old.copy()
    mu = F(fr.mu)
    with np.errstate(all="ignore"):
        mx, my, mz = FT.positions(ix, iy, iz, fr.voxelSize)
        pcx, pcy, pcz = FT.transform(fr.M_d, mx, my, mz)
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
        # ---- the cases on the old weight
        oldW = old["w_depth"].astype(np.int64)
        kept = (oldW != 0) & (oldW >= int(fr.maxW)) if keep_saturated else np.zeros(n, bool)
        unobserved = would & (oldW == 0)
        saturated = would & kept
        reset = would & ~kept & (oldW == 1)
        averaged = would & ~kept & (oldW > 1)
        # ---- the running average, backwards
        oldF = FT.sdf_to_float(old["sdf"], short)
        q = eta / mu
        obs = np.where(F(1.0) < q, F(1.0), q).astype(F)             # MIN(1.0f, eta / mu)
        prod = oldW.astype(F) * oldF
        diff = prod - obs
        newF = diff / (oldW - 1).astype(F)
        lo = np.where(F(1.0) < newF, F(1.0), newF).astype(F)        # MIN(1.0f, F')
        cl = np.where(F(-1.0) < lo, lo, F(-1.0)).astype(F)          # MAX(-1.0f, .)
        clamped = averaged & (cl != newF)
        initial = FT.float_to_sdf(np.ones(n, F), short)             # SDF_initialValue()
        sdf = np.where(averaged, FT.float_to_sdf(cl, short), old["sdf"])
        new["sdf"] = np.where(reset, initial, sdf)
        new["w_depth"] = np.where(reset | averaged, np.where(reset, 0, oldW - 1).astype(np.uint8), old["w_depth"])
        facts = dict(touched=reset | averaged, reset=reset, unobserved=unobserved, saturated=saturated, clamped=clamped, coloured=np.zeros(n, bool),
                     colour_reset=np.zeros(n, bool), eta=eta, would=would, colour_gate=np.zeros(n, bool))
        if not colour:
            return new, facts
        # ---- the colour part: the integration's gate and bounds, then the same cases on w_color
        gate = ~kept & ~((eta > mu) | (np.abs(eta / mu) > F(0.25)))
        M_rgb = FT.matmul4(fr.rgb_to_depth_inv if fr.rgb_to_depth_inv is not None else np.eye(4, dtype=F).reshape(16), fr.M_d)
        qx, qy, qz = FT.transform(M_rgb, mx, my, mz)
        fxc, fyc, cxc, cyc = (F(x) for x in (fr.intr_rgb or fr.intr_d))
        hc, wc = fr.rgb.shape[:2]
        uc = fxc * qx / qz + cxc
        vc = fyc * qy / qz + cyc
        inimg = gate & ~((uc < 1) | (uc > F(wc - 2)) | (vc < 1) | (vc > F(hc - 2)))
        oldWc = old["w_color"].astype(np.int64)
        keptc = (oldWc >= (int(fr.maxW) & 0xff)) if keep_saturated else np.zeros(n, bool)          # the parameter is a uchar
        creset = inimg & (oldWc == 1) & ~keptc
        cavg = inimg & (oldWc > 1) & ~keptc
        k = np.nonzero(cavg)[0]
        wk = oldWc[k].astype(F)
        oc = old["clr"][k].astype(F) / F(255.0)
        meas = FT.bilinear(fr.rgb, uc[k], vc[k]) / F(255.0)
        nc = oc * wk[:, None]
        nc = nc - meas
        nc = nc / (wk - F(1.0))[:, None]
        x = nc * F(255.0)
        vi = np.where(x < 0, x - F(0.5), x + F(0.5)).astype(np.int64)          # TO_UCHAR3: ROUND, then clamp
        clr = new["clr"].copy()
        clr[k] = np.clip(vi, 0, 255).astype(np.uint8)
        clr[creset] = 0
        new["clr"] = clr
        wcol = new["w_color"].copy()
        wcol[k] = (oldWc[k] - 1).astype(np.uint8)
        wcol[creset] = 0
        new["w_color"] = wcol
        facts["coloured"] = creset | cavg
        facts["colour_gate"] = inimg
        facts["colour_reset"] = creset
    return new, facts


def counts(facts):
    """The per-voxel facts added up as itm_deintegrate_stats counts them."""
    return {name: int(np.count_nonzero(facts[fact])) for name, fact in STATS.items()}
