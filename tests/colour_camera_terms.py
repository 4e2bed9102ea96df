"""One integration step restated in float64 (plain numpy, no library call): computeUpdatedVoxelInfo of
DeviceAgnostic/ITMSceneReconstructionEngine.h:9-139 for every voxel the reference's IntegrateIntoScene visits -- the blocks of the
visible list (hash) or the whole volume (dense).

The input is the scene state DOWNLOADED before the step (table, voxel blocks and visible list, or the dense volume), the view and the
scene parameters; the output is what every visited voxel must hold after it.  Each frame is therefore checked on its own, nothing
accumulates.

  depth   pc = M_d p;  u = fx pc.x / pc.z + cx, v likewise;  touched only if 1 <= u <= W - 2, 1 <= v <= H - 2, the depth at pixel
          ((int)(u + 0.5), (int)(v + 0.5)) is positive and eta = depth - pc.z >= -mu;  sdf' = (w sdf + min(1, eta / mu)) / (w + 1),
          w' = min(w + 1, maxW)
  colour  only if touched and !(eta > mu || |eta / mu| > 0.25);  pc = (calib_inv M_d) p through the RGB intrinsics;  only if
          1 <= u <= Wc - 2, 1 <= v <= Hc - 2;  four-tap bilinear blend of the Wc x Hc image;  clr' = (wc clr / 255 + blend / 255) / (wc + 1),
          stored as round-half-away(255 clr') clamped to [0, 255];  wc' = min(wc + 1, maxW & 255)

DECISIONS.  A voxel whose float64 quantity lies within 1e-4 of a decision value -- a bound of either image, a pixel-rounding half,
eta / mu at -1 or 1, |eta / mu| at 0.25 -- is left out (`undecided`): float32 may fall on the other side.  The test caps their share
of the touched voxels at 1 %.

VALUES.  Float sdf within 5e-5: camera-space z below 4 m has float32 spacing 2^-22 = 2.4e-7, the four roundings of the matrix row add
about 1e-6 in all, divided by mu = 0.02 that is 5e-5.  The short voxel types add one quantisation step, 1 / 32767.  Colour levels are
equal except at a rounding tie (255 clr' within 1e-3 of x.5), where one level is allowed.

Measured on the inputs of tests/colour_camera_cases.py, oracle (float32, the reference's operation order) against this restatement,
maxima over the three frames (tests/test_colour_camera.py::test_oracle_matches_the_restatement prints them):
(touched / coloured: summed over the frames; left out: the largest share of a frame)
  larger_213x171  hash_f_rgb   touched 998226  coloured 16580  left out 0.116 %  sdf 1.79e-05  levels: 2 ties off by one, none elsewhere
  larger_213x171  hash_s_rgb   touched 998226  coloured 16580  left out 0.116 %  sdf 4.79e-05  levels: 2 ties off by one, none elsewhere
  larger_213x171  dense_f_rgb  touched 178490  coloured  9517  left out 0.028 %  sdf 9.07e-06  levels: 1 tie off by one, none elsewhere
  smaller_96x72   hash_f_rgb   touched 998226  coloured 21042  left out 0.116 %  sdf 1.79e-05  levels: 3 ties off by one, none elsewhere
  smaller_96x72   hash_s_rgb   touched 998226  coloured 21042  left out 0.116 %  sdf 4.79e-05  levels: 3 ties off by one, none elsewhere
  smaller_96x72   dense_f_rgb  touched 178490  coloured  9877  left out 0.028 %  sdf 9.07e-06  levels: all equal
  wide_224x100    hash_f_rgb   touched 998226  coloured 24342  left out 0.116 %  sdf 1.79e-05  levels: all equal
  wide_224x100    hash_s_rgb   touched 998226  coloured 24342  left out 0.116 %  sdf 4.79e-05  levels: all equal
  wide_224x100    dense_f_rgb  touched 178490  coloured  7845  left out 0.028 %  sdf 9.07e-06  levels: all equal
The HIP kernels give the same figures (they equal the oracle bit for bit).
"""
import numpy as np

DECISION_MARGIN = 1e-4
SDF_TOL = 5e-5
SHORT_STEP = 1.0 / 32767.0
TIE_BAND = 1e-3


def _mat(m16):
    return np.asarray(m16, np.float32).astype(np.float64).reshape(4, 4).T


def _f32_matmul(a16, b16):
    """calib_inv * M_d as the engines form it: float32, column-major storage, sums in index order."""
    A, B = np.asarray(a16, np.float32).reshape(4, 4).T, np.asarray(b16, np.float32).reshape(4, 4).T
    out = np.zeros((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            acc = np.float32(0)
            for i in range(4):
                acc = np.float32(acc + np.float32(A[r, i] * B[i, c]))
            out[r, c] = acc
    return out.astype(np.float64)


def _near(x, value):
    return np.abs(x - value) < DECISION_MARGIN


def voxel_positions(state, cfg):
    """(flat indices into the voxel array, integer voxel coordinates [n, 3]) of every voxel the integration visits."""
    if "hash" in state:
        e = state["hash"][state["visible"]]
        e = e[e["ptr"] >= 0]
        loc = np.arange(512)
        inb = np.stack([loc & 7, (loc >> 3) & 7, loc >> 6], -1)                       # x + 8 y + 64 z
        idx = (e["ptr"].astype(np.int64)[:, None] * 512 + loc[None, :]).reshape(-1)
        pos = (e["pos"].astype(np.int64)[:, None, :] * 8 + inb[None, :, :]).reshape(-1, 3)
        return idx, pos
    sx, sy, sz = cfg["denseSize"]
    loc = np.arange(sx * sy * sz, dtype=np.int64)
    z, rem = loc // (sx * sy), loc % (sx * sy)
    pos = np.stack([rem % sx, rem // sx, z], -1) + np.asarray(cfg["denseOffset"], np.int64)[None, :]
    return loc, pos


def integrate(state, view, cfg):
    """state: {"voxels", and for hash scenes "hash", "visible"} as downloaded BEFORE the step.
    view: M_d, intr_d, depth [H, W] float32, rgb [Hc, Wc, 4] uint8, intr_rgb, rgb_to_depth_inv.
    cfg: voxelSize, mu, maxW (the float32 / int values of the scene), is_float, and denseSize / denseOffset for a dense volume.
    Returns a dict of per-visited-voxel arrays: idx, touched, coloured, undecided, sdf, w_depth, level (float64 [n, 3]: 255 clr'
    before rounding), w_color, and the masks out_left / out_right / out_top / out_bottom of in-band voxels outside the colour image."""
    idx, pos = voxel_positions(state, cfg)
    old = state["voxels"][idx]
    vs, mu = float(np.float32(cfg["voxelSize"])), float(np.float32(cfg["mu"]))
    p = pos.astype(np.float64) * vs              # (the engines round this product to float32: part of the 1e-6 of the derivation)
    depth, rgb = np.asarray(view["depth"]), np.asarray(view["rgb"])
    H, W = depth.shape
    Hc, Wc = rgb.shape[:2]
    fx, fy, cx, cy = [float(np.float32(v)) for v in view["intr_d"]]
    M = _mat(view["M_d"])
    pc = p @ M[:3, :3].T + M[:3, 3]
    assert pc[:, 2].min() > 0.1, "a voxel at or behind the depth camera: outside what this restatement covers"
    u = fx * pc[:, 0] / pc[:, 2] + cx
    v = fy * pc[:, 1] / pc[:, 2] + cy
    inside = (u >= 1) & (u <= W - 2) & (v >= 1) & (v <= H - 2)
    undecided = _near(u, 1) | _near(u, W - 2) | _near(v, 1) | _near(v, H - 2)
    fu, fv = u + 0.5, v + 0.5
    undecided |= inside & (_near(fu, np.round(fu)) | _near(fv, np.round(fv)))
    pu = np.clip(fu.astype(np.int64), 0, W - 1)
    pv = np.clip(fv.astype(np.int64), 0, H - 1)
    dm = depth[pv, pu].astype(np.float64)
    eta = dm - pc[:, 2]
    q = eta / mu
    touched = inside & (dm > 0) & (eta >= -mu)
    seen = inside & (dm > 0)
    undecided |= seen & (_near(q, -1) | _near(q, 1))
    if np.dtype(old["sdf"].dtype).kind == "i":
        old_sdf = old["sdf"].astype(np.float64) / 32767.0
    else:
        old_sdf = old["sdf"].astype(np.float64)
    ow = old["w_depth"].astype(np.float64)
    sdf = np.where(touched, (ow * old_sdf + np.minimum(1.0, q)) / (ow + 1.0), old_sdf)
    w_depth = np.where(touched, np.minimum(ow + 1, cfg["maxW"]), ow).astype(np.int64)
    out = {"idx": idx, "touched": touched, "sdf": sdf, "w_depth": w_depth, "eta_over_mu": q}
    if "clr" not in (old.dtype.names or ()):
        out.update(undecided=undecided, coloured=np.zeros(len(idx), bool))
        return out

    in_band = touched & ~((eta > mu) | (np.abs(q) > 0.25))
    undecided |= seen & _near(np.abs(q), 0.25)
    Mc = _f32_matmul(view["rgb_to_depth_inv"], view["M_d"])
    fxc, fyc, cxc, cyc = [float(np.float32(x)) for x in view["intr_rgb"]]
    qc = p @ Mc[:3, :3].T + Mc[:3, 3]
    assert qc[in_band, 2].min(initial=1.0) > 0.1, "a voxel at or behind the colour camera: no test may reach that"
    uc = fxc * qc[:, 0] / qc[:, 2] + cxc
    vc = fyc * qc[:, 1] / qc[:, 2] + cyc
    inside_c = (uc >= 1) & (uc <= Wc - 2) & (vc >= 1) & (vc <= Hc - 2)
    undecided |= in_band & (_near(uc, 1) | _near(uc, Wc - 2) | _near(vc, 1) | _near(vc, Hc - 2))
    coloured = in_band & inside_c
    px = np.clip(np.floor(uc).astype(np.int64), 0, Wc - 2)
    py = np.clip(np.floor(vc).astype(np.int64), 0, Hc - 2)
    dx, dy = (uc - px)[:, None], (vc - py)[:, None]
    img = rgb[..., :3].astype(np.float64)
    blend = (img[py, px] * (1 - dx) * (1 - dy) + img[py, px + 1] * dx * (1 - dy) + img[py + 1, px] * (1 - dx) * dy + img[py + 1, px + 1] * dx * dy)
    owc = old["w_color"].astype(np.float64)[:, None]
    oclr = old["clr"].astype(np.float64)
    level = np.where(coloured[:, None], (oclr / 255.0 * owc + blend / 255.0) / (owc + 1.0) * 255.0, oclr)
    w_color = np.where(coloured, np.minimum(owc[:, 0] + 1, cfg["maxW"] & 255), owc[:, 0]).astype(np.int64)
    out.update(undecided=undecided, coloured=coloured, level=level, w_color=w_color,
               out_left=in_band & (uc < 1), out_right=in_band & (uc > Wc - 2), out_top=in_band & (vc < 1), out_bottom=in_band & (vc > Hc - 2))
    return out


def compare(terms, before, after, what=""):
    """Holds `after` (the voxel array downloaded after the step) against the restatement.  Returns the measured figures:
    {"visited", "touched", "coloured", "left_out", "left_out_share", "sdf_max", "level_max", "ties_off_by_one"}; asserts the rules of the
    module docstring."""
    idx = terms["idx"]
    old, new = before[idx], after[idx]
    ok = ~terms["undecided"]
    is_short = np.dtype(new["sdf"].dtype).kind == "i"
    changed = (new["sdf"] != old["sdf"]) | (new["w_depth"] != old["w_depth"])
    # whether a voxel was touched shows in its weight (below the cap it grows by one with every touch)
    assert int(old["w_depth"].max(initial=0)) < 100, "weights at the cap: a touch would not show"
    got_touched = new["w_depth"] != old["w_depth"]
    bad = ok & (got_touched != terms["touched"])
    assert not bad.any(), f"{what}: {int(bad.sum())} decided voxels differ in whether they are touched, first {np.nonzero(bad)[0][:5]}"
    assert not (ok & ~terms["touched"] & changed).any(), f"{what}: an untouched voxel changed"
    sel = ok & terms["touched"]
    assert np.array_equal(new["w_depth"][sel], terms["w_depth"][sel]), f"{what}: depth weights"
    got_sdf = new["sdf"].astype(np.float64) / 32767.0 if is_short else new["sdf"].astype(np.float64)
    sdf_err = np.abs(got_sdf - terms["sdf"])[sel]
    tol = SDF_TOL + (SHORT_STEP if is_short else 0.0)
    fig = {"visited": int(len(idx)), "touched": int(terms["touched"].sum()), "coloured": int(terms["coloured"].sum()),
           "left_out": int((terms["undecided"] & (terms["touched"] | got_touched)).sum()), "sdf_max": float(sdf_err.max(initial=0.0)),
           "level_max": 0, "ties_off_by_one": 0}
    fig["left_out_share"] = fig["left_out"] / max(fig["touched"], 1)
    assert fig["sdf_max"] <= tol, f"{what}: sdf differs by {fig['sdf_max']:.3g} (allowed {tol:.3g})"
    if "level" in terms:
        got_coloured = new["w_color"] != old["w_color"]
        bad = ok & (got_coloured != terms["coloured"])
        assert not bad.any(), f"{what}: {int(bad.sum())} decided voxels differ in whether they are coloured, first {np.nonzero(bad)[0][:5]}"
        unc = ok & ~terms["coloured"]
        assert np.array_equal(new["clr"][unc], old["clr"][unc]), f"{what}: an uncoloured voxel changed its colour"
        sel = ok & terms["coloured"]
        assert np.array_equal(new["w_color"][sel], terms["w_color"][sel]), f"{what}: colour weights"
        L = terms["level"][sel]
        want = np.clip(np.floor(L + 0.5), 0, 255).astype(np.int64)
        diff = np.abs(new["clr"][sel].astype(np.int64) - want)
        tie = np.abs(L - np.floor(L) - 0.5) < TIE_BAND
        fig["level_max"] = int(diff.max(initial=0))
        fig["ties_off_by_one"] = int((diff[tie] == 1).sum())
        print(f"{what}: colour levels: max difference {fig['level_max']}, {fig['ties_off_by_one']} ties off by one of {int(tie.sum())} ties")
        assert not (diff[~tie] != 0).any(), f"{what}: {int((diff[~tie] != 0).sum())} colour levels differ away from a rounding tie (max {int(diff[~tie].max())})"
        assert diff.max(initial=0) <= 1, f"{what}: a colour level differs by {int(diff.max())} at a tie"
    print(f"{what}: {fig}")
    assert fig["left_out_share"] <= 0.01, f"{what}: {fig['left_out_share']:.2%} of the touched voxels left out as undecided"
    return fig
