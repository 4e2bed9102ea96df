"""float32 numpy restatement of the pose quality counts and the tracking verdict (include/itm_hip.h: itm_pose_quality_*), term for term,
every product and sum rounded to float32 on its own:

  back-projection       pc = (d * ((x - cx) / fx), d * ((y - cy) / fy), d): the ICP tracker's order
  camera -> world       Matrix4::inv of M_d (scene_query_terms.invert4), the product left to right as Matrix4 * Vector4
  sdf, weight, flags    scene_query_terms.query_points at pw in metres, not rewritten here
  classes, residuals    include/itm_hip.h; the sums of r * r in double through math.fsum (the correctly rounded sum)
  verdict               include/itm_hip.h, compared in double

fed from downloaded scene buffers (scene_query_terms.reader_of)."""
import math

import numpy as np

import scene_query_terms as SQ

F = np.float32
UNKNOWN, NONE = F(1e30), F(-1e30)
FAILED, POOR, GOOD = 0, 1, 2
DEFAULTS = {"minWeight": 1, "minValidFraction": F(0.05), "failOverlap": F(0.10), "poorOverlap": F(0.30), "failInliers": F(0.50), "goodInliers": F(0.90)}


def default_config(mu):
    return dict(DEFAULTS, inlierDistance=F(F(0.5) * F(mu)))


def config_of(cfg):
    """a ctypes PoseQualityConfig as the dict the functions below take"""
    return {n: (int(getattr(cfg, n)) if n == "minWeight" else F(getattr(cfg, n))) for n, _ in cfg._fields_}


def reader_of(scene):
    """scene_query_terms.reader_of, also for a hash scene without a single block (straight after ResetScene): the sorted-key look-up
    needs one key to compare with, so an empty table gets a key that no block position has (they are >= 0)"""
    reader = SQ.reader_of(scene)
    if reader.dense is None and len(reader.keys) == 0:
        reader.keys, reader.ptrs = np.array([-1], np.int64), np.array([0], np.int64)
    return reader


def world_points(depth, M_d, intr):
    """(pw float32 [h * w, 3], some bool [h * w]): the back-projected pixels in the world, and which pixels are not NONE"""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    fx, fy, cx, cy = (F(a) for a in intr)
    inv = SQ.invert4(M_d)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    x, y, d = x.reshape(-1).astype(F), y.reshape(-1).astype(F), depth.reshape(-1)
    with np.errstate(all="ignore"):
        some = d > F(0)                                      # false for -1, 0 and NaN
        px = d * ((x - cx) / fx)
        py = d * ((y - cy) / fy)
        pw = np.stack([((inv[r] * px + inv[4 + r] * py) + inv[8 + r] * d) + inv[12 + r] for r in range(3)], axis=1).astype(F)
    return pw, some


def evaluate(reader, depth, M_d, intr, voxel_size, mu, cfg):
    """itm_pose_quality_evaluate -> (stats dict, residual image float32 [h, w])"""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    pw, some = world_points(depth, M_d, intr)
    with np.errstate(all="ignore"):
        q = SQ.query_points(reader, np.where(some[:, None], pw, F(0)), "metres", voxel_size, ("sdf", "weight", "flags"))
        flags = q["flags"]
        known = some & ((flags & np.uint32(1)) != 0) & ((flags & SQ.INVALID) == 0) & (q["weight"].astype(np.int64) >= int(cfg["minWeight"]))
        r = (q["sdf"] * F(mu)).astype(F)
        inlier = known & (np.abs(r) <= F(cfg["inlierDistance"]))
    image = np.where(known, r, np.where(some, UNKNOWN, NONE)).astype(F).reshape(h, w)
    sq = r.astype(np.float64) * r.astype(np.float64)
    stats = {"noPixels": w * h, "noValid": int(some.sum()), "noKnown": int(known.sum()), "noInliers": int(inlier.sum()),
             "sumSqKnown": math.fsum(sq[known]), "sumSqInliers": math.fsum(sq[inlier])}
    return stats, image


def config_refused(cfg):
    fractions = [float(cfg[n]) for n in ("minValidFraction", "failOverlap", "poorOverlap", "failInliers", "goodInliers")]
    return (not float(cfg["inlierDistance"]) > 0 or int(cfg["minWeight"]) < 1 or not all(0.0 <= f <= 1.0 for f in fractions) or
            float(cfg["failOverlap"]) > float(cfg["poorOverlap"]) or float(cfg["failInliers"]) > float(cfg["goodInliers"]))


def verdict(stats, cfg):
    """itm_pose_quality_verdict: the float32 thresholds widened to double, the counts as doubles"""
    P, V, K, I = (float(stats[n]) for n in ("noPixels", "noValid", "noKnown", "noInliers"))
    c = {n: float(F(v)) for n, v in cfg.items()}
    if V < c["minValidFraction"] * P or K < c["failOverlap"] * V or I < c["failInliers"] * K or stats["noKnown"] == 0:
        return FAILED
    if K < c["poorOverlap"] * V or I < c["goodInliers"] * K:
        return POOR
    return GOOD


# ---- the poses the tests judge ----------------------------------------------------------------------------------------------------------

def shifted(pose, tx=0.0, ty=0.0, tz=0.0):
    """the world -> camera pose with (tx, ty, tz) metres added to its translation: "+3 cm along z" puts every point 3 cm nearer"""
    m = np.array(pose, F).copy()
    m[12], m[13], m[14] = F(m[12] + F(tx)), F(m[13] + F(ty)), F(m[14] + F(tz))
    return m


def yawed(pose, yaw):
    """the pose of a camera at the same position, turned by `yaw` radians about y (synth.pose_matrix_yaw)"""
    from infinitam_amd import synth
    m = np.array(pose, F)
    return synth.pose_matrix_yaw((-m[12], -m[13], -m[14]), yaw)
