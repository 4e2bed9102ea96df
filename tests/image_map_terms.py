"""The three colour maps of the display path restated in float32 numpy, operation for operation in the order of the reference's
host loops (IITMVisualisationEngine::DepthToUchar4 / WeightToUchar4 / NormalToUchar4, Engine/ITMVisualisationEngine.cpp:7-107):
what the kernels of infinitam_amd/csrc/image_maps.hip are compared with, byte for byte.  tests/golden/g_image_maps.* holds what
the reference's own functions give on the inputs of tests/image_map_cases.py; this restatement must reproduce it.

Every operation below is one float32 numpy operation on float32 operands, so every intermediate is rounded to float32 once, as in
the reference built without contraction.  The float -> uchar conversion truncates inside [0, 256) as the reference's cast does;
outside (undefined there) it saturates to 0 / 255 and NaN gives 0, as the kernels do."""
import hashlib

import numpy as np

F = np.float32


def sha256(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def to_uchar(x):
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        y = np.where(np.isnan(x), F(0), np.minimum(np.maximum(x, F(0)), F(255)))
    return y.astype(np.uint8)          # truncation: the operand lies in [0, 255]


def in_conversion_range(x) -> bool:
    """True when every value is one the reference's (uchar) cast is defined for."""
    x = np.asarray(x, F)
    return bool(np.all((x > F(-1)) & (x < F(256))))


def _interpolate(val, y0, x0, y1, x1):
    # (val - x0) * (y1 - y0) / (x1 - x0) + y0: subtract, multiply, divide, add
    return (val - F(x0)) * (F(y1) - F(y0)) / (F(x1) - F(x0)) + F(y0)


def base(val):
    """The chain of <= tests in the reference's order; a NaN fails every test and ends in the final 0."""
    val = np.asarray(val, F)
    with np.errstate(invalid="ignore"):
        return np.select([val <= F(-0.75), val <= F(-0.25), val <= F(0.25), val <= F(0.75)],
                         [F(0), _interpolate(val, 0.0, -0.75, 1.0, -0.25), F(1), _interpolate(val, 1.0, 0.25, 0.0, 0.75)], F(0)).astype(F)


def depth_limits(src):
    """(lo, hi) of DepthToUchar4: MIN / MAX over the pixels > 0 from (100000, -100000)."""
    v = np.asarray(src, F).reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = v[v > F(0)]
    lo, hi = F(100000.0), F(-100000.0)
    if len(valid):
        lo, hi = min(lo, valid.min()), max(hi, valid.max())
    return F(lo), F(hi)


def weight_limit(src):
    v = np.asarray(src, F).reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = v[v > F(0)]
    return F(min(F(1000.0), valid.min())) if len(valid) else F(1000.0)


def depth_to_uchar4(src, parts=None):
    """src (h, w) float32 -> (h, w, 4) uint8.  parts: a dict that receives the float values handed to the conversion."""
    src = np.asarray(src, F)
    out = np.zeros(src.shape + (4,), np.uint8)
    lo, hi = depth_limits(src)
    with np.errstate(all="ignore"):
        scale = F(1) / (hi - lo) if (hi - lo) != 0 else F(1) / hi
        if lo == hi:
            return out
        valid = src > F(0)
        t = (src - lo) * scale
        rgb = [base(t - F(0.5)) * F(255), base(t) * F(255), base(t + F(0.5)) * F(255)]
    if parts is not None:
        parts["values"] = np.stack([c[valid] for c in rgb])
    for i, c in enumerate(rgb):
        out[..., i] = np.where(valid, to_uchar(c), 0)
    out[..., 3] = np.where(valid, 255, 0)
    return out


def weight_to_uchar4(src, parts=None):
    src = np.asarray(src, F)
    out = np.zeros(src.shape + (4,), np.uint8)
    m = weight_limit(src)
    with np.errstate(all="ignore"):
        valid = src > F(0)
        s = m / src * F(0.8) + F(0.2)
        r, g = (F(1) - s) * F(255), s * F(255)
    if parts is not None:
        parts["values"] = np.stack([r[valid], g[valid]])
    out[..., 0] = np.where(valid, to_uchar(r), 0)
    out[..., 1] = np.where(valid, to_uchar(g), 0)
    return out          # blue and alpha stay 0, as in the reference


def normal_to_uchar4(src4, parts=None):
    """src4 (h, w, 4) float32 -> (h, w, 4) uint8"""
    src4 = np.asarray(src4, F)
    out = np.zeros(src4.shape, np.uint8)
    with np.errstate(all="ignore"):
        valid = src4[..., 3] >= F(0)
        c = (F(0.3) + (src4[..., :3] + F(1)) * F(0.35)) * F(255)
    if parts is not None:
        parts["values"] = c[valid]
    out[..., :3] = np.where(valid[..., None], to_uchar(c), 0)
    return out


MAPS = {"depth": depth_to_uchar4, "weight": weight_to_uchar4, "normal": normal_to_uchar4}
