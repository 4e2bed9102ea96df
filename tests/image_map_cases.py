"""Inputs of the colour-map tests (tests/test_get_image.py, tests/golden/make_golden_image_maps.py), generated from seeds.

A case is (map kind, input array): "depth" and "weight" take (h, w) float32, "normal" takes (h, w, 4) float32.  GOLDEN_CASES are
the ones the reference's own functions are run on for tests/golden/g_image_maps.*: every value they hand to the reference's
float -> uchar cast lies inside the range the cast is defined for.  EXTRA_CASES lie outside it (there the kernels are compared with
the saturating restatement alone)."""
import numpy as np

F = np.float32
SIZES = {"vga": (640, 480), "odd": (13, 7), "big": (1280, 960)}
SUBSET_STRIDE = 97          # the golden stores every 97th pixel of every output


def depth_image(w, h, seed):
    """uniform in [0.4, 3] with 10 % of the pixels -1 (no measurement) and 2 % of them 0"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.4, 3.0, (h, w)).astype(F)
    u = rng.random((h, w))
    d[u < 0.10] = F(-1)
    d[(u >= 0.10) & (u < 0.12)] = F(0)
    return d


def uncertainty_image(w, h, seed):
    """sigmaZ-like values in [5e-4, 2e-2], -1 where the view builder rejects a pixel, the 2-pixel border it never writes 0"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(5e-4, 2e-2, (h, w)).astype(F)
    s[rng.random((h, w)) < 0.10] = F(-1)
    s[:2, :] = 0; s[-2:, :] = 0; s[:, :2] = 0; s[:, -2:] = 0
    return s


def normal_image(w, h, seed):
    """unit normals with w = 0 (valid; the ICP maps write 0 there) or -1 (hole)"""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(h, w, 3)).astype(F)
    n = (n / np.sqrt((n * n).sum(-1, dtype=F))[..., None].astype(F)).astype(F)
    n = np.clip(n, F(-1), F(1))
    out = np.zeros((h, w, 4), F)
    out[..., :3] = n
    out[..., 3] = np.where(rng.random((h, w)) < 0.15, F(-1), F(0))
    return out


def _edge_cases():
    w, h = 64, 48
    c = {}
    c["depth_no_valid"] = ("depth", np.full((h, w), -1, F))
    one_value = np.full((h, w), -1, F); one_value[5:20, 7:40] = F(1.25)
    c["depth_one_distinct_value"] = ("depth", one_value)                   # lo == hi: the whole image stays 0
    one_pixel = np.zeros((h, w), F); one_pixel[17, 23] = F(2.5)
    c["depth_one_pixel"] = ("depth", one_pixel)
    two = np.full((h, w), -1, F); two[3, 3] = F(0.5); two[40, 60] = F(2.0)
    c["depth_two_pixels"] = ("depth", two)
    odd = depth_image(w, h, 901)
    odd[1, 1] = np.nan; odd[2, 5] = np.inf; odd[30, 30] = np.nan; odd[31, 2] = -np.inf
    c["depth_nan_inf"] = ("depth", odd)
    nan_only = depth_image(w, h, 902); nan_only[4, 4] = np.nan; nan_only[9, 50] = -np.inf
    c["depth_nan"] = ("depth", nan_only)
    far = depth_image(w, h, 903) * F(1e6)                                  # every valid value above the initial lower limit 100000, which stays
    c["depth_beyond_initial_limits"] = ("depth", far)
    c["weight_no_valid"] = ("weight", np.zeros((h, w), F))
    wp = np.full((h, w), -1, F); wp[10, 10] = F(3e-3)
    c["weight_one_pixel"] = ("weight", wp)
    big = uncertainty_image(w, h, 904) * F(1e7)                            # every value above the initial minimum 1000
    c["weight_above_initial_minimum"] = ("weight", big)
    wn = uncertainty_image(w, h, 905); wn[5, 5] = np.nan; wn[6, 6] = np.inf
    c["weight_nan_inf"] = ("weight", wn)
    nh = normal_image(w, h, 906); nh[..., 3] = F(-1)
    c["normal_all_holes"] = ("normal", nh)
    na = normal_image(w, h, 907); na[..., 3] = F(1)
    na[0, 0, :3] = (1, 0, 0); na[0, 1, :3] = (-1, 0, 0); na[0, 2, :3] = (0, 1, -1)
    c["normal_axes"] = ("normal", na)
    return c


def _golden_cases():
    c = {}
    for i, (tag, (w, h)) in enumerate(SIZES.items()):
        c[f"depth_{tag}"] = ("depth", depth_image(w, h, 100 + i))
        c[f"weight_{tag}"] = ("weight", uncertainty_image(w, h, 200 + i))
        c[f"normal_{tag}"] = ("normal", normal_image(w, h, 300 + i))
    c.update(_edge_cases())
    return c


def _extra_cases():
    """Values the reference's cast is undefined for: components beyond +-1, NaN and infinities in valid normals."""
    w, h = 64, 48
    n = normal_image(w, h, 950)
    n[..., :3] *= F(3.0)
    n[3, 3, :3] = (np.nan, 0.5, -0.5); n[4, 4, :3] = (np.inf, -np.inf, 0); n[3, 3, 3] = 0; n[4, 4, 3] = 0
    n[5, 5, 3] = np.nan                                                    # w = NaN fails w >= 0: a hole
    return {"normal_out_of_range": ("normal", n)}


GOLDEN_CASES = _golden_cases()
EXTRA_CASES = _extra_cases()
ALL_CASES = dict(GOLDEN_CASES, **EXTRA_CASES)
