"""numpy restatements of the view builder: the two raw-depth conversions, the 5x5 bilateral depth filter and the normal /
depth-uncertainty images (tests/test_viewbuilder_terms.py).

Kernels: infinitam_amd/csrc/viewbuilder.hip (filter_depth_kernel, normal_weight_kernel, stage_convert) and the two conversion
kernels of infinitam_amd/csrc/scene.hip.  Reference: convertDepthAffineToFloat, convertDisparityToDepth, filterDepth and
computeNormalAndWeight (DeviceAgnostic/ITMViewBuilder.h), UpdateView (DeviceSpecific/CPU/ITMViewBuilder_CPU.cpp).

Every operation exists twice:

  * `*_seq32`: the reference's operations in np.float32, in its order -- no fused multiply-add, the filter's taps row by row with
    the two running sums growing in that order -- and the host libm's expf / acosf through ctypes.  It reproduces the oracle (and
    the reference) bit for bit, which pins the restatement before it judges a kernel.
  * `*_ref64`: the same formulas in float64 from the same float32 inputs and float32 constants, with the per-pixel quantities the
    error bounds are made of (`FilterRef`, `SigmaRef`).

The bounds (u = 2^-24, first order in u):

  filter     E = (2n + 3) u |r| + sum_i g_i eps_i |t_i - r| / sum_i g_i + n FLT_MIN max_i |t_i - r|,   eps_i = (C_A a_i + 2 K_EXP) u
             r: the float64 result, t_i / g_i / a_i: the n valid taps, their weights exp(-a_i) and exponents.
             First term: the roundings of two sequential float sums of n terms, the n products and the quotient.  Second term:
             out' - r = sum g_i d_i (t_i - r) / sum g_i (1 + d_i) for weights g_i (1 + d_i), because sum g_i (t_i - r) = 0.
             Third term: a weight in the subnormal range may be flushed, an absolute error below FLT_MIN in a sum that is >= 1
             (the centre's weight is exp(0)).
  C_A = 20   the float roundings that go into an exponent a = 0.5 (b k k + d s s), counted as relative errors in units of u:
               d = (tap - centre)^2            subtraction 1, squared 2, the product's rounding 3
               off = centre - 0.4              1;  0.0019 off: 2;  (0.0019 off) off: 4
               0.0001 / sqrt(centre) * 0.25    sqrt 1, quotient 2, times 0.25 exact
               0.0012 + . + .                  sums of positive terms: max of the parts + 1 each: 5, then 6
               s = 1 / .                       7
               (d s) s                         3 + 7 + 1 = 11, then 11 + 7 + 1 = 19
               b k k                           2
               b k k + d s s                   max(19, 2) + 1 = 20;  times -0.5 exact
  sigmaZ     sigma = (A + T2) + T3,  T2 = 0.0019 off off,  T3 = 0.0001 / sqrt(z) s s,  s = theta / (pi/2 - theta),  theta = acosf(nz),
             from the float32 depth z and the float32 normal component nz (the normals are compared bit for bit, so nz is input):
               |d theta| <= K_ACOS 2u theta
               |ds|      <= (pi/2) / (pi/2 - theta)^2 |d theta| + 2u s          (the subtraction's and the quotient's roundings)
               |dT3|     <= 4u T3 + 0.0001 / sqrt(z) (2 s |ds| + ds^2)          (sqrt, quotient, two products)
               |dT2|     <= 4u T2                                              (off 1, the products 2, 4)
               E         =  |dT2| + |dT3| + u (A + T2) + u sigma               (the two sums)
             Where pi/2 - theta < 64 ulp(pi/2) the first-order bound means nothing (`SigmaRef.excluded`)."""
import ctypes
import ctypes.util
from dataclasses import dataclass

import numpy as np

from tracker_terms import expf

F = np.float32
U = 2.0 ** -24
FLT_MIN = float(np.finfo(F).tiny)
A0, A1, A2 = F(0.0012), F(0.0019), F(0.0001)          # the sensor's depth uncertainty: A0 + A1 (z - 0.4)^2 + A2 / sqrt(z) * slope^2
K_SPATIAL = F(1.2232)
HALF_PI = F(3.1415926535897932384626433832795) * F(0.5)
RADIUS = 2
C_A = 20
OFFSETS = [(dy, dx) for dy in range(-RADIUS, RADIUS + 1) for dx in range(-RADIUS, RADIUS + 1)]      # the reference's tap order

_LIBM = ctypes.CDLL(ctypes.util.find_library("m"))
_LIBM.acosf.restype, _LIBM.acosf.argtypes = ctypes.c_float, [ctypes.c_float]
_ACOSF = np.frompyfunc(_LIBM.acosf, 1, 1)


def acosf(x):
    """the host libm's acosf, element by element"""
    x = np.asarray(x, F)
    return np.asarray(_ACOSF(x), dtype=np.float64).astype(F).reshape(x.shape)


def exp_numpy(x):
    """numpy's own float32 exp: a second implementation of the function, for the tripwire's D"""
    return np.exp(np.asarray(x, F)).astype(F)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ulp_distance(a, b):
    """how many floats lie between a and b (finite float32 arrays), counted along the number line"""
    def line(v):
        i = bits(v).astype(np.int64)
        return np.where(i & 0x80000000, -(i & 0x7fffffff), i)
    return np.abs(line(a) - line(b))


# ---- conversions ----------------------------------------------------------------------------------------------------------------
def convert_affine(raw, a, b):
    """convertDepthAffineToFloat: raw * a + b, -1 for raw <= 0 or raw > 32000"""
    raw = np.asarray(raw, np.int16)
    out = raw.astype(F) * F(a) + F(b)
    return np.where((raw <= 0) | (raw > 32000), F(-1), out).astype(F)


def convert_disparity(raw, c0, c1, fx):
    """convertDisparityToDepth: 8 c1 fx / (c0 - raw), 0 where the denominator is 0, then -1 for everything that is not > 0"""
    t = F(c0) - np.asarray(raw, np.int16).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(t == 0, F(0), (F(8) * F(c1) * F(fx)) / t).astype(F)
    return np.where(depth > 0, depth, F(-1)).astype(F)


def convert(raw, calib_type, c0, c1, fx):
    return convert_disparity(raw, c0, c1, fx) if calib_type == 0 else convert_affine(raw, c0, c1)


# ---- filterDepth ----------------------------------------------------------------------------------------------------------------
def _window(img, dy, dx):
    h, w = img.shape
    return img[RADIUS + dy:h - RADIUS + dy, RADIUS + dx:w - RADIUS + dx]


def filter_seq32(img, exp=expf):
    """filterDepth over an image [h, w]: border 0, invalid centre -1, else the weighted mean of the taps that are not negative"""
    img = np.asarray(img, F)
    h, w = img.shape
    out = np.zeros((h, w), F)
    if w <= 2 * RADIUS or h <= 2 * RADIUS:
        return out
    c = _window(img, 0, 0)
    live = ~(c < 0)
    with np.errstate(all="ignore"):
        off = c - F(0.4)
        inv_sigma = F(1) / (A0 + A1 * off * off + A2 / np.sqrt(c) * F(0.25))
        weighted, weights = np.zeros(c.shape, F), np.zeros(c.shape, F)
        for dy, dx in OFFSETS:
            tap = _window(img, dy, dx)
            ok = live & ~(tap < 0)
            diff = tap - c
            diff = diff * diff
            arg = F(-0.5) * (F(abs(dy) + abs(dx)) * K_SPATIAL * K_SPATIAL + diff * inv_sigma * inv_sigma)
            g = np.zeros(c.shape, F)
            g[ok] = exp(arg[ok])
            weights = np.where(ok, weights + g, weights).astype(F)
            weighted = np.where(ok, weighted + g * tap, weighted).astype(F)
        out[RADIUS:h - RADIUS, RADIUS:w - RADIUS] = np.where(live, weighted / weights, F(-1))
    return out


@dataclass
class FilterRef:
    """filterDepth in float64 for the interior [h - 4, w - 4] of an image; the per-tap arrays are [25, h - 4, w - 4]"""
    live: np.ndarray         # the centre is valid: the pixel is filtered
    out: np.ndarray          # float64 result where live
    ok: np.ndarray           # tap i is valid
    n: np.ndarray            # valid-tap count
    g: np.ndarray            # weights exp(-a), 0 for invalid taps
    a: np.ndarray            # exponents
    taps: np.ndarray         # the taps, float64

    def bound(self, k_exp):
        """E (module docstring) per interior pixel"""
        r = self.out
        dev = np.where(self.ok, np.abs(self.taps - r), 0.0)
        eps = (C_A * self.a + 2 * k_exp) * U
        return (2 * self.n + 3) * U * np.abs(r) + (self.g * eps * dev).sum(0) / np.maximum(self.g.sum(0), 1.0) + self.n * FLT_MIN * dev.max(0)


def filter_ref64(img):
    img = np.asarray(img, F)
    D = np.float64
    c = _window(img, 0, 0).astype(D)
    live = ~(c < 0)
    with np.errstate(all="ignore"):
        off = c - D(F(0.4))
        inv_sigma = 1.0 / (D(A0) + D(A1) * off * off + D(A2) / np.sqrt(c) * 0.25)
        taps = np.stack([_window(img, dy, dx).astype(D) for dy, dx in OFFSETS])
        blocks = np.array([abs(dy) + abs(dx) for dy, dx in OFFSETS], D)[:, None, None]
        ok = live[None] & ~(taps < 0)
        diff = (taps - c[None]) ** 2
        a = np.where(ok, 0.5 * (blocks * D(K_SPATIAL) * D(K_SPATIAL) + diff * inv_sigma[None] * inv_sigma[None]), 0.0)
        g = np.where(ok, np.exp(-a), 0.0)
        out = np.where(live, (g * np.where(ok, taps, 0.0)).sum(0) / g.sum(0), -1.0)
    return FilterRef(live, out, ok, ok.sum(0), g, a, taps)


# ---- computeNormalAndWeight -----------------------------------------------------------------------------------------------------
def _normal_parts(depth, intr, T):
    """the interior's accept mask and unnormalised normal, in the type T (np.float32: each operation rounded, in the reference's order)"""
    h, w = depth.shape
    p0, p1, cx, cy = [T(F(v)) for v in intr]
    z = _window(depth, 0, 0).astype(T)
    zE, zW, zS, zN = [_window(depth, dy, dx).astype(T) for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0))]
    ys, xs = np.mgrid[RADIUS:h - RADIUS, RADIUS:w - RADIUS]
    x, y = xs.astype(T), ys.astype(T)
    ok = ~(z < 0) & ~((zE <= 0) | (zS <= 0) | (zW <= 0) | (zN <= 0))
    one = T(1)
    ex, ey = zE * ((x + one) - cx) * p0, zE * (y - cy) * p1
    wx, wy = zW * ((x - one) - cx) * p0, zW * (y - cy) * p1
    sx, sy = zS * (x - cx) * p0, zS * ((y + one) - cy) * p1
    nx_, ny_ = zN * (x - cx) * p0, zN * ((y - one) - cy) * p1
    dxx, dxy, dxz = ex - wx, ey - wy, zE - zW
    dyx, dyy, dyz = sx - nx_, sy - ny_, zS - zN
    n = [dxy * dyz - dxz * dyy, dxz * dyx - dxx * dyz, dxx * dyy - dxy * dyx]
    ok &= ~((n[0] == 0) & (n[1] == 0) & (n[2] == 0))
    return ok, z, n


def normals_seq32(depth, intr, normals, sigma, acos=acosf):
    """computeNormalAndWeight over an image: returns copies of `normals` [h, w, 4] and `sigma` [h, w] with what the reference writes
    -- the normal and the uncertainty of an accepted pixel, w = -1 and sigma = -1 of a rejected one, nothing in the border"""
    depth = np.asarray(depth, F)
    h, w = depth.shape
    normals, sigma = np.array(normals, F).reshape(h, w, 4), np.array(sigma, F).reshape(h, w)
    if w <= 2 * RADIUS or h <= 2 * RADIUS:
        return normals, sigma
    with np.errstate(all="ignore"):
        ok, z, n = _normal_parts(depth, intr, F)
        inv = F(1) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        n = [c * inv for c in n]
        theta = np.zeros(z.shape, F)
        theta[ok] = acos(n[2][ok])
        slope = theta / (HALF_PI - theta)
        off = z - F(0.4)
        s = A0 + A1 * off * off + A2 / np.sqrt(z) * slope * slope
    ni, si = normals[RADIUS:h - RADIUS, RADIUS:w - RADIUS], sigma[RADIUS:h - RADIUS, RADIUS:w - RADIUS]
    for k in range(3):
        ni[..., k] = np.where(ok, n[k], ni[..., k])
    ni[..., 3] = np.where(ok, F(1), F(-1))
    si[...] = np.where(ok, s, F(-1))
    return normals, sigma


@dataclass
class SigmaRef:
    """the uncertainty in float64 from the float32 depth and the float32 normal.z, over a whole image"""
    valid: np.ndarray        # the pixel was accepted and its depth is > 0 (a zero centre gives inf or NaN: class checks only)
    out: np.ndarray
    excluded: np.ndarray     # valid, but pi/2 - theta < 64 ulp(pi/2)
    z: np.ndarray
    theta: np.ndarray

    def bound(self, k_acos):
        """E (module docstring) per pixel"""
        with np.errstate(all="ignore"):
            hp = np.float64(HALF_PI)
            d = np.abs(hp - self.theta)          # (a normal that points away: theta > pi/2, slope < 0; only its square is used)
            s = self.theta / d
            q = np.float64(A2) / np.sqrt(self.z)
            off = self.z - np.float64(F(0.4))
            t2 = np.float64(A1) * off * off
            t3 = q * s * s
            ds = 2 * U * s + hp / (d * d) * k_acos * 2 * U * self.theta
            return 4 * U * t2 + 4 * U * t3 + U * (np.float64(A0) + t2) + U * np.abs(self.out) + q * (2 * s * ds + ds * ds)


def sigma_ref64(depth, normals):
    """from the depth image and the normals image [h, w, 4] that computeNormalAndWeight wrote for it (w == 1: accepted)"""
    z = np.asarray(depth, F).astype(np.float64)
    nrm = np.asarray(normals, F)
    valid = (nrm[..., 3] == 1) & (z > 0)
    with np.errstate(all="ignore"):
        theta = np.arccos(np.clip(nrm[..., 2].astype(np.float64), -1.0, 1.0))
        d = np.float64(HALF_PI) - theta
        s = theta / d
        off = z - np.float64(F(0.4))
        out = (np.float64(A0) + np.float64(A1) * off * off) + np.float64(A2) / np.sqrt(z) * s * s
    excluded = valid & (np.abs(d) < 64 * float(np.spacing(HALF_PI)))
    return SigmaRef(valid, np.where(valid, out, 0.0), excluded, np.where(valid, z, 1.0), np.where(valid, theta, 0.0))


# ---- UpdateView -----------------------------------------------------------------------------------------------------------------
def update_view_seq32(raw, calib_type, c0, c1, intr, bilateral, noise, normals, sigma, exp=expf, acos=acosf):
    """UpdateView: conversion, five filter passes, normals -> (depth, normals, sigma, every pass [5] or [])"""
    depth = convert(raw, calib_type, c0, c1, intr[0])
    passes = []
    if bilateral:
        for _ in range(5):
            depth = filter_seq32(depth, exp)
            passes.append(depth)
    if noise:
        normals, sigma = normals_seq32(depth, intr, normals, sigma, acos)
    return depth, normals, sigma, passes
