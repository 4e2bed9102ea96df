"""Inputs of the view builder tests (tests/test_viewbuilder_terms.py): small depth images at the sizes where a 16 x 16 tile with a
2-pixel halo can go wrong, with the contents where the filter and the normals can go wrong.

Sizes (w x h): no interior (1 x 1, 4 x 7, 7 x 4), one interior pixel (5 x 5), one tile (16 x 16), a last tile column that is all
border while its halo is still read (17 x 17), 18 / 19 / 20 wide (the halo reaches into, up to and past the second tile),
several tiles with ragged ends (33 x 47, 35 x 19, 83 x 61, 163 x 125) and the image of tests/test_viewbuilder.py (160 x 120).

Every case is a float depth image for the filter and the normals, and a raw int16 frame with the calibration that turns it into
(nearly) that image for UpdateView: millimetres where every depth fits, Kinect disparity with an integer origin where the image
holds exact zeros or kilometres (8 c1 fx / (c0 - raw): the t == 0 branch at raw == c0, which the conversion turns into a hole, and
the largest depths next to it).  No conversion yields 0.0; from the second filter pass on the zero border supplies it."""
import functools
from dataclasses import dataclass

import numpy as np

from infinitam_amd import synth

F = np.float32
AFFINE_MM = (1, 0.001, 0.0)
DISPARITY_INT = (0, 1135.0, 0.0819141)      # the integer origin: raw == 1135 is the t == 0 branch


@dataclass(frozen=True)
class Case:
    name: str
    w: int
    h: int
    depth: np.ndarray        # float32 [h, w]
    raw: np.ndarray          # int16 [h, w]
    calib: tuple             # (type, c0, c1) of `raw`

    @property
    def intr(self):
        """(fx, fy, cx, cy), as the reference hands them to computeNormalAndWeight"""
        return synth.intrinsics_for(self.w, self.h)

    @property
    def intr_inverse(self):
        """(1 / fx, 1 / fy, cx, cy): the back-projection proper, whose normals tilt and whose acos argument leaves 1"""
        fx, fy, cx, cy = self.intr
        return (float(F(1) / F(fx)), float(F(1) / F(fy)), cx, cy)


def lcg(seed, n):
    """the suite's generator (s = s * 1664525 + 1013904223), n values in [0, 1) from the top 24 bits"""
    out = np.empty(n, np.float64)
    s = int(seed)
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xffffffff
        out[i] = (s >> 8) / float(1 << 24)
    return out


def sphere_wall(w, h, holes=True):
    """the synthetic sphere in front of its wall, +-2 mm of seeded noise, a lattice of holes and one block of them; at 160 x 120
    this is test_viewbuilder.noisy_depth() value for value"""
    d = synth.depth_frame(w, h, synth.parity_position(1), synth.intrinsics_for(w, h)).astype(F)
    noise = ((lcg(12345, w * h) - 0.5) * 0.004).astype(F)
    d = d + noise.reshape(h, w)
    if holes:
        d[::7, ::5] = -1.0
        d[h // 3:h // 3 + h // 12, 3 * w // 8:9 * w // 16] = -1.0
    return d.astype(F)


def all_invalid(w, h):
    return np.full((h, w), -1.0, F)


def constant(w, h):
    return np.full((h, w), 1.25, F)


def isolated(w, h):
    """valid pixels three apart: the centre is the only valid tap of its window"""
    d = np.full((h, w), -1.0, F)
    ys, xs = np.mgrid[0:h, 0:w]
    at = (xs % 3 == 2) & (ys % 3 == 2)
    d[at] = (0.5 + 3.5 * lcg(99, int(at.sum()))).astype(F)
    return d


def planted_zeros(w, h):
    """exact +0.0 among valid depths: a lattice of zero centres whose four neighbours are valid (their uncertainty is inf or NaN),
    and seeded zeros anywhere (neighbours of valid pixels: averaged in by the filter, a rejection for the normals).  The two smallest
    sizes stand on a constant depth, where normal.z is exactly 1 and the uncertainty of a zero centre is 0 * inf."""
    d = constant(w, h) if w * h <= 400 else sphere_wall(w, h, holes=False)
    ys, xs = np.mgrid[0:h, 0:w]
    d[(xs % 6 == 2) & (ys % 5 == 2)] = 0.0
    r = lcg(4711, w * h).reshape(h, w)
    d[(r < 0.02) & (xs % 6 != 2)] = 0.0
    return d.astype(F)


def kilometres(w, h):
    """metres with sprinkled and patched kilometre depths, and a few holes"""
    ys, xs = np.mgrid[0:h, 0:w]
    d = (1.5 + 0.01 * xs + 0.02 * ys).astype(F)
    r = lcg(2024, w * h).reshape(h, w)
    d[r < 0.05] = (900.0 + 600.0 * lcg(7, int((r < 0.05).sum()))).astype(F)
    patch = (1400.0 * (1.0 + 1e-4 * (lcg(8, w * h) - 0.5))).astype(F).reshape(h, w)
    d[h // 4:h // 2, w // 4:w // 2] = patch[h // 4:h // 2, w // 4:w // 2]
    d[r > 0.97] = -1.0
    return d.astype(F)


PERIOD_X, PERIOD_Y = 5, 7


def periodic(w, h):
    """one seeded 5 x 7 cell repeated: depths in [0.8, 2.5] m, four -1, two 0.0.  Three columns of the cell stand near 0.9 m and two
    near 2.4 m, each within a few millimetres -- the filter's range term is that wide -- so that the taps of a level really blend (a
    tap read from the wrong place changes the result) and the weights across the step underflow."""
    r = lcg(31337, PERIOD_X * PERIOD_Y).reshape(PERIOD_Y, PERIOD_X)
    cell = np.where(np.arange(PERIOD_X)[None, :] < 3, 0.9 + 0.003 * (r - 0.5), 2.4 + 0.02 * (r - 0.5)).astype(F)
    for y, x in ((0, 1), (2, 3), (4, 0), (6, 4)):
        cell[y, x] = -1.0
    for y, x in ((1, 2), (5, 1)):
        cell[y, x] = 0.0
    ys, xs = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(cell[ys % PERIOD_Y, xs % PERIOD_X])


def raw_for(depth, calib, fx):
    """the raw frame whose conversion comes nearest to `depth`; an invalid pixel is raw 0 (millimetres) or beyond the origin (disparity)"""
    kind, c0, c1 = calib
    with np.errstate(all="ignore"):
        if kind == 1:
            raw = np.where(depth > 0, np.round(depth.astype(np.float64) / c0), 0)
        else:
            raw = np.where(depth > 0, np.round(c0 - 8.0 * c1 * fx / np.maximum(depth.astype(np.float64), 1e-3)), np.where(depth == 0, c0, c0 + 100))
    return np.clip(raw, -32768, 32767).astype(np.int16)


CONTENTS = {
    "sphere_wall": (sphere_wall, AFFINE_MM, ((5, 5), (17, 17), (19, 21), (35, 19), (83, 61), (160, 120), (163, 125))),
    "all_invalid": (all_invalid, AFFINE_MM, ((1, 1), (4, 7), (16, 16), (19, 21))),
    "constant": (constant, AFFINE_MM, ((1, 1), (7, 4), (5, 5), (16, 16), (17, 17), (18, 21), (20, 20), (33, 47))),
    "isolated": (isolated, AFFINE_MM, ((5, 5), (17, 17), (19, 21), (33, 47), (83, 61))),
    "planted_zeros": (planted_zeros, DISPARITY_INT, ((5, 5), (18, 21), (20, 20), (35, 19), (83, 61), (163, 125))),
    "kilometres": (kilometres, DISPARITY_INT, ((19, 21), (35, 19), (83, 61))),
    "periodic": (periodic, DISPARITY_INT, ((83, 61),)),
}
NAMES = [f"{content}_{w}x{h}" for content, (_, _, sizes) in CONTENTS.items() for w, h in sizes]
MANDATORY_SIZES = ((19, 21), (83, 61), (163, 125))


@functools.lru_cache(maxsize=None)
def case(name):
    content, size = name.rsplit("_", 1)
    w, h = (int(v) for v in size.split("x"))
    make, calib, sizes = CONTENTS[content]
    assert (w, h) in sizes, name
    depth = np.ascontiguousarray(make(w, h), F)
    raw = raw_for(depth, calib, synth.intrinsics_for(w, h)[0])
    depth.setflags(write=False)
    raw.setflags(write=False)
    return Case(name, w, h, depth, raw, calib)
