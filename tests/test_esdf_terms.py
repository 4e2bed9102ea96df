"""The distance field's restatement (tests/esdf_terms.py) on the CPU, before it is the yardstick on the GPU: the separable transform
equals the definition taken literally (every cell against every site, ties to the smallest index); the classification on a scene
built by hand; the boundary declares the two entry points and the binding binds them."""
import os
import subprocess

import numpy as np
import pytest

import esdf_terms as E
from esdf_cases import random_mask, tie_masks
import itm_testlib as T
from infinitam_amd import capi

F = np.float32
SIZES = [(1, 1, 1), (7, 1, 1), (1, 9, 1), (5, 3, 2), (13, 11, 6)]      # (nx, ny, nz)
RADII = [0, 1, 2, 5]


@pytest.mark.parametrize("size", SIZES)
def test_separable_transform_equals_the_definition(size):
    for density in (0.0, 0.02, 0.3, 1.0):
        for R in RADII:
            m = random_mask(size, density, seed=sum(size) + R)
            if density == 0.02 and m.size > 1:
                m.reshape(-1)[m.size // 2] |= E.SITE                    # never the empty mask by chance
            d_b, n_b = E.transform_brute(m, R)
            d_s, n_s = E.transform_separable(m, R)
            assert np.array_equal(d_s, d_b) and np.array_equal(n_s, n_b), (size, density, R)
            if density == 0.0:
                assert np.all(d_b == E.NONE) and np.all(n_b == -1)
            if density == 1.0:
                assert np.all(d_b == 0) and np.array_equal(n_b.reshape(-1), np.arange(m.size))


def test_ties_go_to_the_smallest_linear_index():
    tied = 0
    for m in tie_masks():
        for R in RADII:
            d_b, n_b = E.transform_brute(m, R)
            d_s, n_s = E.transform_separable(m, R)
            assert np.array_equal(d_s, d_b) and np.array_equal(n_s, n_b), R
        # the masks do what they are for: some cell has two sites at its minimum distance, and the smaller index was taken
        nz, ny, nx = m.shape
        s = np.nonzero(m.reshape(-1) & E.SITE)[0]
        sk, sj, si = np.unravel_index(s, m.shape)
        d_b, n_b = E.transform_brute(m, 0)
        for c in range(m.size):
            k, j, i = np.unravel_index(c, m.shape)
            d = (si - i) ** 2 + (sj - j) ** 2 + (sk - k) ** 2
            at = s[d == d.min()]
            if len(at) > 1:
                tied += 1
                assert n_b.reshape(-1)[c] == at.min()
    assert tied > 50


def test_distance_is_signed_and_infinite_without_a_site():
    state = np.array([[[E.SITE, 0, E.INSIDE, 0]]], np.uint8)
    d2, _ = E.transform_separable(state, 2)
    assert d2.reshape(-1).tolist() == [0, 1, 4, E.NONE]
    got = E.distance(d2, state, 0.005)
    assert np.array_equal(got.reshape(-1), np.array([0.0, F(0.005), -(F(0.005) * F(2)), np.inf], F))
    assert np.array_equal(E.distance(np.full((1, 1, 2), E.NONE), np.array([[[0, E.INSIDE]]], np.uint8), 1.0).reshape(-1), np.array([np.inf, -np.inf], F))


class HandBuiltReader:
    """readVoxel over voxels given as {(x, y, z): (sdf, weight)}; everything else is absent"""

    def __init__(self, voxels):
        self.voxels = voxels

    def _get(self, x, y, z):
        keys = zip(np.asarray(x).reshape(-1).tolist(), np.asarray(y).reshape(-1).tolist(), np.asarray(z).reshape(-1).tolist())
        return [self.voxels.get(k) for k in keys]

    def locate(self, x, y, z):
        found = np.array([v is not None for v in self._get(x, y, z)])
        return np.zeros(len(found), np.int64), found

    def value(self, x, y, z):
        got = self._get(x, y, z)
        return np.array([F(1) if v is None else F(v[0]) for v in got], F), np.array([v is not None for v in got])

    def weight(self, x, y, z):
        return np.array([0 if v is None else v[1] for v in self._get(x, y, z)], np.uint8)


def hand_built_scene():
    """A wall between x = 1 and x = 2 (sdf > 0 for x <= 1, sdf <= 0 for x >= 2) over x in [-2, 5], y in [-3, 3], z in [0, 2]: stored
    everywhere there, weight 3 -- except an unobserved gap (weight 0) at y = 0 and voxels of weight 1 at y = 2; nothing is stored
    outside."""
    voxels = {}
    for x in range(-2, 6):
        for y in range(-3, 4):
            for z in range(0, 3):
                sdf = {1: 0.5, 2: 0.0}.get(x, 1.0 if x < 1 else -0.5)
                voxels[(x, y, z)] = (sdf, 0 if y == 0 else 1 if y == 2 else 3)
    return HandBuiltReader(voxels)


def test_classification_of_a_hand_built_scene():
    reader = hand_built_scene()
    box = ((-3, -3, 0), (9, 7, 3))                                       # one column beyond the stored voxels on either side in x
    st = E.classify(reader, box, E.SITE_SURFACE, 1)
    x = np.arange(-3, 6)
    row = st[1, 0]                                                       # y = -3, z = 1
    assert np.array_equal((row & E.STORED) != 0, (x >= -2) & (x <= 5))
    assert np.array_equal((row & E.OBSERVED) != 0, (x >= -2) & (x <= 5))
    assert np.array_equal((row & E.INSIDE) != 0, (x >= 2) & (x <= 5)), "sdf 0 is inside"
    assert np.array_equal((row & E.SITE) != 0, (x == 1) | (x == 2)), "the plane between observed voxels: both sides of the sign change"
    gap = st[1, 3]                                                       # y = 0: stored, not observed
    assert np.all((gap & E.STORED) == (row & E.STORED)) and not np.any(gap & (E.OBSERVED | E.INSIDE | E.SITE))
    # min_weight 2: the voxels of weight 1 (y = 2) drop out, and so do the sites they made
    st2 = E.classify(reader, box, E.SITE_SURFACE, 2)
    assert np.any(st[:, 5] & E.SITE) and not np.any(st2[:, 5] & (E.OBSERVED | E.SITE)) and np.array_equal(st2[:, 0], st[:, 0])
    # unknown sites: exactly the cells that are not observed; both rules: the union
    un = E.classify(reader, box, E.SITE_UNKNOWN, 1)
    assert np.array_equal((un & E.SITE) != 0, (un & E.OBSERVED) == 0) and np.any(un & E.SITE) and not np.all(un & E.SITE)
    both = E.classify(reader, box, E.SITE_SURFACE | E.SITE_UNKNOWN, 1)
    assert np.array_equal(both & E.SITE, (un | st) & E.SITE) and np.array_equal(both & 7, st & 7)
    # a neighbour outside the box decides a site: the box ends at x = 1, the sign change lies across its face
    cut = E.classify(reader, ((-3, -3, 0), (5, 7, 3)), E.SITE_SURFACE, 1)
    assert np.array_equal(cut, st[:, :, :5]) and np.any(cut[:, :, 4] & E.SITE) and not np.any(cut[:, :, :4] & E.SITE)
    # ... and a sub-box is the crop of the enclosing box
    sub = E.classify(reader, ((0, -1, 1), (4, 3, 2)), E.SITE_SURFACE | E.SITE_UNKNOWN, 1)
    assert np.array_equal(sub, both[1:3, 2:5, 3:7])


def test_header_declares_and_binding_binds_the_entry_points():
    declared = capi.declared_functions()
    bound = set(capi._SIGS) | set(capi._HOST_IO_SIGS)
    for fn in ("scene_esdf", "esdf_transform"):
        assert fn in declared and fn in bound
    text = open(capi.header_path()).read()
    for name, value in (("STORED", 1), ("OBSERVED", 2), ("INSIDE", 4), ("SITE", 8), ("SITE_SURFACE", 1), ("SITE_UNKNOWN", 2), ("NONE", 0x7fffffff)):
        assert getattr(capi, "ESDF_" + name) == getattr(E, name) == value
        assert f"#define ITM_ESDF_{name} {'0x7fffffff' if name == 'NONE' else value}\n" in text
    assert [n for n, _ in capi.EsdfOut._fields_] == list(capi.ESDF_OUTPUTS) == ["dist2", "nearest", "distance", "state"]
    assert set(capi.ESDF_SITES.values()) == {capi.ESDF_SITE_SURFACE, capi.ESDF_SITE_UNKNOWN}


def test_struct_layouts_and_engine_methods_compile(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "itm_hip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(itm_esdf_box), '
                   'sizeof(itm_esdf_out), offsetof(itm_esdf_box, size), offsetof(itm_esdf_out, state)); return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(T.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    import ctypes as C
    assert got == [C.sizeof(capi.EsdfBox), C.sizeof(capi.EsdfOut), capi.EsdfBox.size.offset, capi.EsdfOut.state.offset]
    cpp = tmp_path / "engine.cpp"
    cpp.write_text('#include "itm_hip_engines.hpp"\nusing namespace itmhip;\n'
                   'template void ITMMainEngine_HIP<ITMVoxel_s, ITMVoxelBlockHash>::DistanceField(const itm_esdf_box&, const itm_esdf_out&, int, int, int) const;\n'
                   'template void ITMDistanceFieldEngine_HIP<ITMVoxel_f_rgb, ITMPlainVoxelArray>::Compute(const ITMScene<ITMVoxel_f_rgb, ITMPlainVoxelArray>*, '
                   'const itm_esdf_box&, const itm_esdf_out&, int, int, int) const;\n')
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(T.ROOT, "include"), str(cpp)], check=True, capture_output=True)
