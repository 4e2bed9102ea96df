"""Scenes and boxes of the distance-field tests (tests/test_distance_field.py): the scenes of the scene queries -- every voxel type,
both indexes -- and for each three boxes chosen from the scenario alone, so that the restatement (tests/esdf_terms.py) on the CPU
oracle already shows what they hold: a surface crossing, unobserved cells, cells without a site in reach."""
import contextlib
import os

import numpy as np

import esdf_terms as E
import itm_testlib as T
import mesh_attr_cases as MC
import scene_query_terms as Q
from infinitam_amd.capi import BUF_HASH_ENTRIES

SCENES = dict(MC.SCENES, dense=MC.DENSE)
SCENES.pop("mesh_vga_4mm")
FORMS = {"default": {}, "paged": {"ITM_MIRROR": "paged"}, "mirror_off": {"ITM_MIRROR": "off"}}
FAR_ORIGIN = (40.0, -30.0, 20.0)
SITE_MASKS = {"surface": E.SITE_SURFACE, "unknown": E.SITE_UNKNOWN, "both": E.SITE_SURFACE | E.SITE_UNKNOWN}
R_NEAR = 3


@contextlib.contextmanager
def environment(values):
    """The mirror's form is read from the environment when a scene is created."""
    keys = ("ITM_MIRROR", "ITM_MIRROR_BITS", "ITM_MIRROR_PAGES", "ITM_NO_ACCELERATION_CUBES")
    old = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(values)
    try:
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


class Built:
    """A fused scene on a backend, the restatement's reader of it and its boxes."""

    def __init__(self, be, sc, form="default", moved_away=False):
        self.sc = self.placed = sc
        with environment(FORMS[form]):
            if moved_away:
                # fused 40 m from the origin, then one frame at the origin: both cubes are re-placed around the new camera and every
                # block of the first place lies outside them (the boxes stay on the first place)
                self.placed = T.Scenario(**{**sc.__dict__, "origin": FAR_ORIGIN})
                self.ses = MC.fuse(be, self.placed)
                e = self.ses.scene.download(BUF_HASH_ENTRIES)
                self.old_blocks = e["pos"][e["ptr"] >= 0].astype(np.int32)
                self.ses.sc = sc
                self.ses.frame(0, fused=True)
            else:
                self.ses = MC.fuse(be, sc)
        self.scene = self.ses.scene
        self.reader = Q.reader_of(self.scene)

    def blocks(self):
        """positions of the allocated blocks around the boxes' place (hash scenes)"""
        if self.placed is not self.sc:
            return self.old_blocks.astype(np.int64)
        e = self.scene.download(BUF_HASH_ENTRIES)
        return e["pos"][e["ptr"] >= 0].astype(np.int64)

    def bounds(self):
        """(lo, hi) of the stored voxels around the boxes' place, in voxels"""
        if self.scene.is_hash:
            pos = self.blocks()
            return pos.min(0) * 8, (pos.max(0) + 1) * 8
        lo = np.array(self.scene.cfg.denseOffset[:], np.int64)
        return lo, lo + np.array(self.scene.cfg.denseSize[:], np.int64)

    def first_block(self):
        """an allocated block with no allocated block at a smaller x (dense: the block of the array's first voxel)"""
        if not self.scene.is_hash:
            return self.bounds()[0] >> 3
        pos = self.blocks()
        return pos[np.lexsort((pos[:, 2], pos[:, 1], pos[:, 0]))[0]]

    def surface_voxel(self):
        """the voxel under the surface point seen through the pixel at 3/8 of the first depth image (left of and above the centre:
        negative x and y)"""
        sc = self.placed
        u, v = 3 * sc.w // 8, 3 * sc.h // 8
        d = float(sc.depth(0)[v, u])
        fx, fy, cx, cy = sc.intr()
        cam = np.array([(u - cx) / fx * d, (v - cy) / fy * d, d, 1.0])
        M = np.asarray(sc.pose(0), np.float64).reshape(4, 4).T           # column-major storage
        world = np.linalg.solve(M, cam)[:3]
        return np.round(world / sc.voxelSize).astype(np.int64)

    def boxes(self):
        """{name: (origin, size)}: a 40 x 33 x 17 box on the fused surface whose origin is not block-aligned; a box across the edge of
        the stored voxels (allocated and unallocated blocks); a box wholly outside them"""
        lo, hi = self.bounds()
        o = self.surface_voxel() - (17, 13, 5)
        o -= np.where(o % 8 == 0, 3, 0)
        edge = self.first_block() * 8 + (-9, -2, -3)
        return {"surface": (tuple(int(a) for a in o), (40, 33, 17)),
                "edge": (tuple(int(a) for a in edge), (21, 12, 14)),
                "outside": (tuple(int(a) for a in hi + (5, 7, 9)), (9, 6, 5))}

    def restated(self, box, sites, min_weight, R):
        return E.esdf(self.reader, box, SITE_MASKS[sites], min_weight, R, self.sc.voxelSize)

    def close(self):
        self.ses.close()


def assert_boxes_are_not_vacuous(b):
    """on the restatement alone: a SURFACE site, an unobserved cell and a cell with no site within R_NEAR, over the boxes; the first
    box's origin is unaligned and has a negative coordinate"""
    boxes = b.boxes()
    o = np.array(boxes["surface"][0])
    assert np.all(o % 8 != 0) and np.any(o < 0), o
    got = {name: b.restated(box, "surface", 1, R_NEAR) for name, box in boxes.items()}
    assert np.count_nonzero(got["surface"]["state"] & E.SITE) > 50, "the first box lies on the surface"
    assert sum(np.count_nonzero((g["state"] & E.OBSERVED) == 0) for g in got.values()) > 100
    assert sum(np.count_nonzero(g["dist2"] == E.NONE) for g in got.values()) > 100
    assert np.any(got["surface"]["state"] & E.INSIDE) and np.any(got["surface"]["distance"] < 0)
    st = got["edge"]["state"]
    assert np.any(st & E.STORED) and np.any((st & E.STORED) == 0), "the second box straddles stored and absent voxels"
    assert not np.any(got["outside"]["state"]) and np.all(got["outside"]["dist2"] == E.NONE)
    # min_weight 2 is a different classification
    assert not np.array_equal(b.restated(boxes["surface"], "surface", 2, R_NEAR)["state"], got["surface"]["state"])


# ---- masks of the transform alone ------------------------------------------------------------------------------------------------------

def random_mask(size, density, seed):
    """state [nz, ny, nx] with SITE at about `density` of the cells and INSIDE at random"""
    rng = np.random.default_rng(seed)
    shape = size[::-1]
    site = rng.random(shape) < density if 0 < density < 1 else np.full(shape, density >= 1)
    return (site * E.SITE + (rng.random(shape) < 0.3) * E.INSIDE).astype(np.uint8)


def tie_masks():
    """masks whose cells have several nearest sites: two sites symmetric about a cell along each axis, the corners of a square and
    of a cube around their centre, a full checkerboard"""
    out = []
    for axis in range(3):
        m = np.zeros((5, 7, 9), np.uint8)
        a, b = [2, 3, 4], [2, 3, 4]
        a[axis] -= 2; b[axis] += 2
        m[tuple(a)] = m[tuple(b)] = E.SITE
        out.append(m)
    m = np.zeros((1, 5, 5), np.uint8)
    m[0, 0, 0] = m[0, 0, 4] = m[0, 4, 0] = m[0, 4, 4] = E.SITE
    out.append(m)
    m = np.zeros((5, 5, 5), np.uint8)
    m[::4, ::4, ::4] = E.SITE
    out.append(m)
    k, j, i = np.indices((4, 5, 6))
    out.append((((i + j + k) & 1) * E.SITE).astype(np.uint8))
    return out
