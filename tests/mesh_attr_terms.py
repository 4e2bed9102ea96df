"""float32 numpy restatement of the mesh vertex attributes (include/itm_hip.h: itm_mesh_attributes), term for term:

  sample position   p = vertex / voxelSize                                     three IEEE float divisions
  gradient          computeSingleNormalFromSDF(p)      DeviceAgnostic/ITMRepresentationAccess.h:224-337
  normal            g * (1 / sqrt(g.g)), (0, 0, 0) where that is not finite    (store_normal, sample_device.h)
  colour            readFromSDF_color4u_interpolated(p)  :187-222, bytes as drawPixelColour: (uchar)(c * 255.0f), alpha 255

fed from downloaded scene buffers (hash entries + voxel blocks).  Every product and sum is rounded to float32 on its own, in the
reference's order.  Also the PLY writer that defines the bytes itm_mesh_write_ply must produce."""
import hashlib

import numpy as np

from tracker_terms import VoxelReader

F = np.float32


class MeshVoxelReader(VoxelReader):
    """VoxelReader with a sorted-key block look-up (the meshes have millions of vertices) and the colour beside the sdf."""

    def __init__(self, voxels, entries):
        self.sdf = np.asarray(voxels["sdf"]).reshape(-1)
        self.short = self.sdf.dtype == np.int16
        self.dense = None
        self.clr = np.asarray(voxels["clr"]).reshape(-1, 3) if "clr" in voxels.dtype.names else None
        e = entries[entries["ptr"] >= 0]
        keys = self._key(e["pos"][:, 0].astype(np.int64), e["pos"][:, 1].astype(np.int64), e["pos"][:, 2].astype(np.int64))
        order = np.argsort(keys)
        self.keys, self.ptrs = keys[order], e["ptr"].astype(np.int64)[order]

    @staticmethod
    def _key(bx, by, bz):
        return ((bx + 32768) << 32) | ((by + 32768) << 16) | (bz + 32768)

    def locate(self, x, y, z):
        x, y, z = (np.asarray(a, np.int64) for a in (x, y, z))
        bx, by, bz = x >> 3, y >> 3, z >> 3
        inside = (np.abs(bx + 0.5) < 32768) & (np.abs(by + 0.5) < 32768) & (np.abs(bz + 0.5) < 32768)     # the table's short coordinates
        k = self._key(bx, by, bz)
        at = np.minimum(np.searchsorted(self.keys, k), len(self.keys) - 1)
        found = inside & (self.keys[at] == k)
        return np.where(found, self.ptrs[at] * 512 + (x & 7) + (y & 7) * 8 + (z & 7) * 64, 0), found

    def raw(self, x, y, z):
        lin, found = self.locate(x, y, z)
        return np.where(found, self.sdf[lin].astype(F), F(32767) if self.short else F(1)).astype(F), found

    def colour(self, x, y, z):
        """clr.toFloat() of readVoxel: float32 [n, 3], zeros where no voxel is stored (TVoxel())"""
        lin, found = self.locate(x, y, z)
        return np.where(found[:, None], self.clr[lin].astype(F), F(0)).astype(F)


def sample_positions(vertices, voxel_size):
    """p = vertex / voxelSize for float32 vertices [n, 3]"""
    return (np.asarray(vertices, F).reshape(-1, 3) / F(voxel_size)).astype(F)


def split(p):
    p = np.asarray(p, F).reshape(-1, 3)
    b = np.floor(p)
    return b.astype(np.int64), (p - b).astype(F)


def gradient(reader, p):
    """computeSingleNormalFromSDF at float32 positions [n, 3] -> float32 [n, 3]"""
    i, f = split(p)
    cache = {}

    def raw(d):
        if d not in cache:
            cache[d] = reader.raw(i[:, 0] + d[0], i[:, 1] + d[1], i[:, 2] + d[2])[0]
        return cache[d]

    def component(axis):
        u_axis, v_axis = [a for a in range(3) if a != axis]            # the remaining axes in x < y < z order
        fa, fu, fv = f[:, axis], f[:, u_axis], f[:, v_axis]
        ga, gu, gv = F(1) - fa, F(1) - fu, F(1) - fv

        def plane(k):
            def s(u, v):
                d = [0, 0, 0]
                d[axis], d[u_axis], d[v_axis] = k, u, v
                return raw(tuple(d))
            return s(0, 0) * gu * gv + s(1, 0) * fu * gv + s(0, 1) * gu * fv + s(1, 1) * fu * fv

        lower = plane(0) * fa + plane(-1) * ga
        r = plane(1) * ga + plane(2) * fa - lower
        return (r / F(32767) if reader.short else r).astype(F)           # TVoxel::SDF_valueToFloat

    with np.errstate(all="ignore"):
        return np.stack([component(0), component(1), component(2)], -1).astype(F)


def normals_from_gradient(g):
    g = np.asarray(g, F)
    with np.errstate(all="ignore"):
        sc = F(1) / np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2], dtype=F)
        n = (g * sc[:, None]).astype(F)
    bad = ~np.all(np.isfinite(n), axis=1)
    n[bad] = F(0)
    return n


def colour(reader, p):
    """readFromSDF_color4u_interpolated at float32 positions [n, 3] -> float32 [n, 4] (the Vector4f it returns)"""
    i, c = split(p)
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    nx, ny, nz = F(1) - cx, F(1) - cy, F(1) - cz
    ret = np.zeros((len(i), 3), F)
    for d, w in (((0, 0, 0), nx * ny * nz), ((1, 0, 0), cx * ny * nz), ((0, 1, 0), nx * cy * nz), ((1, 1, 0), cx * cy * nz),
                 ((0, 0, 1), nx * ny * cz), ((1, 0, 1), cx * ny * cz), ((0, 1, 1), nx * cy * cz), ((1, 1, 1), cx * cy * cz)):
        ret = (ret + w[:, None] * reader.colour(i[:, 0] + d[0], i[:, 1] + d[1], i[:, 2] + d[2])).astype(F)
    out = np.empty((len(i), 4), F)
    out[:, :3] = ret / F(255)
    out[:, 3] = F(255) / F(255)
    return out


def colour_bytes(c):
    """drawPixelColour: (uchar)(c * 255.0f) per channel, alpha 255 -> uint8 [n, 4]"""
    out = np.empty((len(c), 4), np.uint8)
    out[:, :3] = (np.asarray(c, F)[:, :3] * F(255)).astype(F).astype(np.int32).astype(np.uint8)
    out[:, 3] = 255
    return out


def over_distinct(fn, p):
    """fn(p) evaluated once per distinct position (compared as bytes) and spread back: the attributes are functions of p alone"""
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    keys = p.view(np.dtype((np.void, 12))).reshape(-1)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    return fn(p[first])[inverse.reshape(-1)]


def attributes(reader, triangles, voxel_size, colours=False):
    """(gradients [n, 3], normals [n, 3], colour floats [n, 4] or None) for the vertices of float32 triangles [t, 3, 3], buffer order"""
    p = sample_positions(triangles, voxel_size)
    g = over_distinct(lambda q: gradient(reader, q), p)
    c = over_distinct(lambda q: colour(reader, q), p) if colours else None
    return g, normals_from_gradient(g), c


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def high_fraction(p, eps):
    """vertices with a component of p whose fractional part exceeds 1 - eps"""
    p = np.asarray(p, F).reshape(-1, 3)
    frac = (p - np.floor(p)).astype(F)
    return np.any(frac > F(1) - F(eps), axis=1)


SUBSET_STRIDE = {"mesh_micro": 16, "mesh_f_rgb": 16, "mesh_s_rgb_yaw": 256}
SUBSET_HALO = 2000


def subset_indices(name, p):
    """the vertices whose values the golden stores: every k-th, plus the first SUBSET_HALO (buffer order) with a fractional part
    above 1 - 1e-3"""
    halo = np.nonzero(high_fraction(p, 1e-3))[0][:SUBSET_HALO]
    return np.arange(0, len(p), SUBSET_STRIDE[name]), halo


def ply_bytes(triangles, normals=None, colours=None):
    """the file itm_mesh_write_ply writes for float32 triangles [n, 3, 3], normals [n, 3, 3] or None, colours uint8 [n, 3, 4] or None"""
    tri = np.ascontiguousarray(triangles, "<f4").reshape(-1, 3, 3)
    n = tri.shape[0]
    head = ["ply", "format binary_little_endian 1.0", "comment itm-hip mesh", f"element vertex {3 * n}",
            "property float x", "property float y", "property float z"]
    fields = [("p", "<f4", 3)]
    if normals is not None:
        head += ["property float nx", "property float ny", "property float nz"]
        fields.append(("n", "<f4", 3))
    if colours is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
        fields.append(("c", "u1", 3))
    head += [f"element face {n}", "property list uchar int vertex_indices", "end_header"]
    v = np.zeros(3 * n, np.dtype(fields))            # packed: no padding between the fields
    v["p"] = tri.reshape(-1, 3)
    if normals is not None:
        v["n"] = np.asarray(normals, "<f4").reshape(-1, 3)
    if colours is not None:
        v["c"] = np.asarray(colours, np.uint8).reshape(-1, 4)[:, :3]
    faces = np.zeros(n, np.dtype([("k", "u1"), ("i", "<i4", 3)]))
    faces["k"] = 3
    i = np.arange(n, dtype=np.int64)
    faces["i"] = np.stack([3 * i + 2, 3 * i + 1, 3 * i], -1)
    return ("\n".join(head) + "\n").encode() + v.tobytes() + faces.tobytes()
