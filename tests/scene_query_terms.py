"""float32 numpy restatement of the scene queries (include/itm_hip.h: itm_scene_query_points, itm_scene_cast_rays), term for term,
every product and sum rounded to float32 on its own:

  sdf_nearest, weight   readFromSDF_float_uninterpolated: the voxel at ROUND(p)           DeviceAgnostic/ITMRepresentationAccess.h:144-158
  sdf                   readFromSDF_float_interpolated, in the reference's order          :160-185
  gradient, normal, colour   tests/mesh_attr_terms.py (pinned to reference goldens), not rewritten here
  flags, the invalid rule    include/itm_hip.h
  cast_rays             the castRay loop, vectorised over rays                            DeviceAgnostic/ITMVisualisationEngine.h:117-156
  camera_rays           castRay's own preamble :102-116 as the input of cast_rays

fed from downloaded scene buffers."""
import numpy as np

import mesh_attr_terms as MT
from tracker_terms import round_ref

F = np.float32
POINT_LIMIT = F(262136)
RAY_LIMIT = F(131072)
RAY_LENGTH_LIMIT = F(4194304)
INVALID = np.uint32(0x80000000)


class SceneReader(MT.MeshVoxelReader):
    """readVoxel from downloaded buffers for either index: sdf, weight and colour of integer positions; absent voxels are TVoxel()."""

    def __init__(self, voxels, entries=None, dense=None):
        self.dense = dense
        if dense is None:
            super().__init__(voxels, entries)
        else:
            self.sdf = np.asarray(voxels["sdf"]).reshape(-1)
            self.short = self.sdf.dtype == np.int16
            self.clr = np.asarray(voxels["clr"]).reshape(-1, 3) if "clr" in voxels.dtype.names else None
        self.w_depth = np.asarray(voxels["w_depth"]).reshape(-1)

    def locate(self, x, y, z):
        if self.dense is None:
            return super().locate(x, y, z)
        x, y, z = (np.asarray(a, np.int64) for a in (x, y, z))
        (sx, sy, sz), (ox, oy, oz) = self.dense
        qx, qy, qz = x - ox, y - oy, z - oz
        found = (qx >= 0) & (qx < sx) & (qy >= 0) & (qy < sy) & (qz >= 0) & (qz < sz)
        return np.where(found, qx + qy * sx + qz * sx * sy, 0), found

    def value(self, x, y, z):
        raw, found = self.raw(x, y, z)
        return self.to_float(raw), found

    def to_float(self, raw):
        return (raw / F(32767) if self.short else raw).astype(F)            # TVoxel::SDF_valueToFloat

    def weight(self, x, y, z):
        lin, found = self.locate(x, y, z)
        return np.where(found, self.w_depth[lin], 0).astype(np.uint8)


def reader_of(scene):
    """SceneReader of a live scene (any backend): downloads the table and the voxels"""
    from infinitam_amd.capi import BUF_HASH_ENTRIES, BUF_VOXEL_BLOCKS
    voxels = scene.download(BUF_VOXEL_BLOCKS)
    if scene.is_hash:
        return SceneReader(voxels, scene.download(BUF_HASH_ENTRIES))
    return SceneReader(voxels, dense=(tuple(scene.cfg.denseSize), tuple(scene.cfg.denseOffset)))


def positions(points, units, voxel_size):
    """p of the points [n, 3]: x / voxelSize (IEEE divisions) for "metres", x for "voxels" """
    x = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return (x / F(voxel_size)).astype(F) if units == "metres" else x.copy()


def invalid(p):
    """a coordinate of p is not finite or !(|c| < 262136)"""
    with np.errstate(all="ignore"):
        return ~np.all(np.abs(p) < POINT_LIMIT, axis=1)


def trilinear(reader, p):
    """readFromSDF_float_interpolated at float32 positions [n, 3] -> (float32 [n], corner presence bits uint32 [n])"""
    i, c = MT.split(p)
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    v, bits = [], np.zeros(len(i), np.uint32)
    for k in range(8):
        raw, found = reader.raw(i[:, 0] + (k & 1), i[:, 1] + ((k >> 1) & 1), i[:, 2] + (k >> 2))
        v.append(raw)
        bits |= found.astype(np.uint32) << np.uint32(k)
    one = F(1)
    res1 = (one - cx) * v[0] + cx * v[1]
    res1 = (one - cy) * res1 + cy * ((one - cx) * v[2] + cx * v[3])
    res2 = (one - cx) * v[4] + cx * v[5]
    res2 = (one - cy) * res2 + cy * ((one - cx) * v[6] + cx * v[7])
    return reader.to_float(((one - cz) * res1 + cz * res2).astype(F)), bits


def nearest(reader, p):
    """readFromSDF_float_uninterpolated -> (sdf float32 [n], found bool [n], w_depth uint8 [n])"""
    x, y, z = round_ref(p[:, 0]), round_ref(p[:, 1]), round_ref(p[:, 2])
    v, found = reader.value(x, y, z)
    return v, found, reader.weight(x, y, z)


def query_points(reader, points, units, voxel_size, want):
    """the outputs of itm_scene_query_points named in `want`, as a dict of arrays"""
    p = positions(points, units, voxel_size)
    bad = invalid(p)
    q = np.where(bad[:, None], F(0), p).astype(F)          # nothing is read at an invalid point: its outputs are the defaults
    out = {}
    with np.errstate(all="ignore"):
        if "sdf" in want or "flags" in want:
            sdf, corners = trilinear(reader, q)
        if "sdf" in want:
            out["sdf"] = np.where(bad, F(1), sdf).astype(F)
        if "sdf_nearest" in want or "weight" in want or "flags" in want:
            near, found, weight = nearest(reader, q)
        if "sdf_nearest" in want:
            out["sdf_nearest"] = np.where(bad, F(1), near).astype(F)
        if "weight" in want:
            out["weight"] = np.where(bad, 0, weight).astype(np.uint8)
        if "gradient" in want or "normal" in want:
            g = MT.over_distinct(lambda r: MT.gradient(reader, r), q)
        if "gradient" in want:
            out["gradient"] = np.where(bad[:, None], F(0), g).astype(F)
        if "normal" in want:
            out["normal"] = np.where(bad[:, None], F(0), MT.normals_from_gradient(g)).astype(F)
        if "colour" in want:
            c = MT.colour_bytes(MT.over_distinct(lambda r: MT.colour(reader, r), q))
            out["colour"] = np.where(bad[:, None], np.uint8(0), c).astype(np.uint8)
        if "flags" in want:
            f = found.astype(np.uint32) | (corners << np.uint32(8)) | np.where(corners == 0xff, np.uint32(2), np.uint32(0))
            out["flags"] = np.where(bad, INVALID, f).astype(np.uint32)
    return out


# ---- rays -------------------------------------------------------------------------------------------------------------------------------

def invert4(m):
    """Matrix4::inv (ORUtils/Matrix.h:162-223) in float32: cofactors of the transposed matrix, then every element times 1 / det"""
    m = np.asarray(m, F).reshape(16)
    s = np.array([m[i * 4 + j] for j in range(4) for i in range(4)], F)          # s[i + 4 j] = m[4 i + j]

    def tri(a, b, c, d, e, f):
        return F(F(F(a * b) + F(c * d)) + F(e * f))
    o = np.zeros(16, F)
    t = [s[10] * s[15], s[11] * s[14], s[9] * s[15], s[11] * s[13], s[9] * s[14], s[10] * s[13], s[8] * s[15], s[11] * s[12],
         s[8] * s[14], s[10] * s[12], s[8] * s[13], s[9] * s[12]]
    o[0] = tri(t[0], s[5], t[3], s[6], t[4], s[7]) - tri(t[1], s[5], t[2], s[6], t[5], s[7])
    o[1] = tri(t[1], s[4], t[6], s[6], t[9], s[7]) - tri(t[0], s[4], t[7], s[6], t[8], s[7])
    o[2] = tri(t[2], s[4], t[7], s[5], t[10], s[7]) - tri(t[3], s[4], t[6], s[5], t[11], s[7])
    o[3] = tri(t[5], s[4], t[8], s[5], t[11], s[6]) - tri(t[4], s[4], t[9], s[5], t[10], s[6])
    det = F(F(F(s[0] * o[0] + s[1] * o[1]) + s[2] * o[2]) + s[3] * o[3])
    o[4] = tri(t[1], s[1], t[2], s[2], t[5], s[3]) - tri(t[0], s[1], t[3], s[2], t[4], s[3])
    o[5] = tri(t[0], s[0], t[7], s[2], t[8], s[3]) - tri(t[1], s[0], t[6], s[2], t[9], s[3])
    o[6] = tri(t[3], s[0], t[6], s[1], t[11], s[3]) - tri(t[2], s[0], t[7], s[1], t[10], s[3])
    o[7] = tri(t[4], s[0], t[9], s[1], t[10], s[2]) - tri(t[5], s[0], t[8], s[1], t[11], s[2])
    t = [s[2] * s[7], s[3] * s[6], s[1] * s[7], s[3] * s[5], s[1] * s[6], s[2] * s[5], s[0] * s[7], s[3] * s[4],
         s[0] * s[6], s[2] * s[4], s[0] * s[5], s[1] * s[4]]
    o[8] = tri(t[0], s[13], t[3], s[14], t[4], s[15]) - tri(t[1], s[13], t[2], s[14], t[5], s[15])
    o[9] = tri(t[1], s[12], t[6], s[14], t[9], s[15]) - tri(t[0], s[12], t[7], s[14], t[8], s[15])
    o[10] = tri(t[2], s[12], t[7], s[13], t[10], s[15]) - tri(t[3], s[12], t[6], s[13], t[11], s[15])
    o[11] = tri(t[5], s[12], t[8], s[13], t[11], s[14]) - tri(t[4], s[12], t[9], s[13], t[10], s[14])
    o[12] = tri(t[2], s[10], t[5], s[11], t[1], s[9]) - tri(t[4], s[11], t[0], s[9], t[3], s[10])
    o[13] = tri(t[8], s[11], t[0], s[8], t[7], s[10]) - tri(t[6], s[10], t[9], s[11], t[1], s[8])
    o[14] = tri(t[6], s[9], t[11], s[11], t[3], s[8]) - tri(t[10], s[11], t[2], s[8], t[7], s[9])
    o[15] = tri(t[10], s[10], t[4], s[8], t[9], s[9]) - tri(t[8], s[9], t[11], s[10], t[5], s[8])
    return (o * F(F(1) / det)).astype(F)


def camera_rays(M, intr, w, h, range_image):
    """castRay's preamble (:102-116) for every pixel, row-major: float32 [h * w, 8] = (s, t0, e, t1) in metres.  range_image: the
    render state's range image as downloaded ([h, w, 2]); pixel (x, y) reads cell floor(x / 8) + floor(y / 8) * w of its flat form."""
    inv = invert4(M)
    fx, fy, cx, cy = (F(a) for a in intr)
    ifx, ify = F(1) / fx, F(1) / fy
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    x, y = x.reshape(-1), y.reshape(-1)
    mm = np.asarray(range_image, F).reshape(-1, 2)[(x >> 3) + (y >> 3) * w]
    rays = np.zeros((w * h, 8), F)
    for k in range(2):
        pz = mm[:, k]
        px = pz * ((x.astype(F) - cx) * ifx)
        py = pz * ((y.astype(F) - cy) * ify)
        acc = F(0) + px * px
        acc = acc + py * py
        acc = acc + pz * pz
        rays[:, 4 * k + 3] = np.sqrt(acc, dtype=F)
        for r in range(3):
            rays[:, 4 * k + r] = ((inv[r] * px + inv[4 + r] * py) + inv[8 + r] * pz) + inv[12 + r] * F(1)
    return rays


def cast_rays(reader, rays, voxel_size, mu):
    """itm_scene_cast_rays for float32 rays [n, 8] -> float32 [n, 4]: (x, y, z, 1) on a hit, zeros otherwise (a miss's xyz is unspecified)"""
    rays = np.asarray(rays, F).reshape(-1, 8)
    n = len(rays)
    oov = F(1) / F(voxel_size)
    step_scale = F(mu) * oov
    with np.errstate(all="ignore"):
        sc = (rays * oov).astype(F)
        p = sc[:, 0:3].copy()
        total, total_max = sc[:, 3].copy(), sc[:, 7].copy()
        d = (sc[:, 4:7] - p).astype(F)
        norm = F(1) / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], dtype=F)
        d = (d * norm[:, None]).astype(F)
        valid = (np.all(np.abs(sc[:, 0:3]) < RAY_LIMIT, axis=1) & np.all(np.abs(sc[:, 4:7]) < RAY_LIMIT, axis=1) & (np.abs(total) < RAY_LENGTH_LIMIT) &
                 (np.abs(total_max) < RAY_LENGTH_LIMIT) & ~np.all(sc[:, 0:3] == sc[:, 4:7], axis=1) & np.all(np.isfinite(d), axis=1))
        sdf = np.ones(n, F)
        live = np.nonzero(valid & (total < total_max))[0]
        while live.size:
            q = p[live]
            val, found = reader.value(round_ref(q[:, 0]), round_ref(q[:, 1]), round_ref(q[:, 2]))
            band = found & (val <= F(0.1)) & (val >= F(-0.5))
            if band.any():
                val[band] = trilinear(reader, q[band])[0]
            sdf[live] = val
            stop = found & (val <= F(0))
            fwd = np.maximum(val * step_scale, F(1)).astype(F)
            step = np.where(found, fwd, F(8)).astype(F)
            go = live[~stop]
            p[go] = (p[go] + step[~stop][:, None] * d[go]).astype(F)
            total[go] = total[go] + step[~stop]
            live = go[total[go] < total_max[go]]
        hit = np.nonzero(valid & (sdf <= F(0)))[0]
        p[hit] = (p[hit] + (sdf[hit] * step_scale)[:, None] * d[hit]).astype(F)
        val = trilinear(reader, p[hit])[0]
        p[hit] = (p[hit] + (val * step_scale)[:, None] * d[hit]).astype(F)
    out = np.zeros((n, 4), F)
    out[hit, :3] = p[hit]
    out[hit, 3] = F(1)
    return out
