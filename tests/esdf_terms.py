"""Integer / float32 numpy restatement of the distance field (include/itm_hip.h: itm_scene_esdf, itm_esdf_transform), no scipy:

  classify             the state byte of every cell of a box, from a scene_query_terms.SceneReader (locate, value, weight)
  transform_brute      the definition as written: all cells x all sites, ties to the smallest linear index
  transform_separable  x, y, z passes, candidates ascending with a strict `<`, a window of +-R per axis: the fast form for larger grids
  distance             voxelSize * sqrt(dist2) in float32, negated where INSIDE, +-inf for NONE

Grids are [nz, ny, nx] arrays: the flat index of cell (i, j, k) is the linear index i + nx * (j + ny * k) of the definition."""
import numpy as np

F = np.float32
STORED, OBSERVED, INSIDE, SITE = 1, 2, 4, 8
SITE_SURFACE, SITE_UNKNOWN = 1, 2
NONE = 0x7fffffff


def classify(reader, box, sites, min_weight):
    """state uint8 [nz, ny, nx] of the box (origin (ox, oy, oz), size (nx, ny, nz)).  sites: mask of SITE_SURFACE / SITE_UNKNOWN."""
    (ox, oy, oz), (nx, ny, nz) = box
    # the box with its one-voxel halo: the surface rule reads neighbours outside the box from the scene
    k, j, i = np.meshgrid(np.arange(oz - 1, oz + nz + 1), np.arange(oy - 1, oy + ny + 1), np.arange(ox - 1, ox + nx + 1), indexing="ij")
    x, y, z = i.reshape(-1), j.reshape(-1), k.reshape(-1)
    stored = np.asarray(reader.locate(x, y, z)[1], bool)
    observed = stored & (reader.weight(x, y, z).astype(np.int64) >= min_weight)
    inside = observed & (reader.value(x, y, z)[0] <= F(0))
    shape = (nz + 2, ny + 2, nx + 2)
    stored, observed, inside = (a.reshape(shape) for a in (stored, observed, inside))
    core = (slice(1, -1),) * 3
    site = np.zeros((nz, ny, nx), bool)
    if sites & SITE_SURFACE:
        for axis in range(3):
            for lo in (0, 2):
                nb = tuple(slice(lo, lo + n) if a == axis else slice(1, -1) for a, n in zip(range(3), (nz, ny, nx)))
                site |= observed[core] & observed[nb] & (inside[nb] != inside[core])
    if sites & SITE_UNKNOWN:
        site |= ~observed[core]
    return (stored[core] * STORED + observed[core] * OBSERVED + inside[core] * INSIDE + site * SITE).astype(np.uint8)


def transform_brute(state, R):
    """(dist2 int32, nearest int32) [nz, ny, nx]: for every cell the minimum over ALL sites of |c - s|^2, the smallest linear index
    among ties; NONE / -1 where that exceeds R^2 (R > 0) or there is no site."""
    state = np.asarray(state)
    nz, ny, nx = state.shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cells = np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)], 1).astype(np.int64)
    s = np.nonzero((state.reshape(-1) & SITE) != 0)[0]          # ascending linear index
    dist2 = np.full(len(cells), NONE, np.int64)
    nearest = np.full(len(cells), -1, np.int64)
    if len(s):
        d = ((cells[:, None, :] - cells[s][None, :, :]) ** 2).sum(2)
        first = d.argmin(1)                                     # the first minimum: the smallest index
        dist2, nearest = d[np.arange(len(cells)), first], s[first]
        if R > 0:
            far = dist2 > R * R
            dist2[far], nearest[far] = NONE, -1
    return dist2.astype(np.int32).reshape(state.shape), nearest.astype(np.int32).reshape(state.shape)


def _pass(f, n, axis, R):
    """one pass along `axis`: min over q of f[q] + (p - q)^2, q ascending, strict `<`, |p - q| <= R when R > 0"""
    f, n = np.moveaxis(f, axis, 0), np.moveaxis(n, axis, 0)
    L = f.shape[0]
    best, site = np.full_like(f, NONE), np.full_like(n, -1)
    for q in range(L):
        lo, hi = (max(0, q - R), min(L, q + R + 1)) if R > 0 else (0, L)
        d = ((np.arange(lo, hi) - q) ** 2).reshape((-1,) + (1,) * (f.ndim - 1))
        cand = np.where(f[q] != NONE, f[q] + d, NONE)
        better = cand < best[lo:hi]
        best[lo:hi] = np.where(better, cand, best[lo:hi])
        site[lo:hi] = np.where(better, n[q], site[lo:hi])
    return np.moveaxis(best, 0, axis), np.moveaxis(site, 0, axis)


def transform_separable(state, R):
    """transform_brute's result through three 1-D passes (x, y, z)"""
    state = np.asarray(state)
    is_site = (state & SITE) != 0
    f = np.where(is_site, 0, NONE).astype(np.int64)
    n = np.where(is_site, np.arange(state.size).reshape(state.shape), -1).astype(np.int64)
    for axis in (2, 1, 0):
        f, n = _pass(f, n, axis, R)
    if R > 0:
        far = f > R * R
        f, n = np.where(far, NONE, f), np.where(far, -1, n)
    return f.astype(np.int32), n.astype(np.int32)


def distance(dist2, state, voxel_size):
    """float32: voxelSize * sqrtf((float)dist2), negated where INSIDE; +-inf for NONE"""
    dist2 = np.asarray(dist2)
    m = np.where(dist2 == NONE, F(np.inf), F(voxel_size) * np.sqrt(dist2.astype(F), dtype=F)).astype(F)
    return np.where((np.asarray(state) & INSIDE) != 0, -m, m).astype(F)


def esdf(reader, box, sites, min_weight, R, voxel_size):
    """every output of itm_scene_esdf"""
    state = classify(reader, box, sites, min_weight)
    dist2, nearest = transform_separable(state, R)
    return {"state": state, "dist2": dist2, "nearest": nearest, "distance": distance(dist2, state, voxel_size)}
