"""numpy restatement of the fixed-point mesh smoothing (include/itm_hip.h: itm_mesh_smooth), written from the header's sequential
definition and not from the kernels: neighbour entries with np.add.at, `//` for the floor division, `>>` for the arithmetic shift,
np.rint of a float64 quotient for the quantisation.  Also the meshes the tests share (icosphere, fan, double cone)."""
import numpy as np

F = np.float32
PIN_IRREGULAR = 1
LIMIT = 1 << 30
MAX_STEPS = 1 << 16                      # ITM_MESH_SMOOTH_MAX_STEPS
STATS = ("noVertices", "noMoving", "noIrregular", "noIsolated", "maxEntries", "steps")


class Refused(Exception):
    """the call answers ITM_ERR_INVALID and changes nothing"""


def config(steps=20, lam=0.5, mu=-0.53, quantum=0.005 / 1024, pin=True, reserved=(0, 0, 0)):
    return dict(steps=int(steps), lambdaQ16=int(round(lam * 65536)), muQ16=int(round(mu * 65536)), quantum=F(quantum),
                flags=PIN_IRREGULAR if pin is True else int(pin), reserved=tuple(reserved))


def check_config(cfg):
    if not 0 <= cfg["steps"] <= MAX_STEPS:
        raise Refused("steps")
    if abs(cfg["lambdaQ16"]) > 65536 or abs(cfg["muQ16"]) > 65536:
        raise Refused("factor")
    q = F(cfg["quantum"])
    if not (np.isfinite(q) and q > 0):
        raise Refused("quantum")
    if cfg["flags"] & ~PIN_IRREGULAR or any(cfg["reserved"]):
        raise Refused("flags / reserved")


def entries(faces, n_vertices):
    """(owner, neighbour) of every neighbour entry: a proper triangle gives each corner one entry per other corner"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= n_vertices):
        raise Refused("face index")
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])]
    owner = np.concatenate([f[:, 0], f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2]])
    other = np.concatenate([f[:, 1], f[:, 2], f[:, 0], f[:, 2], f[:, 0], f[:, 1]])
    return owner, other


def topology(faces, n_vertices):
    """(n, irregular, isolated) per vertex"""
    owner, other = entries(faces, n_vertices)
    n = np.bincount(owner, minlength=n_vertices).astype(np.int64)
    # multiplicity of every distinct (owner, neighbour) pair; irregular iff one of a vertex's pairs occurs other than twice
    pairs, times = np.unique(owner * np.int64(n_vertices) + other, return_counts=True)
    irregular = np.zeros(n_vertices, bool)
    irregular[(pairs // n_vertices)[times != 2]] = True
    return n, irregular, n == 0


def quantise(vertices, quantum):
    v = np.asarray(vertices, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        r = np.rint(v.astype(np.float64) / np.float64(F(quantum)))
    if not np.all(np.isfinite(r)) or np.any(np.abs(r) > LIMIT):
        raise Refused("coordinate")
    return r.astype(np.int64)


def one_pass(x, owner, other, n, moving, f):
    S = np.zeros_like(x)
    np.add.at(S, owner, x[other])
    nn = np.maximum(n, 1)[:, None]
    a = S - n[:, None] * x
    d = (2 * a + nn) // (2 * nn)
    s = (int(f) * d + 32768) >> 16
    out = np.clip(x + s, -LIMIT, LIMIT)
    return np.where(moving[:, None], out, x)


def smooth(vertices, faces, cfg):
    """-> (vertices' float32 [n, 3], flags uint8 [n] (bit 0 irregular, bit 1 isolated), stats dict); raises Refused"""
    check_config(cfg)
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    nV = len(v)
    owner, other = entries(faces, nV)
    n, irregular, isolated = topology(faces, nV)
    moving = ~isolated & ~(irregular if cfg["flags"] & PIN_IRREGULAR else np.zeros(nV, bool))
    flags = (irregular.astype(np.uint8) | (isolated.astype(np.uint8) << 1)).astype(np.uint8)
    stats = dict(noVertices=nV, noMoving=int(moving.sum()), noIrregular=int(irregular.sum()), noIsolated=int(isolated.sum()),
                 maxEntries=int(n.max()) if nV else 0, steps=cfg["steps"] if nV else 0)
    out = v.copy()
    if cfg["steps"] == 0 or nV == 0:
        return out, flags, stats
    x = quantise(v, cfg["quantum"])
    for i in range(cfg["steps"]):
        x = one_pass(x, owner, other, n, moving, cfg["muQ16"] if i & 1 else cfg["lambdaQ16"])
    deq = (x.astype(np.float64) * np.float64(F(cfg["quantum"]))).astype(F)
    out[moving] = deq[moving]
    return out, flags, stats


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- meshes -----------------------------------------------------------------------------------------------------------------------

def icosphere(subdivisions):
    """unit icosphere: (vertices float64 [n, 3], faces int64 [t, 3]), outward winding"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v, np.float64), np.array(f, np.int64)


def noisy_icosphere(subdivisions=4, sigma=0.02, seed=7):
    v, f = icosphere(subdivisions)
    radius = 1.0 + sigma * np.random.RandomState(seed).standard_normal(len(v))
    return (v * radius[:, None]).astype(F), f


def enclosed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def fan(rim=6, closed=True):
    """vertex 0 in the middle of `rim` rim vertices 1 .. rim; closed: a full disc (the centre is interior), open: one triangle missing"""
    ang = 2 * np.pi * np.arange(rim) / rim
    v = np.concatenate([[[0.0, 0.0, 0.25]], np.stack([np.cos(ang), np.sin(ang), np.zeros(rim)], 1)]).astype(F)
    k = np.arange(rim if closed else rim - 1)
    f = np.stack([np.zeros(len(k), np.int64), 1 + k, 1 + (k + 1) % rim], 1)
    return v, f


def double_cone(rim=5000):
    """two apexes (vertices 0 and 1) over one ring of `rim` vertices: `rim` triangles around each apex, n(apex) = 2 rim; closed, manifold"""
    ang = 2 * np.pi * np.arange(rim) / rim
    ring = np.stack([np.cos(ang), np.sin(ang), 0.01 * np.sin(7 * ang)], 1)
    v = np.concatenate([[[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], ring]).astype(F)
    k = np.arange(rim)
    up = np.stack([np.zeros(rim, np.int64), 2 + k, 2 + (k + 1) % rim], 1)
    down = np.stack([np.ones(rim, np.int64), 2 + (k + 1) % rim, 2 + k], 1)
    return v, np.concatenate([up, down])
