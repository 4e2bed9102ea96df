"""numpy restatement of the connected components of the indexed mesh (include/itm_hip.h: itm_mesh_components) and of the fragment
filter (itm_mesh_filter_components).

On the index (vertices [nV, 3], faces [n, 3]): two vertices are linked iff some triangle names both (degenerate triangles count like
any other; nothing is linked by position), a component is a class of the transitive closure, root = its smallest vertex index,
components are numbered by ascending root.  vertexComponent[k] = the number of k's component, triangleComponent[i] = vertexComponent[
faces[i][0]], stats[c] = {firstVertex = root, noVertices, noTriangles, reserved = 0, bbMin, bbMax}; the box is the per-axis minimum and
maximum of the component's vertices in the total order of the IEEE bit patterns (-0.0 < +0.0), stored as the vertices' own bits.

Labelled here by min-label hooking with pointer jumping: every vertex carries a label <= its index; per sweep the two labels of every
edge are compared and the larger label's vertex -- a root, after the jumping -- takes the smaller as its label; label = label[label]
until nothing moves; repeat until every edge agrees."""
import numpy as np

F = np.float32
COMPONENT = np.dtype([("firstVertex", np.uint32), ("noVertices", np.uint32), ("noTriangles", np.uint32), ("reserved", np.uint32),
                      ("bbMin", np.float32, 3), ("bbMax", np.float32, 3)])
assert COMPONENT.itemsize == 40


def order_key(bits):
    """uint32 float bits -> a uint32 that ascends with the IEEE total order (sign-magnitude)"""
    b = np.asarray(bits, np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def order_bits(key):
    k = np.asarray(key, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)


def roots(faces, n_vertices):
    """root(k) for every vertex: the smallest vertex index of its component"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    label = np.arange(n_vertices, dtype=np.int64)
    if len(f) == 0:
        return label
    ea = np.concatenate([f[:, 0], f[:, 0]])
    eb = np.concatenate([f[:, 1], f[:, 2]])
    while True:
        la, lb = label[ea], label[eb]
        differ = la != lb
        if not differ.any():
            return label
        lo, hi = np.minimum(la, lb)[differ], np.maximum(la, lb)[differ]
        order = np.argsort(-lo, kind="stable")           # assignments in descending order of the value: the smallest is written last
        label[hi[order]] = lo[order]                     # hi is a root (label[hi] == hi): it loses no link by taking a smaller label
        while True:
            jumped = label[label]
            if np.array_equal(jumped, label):
                break
            label = jumped


def components(faces, vertices):
    """(vertexComponent [nV] uint32, triangleComponent [n] uint32, stats [nC] COMPONENT) of the index (vertices [nV, 3] float32,
    faces [n, 3])"""
    vtx = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    root = roots(f, len(vtx))
    first = np.flatnonzero(root == np.arange(len(vtx)))                 # the roots, ascending: component c is the c-th of them
    vc = np.searchsorted(first, root).astype(np.uint32)
    tc = vc[f[:, 0]] if len(f) else np.zeros(0, np.uint32)
    stats = np.zeros(len(first), COMPONENT)
    stats["firstVertex"] = first
    stats["noVertices"] = np.bincount(vc, minlength=len(first))
    stats["noTriangles"] = np.bincount(tc, minlength=len(first))
    if len(first):
        order = np.argsort(vc, kind="stable")                           # the vertices component by component (each has at least its root)
        starts = np.searchsorted(vc[order], np.arange(len(first)))
        keys = order_key(vtx.view(np.uint32))[order]
        stats["bbMin"] = order_bits(np.minimum.reduceat(keys, starts, axis=0)).view(F)
        stats["bbMax"] = order_bits(np.maximum.reduceat(keys, starts, axis=0)).view(F)
    return vc, tc, stats


def kept_components(stats, min_triangles=0, keep=None):
    """bool per component: kept by itm_mesh_filter_components(min_triangles, keep)"""
    k = stats["noTriangles"] >= min_triangles
    if keep is not None:
        assert len(keep) == len(stats)
        k = k & (np.asarray(keep) != 0)
    return k


def filtered(tri, triangle_component, stats, min_triangles=0, keep=None):
    """the triangle buffer after the filter: the kept triangles of `tri` [n, 3, 3], in their order"""
    return np.ascontiguousarray(tri)[kept_components(stats, min_triangles, keep)[np.asarray(triangle_component, np.int64)]]


def largest(stats, n=1):
    """the keep mask of Mesh.KeepLargest(n): the n components with the most triangles, ties to the lower number"""
    keep = np.zeros(len(stats), np.uint8)
    keep[np.argsort(-stats["noTriangles"].astype(np.int64), kind="stable")[:n]] = 1
    return keep
