"""numpy restatement of the indexed mesh (include/itm_hip.h: itm_mesh_index) and of the two files written from it.

With s_j the vertices of the triangle buffer in buffer order: two of them are the same vertex iff their three floats have the same
96 bits; first[k] is the smallest j holding the k-th distinct position, first strictly ascending; vertices[k] = s_first[k];
faces[i] = the indices of s_3i, s_3i+1, s_3i+2.  Every triangle is kept, so vertices[faces] is the soup bit for bit."""
import numpy as np

F = np.float32


def index(triangles):
    """(vertices [nV, 3] float32, faces [n, 3] uint32, first [nV] uint32) of float32 triangles [n, 3, 3]"""
    soup = np.ascontiguousarray(triangles, F).reshape(-1, 3)
    if len(soup) == 0:
        return np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32)
    keys = soup.view(np.dtype((np.void, 12))).reshape(-1)           # bytes, not values: -0.0 and +0.0 are two keys
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                         # renumber by ascending first occurrence
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    first = first[order]
    return soup[first], rank[inverse.reshape(-1)].astype(np.uint32).reshape(-1, 3), first.astype(np.uint32)


def ply_bytes_indexed(vertices, faces, normals=None, colours=None):
    """the file itm_mesh_write_ply_indexed writes: vertices [nV, 3], faces uint32 [n, 3], normals [nV, 3] or None, colours uint8
    [nV, 4] or None"""
    vtx = np.ascontiguousarray(vertices, "<f4").reshape(-1, 3)
    fcs = np.asarray(faces).reshape(-1, 3)
    head = ["ply", "format binary_little_endian 1.0", "comment itm-hip mesh", f"element vertex {len(vtx)}",
            "property float x", "property float y", "property float z"]
    fields = [("p", "<f4", 3)]
    if normals is not None:
        head += ["property float nx", "property float ny", "property float nz"]
        fields.append(("n", "<f4", 3))
    if colours is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
        fields.append(("c", "u1", 3))
    head += [f"element face {len(fcs)}", "property list uchar int vertex_indices", "end_header"]
    v = np.zeros(len(vtx), np.dtype(fields))            # packed: no padding between the fields
    v["p"] = vtx
    if normals is not None:
        v["n"] = np.asarray(normals, "<f4").reshape(-1, 3)
    if colours is not None:
        v["c"] = np.asarray(colours, np.uint8).reshape(-1, 4)[:, :3]
    f = np.zeros(len(fcs), np.dtype([("k", "u1"), ("i", "<i4", 3)]))
    f["k"] = 3
    f["i"] = fcs[:, ::-1]                                # WriteOBJ's winding
    return ("\n".join(head) + "\n").encode() + v.tobytes() + f.tobytes()


def obj_text_indexed(vertices, faces):
    """the file itm_mesh_write_obj_indexed writes (ITMMesh::WriteOBJ's format): "v %f %f %f" per unique vertex, "f c+1 b+1 a+1" per
    triangle"""
    vtx = np.asarray(vertices, F).reshape(-1, 3).astype(np.float64)     # what printf's %f receives
    out = ["v %f %f %f\n" % (p[0], p[1], p[2]) for p in vtx]
    out += ["f %d %d %d\n" % (t[2] + 1, t[1] + 1, t[0] + 1) for t in np.asarray(faces).reshape(-1, 3).astype(np.int64)]
    return "".join(out).encode()
