"""Scenarios of the mesh vertex attributes (tests/test_mesh_attributes.py, tests/golden/make_golden_mesh_attributes.py): the five
scenes of test_meshing.test_hip_mesh_equals_oracle_mesh; three of them have reference data in tests/golden/g_mesh_attributes.*."""
import numpy as np

import itm_testlib as T
from infinitam_amd.capi import BUF_HASH_ENTRIES, BUF_VOXEL_BLOCKS, Mesh
from itm_testlib import Scenario

SCENES = {
    "mesh_micro": Scenario(name="mesh_micro", w=160, h=120, voxelSize=0.01, frames=3),
    "mesh_vga_4mm": Scenario(name="mesh_vga_4mm", voxelSize=0.004, frames=3, trajectory="bench"),
    "mesh_f_rgb": Scenario(name="mesh_f_rgb", w=160, h=120, voxelSize=0.01, frames=2, voxelType=T.VOXEL_F_RGB, colour=True),
    "mesh_s_rgb_yaw": Scenario(name="mesh_s_rgb_yaw", w=320, h=240, voxelSize=0.005, frames=3, voxelType=T.VOXEL_S_RGB, colour=True,
                               trajectory="yaw"),
    "mesh_f": Scenario(name="mesh_f", w=160, h=120, voxelSize=0.01, frames=2, voxelType=T.VOXEL_F),
}
GOLDEN_SCENES = {k: SCENES[k] for k in ("mesh_micro", "mesh_f_rgb", "mesh_s_rgb_yaw")}
DENSE = Scenario(name="mesh_dense", w=160, h=120, voxelSize=0.01, frames=2, indexType=T.INDEX_DENSE, denseSize=(64, 64, 64),
                 denseOffset=(-32, -32, 95))


def fuse(be, sc, frames=None, deferred_fusion=True, fused=False):
    ses = T.Session(be, sc, deferred_fusion=deferred_fusion)
    for k in range(sc.frames if frames is None else frames):
        ses.frame(k, fused=fused)
    return ses


def scene_and_mesh(be, sc):
    """(hash entries, voxel blocks, triangles [n, 3, 3]) of the fused scenario on a backend"""
    ses = fuse(be, sc)
    m = Mesh(ses.scene)
    m.MeshScene()
    out = ses.scene.download(BUF_HASH_ENTRIES), ses.scene.download(BUF_VOXEL_BLOCKS), m.triangles()
    m.close()
    ses.close()
    return out


def geometric_normals(tri):
    """normal of every triangle with the winding WriteOBJ writes (p2, p1, p0), float64, not normalised"""
    t = np.asarray(tri, np.float64)
    return np.cross(t[:, 1] - t[:, 2], t[:, 0] - t[:, 2])
