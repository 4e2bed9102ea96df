"""Inputs of the Ren SDF tracker tests (tests/test_ren_tracker.py) and of their golden generator
(tests/golden/make_golden_ren_tracker.py): scenes fused from the first frames of the parity trajectory of infinitam_amd.synth, the
depth frame one step further along it, evaluation poses around its true pose and perturbed starting poses for TrackCamera.
Everything is regenerated from synth; the golden stores SHA-256 digests of the inputs next to the reference's outputs."""
import numpy as np

import itm_testlib as T
from infinitam_amd import synth

FUSED_FRAMES = 3          # frames 0..2 fused into the scene
TRACKED_FRAME = 3         # the depth frame that is tracked

# name -> scenario of the fused scene (the library and the reference fuse the same frames bit for bit).  TrackCamera is compared
# on the 160 x 120 scenes: at 640 x 480 the reference's sequential float energy is ~1e-3 off (300 000 positive terms), ten times
# its 1e-4 stopping threshold, so where it stops is decided by its rounding; VGA_SCENES are compared evaluation by evaluation only.
SCENES = {
    "hash_s": T.Scenario(name="ren_hash_s", w=160, h=120, voxelSize=0.01, frames=FUSED_FRAMES),
    "hash_f_rgb": T.Scenario(name="ren_hash_f_rgb", w=160, h=120, voxelSize=0.01, frames=FUSED_FRAMES, voxelType=T.VOXEL_F_RGB,
                             colour=True),
    "dense_s": T.Scenario(name="ren_dense_s", w=160, h=120, voxelSize=0.01, frames=FUSED_FRAMES, indexType=T.INDEX_DENSE,
                          denseSize=(64, 64, 64), denseOffset=(-32, -32, 95)),
    "vga_hash_s": T.Scenario(name="ren_vga_hash_s", frames=FUSED_FRAMES),
}
VGA_SCENES = ("vga_hash_s",)


def mat(m16):
    return np.asarray(m16, np.float64).reshape(4, 4).T     # column-major storage -> row-major matrix


def col(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).T.reshape(16).astype(np.float32))


def inv_col(m16):
    return col(np.linalg.inv(mat(m16)))


def true_pose(sc):
    return sc.pose(TRACKED_FRAME)


def depth(sc):
    return np.ascontiguousarray(sc.depth(TRACKED_FRAME))


# starting poses of TrackCamera (world -> camera), around the true pose (0.03, 0, 0) of the tracked frame
def starts():
    return {
        "previous": synth.pose_matrix((0.02, 0.0, 0.0)),                              # the pose of the last fused frame
        "yaw": synth.pose_matrix_yaw((0.03, 0.004, 0.0), np.deg2rad(0.5)),
        "both": synth.pose_matrix_yaw((0.036, -0.004, 0.003), np.deg2rad(-0.7)),
    }


# camera -> world matrices F and G are evaluated at
def eval_inv_poses(sc):
    out = {"truth": inv_col(true_pose(sc))}
    for k, v in starts().items():
        out[k] = inv_col(v)
    return out


def unproject(depth_img, intr):
    """Restatement of UnprojectDepthToCam in float32: ooIntrinsics applied to (x z, y z, z); (0, 0, 0, -1) where z <= 0."""
    f32 = np.float32
    h, w = depth_img.shape
    fx, fy, cx, cy = (f32(v) for v in intr)
    ox, oy = f32(1.0) / fx, f32(1.0) / fy
    oz, ow = -cx * ox, -cy * oy
    z = depth_img.astype(f32)
    xs = np.arange(w, dtype=f32)[None, :] * z
    ys = np.arange(h, dtype=f32)[:, None] * z
    out = np.zeros((h, w, 4), f32)
    ok = z > 0
    out[..., 0] = np.where(ok, ox * xs + oz * z, f32(0))
    out[..., 1] = np.where(ok, oy * ys + ow * z, f32(0))
    out[..., 2] = np.where(ok, z, f32(0))
    out[..., 3] = np.where(ok, f32(1), f32(-1))
    return out


def mrp_matrix(step):
    """Restatement of GetMFromParam in float32: translation step[0..2], modified Rodrigues rotation step[3..5] (column-major)."""
    f32 = np.float32
    s = [f32(v) for v in step]
    a, b, c = s[3], s[4], s[5]
    q = a * a + b * b + c * c
    u = f32(1) - q
    four, eight = f32(4), f32(8)
    R = [four * a * a - four * b * b - four * c * c + u * u, eight * a * b - four * c * u, eight * a * c + four * b * u,
         eight * a * b + four * c * u, four * b * b - four * a * a - four * c * c + u * u, eight * b * c - four * a * u,
         eight * a * c - four * b * u, eight * b * c + four * a * u, four * c * c - four * b * b - four * a * a + u * u]
    den = (f32(1) + q) * (f32(1) + q)
    R = [f32(r / den) for r in R]
    m = np.zeros(16, f32)
    for cc in range(3):
        for r in range(3):
            m[4 * cc + r] = R[3 * r + cc]
    m[12:15] = s[:3]
    m[15] = 1
    return m


MRP_STEPS = [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.001, -0.002, 0.0005, 0.003, -0.001, 0.002), (0.01, 0.02, -0.03, -0.05, 0.04, 0.1),
             (-0.2, 0.1, 0.05, 0.3, -0.25, 0.6)]

