"""Inputs of the weighted ICP tracker tests (tests/test_wicp_tracker.py, tests/golden/make_golden_wicp_tracker.py).

A scene is the ICP maps (points, normals) that three frames of fusion of a synth trajectory leave for the last pose, that pose (the
scene pose, and the natural starting pose of the next frame), the next depth frame and its uncertainty image sigmaZ from
ComputeNormalAndWeights (the 2-pixel border left 0, -1 where no normal).  Everything is computed by a CPU backend: the reference's
own engines where the golden is made, the oracle (its bit-exact CPU restatement) in the tests; the golden holds the digests."""
import numpy as np

import itm_testlib as T
from infinitam_amd import synth
from itm_testlib import Scenario

# 160 x 120: on-axis sphere + frontal wall (the roll about the optical axis is nearly unobservable), and the off-axis yawing camera
SCENES = {
    "frontal": Scenario(name="wicp", w=160, h=120, voxelSize=0.01, frames=3),
    "offaxis": Scenario(name="wicp_off", w=160, h=120, voxelSize=0.01, frames=3, stream=3, trajectory="yaw"),
}
SCENE_VGA = Scenario(name="wicp_vga", voxelSize=0.01, frames=3)     # 640 x 480: one level-0 evaluation per mode

LEVELS = 3
REGIME = [3, 3, 1]                 # BOTH BOTH ROTATION (the default regime's first three levels)
DIST_THRESH = 0.1 * 0.1            # ITMLibSettings::depthTrackerICPThreshold
TERMINATION = 1e-3                 # ITMLibSettings::depthTrackerTerminationThreshold
TRACE_STARTS = ("previous", "twist")


def level_thresholds(levels=LEVELS, dist=DIST_THRESH):
    """distThresh per level as the tracker constructors form it: the full value on the coarsest level, one step less per level."""
    d = [np.float32(0)] * levels
    d[levels - 1] = np.float32(dist)
    step = np.float32(dist) / np.float32(levels)
    for l in range(levels - 2, -1, -1):
        d[l] = np.float32(d[l + 1] - step)
    return [float(v) for v in d]


def mat(m16):
    return np.asarray(m16, np.float64).reshape(4, 4).T


def col(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).T.reshape(16), np.float32)


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float64)


def starts(M_prev):
    """Starting poses pose_d of TrackCamera: the previous frame's pose and perturbations of it (camera-side offsets)."""
    P = mat(M_prev)
    shift = np.eye(4); shift[:3, 3] = (0.004, -0.003, 0.002)
    twist = rot_y(0.01) @ shift
    return {"previous": col(P), "shift": col(shift @ P), "twist": col(twist @ P)}


def eval_inv_poses(M_prev):
    """Inverse poses (camera -> world) of the fixed-pose evaluations: the previous pose and one 3 mm / 0.006 rad off it."""
    P = mat(M_prev)
    off = rot_y(-0.006); off[:3, 3] = (-0.003, 0.002, 0.0)
    return {"at_previous": col(np.linalg.inv(P)), "off": col(np.linalg.inv(off @ P))}


def build(be, sc):
    """(points, normals, M_d of the last fused frame, next depth, sigmaZ) as host arrays, computed on backend `be`."""
    ses = T.Session(be, sc)
    try:
        for k in range(sc.frames):
            v = ses.frame(k)
        points, normals = ses.points.numpy(), ses.normals.numpy()
    finally:
        ses.close()
    depth = np.ascontiguousarray(sc.depth(sc.frames), np.float32)
    return points, normals, np.asarray(v.M_d, np.float32), depth, sigma_z(be, depth, sc.intr())


def sigma_z(be, depth, intr):
    h, w = depth.shape
    d = be.to_backend(depth)
    normals = be.to_backend(np.zeros((h, w, 4), np.float32))
    sigma = be.to_backend(np.zeros((h, w), np.float32))          # the border stays 0, as in the reference's cleared image
    intr = np.asarray(intr, np.float32)
    be.check(be.fn["compute_normal_and_weights"](d.ptr, normals.ptr, sigma.ptr, w, h, intr.ctypes.data, None), "compute_normal_and_weights")
    be.sync()
    return sigma.numpy()


def numpy_pyramid(img, levels):
    """FilterSubsampleWithHoles pyramid (values <= 0 are holes), in the reference's float order."""
    out = [np.asarray(img, np.float32)]
    for _ in range(1, levels):
        a = out[-1]
        h, w = a.shape[0] // 2, a.shape[1] // 2
        taps = [a[0:2 * h:2, 0:2 * w:2], a[0:2 * h:2, 1:2 * w:2], a[1:2 * h:2, 0:2 * w:2], a[1:2 * h:2, 1:2 * w:2]]
        acc = np.zeros((h, w), np.float32); good = np.zeros((h, w), np.float32)
        for t in taps:
            m = t > 0
            acc = np.where(m, acc + t, acc).astype(np.float32); good = np.where(m, good + 1, good).astype(np.float32)
        out.append(np.where(good > 0, acc / np.maximum(good, 1), acc).astype(np.float32))
    return out


def digests(sc_inputs):
    points, normals, M_d, depth, sigma = sc_inputs
    return {"points": synth.sha256(points), "normals": synth.sha256(normals), "M_d": synth.sha256(M_d), "depth": synth.sha256(depth),
            "sigma": synth.sha256(sigma)}
