"""Inputs of tests/test_colour_camera.py: a depth camera of 160 x 120 next to a colour camera of ANOTHER size, with intrinsics of its
own and a rigid offset (Objects/ITMRGBDCalib.h: intrinsics_rgb, intrinsics_d, trafo_rgb_to_depth; ITMView: imgSize_rgb / imgSize_d).

  depth     160 x 120 from synth.depth_frame, 0.01 m voxels, mu 0.02, three frames
  poses     in general position: a small yaw plus a translation that is no multiple of the voxel size, varied per frame (an
            axis-aligned camera at the origin puts a quarter of the voxels exactly on a pixel-rounding tie)
  colour    synth.rgb_frame(wc, hc): a wrong stride or a wrong row shows in every channel
  cameras   larger and ragged 213 x 171, smaller 96 x 72, wider but shorter 224 x 100; each with a focal length that is NOT the depth
            camera's scaled by the size ratio (so that voxels of the colour band leave the colour image through each of its four
            edges) and a principal point off the centre by a fraction of a pixel
  extrinsic one rigid rgb -> depth transform: 0.02 rad about a skew axis, a few centimetres of translation, and its float32 inverse

Every voxel stays far in front of the colour camera (the view frustum starts at 0.35 m, the offset is centimetres)."""
import numpy as np

import itm_testlib as T
from infinitam_amd import capi, synth

W, H = 160, 120
VOXEL_SIZE, MU, FRAMES = 0.01, 0.02, 3
INTR_D = tuple(float(v) for v in synth.intrinsics_for(W, H))

# name -> (wc, hc, focal length as a multiple of the proportional one, principal point off the centre)
CAMERAS = {
    "larger_213x171": (213, 171, 1.6, (0.37, -0.41)),
    "smaller_96x72": (96, 72, 1.45, (-0.29, 0.23)),
    "wide_224x100": (224, 100, 1.2, (0.43, 0.31)),
}
CAMERA_NAMES = list(CAMERAS)


def size(cam):
    return CAMERAS[cam][0], CAMERAS[cam][1]


def intr_rgb(cam):
    wc, hc, scale, (ox, oy) = CAMERAS[cam]
    fx = INTR_D[0] * wc / W * scale
    return (float(np.float32(fx)), float(np.float32(fx * 1.013)), float(np.float32(wc / 2.0 + ox)), float(np.float32(hc / 2.0 + oy)))


def mat(m16):
    return np.asarray(m16, np.float64).reshape(4, 4).T     # column-major storage -> row-major matrix


def col(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).T.reshape(16).astype(np.float32))


def extrinsic():
    """(rgb_to_depth, its float32 inverse): Rodrigues rotation of 0.02 rad about (1, 2, -1) / sqrt 6, translation (31, -12, 7) mm."""
    a = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = 0.02
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    M[:3, 3] = (0.031, -0.012, 0.007)
    calib = col(M)
    return calib, col(np.linalg.inv(mat(calib)))


def position(k):
    return (0.0137 + 0.0061 * k, -0.0071 + 0.0023 * k, 0.0043 - 0.0017 * k)


def pose(k):
    return synth.pose_matrix_yaw(position(k), 0.031 - 0.0087 * k)


def pose_rgb(k):
    """World -> colour camera: calib_inv * pose_d in float32, as the engines form it (matmul4 order of ORUtils)."""
    calib_inv = extrinsic()[1]
    A, B = calib_inv.reshape(4, 4).T, pose(k).reshape(4, 4).T          # float32 row-major
    out = np.zeros((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            acc = np.float32(0)
            for i in range(4):
                acc = np.float32(acc + np.float32(A[r, i] * B[i, c]))
            out[r, c] = acc
    return np.ascontiguousarray(out.T.reshape(16))


def depth(k):
    return synth.depth_frame(W, H, tuple(np.float32(v) for v in position(k)), INTR_D)


def scenario(voxelType, indexType=capi.INDEX_HASH, small_pool=True, **kw):
    """small_pool: a table and pool that a test can download whole in no time (the reference is compiled for the default sizes)."""
    if indexType == capi.INDEX_DENSE:
        kw.update(denseSize=(72, 60, 56), denseOffset=(-36, -30, 97))
    elif small_pool:
        kw.update(bucketNum=0x8000, excessNum=0x2000, localBlockNum=0x2000)
    return T.Scenario(name="colour_camera", w=W, h=H, voxelType=voxelType, indexType=indexType, voxelSize=VOXEL_SIZE, mu=MU, frames=FRAMES, **kw)


class ColourSession(T.Session):
    """A Session whose views carry the colour camera `cam`; rs_size "depth" or "colour": the size of the render state."""

    def __init__(self, be, sc, cam, rs_size="depth", deferred_fusion=True, useSwapping=False):
        self.be, self.sc, self.cam = be, sc, cam
        self.scene = be.create_scene(sc.voxelType, sc.indexType, sc.params(), bucketNum=sc.bucketNum, excessNum=sc.excessNum,
                                     localBlockNum=sc.localBlockNum, denseSize=sc.denseSize, denseOffset=sc.denseOffset, useSwapping=useSwapping)
        self.scene.reco.ResetScene()
        self.enable_deferred_fusion(deferred_fusion)
        self.wc, self.hc = size(cam)
        self.rw, self.rh = (self.wc, self.hc) if rs_size == "colour" else (W, H)
        self.rs = self.scene.vis.CreateRenderState((self.rw, self.rh))
        self.points = capi.DevBuffer(be, W * H * 16, np.float32, (H, W, 4))          # ICP maps: only with a render state of the depth size
        self.normals = capi.DevBuffer(be, W * H * 16, np.float32, (H, W, 4))
        self.rgb = be.to_backend(synth.rgb_frame(self.wc, self.hc))
        self.calib, self.calib_inv = extrinsic()
        P = self.rw * self.rh
        self.loc = capi.DevBuffer(be, P * 16, np.float32, (P, 4))
        self.col = capi.DevBuffer(be, P * 16, np.float32, (P, 4))
        self._depth = None

    def view(self, k):
        self._depth = self.be.to_backend(depth(k))
        return capi.View(self._depth, W, H, M_d=pose(k), intr_d=INTR_D, rgb=self.rgb, w_rgb=self.wc, h_rgb=self.hc,
                         intr_rgb=intr_rgb(self.cam), rgb_to_depth=self.calib, rgb_to_depth_inv=self.calib_inv)

    def state(self):
        """What the restatement of an integration step starts from (and what it is compared with afterwards)."""
        s = self.scene
        out = {"voxels": s.download(capi.BUF_VOXEL_BLOCKS)}
        if s.is_hash:
            out["hash"] = s.download(capi.BUF_HASH_ENTRIES)
            n = s.counters(self.rs)["noVisibleEntries"]
            out["visible"] = s.download(capi.BUF_VISIBLE_IDS, self.rs)[:n].copy()
        return out

    def prepare_colour(self, k, v):
        """The TRACKER_COLOR branch of ITMTrackingController::Prepare (Engine/ITMTrackingController.cpp:37-45): expected depths through
        the colour camera, then CreatePointCloud, with skipPoints on and off."""
        s, rs, out = self.scene, self.rs, {}
        for skip in (True, False):
            s.vis.CreateExpectedDepths(pose_rgb(k), intr_rgb(self.cam), rs)
            s.vis.CreatePointCloud(v, rs, self.loc, self.col, skipPoints=skip)
            n = s.counters(rs)["noTotalPoints"]
            out[f"count_{int(skip)}"] = n
            out[f"locations_{int(skip)}"] = self.loc.numpy()[:n].copy()
            out[f"colours_{int(skip)}"] = self.col.numpy()[:n].copy()
            out[f"grey_{int(skip)}"] = s.download(capi.BUF_RAYCAST_IMAGE, rs).copy()
            out[f"range_{int(skip)}"] = T.range_region(s.download(capi.BUF_RANGE_IMAGE, rs), self.rw, self.rh).copy()
        return out


def used_blocks(state):
    """The voxel blocks the table points to, in slot order (what a comparison of two hash scenes needs of the pool)."""
    ptr = state["hash"]["ptr"]
    return state["voxels"].reshape(-1, 512)[ptr[ptr >= 0]]
