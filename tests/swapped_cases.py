"""Swapping scenes for tests: test_swapping's sequence (three frames on the sphere-and-wall scene, four looking at a wall 1.3 rad away,
three back) at 320 x 240 and 1 cm voxels, in a pool of 0x4000 blocks with 0x200 blocks moved per swapping call.  The scene is 932 blocks
then; after the first frame away 512 of them -- the first in TABLE order, which in space is salt and pepper -- have ptr == -1 and live in
the host cache alone: "the half-swapped scene" (HALF frames).

`Run` drives one such scene frame by frame in the call orders the product offers; `swapping_scene` is the fixture the merge, coarsen and
resample tests build on."""
import numpy as np

import test_swapping
from infinitam_amd import capi, synth

W, H = test_swapping.W, test_swapping.H
POOL = 0x4000
TRANSFER = 0x200
VOXEL_SIZE = 0.01
HALF = 4                   # frames after which the scene is half swapped: three on the scene, one away
FRAMES = 10

_sequence = []


def sequence():
    """(intrinsics, [(pose, depth)] * 10), computed once"""
    if not _sequence:
        _sequence.append(test_swapping.poses_and_depths())
    return _sequence[0]


# what a frame is made of (Engine/ITMDenseMapper.cpp:50-64, ITMTrackingController::Prepare)
ORDERS = {
    "build": ("allocate", "integrate", "swap_in", "swap_out"),                                        # the fixture: no free-view calls
    "reference": ("allocate", "integrate", "swap_in", "swap_out", "expected", "icp"),                 # the reference's own order
    "calls": ("allocate", "integrate", "expected", "icp", "swap_in", "swap_out"),                     # what process_frame fuses, then the swap calls
    "fused": ("process_frame", "swap_in", "swap_out"),
    "ahead": ("process_frame_ahead", "swap_in", "swap_out"),
}


class Run:
    """One swapping scene, its render state and its views."""

    def __init__(self, be, voxel=capi.VOXEL_S, colour=False, deferred=False, params=None):
        self.be, self.colour = be, colour
        self.intr, self.seq = sequence()
        self.scene = be.create_scene(voxel, capi.INDEX_HASH, params or capi.default_params(voxelSize=VOXEL_SIZE), useSwapping=True, localBlockNum=POOL,
                                     transferBlockNum=TRANSFER)
        if deferred:
            self.scene.set_deferred_fusion(True)
        self.scene.reco.ResetScene()
        self.rs = self.scene.vis.CreateRenderState((W, H))
        self.points = capi.DevBuffer(be, W * H * 16, np.float32, (H, W, 4))
        self.normals = capi.DevBuffer(be, W * H * 16, np.float32, (H, W, 4))
        self.rgb = be.to_backend(synth.rgb_frame(W, H)) if colour else None
        self._depth = {}
        self.combined = 0          # see frame(count_combined=True)

    def view(self, k):
        M, depth = self.seq[k]
        if k not in self._depth:
            self._depth[k] = self.be.to_backend(depth)
        if self.rgb is None:
            return capi.View(self._depth[k], W, H, M_d=M, intr_d=self.intr)
        return capi.View(self._depth[k], W, H, M_d=M, intr_d=self.intr, rgb=self.rgb, w_rgb=W, h_rgb=H, intr_rgb=self.intr)

    def selected_for_combination(self):
        """How many entries the next IntegrateGlobalIntoLocal combines with a cached block of non-zero weight: the first TRANSFER entries
        in state 1 in table order, of those the flagged ones -- from downloads, not from the call."""
        states, flags = self.scene.download(capi.BUF_SWAP_STATES), self.scene.global_cache_flags()
        n = 0
        for e in np.nonzero(states == 1)[0][:TRANSFER]:
            if flags[e] and np.any(self.scene.global_cache_block(int(e))["w_depth"] > 0):
                n += 1
        return n

    def frame(self, k, order="reference", announce=None, count_combined=False):
        """announce: the frame whose view process_frame_ahead is told comes next (order "ahead")"""
        s, rs, v = self.scene, self.rs, self.view(k)
        for step in ORDERS[order]:
            if step == "allocate":
                s.reco.AllocateSceneFromDepth(v, rs)
            elif step == "integrate":
                s.reco.IntegrateIntoScene(v, rs)
            elif step == "swap_in":
                if count_combined:
                    self.combined += self.selected_for_combination()
                s.swap_integrate_global_into_local(rs)
            elif step == "swap_out":
                s.swap_save_to_global_memory(rs)
            elif step == "expected":
                s.vis.CreateExpectedDepths(v.M_d, v.intr_d, rs)
            elif step == "icp":
                s.vis.CreateICPMaps(v, rs, self.points, self.normals)
            elif step == "process_frame":
                s.process_frame(v, rs, self.points, self.normals)
            elif step == "process_frame_ahead":
                s.process_frame_ahead(v, None if announce is None else self.view(announce), rs, self.points, self.normals)
        return v

    def snapshot(self):
        """What test_swapping.compare reads, with EVERY cached block in the place of its sample."""
        s, rs = self.scene, self.rs
        c = s.counters(rs)
        flags = s.global_cache_flags()
        stored = np.nonzero(flags)[0]
        return dict(counters={k: c[k] for k in ("lastFreeBlockId", "lastFreeExcessListId", "noVisibleEntries")},
                    hash=s.download(capi.BUF_HASH_ENTRIES), alloc=s.download(capi.BUF_ALLOCATION_LIST), voxels=s.download(capi.BUF_VOXEL_BLOCKS),
                    vis_ids=s.download(capi.BUF_VISIBLE_IDS, rs)[: c["noVisibleEntries"]].copy(), vis_type=s.download(capi.BUF_VISIBLE_TYPE, rs),
                    swap=s.download(capi.BUF_SWAP_STATES), flags=flags, sample=stored, blocks=[s.global_cache_block(int(e)) for e in stored],
                    raycast=s.download(capi.BUF_RAYCAST_RESULT, rs), points=self.points.numpy().copy())

    def close(self):
        self.rs.close(); self.scene.close()
        for b in [self.points, self.normals, self.rgb] + list(self._depth.values()):
            if b is not None:
                b.close()


def compare(a, b, what):
    """test_swapping's comparison of one frame's snapshots (here they name every cached block)"""
    test_swapping.compare_frame(a, b, what + ": ")


def build(be, away, voxel=capi.VOXEL_S, colour=False, order="build"):
    """A Run after three frames on the scene and `away` frames looking at the wall."""
    run = Run(be, voxel, colour)
    for k in range(3 + away):
        run.frame(k, order)
    return run


def swapping_scene(be, away, voxel=capi.VOXEL_S, colour=False):
    """(scene, render state) after three frames on the scene and `away` frames looking at a wall, in each of which 0x200 blocks leave for
    the host cache."""
    run = build(be, away, voxel, colour)
    return run.scene, run.rs


def neighbour_census(table):
    """From a downloaded table: (entries with ptr == -1, resident blocks with a swapped-out block among their 7 positive neighbours)."""
    live = table[table["ptr"] >= -1]
    out = {tuple(int(c) for c in p) for p in live["pos"][live["ptr"] == -1]}
    n = 0
    for p in live["pos"][live["ptr"] >= 0]:
        x, y, z = (int(c) for c in p)
        if any((x + dx, y + dy, z + dz) in out for dx in (0, 1) for dy in (0, 1) for dz in (0, 1) if dx or dy or dz):
            n += 1
    return len(out), n
