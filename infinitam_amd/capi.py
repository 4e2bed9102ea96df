"""ctypes binding of the C-ABI declared in include/itm_hip.h.

`Backend(lib_path, prefix)` binds any shared library that exports that ABI under `prefix`
(the product library uses ``itm_``).  On top of the raw functions it offers thin Python mirrors of
the reference's engine interfaces -- `SceneReconstructionEngine` (ResetScene /
AllocateSceneFromDepth / IntegrateIntoScene, reference Engine/ITMSceneReconstructionEngine.h:28-52)
and `VisualisationEngine` (FindVisibleBlocks / CreateExpectedDepths / RenderImage / FindSurface /
CreatePointCloud / CreateICPMaps / ForwardRender / CreateRenderState, reference
Engine/ITMVisualisationEngine.h:18-81) -- so that tests read like calls into the reference.

This module contains no numerics: every method forwards to the library.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

# ---- enums (include/itm_hip.h) ---------------------------------------------------------------
VOXEL_S, VOXEL_F, VOXEL_S_RGB, VOXEL_F_RGB = 0, 1, 2, 3
INDEX_HASH, INDEX_DENSE = 0, 1
RENDER_SHADED_GREYSCALE, RENDER_COLOUR_FROM_VOLUME, RENDER_COLOUR_FROM_NORMAL = 0, 1, 2
(BUF_HASH_ENTRIES, BUF_EXCESS_LIST, BUF_VOXEL_BLOCKS, BUF_ALLOCATION_LIST, BUF_VISIBLE_IDS,
 BUF_VISIBLE_TYPE, BUF_RANGE_IMAGE, BUF_RAYCAST_RESULT, BUF_RAYCAST_IMAGE, BUF_FORWARD_PROJECTION,
 BUF_MISSING_POINTS, BUF_SWAP_STATES) = range(12)
ERR_INVALID, ERR_DEVICE, ERR_UNSUPPORTED = -1, -2, -3
MESH_NORMALS, MESH_COLOURS = 1, 2

VOXEL_NAMES = {VOXEL_S: "ITMVoxel_s", VOXEL_F: "ITMVoxel_f", VOXEL_S_RGB: "ITMVoxel_s_rgb",
               VOXEL_F_RGB: "ITMVoxel_f_rgb"}

# numpy views of the reference's POD layouts (Utils/ITMLibDefines.h:71-82, :100-199)
HASH_ENTRY_DTYPE = np.dtype({"names": ["pos", "offset", "ptr"],
                             "formats": [("<i2", 3), "<i4", "<i4"],
                             "offsets": [0, 8, 12], "itemsize": 16})
VOXEL_DTYPES = {
    VOXEL_S: np.dtype({"names": ["sdf", "w_depth"], "formats": ["<i2", "u1"],
                       "offsets": [0, 2], "itemsize": 4}),
    VOXEL_F: np.dtype({"names": ["sdf", "w_depth"], "formats": ["<f4", "u1"],
                       "offsets": [0, 4], "itemsize": 8}),
    VOXEL_S_RGB: np.dtype({"names": ["sdf", "w_depth", "clr", "w_color"],
                           "formats": ["<i2", "u1", ("u1", 3), "u1"],
                           "offsets": [0, 2, 3, 6], "itemsize": 8}),
    VOXEL_F_RGB: np.dtype({"names": ["sdf", "w_depth", "clr", "w_color"],
                           "formats": ["<f4", "u1", ("u1", 3), "u1"],
                           "offsets": [0, 4, 5, 8], "itemsize": 12}),
}


class SceneParams(C.Structure):
    """itm_scene_params == ITMSceneParams (Objects/ITMSceneParams.h:14-70)."""
    _fields_ = [("voxelSize", C.c_float), ("mu", C.c_float), ("maxW", C.c_int32),
                ("viewFrustum_min", C.c_float), ("viewFrustum_max", C.c_float),
                ("stopIntegratingAtMaxW", C.c_int32)]


class SceneConfig(C.Structure):
    _fields_ = [("voxelType", C.c_int32), ("indexType", C.c_int32), ("bucketNum", C.c_int32),
                ("excessNum", C.c_int32), ("localBlockNum", C.c_int32),
                ("denseSize", C.c_int32 * 3), ("denseOffset", C.c_int32 * 3),
                ("denseOffsetSet", C.c_int32), ("maxRenderingBlocks", C.c_int32), ("useSwapping", C.c_int32), ("transferBlockNum", C.c_int32)]


class ViewStruct(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("rgb", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32),
                ("w_rgb", C.c_int32), ("h_rgb", C.c_int32), ("M_d", C.c_float * 16),
                ("intr_d", C.c_float * 4), ("intr_rgb", C.c_float * 4),
                ("rgb_to_depth", C.c_float * 16), ("rgb_to_depth_inv", C.c_float * 16)]


class Profile(C.Structure):
    _fields_ = [("calls", C.c_int32 * 8), ("total_ms", C.c_double * 8)]


TIMED_KERNELS = ["request", "alloc_sweep", "visible_list", "integrate", "range", "raycast", "icp_maps", "empty"]


class TrackerConfig(C.Structure):
    """itm_tracker_config; defaults of ITMLibSettings (Utils/ITMLibSettings.cpp:12-13,62-71)."""
    _fields_ = [("noHierarchyLevels", C.c_int32), ("trackingRegime", C.c_int32 * 8), ("noICPRunTillLevel", C.c_int32),
                ("distThresh", C.c_float), ("terminationThreshold", C.c_float)]

    @staticmethod
    def default():
        t = TrackerConfig()
        t.noHierarchyLevels = 5
        t.trackingRegime[:5] = [3, 3, 1, 1, 1]
        t.noICPRunTillLevel = 0
        t.distThresh = 0.1 * 0.1
        t.terminationThreshold = 1e-3
        return t


class RGBDCalib(C.Structure):
    """itm_rgbd_calib: calibration text of the reference (ITMLib/Utils/ITMCalibIO.cpp)."""
    _fields_ = [("size_rgb", C.c_float * 2), ("intr_rgb", C.c_float * 4), ("size_d", C.c_float * 2), ("intr_d", C.c_float * 4),
                ("rgb_to_depth", C.c_float * 16), ("rgb_to_depth_inv", C.c_float * 16), ("disparityType", C.c_int32),
                ("disparityParams", C.c_float * 2)]


class TrackerGH(C.Structure):
    _fields_ = [("f", C.c_float), ("nabla", C.c_float * 6), ("hessian", C.c_float * 36), ("noValidPoints", C.c_int32)]


class ColourEval(C.Structure):
    """itm_colour_eval: F_oneLevel / G_oneLevel of the colour tracker (hessian[para + col * numPara])."""
    _fields_ = [("f", C.c_float), ("noValidPoints", C.c_int32), ("numPara", C.c_int32), ("nabla", C.c_float * 6),
                ("hessian", C.c_float * 36)]


class RenEval(C.Structure):
    """itm_ren_eval: F_oneLevel / G_oneLevel of the Ren SDF tracker (hessian[r + c * 6])."""
    _fields_ = [("f", C.c_float), ("noValidPoints", C.c_int32), ("nabla", C.c_float * 6), ("hessian", C.c_float * 36)]


class Counters(C.Structure):
    _fields_ = [("lastFreeBlockId", C.c_int32), ("lastFreeExcessListId", C.c_int32),
                ("noVisibleEntries", C.c_int32), ("noFwdProjMissingPoints", C.c_int32),
                ("noTotalPoints", C.c_int32), ("noRenderingBlocks", C.c_int32),
                ("noAllocRequests", C.c_int32), ("statusFlags", C.c_int32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def default_params(voxelSize=0.005, mu=0.02, maxW=100, vf_min=0.35, vf_max=3.0,
                   stopIntegratingAtMaxW=False) -> SceneParams:
    """Defaults of ITMLibSettings (Utils/ITMLibSettings.cpp:10)."""
    return SceneParams(voxelSize, mu, maxW, vf_min, vf_max, int(stopIntegratingAtMaxW))


IDENTITY16 = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1)


def header_path() -> str:
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "itm_hip.h")


def declared_functions() -> list:
    """Names declared through ITM_FN(...) in include/itm_hip.h (the boundary) and include/itm_debug.h (the test hooks)."""
    text = ""
    for path in (header_path(), os.path.join(os.path.dirname(header_path()), "itm_debug.h")):
        with open(path) as f:
            text += f.read()
    names = re.findall(r"ITM_FN\((\w+)\)\s*\(", text)
    return sorted(set(n for n in names if n != "name"))


class AccelInfo(C.Structure):
    """itm_accel_info (include/itm_hip.h)."""
    _fields_ = [("directory_bytes", C.c_int64), ("slot_directory_bytes", C.c_int64), ("mirror_bytes", C.c_int64),
                ("origin_directory", C.c_int32 * 3), ("origin_mirror", C.c_int32 * 3), ("placed", C.c_int32), ("moves", C.c_int64),
                ("mirror_pages", C.c_int32), ("mirror_pages_mapped", C.c_int32)]


class AccelCensus(C.Structure):
    """itm_accel_census (include/itm_debug.h)."""
    _fields_ = [("directory_cells", C.c_int64), ("slot_directory_cells", C.c_int64), ("mirror_blocks", C.c_int64),
                ("page_counter", C.c_int32), ("mirror_form", C.c_int32), ("has_directory", C.c_int32), ("reserved", C.c_int32)]


class MeshComponent(C.Structure):
    """itm_mesh_component (include/itm_hip.h, itm_mesh_components): 40 bytes."""
    _fields_ = [("firstVertex", C.c_uint32), ("noVertices", C.c_uint32), ("noTriangles", C.c_uint32), ("reserved", C.c_uint32),
                ("bbMin", C.c_float * 3), ("bbMax", C.c_float * 3)]


# the same record as a numpy dtype (Mesh.components)
MESH_COMPONENT_DTYPE = np.dtype([("firstVertex", np.uint32), ("noVertices", np.uint32), ("noTriangles", np.uint32), ("reserved", np.uint32),
                                 ("bbMin", np.float32, 3), ("bbMax", np.float32, 3)])


MESH_SMOOTH_PIN_IRREGULAR = 1


class MeshSmoothConfig(C.Structure):
    """itm_mesh_smooth_config (include/itm_hip.h, itm_mesh_smooth): 32 bytes."""
    _fields_ = [("steps", C.c_uint32), ("lambdaQ16", C.c_int32), ("muQ16", C.c_int32), ("quantum", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class MeshSmoothStats(C.Structure):
    """itm_mesh_smooth_stats (include/itm_hip.h, itm_mesh_smooth): 32 bytes."""
    _fields_ = [(n, C.c_uint32) for n in ("noVertices", "noMoving", "noIrregular", "noIsolated", "maxEntries", "steps")] + [("reserved", C.c_uint32 * 2)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


def mesh_smooth_config(quantum, steps=20, lam=0.5, mu=-0.53, pin_irregular=True) -> MeshSmoothConfig:
    """The factors as Q16 integers, rounded to the nearest (lam = mu: plain Laplacian passes).  quantum: metres per fixed-point unit;
    it has no default here, since a good one follows the scene's voxel size (itm_mesh_smooth_default_config: voxelSize / 1024)."""
    return MeshSmoothConfig(int(steps), int(round(lam * 65536)), int(round(mu * 65536)), float(quantum),
                            MESH_SMOOTH_PIN_IRREGULAR if pin_irregular else 0)


MESH_UPDATE_NO_RUN_TABLE, MESH_UPDATE_ALL_MARKED, MESH_UPDATE_OVERFLOW = 1, 2, 3      # itm_mesh_update_stats::full


class MeshUpdateStats(C.Structure):
    """itm_mesh_update_stats (include/itm_hip.h, itm_mesh_update): 64 bytes."""
    _fields_ = ([(n, C.c_int32) for n in ("full", "allocated", "marked", "ignoredMarks", "appeared", "vanished", "remeshed", "kept")] +
                [(n, C.c_uint32) for n in ("trianglesBefore", "trianglesAfter", "trianglesCopied", "trianglesGenerated", "noChanged", "noRemoved")] +
                [("reserved", C.c_uint32 * 2)])

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class MeshChangedBlock(C.Structure):
    """itm_mesh_changed_block (include/itm_hip.h, itm_mesh_update): 20 bytes."""
    _fields_ = [("slot", C.c_int32), ("pos", C.c_int16 * 3), ("reserved", C.c_int16), ("firstTriangle", C.c_uint32), ("noTriangles", C.c_uint32)]


class MeshRemovedBlock(C.Structure):
    """itm_mesh_removed_block (include/itm_hip.h, itm_mesh_update): 12 bytes."""
    _fields_ = [("slot", C.c_int32), ("pos", C.c_int16 * 3), ("reserved", C.c_int16)]


# the same records as numpy dtypes (Mesh.update_delta)
MESH_CHANGED_DTYPE = np.dtype([("slot", np.int32), ("pos", np.int16, 3), ("reserved", np.int16), ("firstTriangle", np.uint32), ("noTriangles", np.uint32)])
MESH_REMOVED_DTYPE = np.dtype([("slot", np.int32), ("pos", np.int16, 3), ("reserved", np.int16)])


class MergeStats(C.Structure):
    """itm_merge_stats (include/itm_hip.h, itm_scene_merge)."""
    _fields_ = [(n, C.c_int32) for n in ("rounds", "considered", "alreadyPresent", "allocated", "combined", "unserved",
                                         "srcWithoutBlock", "dstSwappedOut")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# itm_prune_config::classes and the bits of a decision byte (include/itm_hip.h, itm_scene_prune)
PRUNE_EMPTY, PRUNE_FREE, PRUNE_WEAK, PRUNE_BOX = 1, 2, 4, 8
PRUNE_IS_EMPTY, PRUNE_IS_FREE, PRUNE_IS_WEAK, PRUNE_IS_SURFACE, PRUNE_IS_INBOX, PRUNE_IS_CANDIDATE, PRUNE_IS_DROPPED = 1, 2, 4, 8, 16, 64, 128


class PruneConfig(C.Structure):
    """itm_prune_config (include/itm_hip.h, itm_scene_prune): 48 bytes."""
    _fields_ = [("classes", C.c_int32), ("freeSdf", C.c_float), ("weakMaxW", C.c_int32), ("protect", C.c_int32),
                ("boxMin", C.c_int32 * 3), ("boxMax", C.c_int32 * 3), ("boxOnly", C.c_int32), ("dryRun", C.c_int32)]

    def replace(self, **kw) -> "PruneConfig":
        out = PruneConfig.from_buffer_copy(self)
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise ItmError(f"PruneConfig has no field {k}")
            if k in ("boxMin", "boxMax"):
                getattr(out, k)[:] = [int(c) for c in v]
            else:
                setattr(out, k, v)
        return out

    def as_dict(self):
        return {n: (list(getattr(self, n)) if n in ("boxMin", "boxMax") else getattr(self, n)) for n, _ in self._fields_}


class PruneStats(C.Structure):
    """itm_prune_stats (include/itm_hip.h, itm_scene_prune): 64 bytes."""
    _fields_ = [(n, C.c_int32) for n in ("considered", "empty", "free_", "weak", "inBox", "candidates", "protectedByNeighbour", "pinnedHeads",
                                         "dropped", "droppedHeads", "droppedExcess", "withoutBlock", "visibleRemoved", "lastFreeBlockId",
                                         "lastFreeExcessListId", "reserved")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class DeintegrateConfig(C.Structure):
    """itm_deintegrate_config (include/itm_hip.h, itm_deintegrate_from_scene): 16 bytes."""
    _fields_ = [("keepSaturated", C.c_int32), ("reserved", C.c_int32 * 3)]


class DeintegrateStats(C.Structure):
    """itm_deintegrate_stats (include/itm_hip.h, itm_deintegrate_from_scene): 64 bytes."""
    _fields_ = [(n, C.c_int32) for n in ("blocks", "visited", "touched", "reset", "unobserved", "saturated", "clamped", "coloured", "colourReset")] + \
               [("reserved", C.c_int32 * 7)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class CoarsenStats(C.Structure):
    """itm_coarsen_stats (include/itm_hip.h, itm_scene_coarsen)."""
    _fields_ = [(n, C.c_int32) for n in ("rounds", "considered", "alreadyPresent", "allocated", "written", "unserved",
                                         "srcWithoutBlock", "dstSwappedOut")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class RigidQ(C.Structure):
    """itm_rigid_q (include/itm_hip.h): a rigid transform in Q30 and voxel units, row-major [3i + j], both directions."""
    _fields_ = [("inv", C.c_int32 * 9), ("invT", C.c_int64 * 3), ("fwd", C.c_int32 * 9), ("fwdT", C.c_int64 * 3)]

    def as_dict(self):
        return {n: [int(v) for v in getattr(self, n)] for n, _ in self._fields_}

    @classmethod
    def from_dict(cls, d):
        q = cls()
        for n, _ in cls._fields_:
            for i, v in enumerate(d[n]):
                getattr(q, n)[i] = int(v)
        return q


class ResampleStats(C.Structure):
    """itm_resample_stats (include/itm_hip.h, itm_scene_resample)."""
    _fields_ = [(n, C.c_int32) for n in ("rounds", "considered", "candidates", "alreadyPresent", "allocated", "resampled", "unserved",
                                         "srcWithoutBlock", "dstSwappedOut", "outOfRange")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def rigid_quantise(M, voxelSize, be=None) -> RigidQ:
    """itm_rigid_quantise: the rigid transform M (4 x 4, x_dst = M x_src, metres; or its 16 floats column-major) in Q30 and voxel
    units.  be: the Backend whose library does it (default: the product library; host only, no device is touched).  Raises ItmError
    with the library's reason for a matrix that is refused."""
    if be is None:
        from . import load
        be = load()
    arr = np.asarray(M, np.float32)
    flat = np.ascontiguousarray(arr.T if arr.ndim == 2 else arr).reshape(16)
    q = RigidQ()
    be.check(be.fn["rigid_quantise"](flat.ctypes.data_as(C.POINTER(C.c_float)), float(voxelSize), C.byref(q)), "rigid_quantise")
    return q


class QueryOut(C.Structure):
    """itm_query_out (include/itm_hip.h, itm_scene_query_points): device pointers, NULL = not wanted."""
    _fields_ = [(n, C.c_void_p) for n in ("sdf", "sdf_nearest", "gradient", "normal", "colour", "weight", "flags")]


QUERY_METRES, QUERY_VOXELS = 0, 1
QUERY_INVALID = 0x80000000
# output name -> (dtype, trailing shape)
QUERY_OUTPUTS = {"sdf": (np.float32, ()), "sdf_nearest": (np.float32, ()), "gradient": (np.float32, (3,)), "normal": (np.float32, (3,)),
                 "colour": (np.uint8, (4,)), "weight": (np.uint8, ()), "flags": (np.uint32, ())}


class EsdfBox(C.Structure):
    """itm_esdf_box (include/itm_hip.h, itm_scene_esdf): first voxel and size of the box, voxel units."""
    _fields_ = [("origin", C.c_int32 * 3), ("size", C.c_int32 * 3)]


class EsdfOut(C.Structure):
    """itm_esdf_out: device pointers, NULL = not wanted, except dist2 (the passes' working storage)."""
    _fields_ = [(n, C.c_void_p) for n in ("dist2", "nearest", "distance", "state")]


ESDF_STORED, ESDF_OBSERVED, ESDF_INSIDE, ESDF_SITE = 1, 2, 4, 8
ESDF_SITE_SURFACE, ESDF_SITE_UNKNOWN = 1, 2
ESDF_NONE = 0x7fffffff
ESDF_SITES = {"surface": ESDF_SITE_SURFACE, "unknown": ESDF_SITE_UNKNOWN}
ESDF_OUTPUTS = {"dist2": np.int32, "nearest": np.int32, "distance": np.float32, "state": np.uint8}
ESDF_MAX_SIDE, ESDF_MAX_CELLS = 1024, 1 << 27


def _esdf_buffers(be, size, want):
    """(EsdfOut, {name: DevBuffer}) for a grid of `size` = (nx, ny, nz): dist2 always, the others where wanted.  A size the library
    will refuse gets one-byte buffers: it is refused before anything is written."""
    unknown = [w for w in want if w not in ESDF_OUTPUTS]
    if unknown:
        raise ItmError(f"distance field: unknown outputs {unknown}")
    nx, ny, nz = (int(v) for v in size)
    ok = all(1 <= v <= ESDF_MAX_SIDE for v in (nx, ny, nz)) and nx * ny * nz <= ESDF_MAX_CELLS
    n, shape = (nx * ny * nz, (nz, ny, nx)) if ok else (0, (0,))
    bufs = {w: DevBuffer(be, n * np.dtype(ESDF_OUTPUTS[w]).itemsize, ESDF_OUTPUTS[w], shape)
            for w in ESDF_OUTPUTS if w == "dist2" or w in want}
    out = EsdfOut()
    for w, b in bufs.items():
        setattr(out, w, b.ptr)
    return out, bufs


class RelocConfig(C.Structure):
    """itm_reloc_config (include/itm_hip.h, the keyframe relocaliser)."""
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("levels", C.c_int32), ("blurRadius", C.c_int32), ("blurTaps", C.c_float * 9),
                ("numFerns", C.c_int32), ("numDecisions", C.c_int32), ("capacity", C.c_int32)]


RELOC_MAX_K, RELOC_MAX_FERNS = 8, 1024


class PoseQualityConfig(C.Structure):
    """itm_pose_quality_config (include/itm_hip.h, the tracking verdict)."""
    _fields_ = [("inlierDistance", C.c_float), ("minWeight", C.c_int32), ("minValidFraction", C.c_float), ("failOverlap", C.c_float),
                ("poorOverlap", C.c_float), ("failInliers", C.c_float), ("goodInliers", C.c_float)]


class PoseQualityStats(C.Structure):
    """itm_pose_quality (include/itm_hip.h)."""
    _fields_ = [("noPixels", C.c_int32), ("noValid", C.c_int32), ("noKnown", C.c_int32), ("noInliers", C.c_int32),
                ("sumSqKnown", C.c_double), ("sumSqInliers", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class AlignConfig(C.Structure):
    """itm_align_config (include/itm_hip.h, scene alignment): the band samples' selection and the aligner's loop.  32 bytes."""
    _fields_ = [("minWeight", C.c_int32), ("maxAbsSdf", C.c_float), ("stride", C.c_int32), ("huberDelta", C.c_float), ("minStep", C.c_float),
                ("maxEvaluations", C.c_int32), ("minValid", C.c_int32), ("minConditioning", C.c_float)]

    def replace(self, **kw) -> "AlignConfig":
        c = AlignConfig.from_buffer_copy(self)
        for k, v in kw.items():
            setattr(c, k, v)
        return c


class AlignEval(C.Structure):
    """itm_align_eval: cost, valid count, gradient and Hessian (hessian[r + c * 6]) of one evaluation.  176 bytes."""
    _fields_ = [("f", C.c_float), ("noValid", C.c_int32), ("nabla", C.c_float * 6), ("hessian", C.c_float * 36)]


class AlignResult(C.Structure):
    """itm_align_result.  40 bytes."""
    _fields_ = [("status", C.c_int32), ("evaluations", C.c_int32), ("noValid", C.c_int32), ("reserved", C.c_int32),
                ("initialCost", C.c_double), ("finalCost", C.c_double), ("conditioning", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


ALIGN_CONVERGED, ALIGN_MAX_EVALUATIONS, ALIGN_STALLED, ALIGN_TOO_FEW_SAMPLES, ALIGN_DEGENERATE = range(5)
ALIGN_STATUS_NAMES = ("converged", "max_evaluations", "stalled", "too_few_samples", "degenerate")


def align_default_config(voxelSize, mu, be=None) -> AlignConfig:
    """itm_align_default_config (host only)."""
    if be is None:
        from . import load
        be = load()
    cfg = AlignConfig()
    be.check(be.fn["align_default_config"](float(voxelSize), float(mu), C.byref(cfg)), "align_default_config")
    return cfg


def _matrix16(M):
    """the 16 floats, column-major, of a 4 x 4 matrix (x_out = M x_in) or of 16 floats that are column-major already"""
    arr = np.asarray(M, np.float32)
    return np.ascontiguousarray(arr.T if arr.ndim == 2 else arr).reshape(16)


TRACKING_FAILED, TRACKING_POOR, TRACKING_GOOD = 0, 1, 2
POSE_QUALITY_UNKNOWN, POSE_QUALITY_NONE = np.float32(1e30), np.float32(-1e30)
DEBUG_POSE_QUALITY_ROWS = 29
# itm_debug_counter (include/itm_debug.h): the forward-only 32-bit counters behind the tagged granules
(COUNTER_LIST_EPOCH, COUNTER_FRAME_PARITY, COUNTER_TABLE_EPOCH, COUNTER_TRACKER_SEQ, COUNTER_TRACKER_SESSION, COUNTER_TRACKER_FALLBACKS,
 COUNTER_TRACKER_RELAUNCHES, COUNTER_COLOUR_SEQ, COUNTER_REN_SEQ, COUNTER_POSE_QUALITY_SEQ, COUNTER_IMAGE_MAP_EPOCH, COUNTER_ALIGN_SEQ) = range(1, 13)


class ItmError(RuntimeError):
    pass


_P = C.c_void_p
_SIGS = {
    "version": (C.c_char_p, []),
    "last_error": (C.c_char_p, []),
    "uses_device_memory": (C.c_int, []),
    "voxel_size_bytes": (C.c_size_t, [C.c_int]),
    "dev_malloc": (C.c_int, [C.POINTER(_P), C.c_size_t]),
    "dev_free": (C.c_int, [_P]),
    "memcpy_h2d": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "memcpy_d2h": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "stream_synchronize": (C.c_int, [_P]),
    "set_device": (C.c_int, [C.c_int]),
    "scene_create": (C.c_int, [C.POINTER(SceneConfig), C.POINTER(SceneParams), C.POINTER(_P)]),
    "scene_destroy": (C.c_int, [_P]),
    "scene_get_config": (C.c_int, [_P, C.POINTER(SceneConfig), C.POINTER(SceneParams)]),
    "reset_scene": (C.c_int, [_P, _P]),
    "render_state_create": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(_P)]),
    "render_state_destroy": (C.c_int, [_P]),
    "allocate_scene_from_depth": (C.c_int, [_P, C.POINTER(ViewStruct), _P, C.c_int, _P]),
    "integrate_into_scene": (C.c_int, [_P, C.POINTER(ViewStruct), _P, _P]),
    "find_visible_blocks": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P]),
    "create_expected_depths": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P]),
    "render_image": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P, C.c_int, _P]),
    "find_surface": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P]),
    "create_point_cloud": (C.c_int, [_P, C.POINTER(ViewStruct), _P, C.c_int, _P, _P, _P]),
    "create_icp_maps": (C.c_int, [_P, C.POINTER(ViewStruct), _P, _P, _P, _P]),
    "forward_render": (C.c_int, [_P, C.POINTER(ViewStruct), _P, _P]),
    "process_frame": (C.c_int, [_P, C.POINTER(ViewStruct), _P, _P, _P, _P]),
    "process_frame_ahead": (C.c_int, [_P, C.POINTER(ViewStruct), C.POINTER(ViewStruct), _P, _P, _P, _P]),
    "flush": (C.c_int, [_P, _P, _P]),
    "cancel_ahead": (C.c_int, [_P, _P, _P]),
    "convert_depth_affine": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, C.c_float, _P]),
    "convert_disparity": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, _P]),
    "filter_depth": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "compute_normal_and_weights": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "update_view": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "filter_subsample_with_holes": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "tracker_compute_g_and_h": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_float), _P, _P, C.c_int, C.c_int, C.POINTER(C.c_float),
                                          C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int, C.POINTER(TrackerGH), _P]),
    "track_camera": (C.c_int, [C.POINTER(TrackerConfig), C.POINTER(ViewStruct), _P, _P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
    "get_counters": (C.c_int, [_P, _P, C.POINTER(Counters), _P]),
    "set_counters": (C.c_int, [_P, _P, C.POINTER(Counters), _P]),
    "buffer_bytes": (C.c_size_t, [_P, _P, C.c_int]),
    "download": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t, _P]),
    "upload": (C.c_int, [_P, _P, C.c_int, _P, C.c_size_t, _P]),
    "buffer_ptr": (_P, [_P, _P, C.c_int]),
    "debug_set": (C.c_int, [C.c_int, C.c_int]),
    "debug_div32767": (C.c_int, [_P, _P, C.c_int, _P]),
    "debug_divide": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int, _P]),
    "profile_enable": (C.c_int, [_P, C.c_uint32]),
    "profile_sample": (C.c_int, [_P, C.c_int]),
    "profile_calibrate": (C.c_int, [_P, C.c_int, _P]),
    "profile_read": (C.c_int, [_P, C.POINTER(Profile), C.c_int]),
    "export_visible_record": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int, _P, _P]),
    "mesh_create": (C.c_int, [_P, C.c_uint32, C.POINTER(_P)]),
    "mesh_destroy": (C.c_int, [_P]),
    "mesh_scene": (C.c_int, [_P, _P, _P]),
    "mesh_info": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(_P), _P]),
    "mesh_download": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(C.c_uint32), _P]),
    "mesh_write_obj": (C.c_int, [_P, C.c_char_p, _P]),
    "mesh_write_stl": (C.c_int, [_P, C.c_char_p, _P]),
}


# host-side file formats: exported by the product and by the reference shim; the CPU oracle has no need for them
_HOST_IO_SIGS = {
    "read_depth_image": (C.c_int, [C.c_char_p, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "read_rgb_image": (C.c_int, [C.c_char_p, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "write_depth_image": (C.c_int, [C.c_char_p, _P, C.c_int, C.c_int]),
    "write_rgb_image": (C.c_int, [C.c_char_p, _P, C.c_int, C.c_int]),
    "write_float_depth_image": (C.c_int, [C.c_char_p, _P, C.c_int, C.c_int]),
    "read_rgbd_calib": (C.c_int, [C.c_char_p, _P]),
    "scene_save": (C.c_int, [_P, _P, C.c_char_p, _P]),
    "scene_load": (C.c_int, [_P, _P, C.c_char_p, _P]),
    # tracker handles (the oracle / reference shims have no use for them: their trackers are stateless)
    "debug_icp_track": (C.c_int, [C.POINTER(TrackerConfig), C.POINTER(C.c_float), _P, _P, C.POINTER(C.c_float)]),
    "debug_wicp_track": (C.c_int, [C.POINTER(TrackerConfig), C.POINTER(C.c_float), _P, _P, C.POINTER(C.c_float)]),
    "tracker_create": (C.c_int, [C.POINTER(_P)]),
    "tracker_destroy": (C.c_int, [_P]),
    "tracker_g_and_h": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(C.c_float), _P, _P, C.c_int, C.c_int, C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int, C.POINTER(TrackerGH), _P]),
    "tracker_track_camera": (C.c_int, [_P, C.POINTER(TrackerConfig), C.POINTER(ViewStruct), _P, _P, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
    "tracker_weighted_g_and_h": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.POINTER(C.c_float), _P, _P, C.c_int, C.c_int,
                                           C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_int,
                                           C.POINTER(TrackerGH), _P]),
    "tracker_weighted_track_camera": (C.c_int, [_P, C.POINTER(TrackerConfig), C.POINTER(ViewStruct), _P, _P, _P, C.POINTER(C.c_float),
                                                C.POINTER(C.c_float), _P]),
    "debug_column_cull_rows": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "debug_dense_classify_check": (C.c_int, [C.POINTER(C.c_int32), C.c_int]),
    "scene_accel_info": (C.c_int, [_P, C.POINTER(AccelInfo)]),
    "scene_set_deferred_fusion": (C.c_int, [_P, C.c_int]),
    # read-only probes of the acceleration cubes (test hooks, product only)
    "debug_accel_probe": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "debug_accel_census": (C.c_int, [_P, C.POINTER(AccelCensus), _P, _P]),
    "debug_ordered_compact": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "debug_memory": (C.c_int, [_P]),
    "debug_get": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "debug_counter": (C.c_int, [C.c_int, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "swap_integrate_global_into_local": (C.c_int, [_P, _P, _P]),
    "swap_save_to_global_memory": (C.c_int, [_P, _P, _P]),
    "global_cache_get": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int)]),
    "global_cache_flags": (C.c_int, [_P, _P, C.c_size_t]),
    "host_malloc": (C.c_int, [C.POINTER(_P), C.c_size_t]),
    "host_free": (C.c_int, [_P]),
    "host_register": (C.c_int, [_P, C.c_size_t]),
    "host_unregister": (C.c_int, [_P]),
    "depth_stager_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "depth_stager_destroy": (C.c_int, [_P]),
    "depth_stager_upload": (C.c_int, [_P, _P]),
    "depth_stager_acquire": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "depth_stager_release": (C.c_int, [_P, _P]),
    "depth_stager_set_conversion": (C.c_int, [_P, C.c_int, C.c_float, C.c_float, C.c_float]),
    "depth_stager_acquire_depth": (C.c_int, [_P, _P, C.POINTER(_P), C.POINTER(_P)]),
    "depth_stager_pending": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "stream_create": (C.c_int, [C.POINTER(_P)]),
    "stream_destroy": (C.c_int, [_P]),
    # multi-stream exchange issued from the library (RCCL); the CPU shims exchange through torch.distributed (streams.py)
    "exchange_unique_id": (C.c_int, [C.POINTER(C.c_ubyte)]),
    "exchange_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.POINTER(_P)]),
    "exchange_destroy": (C.c_int, [_P]),
    "exchange_step": (C.c_int, [_P, _P, C.POINTER(C.c_float), _P]),
    "exchange_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_P)]),
    "exchange_table": (C.c_int, [_P, _P, C.c_size_t]),
    "exchange_self_check": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "exchange_acquire": (C.c_int, [_P, _P, C.POINTER(_P), C.POINTER(C.c_longlong)]),
    "exchange_release": (C.c_int, [_P, _P]),
    "debug_checksum": (C.c_int, [_P, C.c_size_t, C.c_int, _P, _P]),
    # colour tracker handles (product only)
    "colour_tracker_create": (C.c_int, [C.POINTER(_P)]),
    "colour_tracker_destroy": (C.c_int, [_P]),
    "colour_tracker_prepare": (C.c_int, [_P, C.POINTER(ViewStruct), C.c_int, _P]),
    "colour_tracker_read_level": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "colour_tracker_evaluate": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(ColourEval), _P]),
    "colour_tracker_track_camera": (C.c_int, [_P, C.POINTER(TrackerConfig), C.POINTER(ViewStruct), _P, _P, _P, C.c_int,
                                              C.POINTER(C.c_float), _P]),
    "colour_tracker_evaluations": (C.c_int, [_P, C.POINTER(C.c_int)]),
    # Ren SDF tracker handles (product only)
    "ren_tracker_create": (C.c_int, [C.POINTER(_P)]),
    "ren_tracker_destroy": (C.c_int, [_P]),
    "ren_tracker_prepare": (C.c_int, [_P, C.POINTER(ViewStruct), _P, _P]),
    "ren_tracker_evaluate": (C.c_int, [_P, _P, C.POINTER(C.c_float), C.c_int, C.POINTER(RenEval), _P]),
    "ren_tracker_track_camera": (C.c_int, [_P, _P, C.POINTER(ViewStruct), C.POINTER(C.c_float), C.POINTER(C.c_int), _P]),
    # mesh vertex attributes and the PLY writer (product only: the reference's ITMMesh holds positions alone)
    "mesh_attributes": (C.c_int, [_P, _P, C.c_int, _P]),
    "mesh_download_attributes": (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(C.c_uint32), _P]),
    "mesh_write_ply": (C.c_int, [_P, C.c_char_p, _P]),
    # indexed mesh: the soup welded into shared vertices (product only)
    "mesh_index": (C.c_int, [_P, _P]),
    "mesh_index_info": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _P]),
    "mesh_download_indexed": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _P]),
    "mesh_indexed_attributes": (C.c_int, [_P, _P, C.c_int, _P]),
    "mesh_download_indexed_attributes": (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(C.c_uint32), _P]),
    "mesh_write_ply_indexed": (C.c_int, [_P, C.c_char_p, _P]),
    "mesh_write_obj_indexed": (C.c_int, [_P, C.c_char_p, _P]),
    # connected components of the indexed mesh and the fragment filter (product only)
    "mesh_components": (C.c_int, [_P, _P]),
    "mesh_components_info": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), _P]),
    "mesh_download_components": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32), _P]),
    "mesh_filter_components": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _P]),
    "debug_mesh_components": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _P]),
    # fixed-point smoothing of the indexed mesh (product only); default_config is host-only
    "mesh_smooth_default_config": (C.c_int, [C.c_float, C.POINTER(MeshSmoothConfig)]),
    "mesh_smooth": (C.c_int, [_P, C.POINTER(MeshSmoothConfig), C.POINTER(MeshSmoothStats), _P]),
    "debug_mesh_smooth": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.POINTER(MeshSmoothConfig), _P, _P, C.POINTER(MeshSmoothStats), _P]),
    # the mesh of either index type: dense volumes brick by brick (product only: the reference's dense MeshScene is empty)
    "mesh_volume": (C.c_int, [_P, _P, _P]),
    # incremental mesh: re-mesh the blocks a frame touched, keep the other runs (product only)
    "mesh_touch": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "mesh_update": (C.c_int, [_P, _P, C.POINTER(MeshUpdateStats), _P]),
    "mesh_update_info": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(_P), C.POINTER(_P), _P]),
    "mesh_download_update": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _P]),
    # colour maps of the display path (product only: host loops in the reference, Engine/ITMVisualisationEngine.cpp:7-107)
    "depth_to_uchar4": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "weight_to_uchar4": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "normal_to_uchar4": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    # frame de-integration (product only: the reference cannot un-fuse a frame)
    "deintegrate_from_scene": (C.c_int, [_P, C.POINTER(ViewStruct), _P, C.POINTER(DeintegrateConfig), C.POINTER(DeintegrateStats), _P]),
    # scene merge (product only: no reference engine merges scenes)
    "scene_merge": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(MergeStats), _P]),
    "prune_default_config": (C.c_int, [C.POINTER(PruneConfig)]),
    "scene_prune": (C.c_int, [_P, C.POINTER(PruneConfig), _P, C.POINTER(PruneStats), _P]),
    # level of detail (product only: the reference has one resolution per scene)
    "scene_coarsen": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(CoarsenStats), _P]),
    # scene merge under a rigid transform (product only)
    "rigid_quantise": (C.c_int, [C.POINTER(C.c_float), C.c_float, C.POINTER(RigidQ)]),
    "scene_resample": (C.c_int, [_P, _P, C.POINTER(RigidQ), _P, C.c_int, C.POINTER(ResampleStats), _P]),
    # scene queries at caller-supplied points / along caller-supplied rays (product only: the reference reads per pixel, inside its engines)
    "scene_query_points": (C.c_int, [_P, _P, C.c_uint32, C.c_int, C.POINTER(QueryOut), _P]),
    "scene_cast_rays": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    # distance field of a box of the volume and its scene-free transform (product only: the reference has no counterpart)
    "scene_esdf": (C.c_int, [_P, C.POINTER(EsdfBox), C.c_int, C.c_int, C.c_int, C.POINTER(EsdfOut), _P]),
    "esdf_transform": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.c_float, C.POINTER(EsdfOut), _P]),
    # keyframe relocaliser (product only: the reference at this revision has none); the two defaults are host-only
    "reloc_default_config": (C.c_int, [C.c_int, C.c_int, C.POINTER(RelocConfig)]),
    "reloc_default_ferns": (C.c_int, [C.POINTER(RelocConfig), C.c_uint64, C.c_float, C.c_float, _P, _P]),
    "reloc_create": (C.c_int, [C.POINTER(RelocConfig), _P, _P, C.POINTER(_P)]),
    "reloc_destroy": (C.c_int, [_P]),
    "reloc_encode": (C.c_int, [_P, _P, _P]),
    "reloc_find": (C.c_int, [_P, _P, C.c_int, _P, _P, _P]),
    "reloc_process_frame": (C.c_int, [_P, _P, C.POINTER(C.c_float), C.c_int, C.c_float, C.c_int, _P, _P, C.POINTER(C.c_int32), _P]),
    "reloc_info": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(RelocConfig)]),
    "reloc_get_pose": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_float)]),
    "reloc_read": (C.c_int, [_P, _P, _P]),
    "reloc_download": (C.c_int, [_P, _P, _P]),
    "reloc_upload": (C.c_int, [_P, C.c_int32, _P, _P]),
    "reloc_save": (C.c_int, [_P, C.c_char_p]),
    "reloc_load": (C.c_int, [_P, C.c_char_p]),
    "debug_reloc_search_ms": (C.c_int, [_P, C.c_int, C.POINTER(C.c_float)]),
    # pose quality / tracking verdict (product only); default_config and verdict are host-only
    "pose_quality_default_config": (C.c_int, [C.c_float, C.POINTER(PoseQualityConfig)]),
    "pose_quality_verdict": (C.c_int, [C.POINTER(PoseQualityStats), C.POINTER(PoseQualityConfig), C.POINTER(C.c_int32)]),
    "pose_quality_create": (C.c_int, [C.POINTER(_P)]),
    "pose_quality_destroy": (C.c_int, [_P]),
    "pose_quality_evaluate": (C.c_int, [_P, _P, C.POINTER(ViewStruct), C.POINTER(PoseQualityConfig), C.POINTER(PoseQualityStats), _P, _P]),
    # scene alignment (product only); default_config, step and apply_step are host-only
    "align_default_config": (C.c_int, [C.c_float, C.c_float, C.POINTER(AlignConfig)]),
    "align_step": (C.c_int, [C.POINTER(AlignEval), C.c_double, C.POINTER(C.c_float)]),
    "align_apply_step": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "scene_band_samples": (C.c_int, [_P, _P, C.c_int, C.POINTER(AlignConfig), _P, C.c_int32, C.POINTER(C.c_int32), _P]),
    "aligner_create": (C.c_int, [C.POINTER(_P)]),
    "aligner_destroy": (C.c_int, [_P]),
    "aligner_set_samples": (C.c_int, [_P, _P, C.c_int32, _P]),
    "aligner_evaluate": (C.c_int, [_P, _P, C.POINTER(C.c_float), C.POINTER(AlignConfig), C.POINTER(AlignEval), _P]),
    "aligner_align": (C.c_int, [_P, _P, C.POINTER(C.c_float), C.POINTER(AlignConfig), C.POINTER(C.c_float), C.POINTER(AlignResult), _P]),
}


class Backend:
    """One loaded implementation of the C-ABI."""

    def __init__(self, lib_path: str, prefix: str = "itm_"):
        if not os.path.exists(lib_path):
            raise ItmError(f"shared library not found: {lib_path}")
        self.path, self.prefix = lib_path, prefix
        self.lib = C.CDLL(lib_path)
        self.fn = {}
        for name, (res, args) in _SIGS.items():
            f = getattr(self.lib, prefix + name)   # AttributeError => missing symbol, fail loudly
            f.restype, f.argtypes = res, args
            self.fn[name] = f
        for name, (res, args) in _HOST_IO_SIGS.items():
            f = getattr(self.lib, prefix + name, None)
            if f is None:
                if prefix == "itm_":
                    raise ItmError(f"product library lacks {prefix}{name}")
                continue
            f.restype, f.argtypes = res, args
            self.fn[name] = f
        self.on_device = bool(self.fn["uses_device_memory"]())

    # ---- host-side file formats (numpy in / out) -----------------------------------------------
    def read_depth_image(self, path: str) -> np.ndarray:
        cap = 4096 * 4096
        buf = np.empty(cap, np.int16); w, h = C.c_int(), C.c_int()
        self.check(self.fn["read_depth_image"](path.encode(), buf.ctypes.data_as(_P), cap, C.byref(w), C.byref(h)), "read_depth_image")
        return buf[: w.value * h.value].reshape(h.value, w.value).copy()

    def read_rgb_image(self, path: str) -> np.ndarray:
        cap = 4096 * 4096
        buf = np.empty(cap * 4, np.uint8); w, h = C.c_int(), C.c_int()
        self.check(self.fn["read_rgb_image"](path.encode(), buf.ctypes.data_as(_P), cap, C.byref(w), C.byref(h)), "read_rgb_image")
        return buf[: w.value * h.value * 4].reshape(h.value, w.value, 4).copy()

    def write_image(self, path: str, img: np.ndarray):
        img = np.ascontiguousarray(img)
        h, w = img.shape[:2]
        kind = {np.dtype(np.int16): "write_depth_image", np.dtype(np.uint8): "write_rgb_image", np.dtype(np.float32): "write_float_depth_image"}[img.dtype]
        self.check(self.fn[kind](path.encode(), img.ctypes.data_as(_P), w, h), kind)

    def read_rgbd_calib(self, path: str) -> "RGBDCalib":
        out = RGBDCalib()
        self.check(self.fn["read_rgbd_calib"](path.encode(), C.byref(out)), "read_rgbd_calib")
        return out

    def check(self, rc: int, what: str = ""):
        if rc != 0:
            msg = self.fn["last_error"]() or b""
            raise ItmError(f"{self.prefix}{what} failed ({rc}): {msg.decode(errors='replace')}")

    def version(self) -> str:
        return self.fn["version"]().decode()

    def debug_counter(self, which: int, handle, value=None) -> int:
        """itm_debug_counter: the counter `which` (COUNTER_*) of `handle` (a scene / tracker handle, a stream for the image maps; None where
        the header allows it) as it stood; `value`, when given, replaces it (taken modulo 2^32)."""
        h = getattr(handle, "h", handle)
        old = C.c_uint32()
        new = None if value is None else C.byref(C.c_uint32(value & 0xffffffff))
        self.check(self.fn["debug_counter"](which, h if isinstance(h, _P) else _P(h), new, C.byref(old)), "debug_counter")
        return old.value

    # ---- memory in the backend's address space ---------------------------------------------
    def malloc(self, nbytes: int) -> int:
        p = _P()
        self.check(self.fn["dev_malloc"](C.byref(p), nbytes), "dev_malloc")
        return p.value

    def free(self, ptr: int):
        self.check(self.fn["dev_free"](_P(ptr)), "dev_free")

    def to_backend(self, arr: np.ndarray, stream=None) -> "DevBuffer":
        arr = np.ascontiguousarray(arr)
        buf = DevBuffer(self, arr.nbytes, arr.dtype, arr.shape)
        self.check(self.fn["memcpy_h2d"](_P(buf.ptr), arr.ctypes.data_as(_P), arr.nbytes, _P(stream)), "memcpy_h2d")
        self.sync(stream)
        return buf

    def sync(self, stream=None):
        self.check(self.fn["stream_synchronize"](_P(stream)), "stream_synchronize")

    def esdf_transform(self, state, max_distance=0, voxel_size=1.0, want=("dist2", "distance"), stream=None) -> dict:
        """itm_esdf_transform: the distance transform of a caller's own byte grid `state` [nz, ny, nx] (its ESDF_SITE and ESDF_INSIDE
        bits) -> the outputs named in `want` (ESDF_OUTPUTS without "state") as numpy arrays [nz, ny, nx].  Uploads, downloads and
        synchronises `stream`."""
        grid = np.ascontiguousarray(np.asarray(state, np.uint8))
        if grid.ndim != 3:
            raise ItmError("esdf_transform: state is a [nz, ny, nx] array")
        if "state" in want:
            raise ItmError("esdf_transform: state is the input")
        size = (C.c_int32 * 3)(*grid.shape[::-1])
        out, bufs = _esdf_buffers(self, grid.shape[::-1], want)
        dev = self.to_backend(grid, stream) if grid.size else None
        rc = self.fn["esdf_transform"](_P(dev.ptr if dev else None), size, int(max_distance), float(voxel_size), C.byref(out), _P(stream))
        self.sync(stream)
        res = {w: bufs[w].numpy(stream) for w in want} if rc == 0 else None
        for b in list(bufs.values()) + ([dev] if dev else []):
            b.close()
        self.check(rc, "esdf_transform")
        return res

    def create_scene(self, voxelType=VOXEL_S, indexType=INDEX_HASH, params: Optional[SceneParams] = None,
                     bucketNum=0, excessNum=0, localBlockNum=0, denseSize=(0, 0, 0), denseOffset=None,
                     maxRenderingBlocks=0, useSwapping=False, transferBlockNum=0) -> "Scene":
        cfg = SceneConfig()
        cfg.useSwapping, cfg.transferBlockNum = (1 if useSwapping else 0), transferBlockNum
        cfg.voxelType, cfg.indexType = voxelType, indexType
        cfg.bucketNum, cfg.excessNum, cfg.localBlockNum = bucketNum, excessNum, localBlockNum
        cfg.denseSize[:] = denseSize
        cfg.maxRenderingBlocks = maxRenderingBlocks
        if denseOffset is not None:
            cfg.denseOffset[:] = denseOffset
            cfg.denseOffsetSet = 1
        prm = params if params is not None else default_params()
        h = _P()
        self.check(self.fn["scene_create"](C.byref(cfg), C.byref(prm), C.byref(h)), "scene_create")
        return Scene(self, h.value)


class DevBuffer:
    """Owning handle to memory in the backend's address space (HBM for the product)."""

    def __init__(self, be: Backend, nbytes: int, dtype=np.uint8, shape=None):
        self.be, self.nbytes, self.dtype = be, int(nbytes), np.dtype(dtype)
        self.shape = shape if shape is not None else (self.nbytes // self.dtype.itemsize,)
        self.ptr = be.malloc(max(self.nbytes, 1))

    def numpy(self, stream=None) -> np.ndarray:
        out = np.empty(self.shape, dtype=self.dtype)
        self.be.check(self.be.fn["memcpy_d2h"](out.ctypes.data_as(_P), _P(self.ptr), self.nbytes, _P(stream)), "memcpy_d2h")
        self.be.sync(stream)
        return out

    def close(self):
        if self.ptr:
            self.be.free(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class View:
    """Python mirror of what the engines read from ITMView + ITMTrackingState::pose_d."""
    depth: DevBuffer
    w: int
    h: int
    M_d: np.ndarray = field(default_factory=lambda: np.array(IDENTITY16, np.float32))
    intr_d: tuple = (580.0, 580.0, 320.0, 240.0)
    rgb: Optional[DevBuffer] = None
    w_rgb: int = 0
    h_rgb: int = 0
    intr_rgb: Optional[tuple] = None
    rgb_to_depth: np.ndarray = field(default_factory=lambda: np.array(IDENTITY16, np.float32))
    rgb_to_depth_inv: np.ndarray = field(default_factory=lambda: np.array(IDENTITY16, np.float32))

    def struct(self) -> ViewStruct:
        v = ViewStruct()
        v.depth = self.depth.ptr if isinstance(self.depth, DevBuffer) else int(self.depth)
        v.rgb = (self.rgb.ptr if isinstance(self.rgb, DevBuffer) else (int(self.rgb) if self.rgb else None))
        v.w, v.h = self.w, self.h
        v.w_rgb, v.h_rgb = (self.w_rgb or self.w), (self.h_rgb or self.h)
        v.M_d[:] = [float(x) for x in np.asarray(self.M_d, np.float32).reshape(16)]
        v.intr_d[:] = [float(x) for x in self.intr_d]
        v.intr_rgb[:] = [float(x) for x in (self.intr_rgb or self.intr_d)]
        v.rgb_to_depth[:] = [float(x) for x in np.asarray(self.rgb_to_depth, np.float32).reshape(16)]
        v.rgb_to_depth_inv[:] = [float(x) for x in np.asarray(self.rgb_to_depth_inv, np.float32).reshape(16)]
        return v


def _fptr(a):
    arr = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))
    return arr, arr.ctypes.data_as(C.POINTER(C.c_float))


class Scene:
    """ITMScene<TVoxel,TIndex> + the two engines bound to it."""

    def __init__(self, be: Backend, handle: int):
        self.be, self.h = be, handle
        cfg, prm = SceneConfig(), SceneParams()
        be.check(be.fn["scene_get_config"](_P(handle), C.byref(cfg), C.byref(prm)), "scene_get_config")
        self.cfg, self.params = cfg, prm
        self.reco = SceneReconstructionEngine(self)
        self.vis = VisualisationEngine(self)

    @property
    def voxel_dtype(self):
        return VOXEL_DTYPES[self.cfg.voxelType]

    @property
    def is_hash(self):
        return self.cfg.indexType == INDEX_HASH

    def counters(self, rs: Optional["RenderState"] = None, stream=None) -> dict:
        c = Counters()
        self.be.check(self.be.fn["get_counters"](_P(self.h), _P(rs.h if rs else None), C.byref(c), _P(stream)), "get_counters")
        return c.as_dict()

    def save(self, directory: str, rs: Optional["RenderState"] = None, stream=None):
        """Scene checkpoint (itm_scene_save): MemoryBlockPersister-style files in an existing directory."""
        self.be.check(self.be.fn["scene_save"](_P(self.h), _P(rs.h if rs else None), directory.encode(), _P(stream)), "scene_save")

    def load(self, directory: str, rs: Optional["RenderState"] = None, stream=None):
        self.be.check(self.be.fn["scene_load"](_P(self.h), _P(rs.h if rs else None), directory.encode(), _P(stream)), "scene_load")

    def set_counters(self, rs, lastFreeBlockId, lastFreeExcessListId, noVisibleEntries, stream=None):
        c = Counters()
        c.lastFreeBlockId, c.lastFreeExcessListId, c.noVisibleEntries = lastFreeBlockId, lastFreeExcessListId, noVisibleEntries
        self.be.check(self.be.fn["set_counters"](_P(self.h), _P(rs.h if rs else None), C.byref(c), _P(stream)), "set_counters")

    def _dtype_of(self, which):
        return {BUF_HASH_ENTRIES: HASH_ENTRY_DTYPE, BUF_EXCESS_LIST: np.dtype("<i4"),
                BUF_VOXEL_BLOCKS: self.voxel_dtype, BUF_ALLOCATION_LIST: np.dtype("<i4"),
                BUF_VISIBLE_IDS: np.dtype("<i4"), BUF_VISIBLE_TYPE: np.dtype("u1"),
                BUF_RANGE_IMAGE: np.dtype("<f4"), BUF_RAYCAST_RESULT: np.dtype("<f4"),
                BUF_RAYCAST_IMAGE: np.dtype("u1"), BUF_FORWARD_PROJECTION: np.dtype("<f4"),
                BUF_MISSING_POINTS: np.dtype("<i4"), BUF_SWAP_STATES: np.dtype("u1")}[which]

    def profile_enable(self, mask: int):
        self.be.check(self.be.fn["profile_enable"](_P(self.h), mask), "profile_enable")

    def profile_sample(self, every: int):
        self.be.check(self.be.fn["profile_sample"](_P(self.h), every), "profile_sample")

    def profile_calibrate(self, n: int, stream=None):
        self.be.check(self.be.fn["profile_calibrate"](_P(self.h), int(n), _P(stream)), "profile_calibrate")

    def profile_read(self, reset=True) -> dict:
        p = Profile()
        self.be.check(self.be.fn["profile_read"](_P(self.h), C.byref(p), int(reset)), "profile_read")
        return {n: {"calls": int(p.calls[i]), "total_ms": float(p.total_ms[i])} for i, n in enumerate(TIMED_KERNELS)}

    def download(self, which: int, rs: Optional["RenderState"] = None, stream=None) -> np.ndarray:
        rsh = _P(rs.h if rs else None)
        n = self.be.fn["buffer_bytes"](_P(self.h), rsh, which)
        dt = self._dtype_of(which)
        out = np.empty(n // dt.itemsize, dtype=dt)
        self.be.check(self.be.fn["download"](_P(self.h), rsh, which, out.ctypes.data_as(_P), n, _P(stream)), "download")
        if rs is not None and which in (BUF_RANGE_IMAGE, BUF_RAYCAST_RESULT, BUF_FORWARD_PROJECTION, BUF_RAYCAST_IMAGE):
            comps = {BUF_RANGE_IMAGE: 2}.get(which, 4)
            out = out.reshape(rs.height, rs.width, comps)
        return out

    def upload(self, which: int, arr: np.ndarray, rs: Optional["RenderState"] = None, stream=None):
        arr = np.ascontiguousarray(arr)
        self.be.check(self.be.fn["upload"](_P(self.h), _P(rs.h if rs else None), which, arr.ctypes.data_as(_P), arr.nbytes, _P(stream)), "upload")

    def buffer_ptr(self, which, rs=None) -> int:
        return self.be.fn["buffer_ptr"](_P(self.h), _P(rs.h if rs else None), which) or 0

    # ITMSwappingEngine (scenes created with useSwapping)
    def swap_integrate_global_into_local(self, rs, stream=None):
        self.be.check(self.be.fn["swap_integrate_global_into_local"](_P(self.h), _P(rs.h), _P(stream)), "swap_integrate_global_into_local")

    def swap_save_to_global_memory(self, rs, stream=None):
        self.be.check(self.be.fn["swap_save_to_global_memory"](_P(self.h), _P(rs.h), _P(stream)), "swap_save_to_global_memory")

    def global_cache_flags(self) -> np.ndarray:
        n = self.be.fn["buffer_bytes"](_P(self.h), None, BUF_SWAP_STATES)
        out = np.zeros(n, np.uint8)
        self.be.check(self.be.fn["global_cache_flags"](_P(self.h), out.ctypes.data_as(_P), n), "global_cache_flags")
        return out

    def global_cache_block(self, entry: int):
        out = np.zeros(512, self.voxel_dtype)
        has = C.c_int()
        self.be.check(self.be.fn["global_cache_get"](_P(self.h), int(entry), out.ctypes.data_as(_P), C.byref(has)), "global_cache_get")
        return out if has.value else None

    def _slot_list(self, slots, stream):
        """(device pointer, count, buffer to close afterwards) of a slot list: None, a DevBuffer of int32 or a numpy array (uploaded)."""
        if slots is None:
            return None, 0, None
        if isinstance(slots, DevBuffer):
            return slots.ptr, slots.nbytes // 4, None
        arr = np.ascontiguousarray(np.asarray(slots, np.int32).reshape(-1))
        keep = self.be.to_backend(arr, stream)
        return keep.ptr, len(arr), keep

    def _slot_call(self, name, stats, src, slots, stream, *extra) -> dict:
        """extra: the arguments of the entry point between the two scenes and the slot list."""
        ptr, n, keep = self._slot_list(slots, stream)
        rc = self.be.fn[name](_P(self.h), _P(src.h), *extra, _P(ptr), n, C.byref(stats), _P(stream))
        if keep is not None:
            self.be.sync(stream)
            keep.close()
        self.be.check(rc, name)
        return stats.as_dict()

    def merge_from(self, src: "Scene", slots=None, stream=None) -> dict:
        """itm_scene_merge: fuses `src` into this scene on the GPU and returns the statistics.  slots: None (every slot of src's
        table), a DevBuffer of int32 table slots of src, or a numpy array of them (uploaded first)."""
        return self._slot_call("scene_merge", MergeStats(), src, slots, stream)

    def prune_config(self, **kw) -> PruneConfig:
        """itm_prune_default_config with the fields given in kw replaced."""
        cfg = PruneConfig()
        self.be.check(self.be.fn["prune_default_config"](C.byref(cfg)), "prune_default_config")
        return cfg.replace(**kw)

    def prune(self, cfg: Optional[PruneConfig] = None, decisions=False, stream=None) -> dict:
        """itm_scene_prune: returns the blocks `cfg` selects (None: the defaults, empty and free-space blocks) to the pool and gives
        the statistics; with `decisions` the dict also holds "decisions", the PRUNE_IS_* byte of every table entry.  Synchronises
        `stream`."""
        cfg = cfg if cfg is not None else self.prune_config()
        stats = PruneStats()
        n = self.be.fn["buffer_bytes"](_P(self.h), None, BUF_HASH_ENTRIES) // HASH_ENTRY_DTYPE.itemsize
        dev = DevBuffer(self.be, n, np.uint8, (n,)) if decisions else None
        rc = self.be.fn["scene_prune"](_P(self.h), C.byref(cfg), _P(dev.ptr if dev else None), C.byref(stats), _P(stream))
        out = stats.as_dict()
        if dev is not None:
            if rc == 0:
                out["decisions"] = dev.numpy(stream)
            dev.close()
        self.be.check(rc, "scene_prune")
        return out

    def coarsen_from(self, src: "Scene", slots=None, stream=None) -> dict:
        """itm_scene_coarsen: resamples `src` into this scene, which has twice src's voxel size, on the GPU and returns the statistics.
        slots: as merge_from."""
        return self._slot_call("scene_coarsen", CoarsenStats(), src, slots, stream)

    def resample_from(self, src: "Scene", q_or_matrix, slots=None, stream=None) -> dict:
        """itm_scene_resample: resamples `src` into this scene's frame and fuses it here, on the GPU; returns the statistics.
        q_or_matrix: a RigidQ, or the 4 x 4 matrix dstFromSrc in metres (quantised with this scene's voxel size).  slots: as merge_from."""
        q = q_or_matrix if isinstance(q_or_matrix, RigidQ) else rigid_quantise(q_or_matrix, float(self.params.voxelSize), self.be)
        return self._slot_call("scene_resample", ResampleStats(), src, slots, stream, C.byref(q))

    def align_config(self, **kw) -> AlignConfig:
        """itm_align_default_config for this scene's voxelSize and mu, with the fields given in kw replaced."""
        return align_default_config(float(self.params.voxelSize), float(self.params.mu), self.be).replace(**kw)

    def band_samples(self, cfg: Optional[AlignConfig] = None, slots=None, capacity=None, stream=None):
        """itm_scene_band_samples: (DevBuffer of float32 [min(count, capacity), 4] = (x, y, z in metres, sdf * mu), count).  cfg None:
        the defaults; slots: as merge_from; capacity None: asks for the count first and sizes the buffer from it."""
        cfg = cfg if cfg is not None else self.align_config()
        ptr, n, keep = self._slot_list(slots, stream)
        count = C.c_int32(0)
        try:
            if capacity is None:
                self.be.check(self.be.fn["scene_band_samples"](_P(self.h), _P(ptr), n, C.byref(cfg), None, 0, C.byref(count), _P(stream)), "scene_band_samples")
                capacity = count.value
            capacity = int(capacity)
            buf = DevBuffer(self.be, capacity * 16, np.float32, (capacity, 4))
            if capacity > 0:
                rc = self.be.fn["scene_band_samples"](_P(self.h), _P(ptr), n, C.byref(cfg), _P(buf.ptr), capacity, C.byref(count), _P(stream))
                if rc != 0:
                    buf.close()
                self.be.check(rc, "scene_band_samples")
        finally:
            if keep is not None:
                keep.close()
        held = min(capacity, count.value)
        buf.nbytes, buf.shape = held * 16, (held, 4)
        return buf, count.value

    def align_from(self, src: "Scene", init, cfg: Optional[AlignConfig] = None, slots=None, stream=None):
        """The pose dstFromSrc (4 x 4, x_self = M x_src, metres) that registers the band samples of `src` to this scene, refined from
        `init`: (matrix float32 [4, 4], AlignResult).  cfg None: the defaults; slots: the part of src to sample, as merge_from."""
        cfg = cfg if cfg is not None else self.align_config()
        samples, count = src.band_samples(cfg, slots, stream=stream)
        aligner = SceneAligner(self.be)
        try:
            aligner.set_samples(samples, count)
            return aligner.align(self, init, cfg, stream)
        finally:
            aligner.close()
            samples.close()

    def query_points(self, points, units="metres", want=("sdf", "gradient"), stream=None) -> dict:
        """itm_scene_query_points: the outputs named in `want` (QUERY_OUTPUTS) at float32 points [n, 3] in "metres" or "voxels", as a
        dict of numpy arrays.  Uploads the points, downloads the outputs and synchronises `stream`."""
        pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        n = len(pts)
        unknown = [w for w in want if w not in QUERY_OUTPUTS]
        if unknown:
            raise ItmError(f"query_points: unknown outputs {unknown}")
        dev_pts = self.be.to_backend(pts, stream) if n else None
        bufs = {w: DevBuffer(self.be, n * int(np.prod(QUERY_OUTPUTS[w][1] or (1,))) * np.dtype(QUERY_OUTPUTS[w][0]).itemsize, QUERY_OUTPUTS[w][0],
                             (n,) + QUERY_OUTPUTS[w][1]) for w in want}
        out = QueryOut()
        for w, b in bufs.items():
            setattr(out, w, b.ptr)
        rc = self.be.fn["scene_query_points"](_P(self.h), _P(dev_pts.ptr if n else None), n, {"metres": QUERY_METRES, "voxels": QUERY_VOXELS}[units],
                                              C.byref(out), _P(stream))
        self.be.sync(stream)
        res = {w: (b.numpy(stream) if n else np.zeros((0,) + QUERY_OUTPUTS[w][1], QUERY_OUTPUTS[w][0])) for w, b in bufs.items()} if rc == 0 else None
        for b in list(bufs.values()) + ([dev_pts] if n else []):
            b.close()
        self.be.check(rc, "scene_query_points")
        return res

    def cast_rays(self, rays, stream=None) -> np.ndarray:
        """itm_scene_cast_rays: float32 rays [n, 8] = (sx, sy, sz, t0, ex, ey, ez, t1) in metres -> float32 [n, 4] = (x, y, z, w) in
        voxel units, w = 1 a hit.  Uploads, downloads and synchronises `stream`."""
        r = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
        n = len(r)
        if n == 0:
            self.be.check(self.be.fn["scene_cast_rays"](_P(self.h), None, 0, None, _P(stream)), "scene_cast_rays")
            return np.zeros((0, 4), np.float32)
        dev_rays = self.be.to_backend(r, stream)
        hits = DevBuffer(self.be, n * 16, np.float32, (n, 4))
        rc = self.be.fn["scene_cast_rays"](_P(self.h), _P(dev_rays.ptr), n, _P(hits.ptr), _P(stream))
        self.be.sync(stream)
        res = hits.numpy(stream) if rc == 0 else None
        dev_rays.close(); hits.close()
        self.be.check(rc, "scene_cast_rays")
        return res

    def distance_field(self, origin, size, sites=("surface",), min_weight=1, max_distance=0, want=("dist2", "distance", "state"), stream=None) -> dict:
        """itm_scene_esdf: the Euclidean distance transform of the box with first voxel `origin` and `size` = (nx, ny, nz), voxel units.
        sites: names of ESDF_SITES (or the mask itself); max_distance in voxels, 0 = unbounded.  Returns the outputs named in `want`
        (ESDF_OUTPUTS) as numpy arrays [nz, ny, nx].  Downloads the outputs and synchronises `stream`."""
        mask = sites if isinstance(sites, int) else sum({ESDF_SITES[s] for s in sites})
        box = EsdfBox()
        box.origin[:] = [int(v) for v in origin]
        box.size[:] = [int(v) for v in size]
        out, bufs = _esdf_buffers(self.be, size, want)
        rc = self.be.fn["scene_esdf"](_P(self.h), C.byref(box), int(mask), int(min_weight), int(max_distance), C.byref(out), _P(stream))
        self.be.sync(stream)
        res = {w: bufs[w].numpy(stream) for w in want} if rc == 0 else None
        for b in bufs.values():
            b.close()
        self.be.check(rc, "scene_esdf")
        return res

    def accel_info(self) -> dict:
        """Sizes, placement and move count of the directory / mirror cubes (product library only)."""
        a = AccelInfo()
        self.be.check(self.be.fn["scene_accel_info"](_P(self.h), C.byref(a)), "scene_accel_info")
        return {"directory_bytes": a.directory_bytes, "slot_directory_bytes": a.slot_directory_bytes, "mirror_bytes": a.mirror_bytes,
                "mirror_pages": a.mirror_pages, "mirror_pages_mapped": a.mirror_pages_mapped, "origin_directory": list(a.origin_directory), "origin_mirror": list(a.origin_mirror), "placed": bool(a.placed), "moves": a.moves}

    def accel_probe(self, positions, stream=None) -> dict:
        """itm_debug_accel_probe: what the directory cubes and the sdf mirror hold at the block positions (int32[n][3]).  Arrays over
        the positions: dir_covered, dir_ptr, dir_slot, mirror_covered, page (the page-table entry, paged form), no_place, and
        values[n][512] -- the mirror's raw bits in the block's own voxel order (int16 for the short voxel types, uint32 for the float
        ones)."""
        pos = np.ascontiguousarray(np.asarray(positions, np.int32).reshape(-1, 3))
        n = len(pos)
        cells = np.zeros((n, 6), np.int32)
        values = np.zeros((n, 512), np.int16 if self.cfg.voxelType in (VOXEL_S, VOXEL_S_RGB) else np.uint32)
        self.be.check(self.be.fn["debug_accel_probe"](_P(self.h), pos.ctypes.data_as(_P), n, cells.ctypes.data_as(_P), values.ctypes.data_as(_P), _P(stream)),
                      "debug_accel_probe")
        return {"dir_covered": cells[:, 0] != 0, "dir_ptr": cells[:, 1].copy(), "dir_slot": cells[:, 2].copy(), "mirror_covered": cells[:, 3] != 0,
                "page": cells[:, 4].copy(), "no_place": cells[:, 5] != 0, "values": values}

    def accel_census(self, stream=None) -> dict:
        """itm_debug_accel_census: non-empty cells of the two directories, mirror blocks with a cell that is not "absent" (over the
        whole dense cube / over every page of the pool), the 4096-entry page table and the pool's raw page counter."""
        c = AccelCensus()
        table = np.zeros(4096, np.int32)
        self.be.check(self.be.fn["debug_accel_census"](_P(self.h), C.byref(c), table.ctypes.data_as(_P), _P(stream)), "debug_accel_census")
        return {"directory_cells": int(c.directory_cells), "slot_directory_cells": int(c.slot_directory_cells), "mirror_blocks": int(c.mirror_blocks),
                "page_counter": int(c.page_counter), "mirror_form": ("none", "dense", "paged")[c.mirror_form], "has_directory": bool(c.has_directory),
                "page_table": table}

    def deintegrate(self, view: View, rs: "RenderState", keep_saturated=None, stats=False, stream=None):
        """itm_deintegrate_from_scene: takes the depth (and colour) frame `view` back out of the voxels `rs`'s visible list names (a dense
        scene: every voxel).  keep_saturated: None (the scene's stopIntegratingAtMaxW), False or True.  With `stats` the counts come back
        as a dict and `stream` is synchronised; without, nothing is read back and None is returned."""
        vs = view if isinstance(view, ViewStruct) else view.struct()
        cfg = None
        if keep_saturated is not None:
            cfg = DeintegrateConfig()
            cfg.keepSaturated = keep_saturated if isinstance(keep_saturated, int) and not isinstance(keep_saturated, bool) else int(bool(keep_saturated))
        out = DeintegrateStats() if stats else None
        self.be.check(self.be.fn["deintegrate_from_scene"](_P(self.h), C.byref(vs), _P(rs.h if rs is not None else None), (C.byref(cfg) if cfg is not None else None),
                                                           (C.byref(out) if out is not None else None), _P(stream)), "deintegrate_from_scene")
        return out.as_dict() if out is not None else None

    def process_frame(self, view: View, rs: "RenderState", points: DevBuffer, normals: DevBuffer, stream=None):
        """ITMDenseMapper::ProcessFrame + ITMTrackingController::Prepare (Engine/ITMMainEngine.cpp:123-126)."""
        vs = view if isinstance(view, ViewStruct) else view.struct()      # callers on a hot loop keep one ViewStruct and update M_d in place
        self.be.check(self.be.fn["process_frame"](_P(self.h), C.byref(vs), _P(rs.h), _P(points.ptr), _P(normals.ptr), _P(stream)), "process_frame")

    def process_frame_ahead(self, view, next_view, rs: "RenderState", points: DevBuffer, normals: DevBuffer, stream=None):
        """itm_process_frame with the next frame's block requests issued beside this frame's ICP maps (next_view may be None)."""
        vs = view if isinstance(view, ViewStruct) else view.struct()
        ns = None if next_view is None else (next_view if isinstance(next_view, ViewStruct) else next_view.struct())
        self.be.check(self.be.fn["process_frame_ahead"](_P(self.h), C.byref(vs), (C.byref(ns) if ns is not None else None), _P(rs.h), _P(points.ptr), _P(normals.ptr),
                                                        _P(stream)), "process_frame_ahead")

    def set_deferred_fusion(self, on=True):
        """itm_scene_set_deferred_fusion: the four per-frame engine calls may be recorded and launched as one fused frame (the host
        accepts the contract in include/itm_hip.h).  A launch-level matter of the product: other implementations of the ABI ignore it."""
        if "scene_set_deferred_fusion" in self.be.fn:
            self.be.check(self.be.fn["scene_set_deferred_fusion"](_P(self.h), int(bool(on))), "scene_set_deferred_fusion")

    def flush(self, rs: "RenderState" = None, stream=None):
        """Launches the engine calls the library has recorded for this scene / render state (itm_flush)."""
        self.be.check(self.be.fn["flush"](_P(self.h), _P(rs.h if rs is not None else None), _P(stream)), "flush")

    def cancel_ahead(self, rs: "RenderState", stream=None):
        """Abandons the block requests itm_process_frame_ahead issued for the next view (itm_cancel_ahead)."""
        self.be.check(self.be.fn["cancel_ahead"](_P(self.h), _P(rs.h), _P(stream)), "cancel_ahead")

    def close(self):
        if self.h:
            self.be.fn["scene_destroy"](_P(self.h))
            self.h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Relocaliser:
    """itm_reloc: fern codes of depth frames, the keyframe database and its nearest-code search (include/itm_hip.h).

    Relocaliser(be, w, h) takes every default; numFerns / numDecisions / capacity / levels / blurRadius / blurTaps override the
    configuration, seed / lo / hi the default ferns, and pixel + threshold (arrays of numFerns * numDecisions) give explicit ferns."""

    def __init__(self, be: Backend, w: int, h: int, numFerns=None, numDecisions=None, capacity=None, levels=None, blurRadius=None,
                 blurTaps=None, seed=1, lo=0.2, hi=3.0, pixel=None, threshold=None):
        self.be, self.h = be, 0
        cfg = self.default_config(be, w, h)
        for name, v in (("numFerns", numFerns), ("numDecisions", numDecisions), ("capacity", capacity), ("levels", levels), ("blurRadius", blurRadius)):
            if v is not None:
                setattr(cfg, name, int(v))
        if blurTaps is not None:
            taps = [float(t) for t in blurTaps]
            cfg.blurTaps[:] = (taps + [0.0] * 9)[:9]
        if pixel is None:
            pixel, threshold = self.default_ferns(be, cfg, seed, lo, hi)
        self.pixel = np.ascontiguousarray(np.asarray(pixel, np.int32).reshape(-1))
        self.threshold = np.ascontiguousarray(np.asarray(threshold, np.float32).reshape(-1))
        n = max(int(cfg.numFerns), 0) * max(int(cfg.numDecisions), 0)
        if len(self.pixel) != n or len(self.threshold) != n:
            raise ItmError(f"Relocaliser: {n} decisions need {n} pixels and thresholds")
        p = _P()
        be.check(be.fn["reloc_create"](C.byref(cfg), self.pixel.ctypes.data_as(_P), self.threshold.ctypes.data_as(_P), C.byref(p)), "reloc_create")
        self.h, self.cfg = p.value, cfg
        self.small = (int(cfg.h) >> int(cfg.levels), int(cfg.w) >> int(cfg.levels))      # (hs, ws)

    @staticmethod
    def default_config(be: Backend, w: int, h: int) -> RelocConfig:
        cfg = RelocConfig()
        be.check(be.fn["reloc_default_config"](int(w), int(h), C.byref(cfg)), "reloc_default_config")
        return cfg

    @staticmethod
    def default_ferns(be: Backend, cfg: RelocConfig, seed=1, lo=0.2, hi=3.0):
        n = max(int(cfg.numFerns), 0) * max(int(cfg.numDecisions), 0)
        pixel, threshold = np.zeros(n, np.int32), np.zeros(n, np.float32)
        be.check(be.fn["reloc_default_ferns"](C.byref(cfg), int(seed), float(lo), float(hi), pixel.ctypes.data_as(_P), threshold.ctypes.data_as(_P)),
                 "reloc_default_ferns")
        return pixel, threshold

    @staticmethod
    def _dev(depth) -> int:
        return depth.ptr if isinstance(depth, DevBuffer) else int(depth)

    @property
    def count(self) -> int:
        n = C.c_int32()
        self.be.check(self.be.fn["reloc_info"](_P(self.h), C.byref(n), None), "reloc_info")
        return n.value

    def encode(self, depth, stream=None):
        """Enqueues the image and code kernels for a device depth image (DevBuffer or pointer); nothing is waited for."""
        self.be.check(self.be.fn["reloc_encode"](_P(self.h), _P(self._dev(depth)), _P(stream)), "reloc_encode")

    def read(self):
        """(small image float32[hs, ws], code uint8[numFerns]) of the last encode."""
        img, code = np.zeros(self.small, np.float32), np.zeros(int(self.cfg.numFerns), np.uint8)
        self.be.check(self.be.fn["reloc_read"](_P(self.h), img.ctypes.data_as(_P), code.ctypes.data_as(_P)), "reloc_read")
        return img, code

    def find(self, code=None, k=1, stream=None):
        """(ids int32[k], dist float32[k]) of the rows nearest to `code` (uint8[numFerns]; None: the last encoded code)."""
        kk = max(int(k), 1)
        ids, dist = np.zeros(kk, np.int32), np.zeros(kk, np.float32)
        c = None
        if code is not None:
            c = np.ascontiguousarray(np.asarray(code, np.uint8).reshape(-1))
            if len(c) != int(self.cfg.numFerns):
                raise ItmError("Relocaliser.find: a code has numFerns bytes")
        self.be.check(self.be.fn["reloc_find"](_P(self.h), c.ctypes.data_as(_P) if c is not None else None, int(k), ids.ctypes.data_as(_P),
                                               dist.ctypes.data_as(_P), _P(stream)), "reloc_find")
        return ids, dist

    def process_frame(self, depth, M_d=None, harvest=True, harvestThreshold=0.2, k=1, stream=None):
        """itm_reloc_process_frame: (ids, dist, added)."""
        kk = max(int(k), 1)
        ids, dist, added = np.zeros(kk, np.int32), np.zeros(kk, np.float32), C.c_int32()
        Mp = _fptr(M_d)[1] if M_d is not None else None
        self.be.check(self.be.fn["reloc_process_frame"](_P(self.h), _P(self._dev(depth)), Mp, int(bool(harvest)), float(harvestThreshold), int(k),
                                                        ids.ctypes.data_as(_P), dist.ctypes.data_as(_P), C.byref(added), _P(stream)), "reloc_process_frame")
        return ids, dist, added.value

    def pose(self, id: int) -> np.ndarray:
        M = (C.c_float * 16)()
        self.be.check(self.be.fn["reloc_get_pose"](_P(self.h), int(id), M), "reloc_get_pose")
        return np.array(M[:], np.float32)

    def codes(self):
        """(codes uint8[count, numFerns], poses float32[count, 16]) of the database."""
        n = self.count
        codes, poses = np.zeros((n, int(self.cfg.numFerns)), np.uint8), np.zeros((n, 16), np.float32)
        self.be.check(self.be.fn["reloc_download"](_P(self.h), codes.ctypes.data_as(_P), poses.ctypes.data_as(_P)), "reloc_download")
        return codes, poses

    def upload(self, codes, poses):
        codes = np.ascontiguousarray(np.asarray(codes, np.uint8).reshape(-1, int(self.cfg.numFerns)))
        poses = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 16))
        if len(codes) != len(poses):
            raise ItmError("Relocaliser.upload: one pose per code")
        self.be.check(self.be.fn["reloc_upload"](_P(self.h), len(codes), codes.ctypes.data_as(_P), poses.ctypes.data_as(_P)), "reloc_upload")

    def save(self, directory: str):
        self.be.check(self.be.fn["reloc_save"](_P(self.h), directory.encode()), "reloc_save")

    def load(self, directory: str):
        self.be.check(self.be.fn["reloc_load"](_P(self.h), directory.encode()), "reloc_load")

    def close(self):
        if self.h:
            self.be.fn["reloc_destroy"](_P(self.h))
            self.h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PoseQuality:
    """itm_pose_quality_handle: a depth image under a pose judged against the fused volume (include/itm_hip.h).  One handle per host
    thread; evaluate returns the counts (PoseQualityStats), with residuals=True also the per-pixel image float32[h, w]."""

    def __init__(self, be: Backend):
        self.be, self.h = be, 0
        p = _P()
        be.check(be.fn["pose_quality_create"](C.byref(p)), "pose_quality_create")
        self.h = p.value

    @staticmethod
    def default_config(be: Backend, mu: float) -> PoseQualityConfig:
        cfg = PoseQualityConfig()
        be.check(be.fn["pose_quality_default_config"](float(mu), C.byref(cfg)), "pose_quality_default_config")
        return cfg

    @staticmethod
    def verdict(be: Backend, stats: PoseQualityStats, cfg: PoseQualityConfig) -> int:
        out = C.c_int32(-1)
        be.check(be.fn["pose_quality_verdict"](C.byref(stats), C.byref(cfg), C.byref(out)), "pose_quality_verdict")
        return out.value

    def evaluate(self, scene: "Scene", view: "View", cfg: Optional[PoseQualityConfig] = None, residuals=False, stream=None):
        """itm_pose_quality_evaluate of view.depth under view.M_d; cfg None: the defaults for the scene's mu.  Returns the stats, or
        (stats, residual image) with residuals=True (downloaded: synchronises `stream`)."""
        if cfg is None:
            cfg = self.default_config(self.be, scene.params.mu)
        vs = view.struct()
        out = PoseQualityStats()
        buf = DevBuffer(self.be, view.w * view.h * 4, np.float32, (view.h, view.w)) if residuals else None
        rc = self.be.fn["pose_quality_evaluate"](_P(self.h), _P(scene.h), C.byref(vs), C.byref(cfg), C.byref(out), _P(buf.ptr if buf else None), _P(stream))
        img = buf.numpy(stream) if (buf is not None and rc == 0) else None
        if buf is not None:
            buf.close()
        self.be.check(rc, "pose_quality_evaluate")
        return (out, img) if residuals else out

    def close(self):
        if self.h:
            self.be.fn["pose_quality_destroy"](_P(self.h))
            self.h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SceneAligner:
    """itm_aligner: sdf samples (float4: a point in metres in the source frame and the signed distance in metres it should read)
    registered against a TSDF scene (include/itm_hip.h).  One handle per host thread.  The samples stay the caller's: set_samples keeps
    the buffer alive but does not copy it."""

    def __init__(self, be: Backend):
        self.be, self.h, self.samples = be, 0, None
        p = _P()
        be.check(be.fn["aligner_create"](C.byref(p)), "aligner_create")
        self.h = p.value

    def set_samples(self, samples, n=None, stream=None):
        """samples: a DevBuffer of float32 [n, 4] (Scene.band_samples), or a numpy array of them (uploaded)."""
        if not isinstance(samples, DevBuffer):
            arr = np.ascontiguousarray(np.asarray(samples, np.float32).reshape(-1, 4))
            samples = self.be.to_backend(arr, stream) if len(arr) else DevBuffer(self.be, 0, np.float32, (0, 4))
        n = samples.nbytes // 16 if n is None else int(n)
        self.be.check(self.be.fn["aligner_set_samples"](_P(self.h), _P(samples.ptr if n else None), n, _P(stream)), "aligner_set_samples")
        self.samples = samples

    def evaluate(self, dst: "Scene", M, cfg: Optional[AlignConfig] = None, stream=None) -> AlignEval:
        """itm_aligner_evaluate at dstFromSrc = M (4 x 4, or its 16 floats column-major)."""
        cfg = cfg if cfg is not None else dst.align_config()
        flat = _matrix16(M)
        out = AlignEval()
        self.be.check(self.be.fn["aligner_evaluate"](_P(self.h), _P(dst.h), flat.ctypes.data_as(C.POINTER(C.c_float)), C.byref(cfg), C.byref(out), _P(stream)),
                      "aligner_evaluate")
        return out

    def align(self, dst: "Scene", init, cfg: Optional[AlignConfig] = None, stream=None):
        """itm_aligner_align from dstFromSrc = init: (matrix float32 [4, 4], AlignResult)."""
        cfg = cfg if cfg is not None else dst.align_config()
        flat = _matrix16(init)
        out = np.zeros(16, np.float32)
        res = AlignResult()
        self.be.check(self.be.fn["aligner_align"](_P(self.h), _P(dst.h), flat.ctypes.data_as(C.POINTER(C.c_float)), C.byref(cfg),
                                                  out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res), _P(stream)), "aligner_align")
        return np.ascontiguousarray(out.reshape(4, 4).T), res

    def close(self):
        if self.h:
            self.be.fn["aligner_destroy"](_P(self.h))
            self.h = 0
        self.samples = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mesh:
    """ITMMesh + ITMMeshingEngine::MeshScene (Objects/ITMMesh.h, Engine/ITMMeshingEngine.h)."""

    def __init__(self, scene: "Scene", max_triangles: int = 0):
        self.scene = scene
        p = _P()
        scene.be.check(scene.be.fn["mesh_create"](_P(scene.h), max_triangles, C.byref(p)), "mesh_create")
        self.h = p.value

    def MeshScene(self, stream=None):
        self.scene.be.check(self.scene.be.fn["mesh_scene"](_P(self.scene.h), _P(self.h), _P(stream)), "mesh_scene")

    def MeshVolume(self, stream=None):
        """itm_mesh_volume: MeshScene for a hash scene; a dense scene is meshed brick by brick (MeshScene leaves it empty)."""
        self.scene.be.check(self.scene.be.fn["mesh_volume"](_P(self.scene.h), _P(self.h), _P(stream)), "mesh_volume")

    def info(self, stream=None):
        n, cap = C.c_uint32(), C.c_uint32()
        self.scene.be.check(self.scene.be.fn["mesh_info"](_P(self.h), C.byref(n), C.byref(cap), None, _P(stream)), "mesh_info")
        return n.value, cap.value

    def triangles(self, stream=None) -> np.ndarray:
        """(noTotalTriangles, 3, 3) float32: p0, p1, p2 per triangle."""
        n, _ = self.info(stream)
        out = np.zeros((n, 3, 3), np.float32)
        got = C.c_uint32()
        self.scene.be.check(self.scene.be.fn["mesh_download"](_P(self.h), out.ctypes.data_as(_P), n, C.byref(got), _P(stream)), "mesh_download")
        return out

    def WriteOBJ(self, path: str, stream=None):
        self.scene.be.check(self.scene.be.fn["mesh_write_obj"](_P(self.h), path.encode(), _P(stream)), "mesh_write_obj")

    def WriteSTL(self, path: str, stream=None):
        self.scene.be.check(self.scene.be.fn["mesh_write_stl"](_P(self.h), path.encode(), _P(stream)), "mesh_write_stl")

    def ComputeAttributes(self, what: int = MESH_NORMALS, stream=None):
        """Per-vertex normals (MESH_NORMALS) and / or colours (MESH_COLOURS) of the triangles MeshScene left in the buffer."""
        self.scene.be.check(self.scene.be.fn["mesh_attributes"](_P(self.scene.h), _P(self.h), int(what), _P(stream)), "mesh_attributes")

    def _attributes(self, normals: bool, stream):
        n, _ = self.info(stream)
        out = np.zeros((n, 3, 3), np.float32) if normals else np.zeros((n, 3, 4), np.uint8)
        got = C.c_uint32()
        p = out.ctypes.data_as(_P)
        self.scene.be.check(self.scene.be.fn["mesh_download_attributes"](_P(self.h), p if normals else None, None if normals else p, n,
                                                                         C.byref(got), _P(stream)), "mesh_download_attributes")
        return out

    def normals(self, stream=None) -> np.ndarray:
        """(noTotalTriangles, 3, 3) float32: the unit normal of p0, p1, p2 per triangle."""
        return self._attributes(True, stream)

    def colours(self, stream=None) -> np.ndarray:
        """(noTotalTriangles, 3, 4) uint8: r, g, b, 255 of p0, p1, p2 per triangle."""
        return self._attributes(False, stream)

    def WritePLY(self, path: str, stream=None):
        self.scene.be.check(self.scene.be.fn["mesh_write_ply"](_P(self.h), path.encode(), _P(stream)), "mesh_write_ply")

    def Index(self, stream=None):
        """Welds the triangles MeshScene left in the buffer into shared vertices (bit-equal positions are one vertex)."""
        self.scene.be.check(self.scene.be.fn["mesh_index"](_P(self.h), _P(stream)), "mesh_index")

    def index_info(self, stream=None):
        """(number of unique vertices, number of triangles) of the index"""
        nv, nt = C.c_uint32(), C.c_uint32()
        self.scene.be.check(self.scene.be.fn["mesh_index_info"](_P(self.h), C.byref(nv), C.byref(nt), None, None, None, _P(stream)), "mesh_index_info")
        return nv.value, nt.value

    def _indexed(self, which: int, stream):
        nv, nt = self.index_info(stream)
        out = (np.zeros((nv, 3), np.float32), np.zeros(nv, np.uint32), np.zeros((nt, 3), np.uint32))[which]
        p = [None, None, None]
        p[which] = out.ctypes.data_as(_P)
        self.scene.be.check(self.scene.be.fn["mesh_download_indexed"](_P(self.h), p[0], p[1], nv, p[2], nt, None, None, _P(stream)), "mesh_download_indexed")
        return out

    def vertices(self, stream=None) -> np.ndarray:
        """(noVertices, 3) float32: the distinct positions in the order of their first occurrence in the triangle buffer."""
        return self._indexed(0, stream)

    def first(self, stream=None) -> np.ndarray:
        """(noVertices,) uint32: the first soup vertex (3 * triangle + corner) that holds each unique vertex, strictly ascending."""
        return self._indexed(1, stream)

    def faces(self, stream=None) -> np.ndarray:
        """(noTotalTriangles, 3) uint32: vertices()[faces()] is triangles()."""
        return self._indexed(2, stream)

    def ComputeIndexedAttributes(self, what: int = MESH_NORMALS, stream=None):
        """Normals and / or colours per unique vertex of the index, evaluated once per vertex."""
        self.scene.be.check(self.scene.be.fn["mesh_indexed_attributes"](_P(self.scene.h), _P(self.h), int(what), _P(stream)), "mesh_indexed_attributes")

    def _indexed_attributes(self, normals: bool, stream):
        nv, _ = self.index_info(stream)
        out = np.zeros((nv, 3), np.float32) if normals else np.zeros((nv, 4), np.uint8)
        got = C.c_uint32()
        p = out.ctypes.data_as(_P)
        self.scene.be.check(self.scene.be.fn["mesh_download_indexed_attributes"](_P(self.h), p if normals else None, None if normals else p, nv,
                                                                                 C.byref(got), _P(stream)), "mesh_download_indexed_attributes")
        return out

    def vertex_normals(self, stream=None) -> np.ndarray:
        """(noVertices, 3) float32: the unit normal of every unique vertex."""
        return self._indexed_attributes(True, stream)

    def vertex_colours(self, stream=None) -> np.ndarray:
        """(noVertices, 4) uint8: r, g, b, 255 of every unique vertex."""
        return self._indexed_attributes(False, stream)

    def WriteIndexedPLY(self, path: str, stream=None):
        self.scene.be.check(self.scene.be.fn["mesh_write_ply_indexed"](_P(self.h), path.encode(), _P(stream)), "mesh_write_ply_indexed")

    def WriteIndexedOBJ(self, path: str, stream=None):
        self.scene.be.check(self.scene.be.fn["mesh_write_obj_indexed"](_P(self.h), path.encode(), _P(stream)), "mesh_write_obj_indexed")

    def Components(self, stream=None):
        """Labels the connected components of the present index (vertices are linked iff a triangle names both)."""
        self.scene.be.check(self.scene.be.fn["mesh_components"](_P(self.h), _P(stream)), "mesh_components")

    def components_info(self, stream=None):
        """(number of components, union rounds the labelling took)"""
        nc, rounds = C.c_uint32(), C.c_uint32()
        self.scene.be.check(self.scene.be.fn["mesh_components_info"](_P(self.h), C.byref(nc), C.byref(rounds), None, None, None, _P(stream)),
                            "mesh_components_info")
        return nc.value, rounds.value

    def _components(self, which: int, stream):
        nc, _ = self.components_info(stream)
        nv, nt = self.index_info(stream)
        out = (np.zeros(nv, np.uint32), np.zeros(nt, np.uint32), np.zeros(nc, MESH_COMPONENT_DTYPE))[which]
        p = [None, None, None]
        p[which] = out.ctypes.data_as(_P)
        self.scene.be.check(self.scene.be.fn["mesh_download_components"](_P(self.h), p[0], nv, p[1], nt, p[2], nc, None, _P(stream)),
                            "mesh_download_components")
        return out

    def vertex_component(self, stream=None) -> np.ndarray:
        """(noVertices,) uint32: the component number of every unique vertex."""
        return self._components(0, stream)

    def triangle_component(self, stream=None) -> np.ndarray:
        """(noTotalTriangles,) uint32: the component of every triangle's first corner."""
        return self._components(1, stream)

    def components(self, stream=None) -> np.ndarray:
        """(noComponents,) MESH_COMPONENT_DTYPE: firstVertex (the root), noVertices, noTriangles, reserved, bbMin, bbMax."""
        return self._components(2, stream)

    def FilterComponents(self, min_triangles: int = 0, keep=None, stream=None):
        """Keeps the triangles of the components with at least min_triangles triangles and, keep given (one entry per component), a
        non-zero entry there; the kept triangles are packed to the front of the buffer in their order.  Attributes, index and components
        are stale afterwards.  Returns (kept triangles, kept components)."""
        kt, kc = C.c_uint32(), C.c_uint32()
        mask = None if keep is None else np.ascontiguousarray(np.asarray(keep) != 0, np.uint8).reshape(-1)
        buf = mask if mask is None or len(mask) else np.zeros(1, np.uint8)       # an empty mask is still a mask: never a null pointer
        rc = self.scene.be.fn["mesh_filter_components"](_P(self.h), int(min_triangles), None if mask is None else buf.ctypes.data_as(_P),
                                                        0 if mask is None else len(mask), C.byref(kt), C.byref(kc), _P(stream))
        self.scene.be.check(rc, "mesh_filter_components")
        return kt.value, kc.value

    def KeepLargest(self, n: int = 1, stream=None):
        """FilterComponents keeping the n components with the most triangles; ties go to the lower component number."""
        tri = self.components(stream)["noTriangles"].astype(np.int64)
        keep = np.zeros(len(tri), np.uint8)
        keep[np.argsort(-tri, kind="stable")[:max(int(n), 0)]] = 1
        return self.FilterComponents(0, keep, stream)

    def Smooth(self, steps: int = 20, lam: float = 0.5, mu: float = -0.53, quantum=None, pin_irregular: bool = True, stream=None) -> dict:
        """Fixed-point Taubin (lam, mu) or Laplacian (mu = lam) passes over the present index: positions move, faces / first / counts
        stay; vertices() and triangles() change together.  quantum None: voxelSize / 1024.  The soup's and the indexed attributes and
        the components are stale afterwards; the index stays current.  Returns the statistics."""
        be = self.scene.be
        cfg = MeshSmoothConfig()
        if quantum is None:
            be.check(be.fn["mesh_smooth_default_config"](float(self.scene.params.voxelSize), C.byref(cfg)), "mesh_smooth_default_config")
            quantum = cfg.quantum
        cfg = mesh_smooth_config(quantum, steps, lam, mu, pin_irregular)
        stats = MeshSmoothStats()
        be.check(be.fn["mesh_smooth"](_P(self.h), C.byref(cfg), C.byref(stats), _P(stream)), "mesh_smooth")
        return stats.as_dict()

    def Touch(self, rs: Optional["RenderState"] = None, slots=None, everything: bool = False, stream=None):
        """itm_mesh_touch: marks the blocks that were rewritten since the mesh was last up to date -- the visible list of `rs` (what a
        fused frame wrote), the table slots `slots` (a DevBuffer of int32 or a numpy array, uploaded first), or everything.  Marks
        accumulate until Update consumes them."""
        be = self.scene.be
        if everything:
            be.check(be.fn["mesh_touch"](_P(self.h), _P(self.scene.h), None, None, -1, _P(stream)), "mesh_touch")
        if rs is None and slots is None:
            return
        empty = slots is not None and not isinstance(slots, DevBuffer) and np.asarray(slots).size == 0
        ptr, n, keep = self.scene._slot_list(np.zeros(1, np.int32) if empty else slots, stream)      # an empty list is still a list: never a null pointer
        n = 0 if empty or slots is None else n
        rc = be.fn["mesh_touch"](_P(self.h), _P(self.scene.h), _P(rs.h if rs is not None else None), _P(ptr), n, _P(stream))
        if keep is not None:
            be.sync(stream)
            keep.close()
        be.check(rc, "mesh_touch")

    def Update(self, stream=None) -> dict:
        """itm_mesh_update: re-meshes the marked blocks, those that appeared or vanished and their -d neighbours, and keeps every other
        run; equal to MeshScene bit for bit when every rewritten block was marked.  triangles() may live at another address afterwards.
        Returns the statistics; "full" is 0 or the MESH_UPDATE_* reason for which the call was MeshScene."""
        stats = MeshUpdateStats()
        self.scene.be.check(self.scene.be.fn["mesh_update"](_P(self.scene.h), _P(self.h), C.byref(stats), _P(stream)), "mesh_update")
        return stats.as_dict()

    def update_delta(self, stream=None) -> dict:
        """The delta of the last Update: "changed" (MESH_CHANGED_DTYPE: slot, pos, firstTriangle, noTriangles of every re-meshed block,
        ascending slots) and "removed" (MESH_REMOVED_DTYPE: the old slot and position of the blocks that are gone)."""
        be = self.scene.be
        nc, nr = C.c_uint32(), C.c_uint32()
        be.check(be.fn["mesh_update_info"](_P(self.h), C.byref(nc), C.byref(nr), None, None, _P(stream)), "mesh_update_info")
        changed, removed = np.zeros(nc.value, MESH_CHANGED_DTYPE), np.zeros(nr.value, MESH_REMOVED_DTYPE)
        be.check(be.fn["mesh_download_update"](_P(self.h), changed.ctypes.data_as(_P), nc.value, removed.ctypes.data_as(_P), nr.value, None, None,
                                               _P(stream)), "mesh_download_update")
        return {"changed": changed, "removed": removed}

    def close(self):
        if self.h:
            self.scene.be.fn["mesh_destroy"](_P(self.h))
            self.h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RenderState:
    """ITMRenderState / ITMRenderState_VH (Objects/ITMRenderState.h, ITMRenderState_VH.h)."""

    def __init__(self, scene: Scene, w: int, h: int):
        self.scene, self.width, self.height = scene, w, h
        p = _P()
        scene.be.check(scene.be.fn["render_state_create"](_P(scene.h), w, h, C.byref(p)), "render_state_create")
        self.h = p.value

    def close(self):
        if self.h:
            self.scene.be.fn["render_state_destroy"](_P(self.h))
            self.h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SceneReconstructionEngine:
    """Mirror of ITMSceneReconstructionEngine<TVoxel,TIndex> (Engine/ITMSceneReconstructionEngine.h:28-52)."""

    def __init__(self, scene: Scene):
        self.s = scene

    def ResetScene(self, stream=None):
        self.s.be.check(self.s.be.fn["reset_scene"](_P(self.s.h), _P(stream)), "reset_scene")

    def AllocateSceneFromDepth(self, view: View, renderState: RenderState, onlyUpdateVisibleList=False, stream=None):
        vs = view.struct()
        self.s.be.check(self.s.be.fn["allocate_scene_from_depth"](_P(self.s.h), C.byref(vs), _P(renderState.h), int(onlyUpdateVisibleList), _P(stream)), "allocate_scene_from_depth")

    def IntegrateIntoScene(self, view: View, renderState: RenderState, stream=None):
        vs = view.struct()
        self.s.be.check(self.s.be.fn["integrate_into_scene"](_P(self.s.h), C.byref(vs), _P(renderState.h), _P(stream)), "integrate_into_scene")


class VisualisationEngine:
    """Mirror of IITMVisualisationEngine (Engine/ITMVisualisationEngine.h:18-81)."""

    def __init__(self, scene: Scene):
        self.s = scene

    def CreateRenderState(self, imgSize) -> RenderState:
        return RenderState(self.s, int(imgSize[0]), int(imgSize[1]))

    def _pose_call(self, name, M, intr, rs, stream, *extra):
        Ma, Mp = _fptr(M)
        Ia, Ip = _fptr(intr)
        self.s.be.check(self.s.be.fn[name](_P(self.s.h), Mp, Ip, _P(rs.h), *extra, _P(stream)), name)

    def FindVisibleBlocks(self, pose_M, intrinsics, renderState, stream=None):
        self._pose_call("find_visible_blocks", pose_M, intrinsics, renderState, stream)

    def CreateExpectedDepths(self, pose_M, intrinsics, renderState, stream=None):
        self._pose_call("create_expected_depths", pose_M, intrinsics, renderState, stream)

    def RenderImage(self, pose_M, intrinsics, renderState, outputImage: Optional[DevBuffer] = None,
                    type=RENDER_SHADED_GREYSCALE, stream=None):
        self._pose_call("render_image", pose_M, intrinsics, renderState, stream,
                        _P(outputImage.ptr if outputImage else None), int(type))

    def FindSurface(self, pose_M, intrinsics, renderState, stream=None):
        self._pose_call("find_surface", pose_M, intrinsics, renderState, stream)

    # the static colour maps of IITMVisualisationEngine (Engine/ITMVisualisationEngine.cpp:19-107) on device images:
    # dst uchar4[h*w], src float[h*w] (float4[h*w] for the normals), imgSize = (w, h)
    def _image_map(self, name, dst: DevBuffer, src: DevBuffer, imgSize, stream):
        self.s.be.check(self.s.be.fn[name](_P(src.ptr), _P(dst.ptr), int(imgSize[0]), int(imgSize[1]), _P(stream)), name)

    def DepthToUchar4(self, dst: DevBuffer, src: DevBuffer, imgSize, stream=None):
        self._image_map("depth_to_uchar4", dst, src, imgSize, stream)

    def WeightToUchar4(self, dst: DevBuffer, src: DevBuffer, imgSize, stream=None):
        self._image_map("weight_to_uchar4", dst, src, imgSize, stream)

    def NormalToUchar4(self, dst: DevBuffer, src: DevBuffer, imgSize, stream=None):
        self._image_map("normal_to_uchar4", dst, src, imgSize, stream)

    def CreatePointCloud(self, view: View, renderState, locations: DevBuffer, colours: DevBuffer, skipPoints=False, stream=None):
        vs = view.struct()
        self.s.be.check(self.s.be.fn["create_point_cloud"](_P(self.s.h), C.byref(vs), _P(renderState.h), int(skipPoints), _P(locations.ptr), _P(colours.ptr), _P(stream)), "create_point_cloud")

    def CreateICPMaps(self, view: View, renderState, points: DevBuffer, normals: DevBuffer, stream=None):
        vs = view.struct()
        self.s.be.check(self.s.be.fn["create_icp_maps"](_P(self.s.h), C.byref(vs), _P(renderState.h), _P(points.ptr), _P(normals.ptr), _P(stream)), "create_icp_maps")

    def ForwardRender(self, view: View, renderState, stream=None):
        vs = view.struct()
        self.s.be.check(self.s.be.fn["forward_render"](_P(self.s.h), C.byref(vs), _P(renderState.h), _P(stream)), "forward_render")
