// itm_hip_engines.hpp -- C++ host side above the C-ABI (include/itm_hip.h).
//
// Header-only adapter classes with the method names, argument meaning and (void / throwing) error
// behaviour of the reference's engine interfaces, so that code written against
//   ITMLib::Engine::ITMSceneReconstructionEngine<TVoxel,TIndex>   (Engine/ITMSceneReconstructionEngine.h:28-52)
//   ITMLib::Engine::ITMVisualisationEngine<TVoxel,TIndex>         (Engine/ITMVisualisationEngine.h:18-107)
// reads the same against the HIP back-end.  The reference's own object headers are NOT included:
// the few host-side value types the methods take (pose, intrinsics, view, tracking state, scene
// shell, render-state shell) are re-declared here as thin shells over device handles.  A maintainer
// of the reference instead derives two classes from the reference's abstract engines and forwards
// to the same C functions -- see INTEGRATION.md for that stub.
//
// Everything lives in HBM and is owned by the C library; the shells only carry handles.  Device
// errors become std::runtime_error (the reference prints and exit(-1)s: ORUtils/CUDADefines.h:27-36).
#pragma once

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "itm_hip.h"

namespace itmhip {

inline void check(int rc, const char* what) {
  if (rc != ITM_OK) throw std::runtime_error(std::string(what) + ": " + itm_last_error());
}

// voxel / index tags replacing the reference's TVoxel / TIndex template arguments
struct ITMVoxel_s { static constexpr int kType = ITM_VOXEL_S; };
struct ITMVoxel_f { static constexpr int kType = ITM_VOXEL_F; };
struct ITMVoxel_s_rgb { static constexpr int kType = ITM_VOXEL_S_RGB; };
struct ITMVoxel_f_rgb { static constexpr int kType = ITM_VOXEL_F_RGB; };
struct ITMVoxelBlockHash { static constexpr int kType = ITM_INDEX_HASH; };
struct ITMPlainVoxelArray { static constexpr int kType = ITM_INDEX_DENSE; };

struct Vector2i { int x, y; };
struct Vector2f { float x, y; };
struct Vector4u { uint8_t x, y, z, w; };
// ORUtils::Matrix4<float> as far as the path needs it: 16 floats, column-major (m[4 * column + row]), like every matrix of the C-ABI
struct Matrix4f {
  float m[16];
  Matrix4f() { std::memset(m, 0, sizeof m); m[0] = m[5] = m[10] = m[15] = 1.0f; }
  explicit Matrix4f(const float* values) { std::memcpy(m, values, sizeof m); }
};

// ITMUChar4Image (Utils/ITMLibDefines.h, ORUtils/Image.h) as far as ITMMainEngine::GetImage needs it: a host image of Vector4u
class ITMUChar4Image {
  std::vector<Vector4u> data;

 public:
  Vector2i noDims{0, 0};
  size_t dataSize = 0;
  ITMUChar4Image() {}
  explicit ITMUChar4Image(Vector2i dims) { ChangeDims(dims); Clear(); }
  // ORUtils/Image.h:50-59: a new size gives a new buffer; the pixels are the caller's to fill
  void ChangeDims(Vector2i newDims) {
    if (newDims.x == noDims.x && newDims.y == noDims.y) return;
    noDims = newDims; dataSize = (size_t)newDims.x * (size_t)newDims.y;
    data.assign(dataSize, Vector4u{0, 0, 0, 0});
  }
  void Clear(uint8_t defaultValue = 0) { if (dataSize) std::memset(data.data(), defaultValue, dataSize * sizeof(Vector4u)); }
  Vector4u* GetData() { return data.data(); }
  const Vector4u* GetData() const { return data.data(); }
};

// ITMPose: only the model-view matrix is needed by the path (Objects/ITMPose.h GetM()).
struct ITMPose {
  float M[16];
  ITMPose() { std::memset(M, 0, sizeof M); M[0] = M[5] = M[10] = M[15] = 1.0f; }
  void SetM(const float* m) { std::memcpy(M, m, sizeof M); }
  const float* GetM() const { return M; }
};

// ITMIntrinsics::projectionParamsSimple.all (Objects/ITMIntrinsics.h)
struct ITMIntrinsics {
  float all[4];
  ITMIntrinsics() { SetFrom(580, 580, 320, 240); }
  void SetFrom(float fx, float fy, float cx, float cy) { all[0] = fx; all[1] = fy; all[2] = cx; all[3] = cy; }
};

// ITMRGBDCalib (Objects/ITMRGBDCalib.h): intrinsics + rgb->depth extrinsics
struct ITMRGBDCalib {
  ITMIntrinsics intrinsics_rgb, intrinsics_d;
  float trafo_rgb_to_depth_calib[16], trafo_rgb_to_depth_calib_inv[16];
  ITMRGBDCalib() {
    std::memset(trafo_rgb_to_depth_calib, 0, 64);
    trafo_rgb_to_depth_calib[0] = trafo_rgb_to_depth_calib[5] = trafo_rgb_to_depth_calib[10] = trafo_rgb_to_depth_calib[15] = 1.0f;
    std::memcpy(trafo_rgb_to_depth_calib_inv, trafo_rgb_to_depth_calib, 64);
  }
};

// ITMView (Objects/ITMView.h): device images + calibration
struct ITMView {
  ITMRGBDCalib calib;
  const float* depth = nullptr;  // device float[h*w]
  const uint8_t* rgb = nullptr;  // device uchar4[h_rgb*w_rgb]
  const float* depthUncertainty = nullptr;  // device float[h*w]: sigmaZ of ComputeNormalAndWeights (modelSensorNoise, TRACKER_WICP)
  Vector2i depthSize{0, 0}, rgbSize{0, 0};
};

struct ITMSceneParamsDefaults { float mu = 0.02f; int maxW = 100; float voxelSize = 0.005f, viewFrustum_min = 0.35f, viewFrustum_max = 3.0f; bool stopIntegratingAtMaxW = false; };

// ITMTrackingState (Objects/ITMTrackingState.h): pose + the ICP maps written by CreateICPMaps
struct ITMTrackingState {
  ITMPose pose_d, pose_pointCloud;
  float* pointCloud_locations = nullptr;  // device Vector4f[h*w]
  float* pointCloud_colours = nullptr;    // device Vector4f[h*w] (normals for the ICP tracker)
  int age_pointCloud = -1;
  bool requiresFullRendering = true;

  // camera centre -1 * (R^T T) of a world->camera matrix, component i = column i of R dotted with T, summed left to right
  // (Matrix3::t() and Matrix3 * Vector3 of ORUtils/Matrix.h:270-296)
  static void CameraCentre(const float* M, float c[3]) {
    for (int i = 0; i < 3; ++i) c[i] = -1.0f * (M[0 + 4 * i] * M[12] + M[1 + 4 * i] * M[13] + M[2 + 4 * i] * M[14]);
  }
  // ITMTrackingState::TrackerFarFromPointCloud (Objects/ITMTrackingState.h:41-59)
  bool TrackerFarFromPointCloud() const {
    if (age_pointCloud < 0) return true;       // no point cloud exists yet
    if (age_pointCloud > 5) return true;       // older than n frames
    float pc[3], live[3];
    CameraCentre(pose_pointCloud.GetM(), pc);
    CameraCentre(pose_d.GetM(), live);
    const float dx = pc[0] - live[0], dy = pc[1] - live[1], dz = pc[2] - live[2];
    const float diff = dx * dx + dy * dy + dz * dz;
    return diff > 0.0005f;                     // the camera centre has moved by more than the threshold
  }
};

// ITMLibSettings (Utils/ITMLibSettings.h / .cpp:9-90): the members the path's callers read, with the reference's defaults
struct ITMLibSettings {
  enum TrackerType { TRACKER_COLOR, TRACKER_ICP, TRACKER_EXTERNAL, TRACKER_REN, TRACKER_WICP };   // TRACKER_REN, TRACKER_WICP appended: the others keep their values
  ITMSceneParamsDefaults sceneParamsDefaults;   // (0.02, 100, 0.005, 0.35, 3.0, false), ITMLibSettings.cpp:10
  float depthTrackerICPThreshold = 0.1f * 0.1f;
  float depthTrackerTerminationThreshold = 1e-3f;
  bool skipPoints = true;
  bool useApproximateRaycast = false;
  bool useBilateralFilter = false;
  bool modelSensorNoise = false;
  TrackerType trackerType = TRACKER_EXTERNAL;   // this fork's default: poses come from outside (ITMExternalTracker.cpp:27-30)
  int noHierarchyLevels = 5;
  int trackingRegime[8] = {ITM_TRACKER_ITERATION_BOTH, ITM_TRACKER_ITERATION_BOTH, ITM_TRACKER_ITERATION_ROTATION, ITM_TRACKER_ITERATION_ROTATION,
                           ITM_TRACKER_ITERATION_ROTATION, 0, 0, 0};
  int noICPRunTillLevel = 0;
  // TRACKER_COLOR: false (default) keeps this fork's behaviour, poses from outside; true builds ITMColorTracker_HIP
  bool useColourTracker = false;
  // Keyframe relocaliser (ITMRelocaliser_HIP; the reference at this revision has none).  false (default): nothing is created and no
  // code path changes.  true: ITMMainEngine_HIP harvests keyframes while it fuses and offers Relocalise().
  bool useRelocalisation = false;
  float relocHarvestingThreshold = 0.2f;      // a frame becomes a keyframe when its nearest keyframe is further than this
  int relocCapacity = 65536;                  // rows of the keyframe database
  // Tracking verdict (ITMPoseQuality_HIP, itm_pose_quality_*; the reference at this revision has none).  false (default): nothing is
  // created and no code path changes.  true: ITMMainEngine_HIP judges every tracked pose against the fused volume, fuses and
  // harvests GOOD frames only and, with useRelocalisation, recovers a FAILED pose from the nearest keyframe.
  bool useTrackingVerdict = false;
  // The verdict's thresholds: filled by itm_pose_quality_default_config(mu) when inlierDistance is 0.  The defaults are policy,
  // chosen on a synthetic scene and not tuned on sensor data (include/itm_hip.h).
  itm_pose_quality_config poseQuality = {0.0f, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  int relocFusionDelay = 10;                  // GOOD frames that are tracked but not fused after a recovery
  // Scene pruning (itm_scene_prune; the reference has none).  0 (default): never, and no code path changes.  N > 0: ITMMainEngine_HIP
  // prunes its scene with pruneConfig after every N-th frame it has fused, once that frame's maps are prepared.
  int pruneEveryNFrames = 0;
  itm_prune_config pruneConfig = {ITM_PRUNE_EMPTY | ITM_PRUNE_FREE, 1.0f, 1, 1, {0, 0, 0}, {0, 0, 0}, 0, 0};      // itm_prune_default_config
  // Live mesh (itm_mesh_touch / itm_mesh_update; the reference meshes on request only).  0 (default): none, and no code path changes.
  // N > 0: ITMMainEngine_HIP (hash scenes) owns a mesh that follows its scene: every fused frame marks the blocks it wrote, and after
  // every N-th fused frame, once that frame's maps are prepared, the marked blocks are re-meshed (GetLiveMesh, GetLastMeshUpdateStats).
  int liveMeshEveryNFrames = 0;
};

struct ITMSceneParams : itm_scene_params {
  ITMSceneParams(float mu_, int maxW_, float voxelSize_, float vfMin, float vfMax, bool stopAtMax) {
    mu = mu_; maxW = maxW_; voxelSize = voxelSize_; viewFrustum_min = vfMin; viewFrustum_max = vfMax;
    stopIntegratingAtMaxW = stopAtMax ? 1 : 0;
  }
};

// ITMScene<TVoxel,TIndex> (Objects/ITMScene.h:37-43): owns the device scene
template <class TVoxel, class TIndex>
class ITMScene {
 public:
  itm_scene* handle = nullptr;
  const ITMSceneParams* sceneParams;
  bool useSwapping;
  explicit ITMScene(const ITMSceneParams* params, int localBlockNum = 0, int bucketNum = 0, int excessNum = 0, bool useSwapping_ = false)
      : sceneParams(params), useSwapping(useSwapping_) {
    itm_scene_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.voxelType = TVoxel::kType; cfg.indexType = TIndex::kType;
    cfg.localBlockNum = localBlockNum; cfg.bucketNum = bucketNum; cfg.excessNum = excessNum;
    cfg.useSwapping = useSwapping ? 1 : 0;        // the scene then owns an ITMGlobalCache in host memory (Objects/ITMScene.h:37-43)
    check(itm_scene_create(&cfg, params, &handle), "itm_scene_create");
    // the engines below are driven in the reference's call order by hosts that read results through the engines: the library may
    // record AllocateSceneFromDepth / IntegrateIntoScene / CreateExpectedDepths and launch the fused frame at CreateICPMaps
    // (include/itm_hip.h, "the four calls of a frame")
    check(itm_scene_set_deferred_fusion(handle, 1), "itm_scene_set_deferred_fusion");
  }
  ~ITMScene() { itm_scene_destroy(handle); }
  ITMScene(const ITMScene&) = delete;
  ITMScene& operator=(const ITMScene&) = delete;
};

// ITMRenderState / ITMRenderState_VH (Objects/ITMRenderState.h, ITMRenderState_VH.h)
class ITMRenderState {
 public:
  itm_render_state* handle = nullptr;
  Vector2i imgSize;
  ITMRenderState(itm_render_state* h, Vector2i s) : handle(h), imgSize(s) {}
  ~ITMRenderState() { itm_render_state_destroy(handle); }
  ITMRenderState(const ITMRenderState&) = delete;
  ITMRenderState& operator=(const ITMRenderState&) = delete;
};

inline itm_view make_view(const ITMView* view, const ITMTrackingState* ts) {
  itm_view v;
  std::memset(&v, 0, sizeof v);
  v.depth = view->depth; v.rgb = view->rgb;
  v.w = view->depthSize.x; v.h = view->depthSize.y; v.w_rgb = view->rgbSize.x; v.h_rgb = view->rgbSize.y;
  std::memcpy(v.M_d, ts->pose_d.GetM(), 64);
  std::memcpy(v.intr_d, view->calib.intrinsics_d.all, 16);
  std::memcpy(v.intr_rgb, view->calib.intrinsics_rgb.all, 16);
  std::memcpy(v.rgb_to_depth, view->calib.trafo_rgb_to_depth_calib, 64);
  std::memcpy(v.rgb_to_depth_inv, view->calib.trafo_rgb_to_depth_calib_inv, 64);
  return v;
}

// ITMSceneReconstructionEngine_HIP: same three methods as the reference interface
template <class TVoxel, class TIndex>
class ITMSceneReconstructionEngine_HIP {
 public:
  itm_stream stream = nullptr;
  void ResetScene(ITMScene<TVoxel, TIndex>* scene) { check(itm_reset_scene(scene->handle, stream), "ResetScene"); }
  void AllocateSceneFromDepth(ITMScene<TVoxel, TIndex>* scene, const ITMView* view, const ITMTrackingState* trackingState,
                              const ITMRenderState* renderState, bool onlyUpdateVisibleList = false) {
    itm_view v = make_view(view, trackingState);
    check(itm_allocate_scene_from_depth(scene->handle, &v, renderState->handle, onlyUpdateVisibleList ? 1 : 0, stream), "AllocateSceneFromDepth");
  }
  void IntegrateIntoScene(ITMScene<TVoxel, TIndex>* scene, const ITMView* view, const ITMTrackingState* trackingState,
                          const ITMRenderState* renderState) {
    itm_view v = make_view(view, trackingState);
    check(itm_integrate_into_scene(scene->handle, &v, renderState->handle, stream), "IntegrateIntoScene");
  }
  // Not in the reference interface: takes the frame `view`, fused under trackingState->pose_d, back out of the voxels that
  // renderState's visible list names (itm_deintegrate_from_scene; a dense scene: every voxel).  cfg == nullptr: a voxel whose weight
  // has reached maxW stays as it is exactly when the scene stops integrating there.  With `stats` the stream is synchronised.
  void DeintegrateFromScene(ITMScene<TVoxel, TIndex>* scene, const ITMView* view, const ITMTrackingState* trackingState,
                            const ITMRenderState* renderState, const itm_deintegrate_config* cfg = nullptr, itm_deintegrate_stats* stats = nullptr) {
    itm_view v = make_view(view, trackingState);
    check(itm_deintegrate_from_scene(scene->handle, &v, renderState->handle, cfg, stats, stream), "DeintegrateFromScene");
  }
};

// ITMVisualisationEngine_HIP: the IITMVisualisationEngine methods
template <class TVoxel, class TIndex>
class ITMVisualisationEngine_HIP {
  const ITMScene<TVoxel, TIndex>* scene;

 public:
  enum RenderImageType { RENDER_SHADED_GREYSCALE, RENDER_COLOUR_FROM_VOLUME, RENDER_COLOUR_FROM_NORMAL };
  itm_stream stream = nullptr;
  explicit ITMVisualisationEngine_HIP(const ITMScene<TVoxel, TIndex>* s) : scene(s) {}

  ITMRenderState* CreateRenderState(const Vector2i& imgSize) const {
    itm_render_state* h = nullptr;
    check(itm_render_state_create(scene->handle, imgSize.x, imgSize.y, &h), "CreateRenderState");
    return new ITMRenderState(h, imgSize);
  }
  void FindVisibleBlocks(const ITMPose* pose, const ITMIntrinsics* intrinsics, ITMRenderState* renderState) const {
    check(itm_find_visible_blocks(scene->handle, pose->GetM(), intrinsics->all, renderState->handle, stream), "FindVisibleBlocks");
  }
  void CreateExpectedDepths(const ITMPose* pose, const ITMIntrinsics* intrinsics, ITMRenderState* renderState) const {
    check(itm_create_expected_depths(scene->handle, pose->GetM(), intrinsics->all, renderState->handle, stream), "CreateExpectedDepths");
  }
  // outputImage: device uchar4[h*w]; nullptr renders into renderState->raycastImage
  void RenderImage(const ITMPose* pose, const ITMIntrinsics* intrinsics, const ITMRenderState* renderState, uint8_t* outputImage,
                   RenderImageType type = RENDER_SHADED_GREYSCALE) const {
    check(itm_render_image(scene->handle, pose->GetM(), intrinsics->all, renderState->handle, outputImage, (int)type, stream), "RenderImage");
  }
  void FindSurface(const ITMPose* pose, const ITMIntrinsics* intrinsics, const ITMRenderState* renderState) const {
    check(itm_find_surface(scene->handle, pose->GetM(), intrinsics->all, renderState->handle, stream), "FindSurface");
  }
  void CreatePointCloud(const ITMView* view, ITMTrackingState* trackingState, ITMRenderState* renderState, bool skipPoints) const {
    itm_view v = make_view(view, trackingState);
    check(itm_create_point_cloud(scene->handle, &v, renderState->handle, skipPoints ? 1 : 0, trackingState->pointCloud_locations,
                                 trackingState->pointCloud_colours, stream), "CreatePointCloud");
    trackingState->pose_pointCloud = trackingState->pose_d;
  }
  void CreateICPMaps(const ITMView* view, ITMTrackingState* trackingState, ITMRenderState* renderState) const {
    itm_view v = make_view(view, trackingState);
    check(itm_create_icp_maps(scene->handle, &v, renderState->handle, trackingState->pointCloud_locations,
                              trackingState->pointCloud_colours, stream), "CreateICPMaps");
    trackingState->pose_pointCloud = trackingState->pose_d;   // ITMVisualisationEngine_CPU.cpp:272
  }
  void ForwardRender(const ITMView* view, ITMTrackingState* trackingState, ITMRenderState* renderState) const {
    itm_view v = make_view(view, trackingState);
    check(itm_forward_render(scene->handle, &v, renderState->handle, stream), "ForwardRender");
  }
};

// The callers of the path, same call order and state machine as
// ITMDenseMapper::ProcessFrame / UpdateVisibleList (Engine/ITMDenseMapper.cpp:50-71) and
// ITMTrackingController::Prepare (Engine/ITMTrackingController.cpp:18-46, non-colour trackers).
// ITMSwappingEngine<TVoxel, TIndex> (Engine/ITMSwappingEngine.h:19-36)
template <class TVoxel, class TIndex>
class ITMSwappingEngine_HIP {
 public:
  itm_stream stream = nullptr;
  void IntegrateGlobalIntoLocal(ITMScene<TVoxel, TIndex>* scene, ITMRenderState* renderState) {
    check(itm_swap_integrate_global_into_local(scene->handle, renderState->handle, stream), "IntegrateGlobalIntoLocal");
  }
  void SaveToGlobalMemory(ITMScene<TVoxel, TIndex>* scene, ITMRenderState* renderState) {
    check(itm_swap_save_to_global_memory(scene->handle, renderState->handle, stream), "SaveToGlobalMemory");
  }
};

// The slot list of a scene operation: the visible list of `srcVisible`, a render state of src (nullptr: no list, every block of src).
template <class TVoxel, class TIndex>
inline void visible_slots(const ITMScene<TVoxel, TIndex>* src, const ITMRenderState* srcVisible, itm_stream stream, const char* what, const int32_t** slots, int* n) {
  if (!srcVisible) return;
  itm_counters c;
  check(itm_get_counters(src->handle, srcVisible->handle, &c, stream), (std::string(what) + " (visible list)").c_str());
  *slots = (const int32_t*)itm_buffer_ptr(src->handle, srcVisible->handle, ITM_BUF_VISIBLE_IDS);
  *n = c.noVisibleEntries;
  if (!*slots) throw std::runtime_error(std::string(what) + ": the render state has no visible list");
}

// Scene merge (itm_scene_merge; no reference class): fuses `src` into `dst` on the GPU -- the blocks src has are allocated in dst by the
// reference's two-phase allocation, then every voxel is combined as the swapping engine combines a stored block (src in that role).
// Same voxel type, index type and voxelSize; both scenes on one device.  srcVisible: a render state of src whose visible list selects
// the blocks (nullptr: every block of src).  dst's render states are not touched; new blocks become visible when a frame sees them.
template <class TVoxel, class TIndex>
class ITMSceneMergeEngine_HIP {
 public:
  itm_stream stream = nullptr;
  void MergeScene(ITMScene<TVoxel, TIndex>* dst, const ITMScene<TVoxel, TIndex>* src, const ITMRenderState* srcVisible = nullptr, itm_merge_stats* stats = nullptr) {
    const int32_t* slots = nullptr;
    int n = 0;
    visible_slots(src, srcVisible, stream, "MergeScene", &slots, &n);
    check(itm_scene_merge(dst->handle, src->handle, slots, n, stats, stream), "MergeScene");
  }
};

// Scene pruning (itm_scene_prune; no reference class): the blocks of `scene` that `cfg` selects (nullptr: the defaults -- blocks without
// an observed voxel and blocks whose observed voxels all read "free") go back to the pool, their entries leave the table and every
// render state of the scene loses them from its visible list.  Hash scenes without swapping.
template <class TVoxel, class TIndex>
class ITMScenePruneEngine_HIP {
 public:
  itm_stream stream = nullptr;
  void PruneScene(ITMScene<TVoxel, TIndex>* scene, const itm_prune_config* cfg = nullptr, itm_prune_stats* stats = nullptr) {
    itm_prune_config def;
    if (!cfg) { check(itm_prune_default_config(&def), "PruneScene (default config)"); cfg = &def; }
    check(itm_scene_prune(scene->handle, cfg, nullptr, stats, stream), "PruneScene");
  }
};

// Level of detail (itm_scene_coarsen; no reference class): resamples `src` into `dst`, a scene of TWICE the voxel size and the same mu on
// the same GPU -- the blocks of dst come from the reference's two-phase allocation with src's block positions halved, every coarse voxel
// is the weighted 3 x 3 x 3 tent over the fine voxels around it, and the blocks touched are overwritten.  srcVisible: a render state of
// src whose visible list selects the blocks that take part (nullptr: every block of src).  dst's render states are not touched.
template <class TVoxel, class TIndex>
class ITMSceneCoarsenEngine_HIP {
 public:
  itm_stream stream = nullptr;
  void CoarsenScene(ITMScene<TVoxel, TIndex>* dst, const ITMScene<TVoxel, TIndex>* src, const ITMRenderState* srcVisible = nullptr, itm_coarsen_stats* stats = nullptr) {
    const int32_t* slots = nullptr;
    int n = 0;
    visible_slots(src, srcVisible, stream, "CoarsenScene", &slots, &n);
    check(itm_scene_coarsen(dst->handle, src->handle, slots, n, stats, stream), "CoarsenScene");
  }
};

// Scene merge under a rigid transform (itm_rigid_quantise + itm_scene_resample; no reference class): `src` is resampled at dst's voxels
// through dstFromSrc (x_dst = dstFromSrc x_src, metres: a relocalisation's relative pose, the poses the exchange gathers) and fused into
// `dst` as MergeScene fuses.  Same voxel type, index type, voxelSize and mu; both scenes on one device.  srcVisible: a render state of src
// whose visible list selects the blocks that take part (nullptr: every block of src).  dst's render states are not touched.
template <class TVoxel, class TIndex>
class ITMSceneResampleEngine_HIP {
 public:
  itm_stream stream = nullptr;
  void ResampleScene(ITMScene<TVoxel, TIndex>* dst, const ITMScene<TVoxel, TIndex>* src, const Matrix4f& dstFromSrc, const ITMRenderState* srcVisible = nullptr,
                     itm_resample_stats* stats = nullptr) {
    itm_rigid_q q;
    check(itm_rigid_quantise(dstFromSrc.m, dst->sceneParams->voxelSize, &q), "ResampleScene (itm_rigid_quantise)");
    const int32_t* slots = nullptr;
    int n = 0;
    visible_slots(src, srcVisible, stream, "ResampleScene", &slots, &n);
    check(itm_scene_resample(dst->handle, src->handle, &q, slots, n, stats, stream), "ResampleScene");
  }
};

// Scene alignment (itm_scene_band_samples + itm_aligner_*; no reference class): the pose dstFromSrc that ResampleScene wants, refined
// from a coarse one (a relocalisation, the poses the exchange gathers) by registering sdf samples against `dst`.  The engine owns one
// aligner handle and the sample buffer it fills; one engine per host thread.
template <class TVoxel, class TIndex>
class ITMSceneAlignEngine_HIP {
  itm_aligner* aligner = nullptr;
  void* samples = nullptr;
  int32_t capacity = 0, count = 0;

 public:
  itm_stream stream = nullptr;
  ITMSceneAlignEngine_HIP() { check(itm_aligner_create(&aligner), "itm_aligner_create"); }
  ~ITMSceneAlignEngine_HIP() { itm_aligner_destroy(aligner); if (samples) itm_dev_free(samples); }
  ITMSceneAlignEngine_HIP(const ITMSceneAlignEngine_HIP&) = delete;
  ITMSceneAlignEngine_HIP& operator=(const ITMSceneAlignEngine_HIP&) = delete;

  static itm_align_config DefaultConfig(const ITMSceneParams* p) {
    itm_align_config cfg;
    check(itm_align_default_config(p->voxelSize, p->mu, &cfg), "itm_align_default_config");
    return cfg;
  }
  // The samples are the band voxels of `src` (srcVisible: a render state of src whose visible list selects the blocks; nullptr: all);
  // returns how many there are.
  int32_t SetSamplesFromScene(const ITMScene<TVoxel, TIndex>* src, const itm_align_config& cfg, const ITMRenderState* srcVisible = nullptr) {
    const int32_t* slots = nullptr;
    int n = 0;
    visible_slots(src, srcVisible, stream, "AlignScene", &slots, &n);
    for (int pass = 0; pass < 2; ++pass) {      // the second pass only when the buffer had to grow
      check(itm_scene_band_samples(src->handle, slots, n, &cfg, (float*)samples, capacity, &count, stream), "AlignScene (itm_scene_band_samples)");
      if (count <= capacity) break;
      if (samples) { itm_dev_free(samples); samples = nullptr; capacity = 0; }
      check(itm_dev_malloc(&samples, (size_t)count * 16), "AlignScene (samples)");
      capacity = count;
    }
    check(itm_aligner_set_samples(aligner, (const float*)samples, count, stream), "AlignScene (itm_aligner_set_samples)");
    return count;
  }
  // The caller's own samples: device float4 (x, y, z in metres in the source frame, the signed distance in metres to read there); kept, not copied
  void SetSamples(const float* samples_dev, int32_t n) { check(itm_aligner_set_samples(aligner, samples_dev, n, stream), "itm_aligner_set_samples"); }
  void Evaluate(const ITMScene<TVoxel, TIndex>* dst, const Matrix4f& dstFromSrc, const itm_align_config& cfg, itm_align_eval* out) {
    check(itm_aligner_evaluate(aligner, dst->handle, dstFromSrc.m, &cfg, out, stream), "itm_aligner_evaluate");
  }
  // dstFromSrc: the coarse pose on entry, the refined one on return.  res->status says what the result is worth (ITM_ALIGN_*).
  void Align(const ITMScene<TVoxel, TIndex>* dst, Matrix4f& dstFromSrc, const itm_align_config& cfg, itm_align_result* res = nullptr) {
    float out[16];
    check(itm_aligner_align(aligner, dst->handle, dstFromSrc.m, &cfg, out, res, stream), "itm_aligner_align");
    dstFromSrc = Matrix4f(out);
  }
  void AlignScene(const ITMScene<TVoxel, TIndex>* dst, const ITMScene<TVoxel, TIndex>* src, Matrix4f& dstFromSrc, itm_align_result* res = nullptr,
                  const itm_align_config* cfg = nullptr) {
    const itm_align_config c = cfg ? *cfg : DefaultConfig(dst->sceneParams);
    SetSamplesFromScene(src, c);
    Align(dst, dstFromSrc, c, res);
  }
};

// Scene queries (itm_scene_query_points / itm_scene_cast_rays; the reference makes these reads only per pixel, inside its engines):
// readFromSDF_float_interpolated, computeSingleNormalFromSDF, readFromSDF_color4u_interpolated at caller-supplied points, castRay along
// caller-supplied segments.  All pointers are DEVICE memory; one launch on `stream`, nothing is synchronised.
template <class TVoxel, class TIndex>
class ITMSceneQueryEngine_HIP {
 public:
  itm_stream stream = nullptr;
  // points: float[3 n] in metres (units = ITM_QUERY_METRES) or voxels; out: the wanted outputs, NULL = not wanted
  void QueryPoints(const ITMScene<TVoxel, TIndex>* scene, const float* points, uint32_t n, const itm_query_out& out, int units = ITM_QUERY_METRES) const {
    check(itm_scene_query_points(scene->handle, points, n, units, &out, stream), "QueryPoints");
  }
  // rays: float[8 n] = (s, t0, e, t1) in metres; hits: float[4 n] = (x, y, z, w) in voxel units, w = 1 a hit
  void CastRays(const ITMScene<TVoxel, TIndex>* scene, const float* rays, uint32_t n, float* hits) const {
    check(itm_scene_cast_rays(scene->handle, rays, n, hits, stream), "CastRays");
  }
};

// Distance field (itm_scene_esdf; no counterpart in the reference): the Euclidean distance transform of a box of the volume -- for
// every cell the squared distance in voxels to the nearest site (surface crossing and / or unobserved voxel), which site that is, the
// signed metric distance and the classification byte.  Device pointers; launches on `stream`, nothing is synchronised.
template <class TVoxel, class TIndex>
class ITMDistanceFieldEngine_HIP {
 public:
  itm_stream stream = nullptr;
  // box: first voxel and size in voxels; out: dist2 is required, the others NULL = not wanted; maxDistance in voxels, 0 = unbounded
  void Compute(const ITMScene<TVoxel, TIndex>* scene, const itm_esdf_box& box, const itm_esdf_out& out, int sites = ITM_ESDF_SITE_SURFACE, int minWeight = 1,
               int maxDistance = 0) const {
    check(itm_scene_esdf(scene->handle, &box, sites, minWeight, maxDistance, &out, stream), "DistanceField");
  }
};

template <class TVoxel, class TIndex>
class ITMDenseMapper_HIP {
  ITMSceneReconstructionEngine_HIP<TVoxel, TIndex> reco;
  ITMSwappingEngine_HIP<TVoxel, TIndex> swappingEngine;

 public:
  void SetStream(itm_stream s) { reco.stream = s; swappingEngine.stream = s; }
  void ResetScene(ITMScene<TVoxel, TIndex>* scene) { reco.ResetScene(scene); }
  void ProcessFrame(const ITMView* view, const ITMTrackingState* ts, ITMScene<TVoxel, TIndex>* scene, ITMRenderState* rs) {
    reco.AllocateSceneFromDepth(scene, view, ts, rs);
    reco.IntegrateIntoScene(scene, view, ts, rs);
    if (scene->useSwapping) {                     // ITMDenseMapper.cpp:59-64 (settings->useSwapping)
      swappingEngine.IntegrateGlobalIntoLocal(scene, rs);     // swapping: host -> device
      swappingEngine.SaveToGlobalMemory(scene, rs);           // swapping: device -> host
    }
  }
  void UpdateVisibleList(const ITMView* view, const ITMTrackingState* ts, ITMScene<TVoxel, TIndex>* scene, ITMRenderState* rs) {
    reco.AllocateSceneFromDepth(scene, view, ts, rs, true);
  }
};

// ITMViewBuilder (Engine/ITMViewBuilder.h:17-60): raw depth frame (device short image) -> ITMView::depth in metres,
// optional 5-pass bilateral filter and normal / uncertainty images.  The caller owns the device images.
class ITMViewBuilder_HIP {
  const ITMRGBDCalib* calib;
  int calibType; float c0, c1;

 public:
  itm_stream stream = nullptr;
  // calibType: 0 = ITMDisparityCalib::TRAFO_KINECT (params c0, c1), 1 = TRAFO_AFFINE (depth = raw * c0 + c1)
  ITMViewBuilder_HIP(const ITMRGBDCalib* calib_, int calibType_, float c0_, float c1_) : calib(calib_), calibType(calibType_), c0(c0_), c1(c1_) {}
  void ConvertDisparityToDepth(float* depth_out, const int16_t* disp_in, Vector2i size) {
    check(itm_convert_disparity(disp_in, depth_out, size.x, size.y, c0, c1, calib->intrinsics_d.all[0], stream), "ConvertDisparityToDepth");
  }
  void ConvertDepthAffineToFloat(float* depth_out, const int16_t* depth_in, Vector2i size) {
    check(itm_convert_depth_affine(depth_in, depth_out, size.x, size.y, c0, c1, stream), "ConvertDepthAffineToFloat");
  }
  void DepthFiltering(float* image_out, const float* image_in, Vector2i size) {
    check(itm_filter_depth(image_in, image_out, size.x, size.y, stream), "DepthFiltering");
  }
  void ComputeNormalAndWeights(float* normal_out, float* sigmaZ_out, const float* depth_in, Vector2i size) {
    check(itm_compute_normal_and_weights(depth_in, normal_out, sigmaZ_out, size.x, size.y, calib->intrinsics_d.all, stream), "ComputeNormalAndWeights");
  }
  // UpdateView(view, rgb, rawDepth, useBilateralFilter, modelSensorNoise): fills view->depth (and the optional images)
  void UpdateView(ITMView* view, const int16_t* rawDepth, float* depth, float* scratch, bool useBilateralFilter,
                  bool modelSensorNoise = false, float* depthNormal = nullptr, float* depthUncertainty = nullptr) {
    check(itm_update_view(rawDepth, view->depthSize.x, view->depthSize.y, calibType, c0, c1, calib->intrinsics_d.all, useBilateralFilter ? 1 : 0,
                          modelSensorNoise ? 1 : 0, depth, scratch, depthNormal, depthUncertainty, stream), "UpdateView");
    view->depth = depth;
  }
  // The reference's UpdateView takes HOST images and opens with a synchronous copy (shortImage->SetFrom(rawDepthImage, CPU_TO_CUDA),
  // DeviceSpecific/CUDA/ITMViewBuilder_CUDA.cu:53).  Here a raw frame in pinned host memory travels on the stager's copy stream;
  // Prefetch(next frame) while the current one is fused hides the transfer altogether.
  void Prefetch(const int16_t* rawDepthHost, Vector2i size) {
    if (!stager) check(itm_depth_stager_create(size.x, size.y, 4, &stager), "depth stager");
    check(itm_depth_stager_upload(stager, rawDepthHost), "Prefetch");
    prefetched = rawDepthHost;
  }
  void UpdateViewFromHost(ITMView* view, const int16_t* rawDepthHost, float* depth, float* scratch, bool useBilateralFilter,
                          bool modelSensorNoise = false, float* depthNormal = nullptr, float* depthUncertainty = nullptr) {
    // the slot of the PREVIOUS frame: everything that read its depth has been submitted to the stream by now
    if (holding) { check(itm_depth_stager_release(stager, stream), "UpdateView (release)"); holding = false; }
    // without filter and noise model the float depth is the conversion alone: the stager's copy does it (itm_depth_stager_set_conversion)
    // and the view's depth is the slot's image -- no conversion launch on the frame's stream
    const bool plain = !useBilateralFilter && !modelSensorNoise;
    auto discard_waiting = [&]() {
      int waiting = 0;
      check(itm_depth_stager_pending(stager, &waiting, nullptr), "UpdateView (pending)");
      for (; waiting > 0; --waiting) {
        const int16_t* stale = nullptr;
        check(itm_depth_stager_acquire(stager, stream, &stale), "UpdateView (discard)");
        check(itm_depth_stager_release(stager, stream), "UpdateView (discard)");
      }
      prefetched = nullptr;
    };
    if (!stager) check(itm_depth_stager_create(view->depthSize.x, view->depthSize.y, 4, &stager), "depth stager");
    // frames uploaded ahead that are not the one asked for (the image source changed its mind), or uploaded in the other form: taken off
    // the ring unread, else the stager -- strictly first in, first out -- would hand the stale frame to this call and stay one frame behind
    if (prefetched != rawDepthHost || plain != converting) discard_waiting();
    if (plain != converting) {
      if (plain) check(itm_depth_stager_set_conversion(stager, calibType, c0, c1, calib->intrinsics_d.all[0]), "depth stager (conversion)");
      converting = plain;
    }
    if (prefetched != rawDepthHost) Prefetch(rawDepthHost, view->depthSize);
    prefetched = nullptr;
    if (plain) {
      const float* converted = nullptr;
      check(itm_depth_stager_acquire_depth(stager, stream, nullptr, &converted), "UpdateView (acquire)");
      view->depth = converted;
      holding = true;           // released by the next call: the frame's launches read it
      return;
    }
    const int16_t* raw = nullptr;
    check(itm_depth_stager_acquire(stager, stream, &raw), "UpdateView (acquire)");
    UpdateView(view, raw, depth, scratch, useBilateralFilter, modelSensorNoise, depthNormal, depthUncertainty);
    check(itm_depth_stager_release(stager, stream), "UpdateView (release)");
  }
  // true once the copy stream has READ every host frame handed to Prefetch / UpdateViewFromHost so far: from then on the image source
  // may rewrite those buffers (the uploads are asynchronous; a source that reuses ONE raw buffer asks -- or waits -- before it refills it)
  bool HostFramesRead() const {
    int busy = 0;
    if (stager) check(itm_depth_stager_pending(stager, nullptr, &busy), "HostFramesRead");
    return busy == 0;
  }
  void WaitHostFramesRead() const { while (!HostFramesRead()) {} }
  ~ITMViewBuilder_HIP() { if (stager) itm_depth_stager_destroy(stager); }
  ITMViewBuilder_HIP(const ITMViewBuilder_HIP&) = delete;
  ITMViewBuilder_HIP& operator=(const ITMViewBuilder_HIP&) = delete;

 private:
  itm_depth_stager* stager = nullptr;
  const int16_t* prefetched = nullptr;
  bool converting = false, holding = false;
};

// ITMDepthTracker (Engine/ITMDepthTracker.h): TrackCamera refines trackingState->pose_d against the ICP maps
// of the previous frame; the gradient / Hessian reduction and the depth pyramid run on the GPU.
class ITMDepthTracker_HIP {
  itm_tracker_config cfg;
  itm_tracker* tracker = nullptr;     // this object's hierarchy + reduction buffers (ITMDepthTracker.cpp:18-44); one per tracker object

 public:
  itm_stream stream = nullptr;
  ITMDepthTracker_HIP(const int* trackingRegime, int noHierarchyLevels, int noICPRunTillLevel, float distThresh, float terminationThreshold) {
    std::memset(&cfg, 0, sizeof cfg);
    cfg.noHierarchyLevels = noHierarchyLevels;
    for (int i = 0; i < noHierarchyLevels && i < 8; ++i) cfg.trackingRegime[i] = trackingRegime[i];
    cfg.noICPRunTillLevel = noICPRunTillLevel; cfg.distThresh = distThresh; cfg.terminationThreshold = terminationThreshold;
    check(itm_tracker_create(&tracker), "itm_tracker_create");
  }
  ~ITMDepthTracker_HIP() { itm_tracker_destroy(tracker); }
  ITMDepthTracker_HIP(const ITMDepthTracker_HIP&) = delete;
  ITMDepthTracker_HIP& operator=(const ITMDepthTracker_HIP&) = delete;
  void TrackCamera(ITMTrackingState* trackingState, const ITMView* view) {
    itm_view v = make_view(view, trackingState);
    float M[16];
    check(itm_tracker_track_camera(tracker, &cfg, &v, trackingState->pointCloud_locations, trackingState->pointCloud_colours,
                                   trackingState->pose_pointCloud.GetM(), M, stream), "TrackCamera");
    trackingState->pose_d.SetM(M);
  }
};

// ITMTracker (Engine/ITMTracker.h): what ITMTrackingController::Track calls
class ITMTracker {
 public:
  virtual void TrackCamera(ITMTrackingState* trackingState, const ITMView* view) = 0;
  virtual ~ITMTracker() {}
};
// ITMExternalTracker of this fork (Engine/ITMExternalTracker.cpp:27-30): the pose was put into trackingState->pose_d from outside
class ITMExternalTracker : public ITMTracker {
 public:
  void TrackCamera(ITMTrackingState*, const ITMView*) override {}
};
// adapter: ITMDepthTracker_HIP behind the ITMTracker interface
class ITMDepthTrackerAdapter : public ITMTracker {
  ITMDepthTracker_HIP* t;
 public:
  explicit ITMDepthTrackerAdapter(ITMDepthTracker_HIP* t_) : t(t_) {}
  void TrackCamera(ITMTrackingState* ts, const ITMView* view) override { t->TrackCamera(ts, view); }
};

// ITMWeightedICPTracker (Engine/ITMWeightedICPTracker.h, .cpp): ICP with a per-pixel weight from the view's uncertainty image
// (view->depthUncertainty); depth and weight pyramids, weighted evaluation and reduction on the GPU (itm_tracker_weighted_*).
class ITMWeightedICPTracker_HIP {
  itm_tracker_config cfg;
  itm_tracker* tracker = nullptr;     // this object's hierarchies + reduction buffers; one per tracker object

 public:
  itm_stream stream = nullptr;
  ITMWeightedICPTracker_HIP(const int* trackingRegime, int noHierarchyLevels, int noICPRunTillLevel, float distThresh, float terminationThreshold) {
    std::memset(&cfg, 0, sizeof cfg);
    cfg.noHierarchyLevels = noHierarchyLevels;
    for (int i = 0; i < noHierarchyLevels && i < 8; ++i) cfg.trackingRegime[i] = trackingRegime[i];
    cfg.noICPRunTillLevel = noICPRunTillLevel; cfg.distThresh = distThresh; cfg.terminationThreshold = terminationThreshold;
    check(itm_tracker_create(&tracker), "itm_tracker_create");
  }
  ~ITMWeightedICPTracker_HIP() { itm_tracker_destroy(tracker); }
  ITMWeightedICPTracker_HIP(const ITMWeightedICPTracker_HIP&) = delete;
  ITMWeightedICPTracker_HIP& operator=(const ITMWeightedICPTracker_HIP&) = delete;
  void TrackCamera(ITMTrackingState* trackingState, const ITMView* view) {
    if (!view->depthUncertainty) throw std::runtime_error("TrackCamera: the weighted ICP tracker needs the view's uncertainty image");
    itm_view v = make_view(view, trackingState);
    float M[16];
    check(itm_tracker_weighted_track_camera(tracker, &cfg, &v, view->depthUncertainty, trackingState->pointCloud_locations,
                                            trackingState->pointCloud_colours, trackingState->pose_pointCloud.GetM(), M, stream), "TrackCamera");
    trackingState->pose_d.SetM(M);
  }
};
// adapter: ITMWeightedICPTracker_HIP behind the ITMTracker interface
class ITMWeightedICPTrackerAdapter : public ITMTracker {
  ITMWeightedICPTracker_HIP* t;
 public:
  explicit ITMWeightedICPTrackerAdapter(ITMWeightedICPTracker_HIP* t_) : t(t_) {}
  void TrackCamera(ITMTrackingState* ts, const ITMView* view) override { t->TrackCamera(ts, view); }
};

// ITMColorTracker (Engine/ITMColorTracker.h, .cpp:25-47): TrackCamera aligns the view's rgb image with the coloured point cloud that
// Prepare's CreatePointCloud left in the tracking state; pyramid, evaluation and reduction on the GPU (itm_colour_tracker_*).  The
// point count is read on the device from the render state CreatePointCloud wrote into.
class ITMColorTracker_HIP {
  itm_tracker_config cfg;
  itm_colour_tracker* tracker = nullptr;   // this object's rgb hierarchy + reduction buffers; one per tracker object

 public:
  itm_stream stream = nullptr;
  ITMColorTracker_HIP(const int* trackingRegime, int noHierarchyLevels) {
    std::memset(&cfg, 0, sizeof cfg);
    cfg.noHierarchyLevels = noHierarchyLevels;
    for (int i = 0; i < noHierarchyLevels && i < 8; ++i) cfg.trackingRegime[i] = trackingRegime[i];
    check(itm_colour_tracker_create(&tracker), "itm_colour_tracker_create");
  }
  ~ITMColorTracker_HIP() { itm_colour_tracker_destroy(tracker); }
  ITMColorTracker_HIP(const ITMColorTracker_HIP&) = delete;
  ITMColorTracker_HIP& operator=(const ITMColorTracker_HIP&) = delete;
  void TrackCamera(ITMTrackingState* trackingState, const ITMView* view, const ITMRenderState* renderState) {
    itm_view v = make_view(view, trackingState);
    float M[16];
    check(itm_colour_tracker_track_camera(tracker, &cfg, &v, renderState->handle, trackingState->pointCloud_locations,
                                          trackingState->pointCloud_colours, 0, M, stream), "TrackCamera");
    trackingState->pose_d.SetM(M);
  }
};
// adapter: ITMColorTracker_HIP behind the ITMTracker interface, with the render state that holds the point count
class ITMColorTrackerAdapter : public ITMTracker {
  ITMColorTracker_HIP* t;
  const ITMRenderState* renderState;
 public:
  ITMColorTrackerAdapter(ITMColorTracker_HIP* t_, const ITMRenderState* rs) : t(t_), renderState(rs) {}
  void TrackCamera(ITMTrackingState* ts, const ITMView* view) override { t->TrackCamera(ts, view, renderState); }
};

// ITMRenTracker (Engine/ITMRenTracker.h, .cpp; ITMTrackerFactory::MakeRenTracker): TrackCamera registers the view's depth image
// directly against the scene's TSDF, level 0 only; unprojection, evaluation and reduction on the GPU (itm_ren_tracker_*).  Reads the
// scene as the last frame left it (engine calls the library recorded are launched first).
template <class TVoxel, class TIndex>
class ITMRenTracker_HIP {
  const ITMScene<TVoxel, TIndex>* scene;
  itm_ren_tracker* tracker = nullptr;      // this object's point image + reduction buffers; one per tracker object

 public:
  itm_stream stream = nullptr;
  explicit ITMRenTracker_HIP(const ITMScene<TVoxel, TIndex>* scene_) : scene(scene_) {
    check(itm_ren_tracker_create(&tracker), "itm_ren_tracker_create");
  }
  ~ITMRenTracker_HIP() { itm_ren_tracker_destroy(tracker); }
  ITMRenTracker_HIP(const ITMRenTracker_HIP&) = delete;
  ITMRenTracker_HIP& operator=(const ITMRenTracker_HIP&) = delete;
  void TrackCamera(ITMTrackingState* trackingState, const ITMView* view) {
    itm_view v = make_view(view, trackingState);
    float M[16];
    check(itm_ren_tracker_track_camera(tracker, scene->handle, &v, M, nullptr, stream), "TrackCamera");
    trackingState->pose_d.SetM(M);
  }
};
// adapter: ITMRenTracker_HIP behind the ITMTracker interface
template <class TVoxel, class TIndex>
class ITMRenTrackerAdapter : public ITMTracker {
  ITMRenTracker_HIP<TVoxel, TIndex>* t;
 public:
  explicit ITMRenTrackerAdapter(ITMRenTracker_HIP<TVoxel, TIndex>* t_) : t(t_) {}
  void TrackCamera(ITMTrackingState* ts, const ITMView* view) override { t->TrackCamera(ts, view); }
};

// 4x4 product as ORUtils/Matrix.h:96-104 forms it (column-major, r(x, y) accumulated from zero over k)
inline void matmul4(const float* lhs, const float* rhs, float* out) {
  for (int x = 0; x < 4; ++x) for (int y = 0; y < 4; ++y) {
    float r = 0.0f;
    for (int k = 0; k < 4; ++k) r += lhs[k * 4 + y] * rhs[x * 4 + k];
    out[x * 4 + y] = r;
  }
}

// Keyframe relocaliser (itm_reloc_*, include/itm_hip.h): fern codes of the depth frames, a database of keyframe codes with their
// poses, the nearest-code search.  range: the depths in metres the default ferns' thresholds are drawn from.
class ITMRelocaliser_HIP {
  itm_reloc* handle = nullptr;
  float harvestingThreshold;

 public:
  itm_stream stream = nullptr;
  ITMRelocaliser_HIP(Vector2i imgSize, Vector2f range, float harvestingThreshold_ = 0.2f, int numFerns = 500, int numDecisions = 4, int capacity = 65536,
                     uint64_t seed = 1)
      : harvestingThreshold(harvestingThreshold_) {
    itm_reloc_config cfg;
    check(itm_reloc_default_config(imgSize.x, imgSize.y, &cfg), "itm_reloc_default_config");
    cfg.numFerns = numFerns; cfg.numDecisions = numDecisions; cfg.capacity = capacity;
    const size_t n = (size_t)(numFerns > 0 ? numFerns : 0) * (size_t)(numDecisions > 0 ? numDecisions : 0);
    std::vector<int32_t> pixel(n ? n : 1);
    std::vector<float> threshold(n ? n : 1);
    check(itm_reloc_default_ferns(&cfg, seed, range.x, range.y, pixel.data(), threshold.data()), "itm_reloc_default_ferns");
    check(itm_reloc_create(&cfg, pixel.data(), threshold.data(), &handle), "itm_reloc_create");
  }
  ~ITMRelocaliser_HIP() { itm_reloc_destroy(handle); }
  ITMRelocaliser_HIP(const ITMRelocaliser_HIP&) = delete;
  ITMRelocaliser_HIP& operator=(const ITMRelocaliser_HIP&) = delete;

  // depth: device float image of imgSize.  The k nearest keyframes of the database as it was before the call into nearest[] /
  // distances[] (-1 / 1.0 where there are fewer); with harvest, the frame becomes a keyframe with `pose` when its nearest one is
  // further than the harvesting threshold.  Returns the id added, or -1 (also when the database is full).
  int ProcessFrame(const float* depth, const ITMPose* pose, int k, int nearest[], float distances[], bool harvest) {
    int32_t ids[ITM_RELOC_MAX_K], added = -1;
    float dist[ITM_RELOC_MAX_K];
    check(itm_reloc_process_frame(handle, depth, pose ? pose->GetM() : nullptr, harvest && pose ? 1 : 0, harvestingThreshold, k, ids, dist, &added, stream),
          "ITMRelocaliser_HIP::ProcessFrame");
    for (int j = 0; j < k; ++j) { nearest[j] = ids[j]; distances[j] = dist[j]; }
    return added >= 0 ? added : -1;
  }
  ITMPose RetrievePose(int id) const {
    ITMPose p;
    float M[16];
    check(itm_reloc_get_pose(handle, id, M), "ITMRelocaliser_HIP::RetrievePose");
    p.SetM(M);
    return p;
  }
  int NumKeyframes() const {
    int32_t n = 0;
    check(itm_reloc_info(handle, &n, nullptr), "itm_reloc_info");
    return n;
  }
  void SaveToDirectory(const char* dir) { check(itm_reloc_save(handle, dir), "ITMRelocaliser_HIP::SaveToDirectory"); }
  void LoadFromDirectory(const char* dir) { check(itm_reloc_load(handle, dir), "ITMRelocaliser_HIP::LoadFromDirectory"); }
  itm_reloc* Handle() { return handle; }
};

// Pose quality (itm_pose_quality_*, include/itm_hip.h): a view's depth image under the tracking state's pose, judged against the
// fused volume.  One launch per Evaluate; the counts are on the host when it returns.
class ITMPoseQuality_HIP {
  itm_pose_quality_handle* handle = nullptr;

 public:
  enum TrackingResult { TRACKING_FAILED = ITM_TRACKING_FAILED, TRACKING_POOR = ITM_TRACKING_POOR, TRACKING_GOOD = ITM_TRACKING_GOOD };
  itm_pose_quality_config config;
  itm_stream stream = nullptr;
  // config_.inlierDistance == 0: the defaults for `mu`
  ITMPoseQuality_HIP(float mu, const itm_pose_quality_config& config_) : config(config_) {
    if (config.inlierDistance == 0.0f) check(itm_pose_quality_default_config(mu, &config), "itm_pose_quality_default_config");
    check(itm_pose_quality_create(&handle), "itm_pose_quality_create");
  }
  explicit ITMPoseQuality_HIP(float mu) : ITMPoseQuality_HIP(mu, itm_pose_quality_config{0.0f, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}) {}
  ~ITMPoseQuality_HIP() { itm_pose_quality_destroy(handle); }
  ITMPoseQuality_HIP(const ITMPoseQuality_HIP&) = delete;
  ITMPoseQuality_HIP& operator=(const ITMPoseQuality_HIP&) = delete;

  // residuals: device float[h * w] or nullptr (ITM_POSE_QUALITY_UNKNOWN / _NONE mark the pixels without a residual)
  template <class TVoxel, class TIndex>
  itm_pose_quality Evaluate(const ITMScene<TVoxel, TIndex>* scene, const ITMView* view, const ITMTrackingState* trackingState, float* residuals = nullptr) {
    itm_view v = make_view(view, trackingState);
    itm_pose_quality out;
    check(itm_pose_quality_evaluate(handle, scene->handle, &v, &config, &out, residuals, stream), "ITMPoseQuality_HIP::Evaluate");
    return out;
  }
  TrackingResult Verdict(const itm_pose_quality& stats) const {
    int32_t r = ITM_TRACKING_FAILED;
    check(itm_pose_quality_verdict(&stats, &config, &r), "ITMPoseQuality_HIP::Verdict");
    return (TrackingResult)r;
  }
};

// ITMTrackingController (Engine/ITMTrackingController.cpp:11-46): Track and Prepare, statement for statement
template <class TVoxel, class TIndex>
class ITMTrackingController_HIP {
  ITMTracker* tracker;
  const ITMVisualisationEngine_HIP<TVoxel, TIndex>* visualisationEngine;
  const ITMLibSettings* settings;
  ITMLibSettings ownSettings;

 public:
  ITMTrackingController_HIP(ITMTracker* tracker_, const ITMVisualisationEngine_HIP<TVoxel, TIndex>* vis, const ITMLibSettings* settings_)
      : tracker(tracker_), visualisationEngine(vis), settings(settings_) {}
  // external poses (no tracker object), `approximate` = ITMLibSettings::useApproximateRaycast
  explicit ITMTrackingController_HIP(const ITMVisualisationEngine_HIP<TVoxel, TIndex>* vis, bool approximate = false)
      : tracker(nullptr), visualisationEngine(vis), settings(&ownSettings) { ownSettings.useApproximateRaycast = approximate; }

  void Track(ITMTrackingState* trackingState, const ITMView* view) {
    if (trackingState->age_pointCloud != -1 && tracker) tracker->TrackCamera(trackingState, view);
    trackingState->requiresFullRendering = trackingState->TrackerFarFromPointCloud() || !settings->useApproximateRaycast;
  }
  void Prepare(ITMTrackingState* trackingState, const ITMView* view, ITMRenderState* renderState) {
    if (settings->trackerType == ITMLibSettings::TRACKER_COLOR) {
      ITMPose pose_rgb;
      float M[16];
      matmul4(view->calib.trafo_rgb_to_depth_calib_inv, trackingState->pose_d.GetM(), M);
      pose_rgb.SetM(M);
      visualisationEngine->CreateExpectedDepths(&pose_rgb, &view->calib.intrinsics_rgb, renderState);
      visualisationEngine->CreatePointCloud(view, trackingState, renderState, settings->skipPoints);
      trackingState->age_pointCloud = 0;
    } else {
      visualisationEngine->CreateExpectedDepths(&trackingState->pose_d, &view->calib.intrinsics_d, renderState);
      if (trackingState->requiresFullRendering) {
        visualisationEngine->CreateICPMaps(view, trackingState, renderState);
        trackingState->pose_pointCloud = trackingState->pose_d;
        if (trackingState->age_pointCloud == -1) trackingState->age_pointCloud = -2;
        else trackingState->age_pointCloud = 0;
      } else {
        visualisationEngine->ForwardRender(view, trackingState, renderState);
        trackingState->age_pointCloud++;
      }
    }
  }
};

// ITMMainEngine (Engine/ITMMainEngine.cpp:7-127,194-197) for raw frames already in device memory: builds the view, tracks, fuses
// unless integration is switched off, and prepares the maps for the next frame -- with the reference's switches.  Owns the scene,
// the engines, the live render state, the tracking state and the view's depth images.
template <class TVoxel, class TIndex>
class ITMMainEngine_HIP {
  ITMLibSettings settings;
  ITMSceneParams sceneParams;
  ITMScene<TVoxel, TIndex> scene;
  ITMDenseMapper_HIP<TVoxel, TIndex> denseMapper;
  ITMVisualisationEngine_HIP<TVoxel, TIndex> visualisationEngine;
  ITMDepthTracker_HIP* depthTracker = nullptr;
  ITMColorTracker_HIP* colourTracker = nullptr;
  ITMRenTracker_HIP<TVoxel, TIndex>* renTracker = nullptr;
  ITMWeightedICPTracker_HIP* wicpTracker = nullptr;
  ITMTracker* tracker = nullptr;
  ITMTrackingController_HIP<TVoxel, TIndex>* trackingController = nullptr;
  ITMViewBuilder_HIP* viewBuilder = nullptr;
  ITMRenderState* renderState_live = nullptr;
  ITMTrackingState trackingState;
  ITMView view;
  void *depthBuf = nullptr, *scratchBuf = nullptr, *normalBuf = nullptr, *sigmaBuf = nullptr, *pointsBuf = nullptr, *coloursBuf = nullptr;
  bool fusionActive = true, mainProcessingActive = true;
  itm_mesh* exportMesh = nullptr;      // created by the first SaveSceneTo* call
  // SaveSceneToCoarsePLY: the scene at twice the voxel size and its mesh, created by the first call
  int localBlockNum_;
  ITMSceneParams coarseParams;
  ITMScene<TVoxel, TIndex>* coarseScene = nullptr;
  itm_mesh* coarseMesh = nullptr;
  ITMRenderState* renderState_freeview = nullptr;      // created by the first free-camera GetImage
  ITMRenderState* renderState_poseUpdate = nullptr;    // created by the first RemoveFrame / ReintegrateFrame: the visible list of the frame being moved
  void* depthImageBuf = nullptr;                       // device uchar4 of the depth size: the coloured depth / uncertainty image of GetImage
  ITMRelocaliser_HIP* relocaliser = nullptr;           // settings.useRelocalisation
  bool harvestingActive = true;
  // settings.useTrackingVerdict (all unused without it)
  ITMPoseQuality_HIP* poseQuality = nullptr;
  ITMPoseQuality_HIP::TrackingResult trackingResult = ITMPoseQuality_HIP::TRACKING_GOOD;
  itm_pose_quality lastQuality = {0, 0, 0, 0, 0.0, 0.0};
  ITMPose endPose;                 // pose_d as the previous frame left it
  bool haveEndPose = false, anyFrameFused = false, lastFrameFused = false;
  int fusionDelay = 0, relocalisationCount = 0;
  int fusedSincePrune = 0;         // settings.pruneEveryNFrames
  itm_prune_stats lastPrune = {};
  itm_mesh* liveMesh = nullptr;    // settings.liveMeshEveryNFrames
  int fusedSinceMeshUpdate = 0;
  itm_mesh_update_stats lastMeshUpdate = {};

 public:
  // calibType / c0 / c1: ITMDisparityCalib (0 = TRAFO_KINECT, 1 = TRAFO_AFFINE); sizes as ITMMainEngine's imgSize_rgb / imgSize_d
  ITMMainEngine_HIP(const ITMLibSettings& settings_, const ITMSceneParams& params, const ITMRGBDCalib& calib, Vector2i imgSize_rgb, Vector2i imgSize_d,
                    int calibType = 1, float c0 = 0.001f, float c1 = 0.0f, int localBlockNum = 0)
      : settings((check_settings(settings_), settings_)), sceneParams(params), scene(&sceneParams, localBlockNum), visualisationEngine(&scene),
        localBlockNum_(localBlockNum), coarseParams(params.mu, params.maxW, 2.0f * params.voxelSize, params.viewFrustum_min, params.viewFrustum_max, params.stopIntegratingAtMaxW != 0) {
    view.calib = calib;
    view.depthSize = imgSize_d; view.rgbSize = imgSize_rgb;
    const size_t P = (size_t)imgSize_d.x * imgSize_d.y;
    // the tracked image: rgb for the colour tracker, depth otherwise (ITMTrackingController::GetTrackedImageSize)
    const Vector2i tracked = settings.trackerType == ITMLibSettings::TRACKER_COLOR ? imgSize_rgb : imgSize_d;
    const size_t PT = (size_t)tracked.x * tracked.y;
    check(itm_dev_malloc(&depthBuf, P * 4), "malloc"); check(itm_dev_malloc(&scratchBuf, P * 4), "malloc");
    check(itm_dev_malloc(&normalBuf, P * 16), "malloc"); check(itm_dev_malloc(&sigmaBuf, P * 4), "malloc");
    check(itm_dev_malloc(&pointsBuf, PT * 16), "malloc"); check(itm_dev_malloc(&coloursBuf, PT * 16), "malloc");
    trackingState.pointCloud_locations = (float*)pointsBuf; trackingState.pointCloud_colours = (float*)coloursBuf;
    {   // ComputeNormalAndWeights writes the interior only: the 2-pixel border keeps the 0 of the reference's cleared image (weight 0)
      std::vector<float> zeros(P, 0.0f);
      check(itm_memcpy_h2d(sigmaBuf, zeros.data(), P * 4, nullptr), "clear sigmaZ");
      check(itm_stream_synchronize(nullptr), "clear sigmaZ");
    }
    denseMapper.ResetScene(&scene);
    viewBuilder = new ITMViewBuilder_HIP(&view.calib, calibType, c0, c1);
    renderState_live = visualisationEngine.CreateRenderState(tracked);
    if (settings.trackerType == ITMLibSettings::TRACKER_ICP) {
      depthTracker = new ITMDepthTracker_HIP(settings.trackingRegime, settings.noHierarchyLevels, settings.noICPRunTillLevel,
                                             settings.depthTrackerICPThreshold, settings.depthTrackerTerminationThreshold);
      tracker = new ITMDepthTrackerAdapter(depthTracker);
    } else if (settings.trackerType == ITMLibSettings::TRACKER_COLOR && settings.useColourTracker) {
      colourTracker = new ITMColorTracker_HIP(settings.trackingRegime, settings.noHierarchyLevels);
      tracker = new ITMColorTrackerAdapter(colourTracker, renderState_live);
    } else if (settings.trackerType == ITMLibSettings::TRACKER_REN) {
      renTracker = new ITMRenTracker_HIP<TVoxel, TIndex>(&scene);     // MakeRenTracker: the Ren tracker alone, not a composite with ICP
      tracker = new ITMRenTrackerAdapter<TVoxel, TIndex>(renTracker);
    } else if (settings.trackerType == ITMLibSettings::TRACKER_WICP) {
      wicpTracker = new ITMWeightedICPTracker_HIP(settings.trackingRegime, settings.noHierarchyLevels, settings.noICPRunTillLevel,
                                                  settings.depthTrackerICPThreshold, settings.depthTrackerTerminationThreshold);
      tracker = new ITMWeightedICPTrackerAdapter(wicpTracker);
    } else {
      tracker = new ITMExternalTracker();          // TRACKER_EXTERNAL, and TRACKER_COLOR with poses from outside (useColourTracker = false)
    }
    trackingController = new ITMTrackingController_HIP<TVoxel, TIndex>(tracker, &visualisationEngine, &settings);
    if (settings.useRelocalisation)
      relocaliser = new ITMRelocaliser_HIP(imgSize_d, Vector2f{params.viewFrustum_min, params.viewFrustum_max}, settings.relocHarvestingThreshold, 500, 4,
                                           settings.relocCapacity);
    if (settings.useTrackingVerdict) poseQuality = new ITMPoseQuality_HIP(params.mu, settings.poseQuality);
    if (settings.liveMeshEveryNFrames > 0 && TIndex::kType == ITM_INDEX_HASH) check(itm_mesh_create(scene.handle, 0, &liveMesh), "itm_mesh_create (live mesh)");
  }
  ~ITMMainEngine_HIP() {
    delete poseQuality;
    delete relocaliser;
    itm_mesh_destroy(exportMesh);
    itm_mesh_destroy(liveMesh);
    itm_mesh_destroy(coarseMesh); delete coarseScene;
    delete renderState_freeview; itm_dev_free(depthImageBuf);
    delete renderState_poseUpdate;
    delete renderState_live; delete trackingController; delete tracker; delete depthTracker; delete colourTracker; delete renTracker; delete wicpTracker; delete viewBuilder;
    for (void* p : {depthBuf, scratchBuf, normalBuf, sigmaBuf, pointsBuf, coloursBuf}) itm_dev_free(p);
  }
  ITMMainEngine_HIP(const ITMMainEngine_HIP&) = delete;
  ITMMainEngine_HIP& operator=(const ITMMainEngine_HIP&) = delete;

  // ITMLibSettings.cpp:81: the colour tracker needs a voxel type with colour information
  static void check_settings(const ITMLibSettings& st) {
    if (st.trackerType == ITMLibSettings::TRACKER_COLOR && st.useColourTracker && TVoxel::kType != ITM_VOXEL_S_RGB && TVoxel::kType != ITM_VOXEL_F_RGB)
      throw std::runtime_error("Color tracker requires a voxel type with color information");
  }

  ITMView* GetView() { return &view; }
  ITMTrackingState* GetTrackingState() { return &trackingState; }
  ITMScene<TVoxel, TIndex>* GetScene() { return &scene; }
  // Fuses the whole scene of `other` (same GPU, same voxel size) into this engine's scene (itm_scene_merge).  Tracking state, render
  // states and `other` stay as they are: the merged blocks are seen by the next ProcessFrame whose view holds them.
  void MergeSceneFrom(const ITMMainEngine_HIP& other, itm_merge_stats* stats = nullptr) {
    ITMSceneMergeEngine_HIP<TVoxel, TIndex>().MergeScene(&scene, &other.scene, nullptr, stats);
    TouchLiveMeshEverywhere();
  }
  // Returns the blocks of this engine's scene that `cfg` selects (nullptr: settings.pruneConfig) to the pool (itm_scene_prune).  The
  // live render state's visible list loses them; tracking state and maps stay as they are.
  void PruneScene(const itm_prune_config* cfg = nullptr, itm_prune_stats* stats = nullptr) {
    ITMScenePruneEngine_HIP<TVoxel, TIndex>().PruneScene(&scene, cfg ? cfg : &settings.pruneConfig, &lastPrune);
    if (stats) *stats = lastPrune;
  }
  const itm_prune_stats& GetLastPruneStats() const { return lastPrune; }      // of the last PruneScene, by the host or by pruneEveryNFrames
  // The live mesh (settings.liveMeshEveryNFrames; nullptr without it or for a dense scene): the mesh of the scene as of the last update.
  // Every fused frame, RemoveFrame and ReintegrateFrame mark the blocks they wrote, MergeSceneFrom marks everything, PruneScene needs no
  // mark (itm_mesh_update finds the blocks that are gone).  UpdateLiveMesh brings it up to date now, whatever the frame count says.
  itm_mesh* GetLiveMesh() { return liveMesh; }
  const itm_mesh_update_stats& GetLastMeshUpdateStats() const { return lastMeshUpdate; }
  void UpdateLiveMesh() {
    if (!liveMesh) return;
    fusedSinceMeshUpdate = 0;
    check(itm_mesh_update(scene.handle, liveMesh, &lastMeshUpdate, nullptr), "UpdateLiveMesh");
  }
  // The same for an `other` that lives in a frame of its own: thisFromOther maps its world to this engine's (x_this = thisFromOther
  // x_other, metres).  The scene of `other` is resampled at this scene's voxels and fused (itm_scene_resample).
  void MergeSceneFrom(const ITMMainEngine_HIP& other, const Matrix4f& thisFromOther, itm_resample_stats* stats = nullptr) {
    ITMSceneResampleEngine_HIP<TVoxel, TIndex>().ResampleScene(&scene, &other.scene, thisFromOther, nullptr, stats);
    TouchLiveMeshEverywhere();
  }
  // Refines thisFromOther (the coarse pose on entry, the refined one on return) by registering the band voxels of `other`'s scene
  // against this engine's scene (ITMSceneAlignEngine_HIP); its natural use is followed by MergeSceneFrom(other, thisFromOther).  Neither
  // scene is written.  res->status: ITM_ALIGN_DEGENERATE when the geometry does not determine the pose -- the caller decides.
  void AlignSceneFrom(const ITMMainEngine_HIP& other, Matrix4f& thisFromOther, itm_align_result* res = nullptr) {
    ITMSceneAlignEngine_HIP<TVoxel, TIndex>().AlignScene(&scene, &other.scene, thisFromOther, res);
  }
  // Resamples this engine's scene into `coarse`, a scene of twice the voxel size and the same mu (itm_scene_coarsen).  This engine's
  // scene, tracking state and render states stay as they are.
  void CoarsenSceneInto(ITMScene<TVoxel, TIndex>* coarse, itm_coarsen_stats* stats = nullptr) {
    ITMSceneCoarsenEngine_HIP<TVoxel, TIndex>().CoarsenScene(coarse, &scene, nullptr, stats);
  }
  // The fused volume asked at the caller's own points / along the caller's own rays (ITMSceneQueryEngine_HIP; device pointers)
  void QueryPoints(const float* points, uint32_t n, const itm_query_out& out, int units = ITM_QUERY_METRES) const {
    ITMSceneQueryEngine_HIP<TVoxel, TIndex>().QueryPoints(&scene, points, n, out, units);
  }
  void CastRays(const float* rays, uint32_t n, float* hits) const { ITMSceneQueryEngine_HIP<TVoxel, TIndex>().CastRays(&scene, rays, n, hits); }
  // The distance transform of a box of the fused volume (ITMDistanceFieldEngine_HIP; device pointers)
  void DistanceField(const itm_esdf_box& box, const itm_esdf_out& out, int sites = ITM_ESDF_SITE_SURFACE, int minWeight = 1, int maxDistance = 0) const {
    ITMDistanceFieldEngine_HIP<TVoxel, TIndex>().Compute(&scene, box, out, sites, minWeight, maxDistance);
  }
  // A pose update (a loop closure, a batch optimisation): `frame` -- its images still on the device -- was fused under oldPose and is
  // taken back out of the scene: the visible blocks under oldPose are found through a render state of the engine's own that nothing
  // else uses, then de-integrated (itm_deintegrate_from_scene has the definition and what the operation is not).  The engine's tracking
  // pose, its live render state and its maps stay as they were.  With `stats` the stream is synchronised.
  void RemoveFrame(const ITMView* frame, const ITMPose& pose, itm_deintegrate_stats* stats = nullptr) {
    ITMRenderState* rs = PoseUpdateRenderState(frame);
    ITMTrackingState at;
    at.pose_d = pose;
    visualisationEngine.FindVisibleBlocks(&at.pose_d, &frame->calib.intrinsics_d, rs);
    ITMSceneReconstructionEngine_HIP<TVoxel, TIndex>().DeintegrateFromScene(&scene, frame, &at, rs, nullptr, stats);
    TouchLiveMesh(rs);
  }
  // ... and fused again under newPose: RemoveFrame, then AllocateSceneFromDepth and IntegrateIntoScene as ProcessFrame issues them, through
  // the same render state.  Everything is enqueued when the call returns (the frame's images may be reused).  The blocks the new pose
  // allocates reach the live visible list with the next ProcessFrame that sees them.
  void ReintegrateFrame(const ITMView* frame, const ITMPose& oldPose, const ITMPose& newPose, itm_deintegrate_stats* stats = nullptr) {
    RemoveFrame(frame, oldPose, stats);
    ITMRenderState* rs = PoseUpdateRenderState(frame);
    ITMTrackingState at;
    at.pose_d = newPose;
    ITMSceneReconstructionEngine_HIP<TVoxel, TIndex> reco;
    reco.AllocateSceneFromDepth(&scene, frame, &at, rs);
    reco.IntegrateIntoScene(&scene, frame, &at, rs);
    check(itm_flush(scene.handle, rs->handle, nullptr), "ReintegrateFrame (flush)");
    TouchLiveMesh(rs);
  }
  ITMRenderState* GetRenderState() { return renderState_live; }
  const ITMVisualisationEngine_HIP<TVoxel, TIndex>* GetVisualisationEngine() const { return &visualisationEngine; }
  const ITMViewBuilder_HIP* GetViewBuilder() const { return viewBuilder; }

  // rgbImage: device uchar4 (may be null without colour), rawDepthImage: device short
  // ITMLibSettings.cpp:51-54: the weighted ICP tracker switches the sensor-noise model on
  bool ModelSensorNoise() const { return settings.modelSensorNoise || settings.trackerType == ITMLibSettings::TRACKER_WICP; }
  void ProcessFrame(const uint8_t* rgbImage, const int16_t* rawDepthImage) {
    // prepare image and turn it into a depth image
    view.rgb = rgbImage;
    viewBuilder->UpdateView(&view, rawDepthImage, (float*)depthBuf, (float*)scratchBuf, settings.useBilateralFilter, ModelSensorNoise(),
                            (float*)normalBuf, (float*)sigmaBuf);
    view.depthUncertainty = ModelSensorNoise() ? (const float*)sigmaBuf : nullptr;
    ProcessView();
  }
  // The reference's own signature takes the raw frame in HOST memory (Engine/ITMMainEngine.cpp:111): rawDepthHost in page-locked memory
  // (itm_host_malloc); nextRawDepthHost, when the image source already has it, is uploaded while this frame is tracked and fused.
  // The uploads are asynchronous: a buffer handed over here may be REWRITTEN only once GetViewBuilder()->HostFramesRead() says so
  // (WaitHostFramesRead() waits; ~25 us after the call for a frame that was not announced).  The reference's CUDA build blocks in the
  // copy instead (ITMViewBuilder_CUDA.cu:53); an image source with two buffers never has to wait here.
  void ProcessFrameFromHost(const uint8_t* rgbImage, const int16_t* rawDepthHost, const int16_t* nextRawDepthHost = nullptr) {
    view.rgb = rgbImage;
    viewBuilder->UpdateViewFromHost(&view, rawDepthHost, (float*)depthBuf, (float*)scratchBuf, settings.useBilateralFilter, ModelSensorNoise(),
                                    (float*)normalBuf, (float*)sigmaBuf);
    view.depthUncertainty = ModelSensorNoise() ? (const float*)sigmaBuf : nullptr;
    if (nextRawDepthHost) viewBuilder->Prefetch(nextRawDepthHost, view.depthSize);
    ProcessView();
  }

 private:
  void ProcessView() {
    if (!mainProcessingActive) return;
    if (poseQuality) { ProcessViewJudged(); return; }
    // pose of this frame against the maps of the last ray cast
    trackingController->Track(&trackingState, &view);
    // allocate + integrate (the library records both; they launch with the two calls of Prepare as ONE fused frame, pending.hip)
    if (fusionActive) denseMapper.ProcessFrame(&view, &trackingState, &scene, renderState_live);
    // expected depths + ICP maps (or the forward projection) from the new pose: what the next Track call and the UI read
    trackingController->Prepare(&trackingState, &view, renderState_live);
    // the frame as a keyframe candidate, under the pose it was fused with
    if (relocaliser && fusionActive && harvestingActive) {
      int nearest; float distance;
      relocaliser->ProcessFrame(view.depth, &trackingState.pose_d, 1, &nearest, &distance, true);
    }
    if (fusionActive) { TouchLiveMesh(renderState_live); PruneIfDue(); UpdateLiveMeshIfDue(); }
  }

  // settings.pruneEveryNFrames: after the frame's maps are prepared, so that the recorded frame is launched as one fused frame as ever
  void PruneIfDue() {
    if (settings.pruneEveryNFrames <= 0 || ++fusedSincePrune < settings.pruneEveryNFrames) return;
    fusedSincePrune = 0;
    PruneScene();
  }
  // settings.liveMeshEveryNFrames: the blocks a frame wrote are those of its render state's visible list; the update runs where the
  // pruning does, after the frame's maps are prepared, so that the recorded frame is launched as one fused frame as ever
  void TouchLiveMesh(const ITMRenderState* rs) {
    if (liveMesh) check(itm_mesh_touch(liveMesh, scene.handle, rs->handle, nullptr, 0, nullptr), "TouchLiveMesh");
  }
  void TouchLiveMeshEverywhere() {
    if (liveMesh) check(itm_mesh_touch(liveMesh, scene.handle, nullptr, nullptr, -1, nullptr), "TouchLiveMesh (everything)");
  }
  void UpdateLiveMeshIfDue() {
    if (!liveMesh || ++fusedSinceMeshUpdate < settings.liveMeshEveryNFrames) return;
    UpdateLiveMesh();
  }

 public:
  // Keyframe relocaliser (settings.useRelocalisation; nullptr without it).  While fusion is active every frame is offered to it as a
  // keyframe under its pose; SetKeyframeHarvesting(false) stops that (a host that knows its poses are poor).
  ITMRelocaliser_HIP* GetRelocaliser() { return relocaliser; }
  void SetKeyframeHarvesting(bool on) { harvestingActive = on; }
  // The pose is lost (the host decides when): builds the view from the raw frame as ProcessFrame does and asks for the nearest
  // keyframe, without harvesting.  None (or no relocaliser): returns -1 and changes nothing else.  Otherwise pose_d becomes the
  // keyframe's pose, the live visible list is rebuilt for it (FindVisibleBlocks), and Prepare, Track, Prepare run with a full ray
  // cast: the tracker refines against maps rendered from the keyframe's pose, and the maps the next frame tracks against are
  // rendered from the refined pose.  Nothing is integrated.  Returns the keyframe's id.
  int Relocalise(const uint8_t* rgbImage, const int16_t* rawDepthImage) {
    view.rgb = rgbImage;
    viewBuilder->UpdateView(&view, rawDepthImage, (float*)depthBuf, (float*)scratchBuf, settings.useBilateralFilter, ModelSensorNoise(),
                            (float*)normalBuf, (float*)sigmaBuf);
    view.depthUncertainty = ModelSensorNoise() ? (const float*)sigmaBuf : nullptr;
    return RecoverFromKeyframe();
  }

 private:
  // the render state of RemoveFrame / ReintegrateFrame, of the frame's depth size
  ITMRenderState* PoseUpdateRenderState(const ITMView* frame) {
    if (renderState_poseUpdate && (renderState_poseUpdate->imgSize.x != frame->depthSize.x || renderState_poseUpdate->imgSize.y != frame->depthSize.y)) {
      delete renderState_poseUpdate;
      renderState_poseUpdate = nullptr;
    }
    if (!renderState_poseUpdate) renderState_poseUpdate = visualisationEngine.CreateRenderState(frame->depthSize);
    return renderState_poseUpdate;
  }
  // the live visible list rebuilt for pose_d
  void FindVisibleBlocksAtPose() {
    if (settings.trackerType == ITMLibSettings::TRACKER_COLOR) {      // the live render state is the colour camera's (Prepare)
      ITMPose pose_rgb;
      float M[16];
      matmul4(view.calib.trafo_rgb_to_depth_calib_inv, trackingState.pose_d.GetM(), M);
      pose_rgb.SetM(M);
      visualisationEngine.FindVisibleBlocks(&pose_rgb, &view.calib.intrinsics_rgb, renderState_live);
    } else {
      visualisationEngine.FindVisibleBlocks(&trackingState.pose_d, &view.calib.intrinsics_d, renderState_live);
    }
  }

  // The recovery of Relocalise for the view as it stands (also what a FAILED verdict runs): -1 and nothing changed without a
  // relocaliser or a keyframe, else the keyframe's id.
  int RecoverFromKeyframe() {
    if (!relocaliser) return -1;
    int nearest = -1; float distance = 1.0f;
    relocaliser->ProcessFrame(view.depth, nullptr, 1, &nearest, &distance, false);
    if (nearest < 0) return -1;
    trackingState.pose_d = relocaliser->RetrievePose(nearest);
    FindVisibleBlocksAtPose();
    trackingState.requiresFullRendering = true;
    trackingController->Prepare(&trackingState, &view, renderState_live);
    trackingController->Track(&trackingState, &view);
    trackingController->Prepare(&trackingState, &view, renderState_live);
    return nearest;
  }

  // view.depth under pose_d against the fused volume; the counts stay in lastQuality
  ITMPoseQuality_HIP::TrackingResult Judge() {
    lastQuality = poseQuality->Evaluate(&scene, &view, &trackingState);
    return poseQuality->Verdict(lastQuality);
  }

  // ProcessView with settings.useTrackingVerdict: the tracked pose is judged before anything is written.  GOOD: the frame is fused
  // and offered as a keyframe as ever (unless a recovery's delay is pending: it counts down on GOOD frames only).  POOR: neither,
  // the maps are prepared from the tracked pose.  FAILED: neither, pose_d goes back to the pose the frame started from -- for poses
  // from outside (ITMExternalTracker: the host has overwritten pose_d before the call) the pose the previous frame ended with --
  // and, with a relocaliser, the recovery of Relocalise runs and is judged in its turn: it stands unless it FAILED too.
  void ProcessViewJudged() {
    typedef ITMPoseQuality_HIP Q;
    const bool posesFromOutside = !depthTracker && !colourTracker && !renTracker && !wicpTracker;
    const ITMPose remembered = (posesFromOutside && haveEndPose) ? endPose : trackingState.pose_d;
    trackingController->Track(&trackingState, &view);
    lastFrameFused = false;
    Q::TrackingResult result = Q::TRACKING_GOOD;      // nothing fused yet: the map is empty and every pose is as good as another
    if (anyFrameFused) result = Judge();
    else lastQuality = itm_pose_quality{0, 0, 0, 0, 0.0, 0.0};
    if (result == Q::TRACKING_GOOD) {
      const bool delayed = fusionDelay > 0;
      if (fusionActive && !delayed) {
        denseMapper.ProcessFrame(&view, &trackingState, &scene, renderState_live);
        anyFrameFused = lastFrameFused = true;
      }
      trackingController->Prepare(&trackingState, &view, renderState_live);
      if (relocaliser && fusionActive && harvestingActive && !delayed) {
        int nearest; float distance;
        relocaliser->ProcessFrame(view.depth, &trackingState.pose_d, 1, &nearest, &distance, true);
      }
      if (delayed) --fusionDelay;
      if (lastFrameFused) { TouchLiveMesh(renderState_live); PruneIfDue(); UpdateLiveMeshIfDue(); }
    } else if (result == Q::TRACKING_POOR) {
      trackingController->Prepare(&trackingState, &view, renderState_live);
    } else {
      trackingState.pose_d = remembered;
      bool recovered = false;
      if (RecoverFromKeyframe() >= 0) {
        const Q::TrackingResult again = Judge();
        if (again != Q::TRACKING_FAILED) {
          recovered = true; result = again;
          fusionDelay = settings.relocFusionDelay;
          ++relocalisationCount;
        } else {
          trackingState.pose_d = remembered;
          FindVisibleBlocksAtPose();      // the recovery left the keyframe's visible list behind
        }
      }
      if (!recovered) {
        trackingState.requiresFullRendering = true;
        trackingController->Prepare(&trackingState, &view, renderState_live);
      }
    }
    trackingResult = result;
    endPose = trackingState.pose_d; haveEndPose = true;
  }

 public:
  // Tracking verdict (settings.useTrackingVerdict; without it: GOOD, zero counts, 0, false).  The result and counts of the last
  // frame -- after a recovery those of the second evaluation, at the recovered pose --, the recoveries so far, and whether the
  // last frame was integrated.
  ITMPoseQuality_HIP::TrackingResult GetTrackingResult() const { return trackingResult; }
  const itm_pose_quality& GetPoseQuality() const { return lastQuality; }
  int GetRelocalisationCount() const { return relocalisationCount; }
  bool LastFrameFused() const { return lastFrameFused; }
  void turnOnIntegration() { fusionActive = true; }
  void turnOffIntegration() { fusionActive = false; }
  void turnOnMainProcessing() { mainProcessingActive = true; }
  void turnOffMainProcessing() { mainProcessingActive = false; }

  // ITMMainEngine::GetImageType (Engine/ITMMainEngine.h:88-97)
  enum GetImageType {
    InfiniTAM_IMAGE_ORIGINAL_RGB,
    InfiniTAM_IMAGE_ORIGINAL_DEPTH,
    InfiniTAM_IMAGE_SCENERAYCAST,
    InfiniTAM_IMAGE_FREECAMERA_SHADED,
    InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME,
    InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL,
    InfiniTAM_IMAGE_UNKNOWN
  };
  // ITMMainEngine::GetImageSize (Engine/ITMMainEngine.cpp:129-132): the live render state's raycastImage->noDims
  Vector2i GetImageSize() const { return renderState_live->imgSize; }

  // The images of GetImage left in DEVICE memory: returns the device uchar4 image and its size, no host copy -- a host that displays
  // through its own GPU path pays no PCIe trip.  Everything is submitted on the engine's stream (the default one); the pointer is the
  // engine's or the view's and holds the image until the next ProcessFrame / GetImage call of the same type.  nullptr (size 0 x 0)
  // before the first frame and for InfiniTAM_IMAGE_UNKNOWN.  freeviewSize: the size of a free-camera image (GetImage passes
  // out->noDims); pose / intrinsics are read by the free-camera types only.
  // Tracking and fusion are not disturbed: the free camera has a render state of its own, so the live visible list, range image and
  // ICP maps stay as the frame left them; calls that name the scene launch what the library had recorded first (include/itm_hip.h).
  const uint8_t* GetImageDevice(Vector2i* size, GetImageType getImageType, const ITMPose* pose = nullptr, const ITMIntrinsics* intrinsics = nullptr,
                                Vector2i freeviewSize = Vector2i{0, 0}) {
    *size = Vector2i{0, 0};
    if (view.depth == nullptr) return nullptr;      // `if (view == NULL) return;`: no frame has been processed
    switch (getImageType) {
      case InfiniTAM_IMAGE_ORIGINAL_RGB:
        *size = view.rgbSize;
        return view.rgb;
      case InfiniTAM_IMAGE_ORIGINAL_DEPTH: {
        if (!depthImageBuf) check(itm_dev_malloc(&depthImageBuf, (size_t)view.depthSize.x * view.depthSize.y * 4), "malloc");
        // WeightToUchar4 of the uncertainty image for the weighted ICP tracker (its 2-pixel border is the 0 the constructor cleared),
        // DepthToUchar4 of the depth image otherwise -- on the device, where both images live
        if (settings.trackerType == ITMLibSettings::TRACKER_WICP)
          check(itm_weight_to_uchar4(view.depthUncertainty, (uint8_t*)depthImageBuf, view.depthSize.x, view.depthSize.y, nullptr), "WeightToUchar4");
        else
          check(itm_depth_to_uchar4(view.depth, (uint8_t*)depthImageBuf, view.depthSize.x, view.depthSize.y, nullptr), "DepthToUchar4");
        *size = view.depthSize;
        return (const uint8_t*)depthImageBuf;
      }
      case InfiniTAM_IMAGE_SCENERAYCAST:
        check(itm_flush(scene.handle, renderState_live->handle, nullptr), "itm_flush");
        *size = renderState_live->imgSize;
        return (const uint8_t*)itm_buffer_ptr(scene.handle, renderState_live->handle, ITM_BUF_RAYCAST_IMAGE);
      case InfiniTAM_IMAGE_FREECAMERA_SHADED:
      case InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME:
      case InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL: {
        typedef ITMVisualisationEngine_HIP<TVoxel, TIndex> Vis;
        typename Vis::RenderImageType type = Vis::RENDER_SHADED_GREYSCALE;
        if (getImageType == InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME) type = Vis::RENDER_COLOUR_FROM_VOLUME;
        else if (getImageType == InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL) type = Vis::RENDER_COLOUR_FROM_NORMAL;
        if (!pose || !intrinsics) throw std::runtime_error("GetImage: the free camera needs a pose and intrinsics");
        if (freeviewSize.x <= 0 || freeviewSize.y <= 0) throw std::runtime_error("GetImage: the free camera needs an image size");
        // The reference creates renderState_freeview once, at the size of the first call, and never again
        // (Engine/ITMMainEngine.cpp:178): a later call with an image of another size renders into the old one -- a latent bug
        // there.  Here the state is recreated when the size differs.
        if (renderState_freeview && (renderState_freeview->imgSize.x != freeviewSize.x || renderState_freeview->imgSize.y != freeviewSize.y)) {
          check(itm_stream_synchronize(nullptr), "GetImage (free view)");      // nothing still renders into the state that goes away
          delete renderState_freeview; renderState_freeview = nullptr;
        }
        if (renderState_freeview == nullptr) renderState_freeview = visualisationEngine.CreateRenderState(freeviewSize);
        visualisationEngine.FindVisibleBlocks(pose, intrinsics, renderState_freeview);
        visualisationEngine.CreateExpectedDepths(pose, intrinsics, renderState_freeview);
        visualisationEngine.RenderImage(pose, intrinsics, renderState_freeview, nullptr, type);      // into renderState_freeview->raycastImage
        *size = renderState_freeview->imgSize;
        return (const uint8_t*)itm_buffer_ptr(scene.handle, renderState_freeview->handle, ITM_BUF_RAYCAST_IMAGE);
      }
      case InfiniTAM_IMAGE_UNKNOWN:
        break;
    }
    return nullptr;
  }

  // ITMMainEngine::GetImage (Engine/ITMMainEngine.cpp:134-192), statement for statement: GetImageDevice plus one copy to the host
  // and a stream synchronise.  Before the first frame `out` is not touched; InfiniTAM_IMAGE_UNKNOWN leaves it cleared.
  void GetImage(ITMUChar4Image* out, GetImageType getImageType, const ITMPose* pose = nullptr, const ITMIntrinsics* intrinsics = nullptr) {
    if (view.depth == nullptr) return;
    out->Clear();
    Vector2i size;
    const uint8_t* image = GetImageDevice(&size, getImageType, pose, intrinsics, out->noDims);
    if (!image) return;
    out->ChangeDims(size);
    check(itm_memcpy_d2h(out->GetData(), image, out->dataSize * sizeof(Vector4u), nullptr), "GetImage");
    check(itm_stream_synchronize(nullptr), "GetImage");
  }

  // ITMMainEngine::SaveSceneToMesh (Engine/ITMMainEngine.cpp:104-109): meshes the scene and writes it as binary STL
  void SaveSceneToMesh(const char* fileName) {
    MeshForExport(0);
    check(itm_mesh_write_stl(exportMesh, fileName, nullptr), "WriteSTL");
  }
  // SaveSceneToMesh through itm_mesh_volume: also a dense scene (ITMPlainVoxelArray) gives its surface, meshed brick by brick;
  // a hash scene gives the file SaveSceneToMesh writes
  void SaveVolumeToMesh(const char* fileName) {
    if (!exportMesh) check(itm_mesh_create(scene.handle, 0, &exportMesh), "itm_mesh_create");
    check(itm_mesh_volume(scene.handle, exportMesh, nullptr), "MeshVolume");
    check(itm_mesh_write_stl(exportMesh, fileName, nullptr), "WriteSTL");
  }
  // the same mesh as a binary PLY with per-vertex normals and, for the voxel types that store colour, colours (itm_mesh_attributes)
  void SaveSceneToPLY(const char* fileName) {
    const bool colour = TVoxel::kType == ITM_VOXEL_S_RGB || TVoxel::kType == ITM_VOXEL_F_RGB;
    MeshForExport(ITM_MESH_NORMALS | (colour ? ITM_MESH_COLOURS : 0));
    check(itm_mesh_write_ply(exportMesh, fileName, nullptr), "WritePLY");
  }
  // the mesh welded into shared vertices (itm_mesh_index): a binary PLY with one vertex per distinct position, faces through the
  // index, and the same attributes evaluated once per unique vertex (itm_mesh_indexed_attributes)
  void SaveSceneToIndexedPLY(const char* fileName) {
    const bool colour = TVoxel::kType == ITM_VOXEL_S_RGB || TVoxel::kType == ITM_VOXEL_F_RGB;
    MeshForExport(0);
    check(itm_mesh_index(exportMesh, nullptr), "itm_mesh_index");
    check(itm_mesh_indexed_attributes(scene.handle, exportMesh, ITM_MESH_NORMALS | (colour ? ITM_MESH_COLOURS : 0), nullptr), "itm_mesh_indexed_attributes");
    check(itm_mesh_write_ply_indexed(exportMesh, fileName, nullptr), "WriteIndexedPLY");
  }
  // SaveSceneToIndexedPLY without the floating fragments: the mesh is indexed, its connected components are labelled
  // (itm_mesh_components) and those with fewer than minTriangles triangles dropped (itm_mesh_filter_components); what is left is
  // indexed again and written with its attributes
  void SaveSceneToCleanPLY(const char* fileName, uint32_t minTriangles) { SaveCleanPLY(fileName, minTriangles, nullptr); }
  // SaveSceneToCleanPLY with a smoothing step (itm_mesh_smooth: `steps` Taubin passes at the default factors and quantum, border and
  // non-manifold vertices pinned) between the second index and the indexed attributes, which are read at the smoothed positions
  void SaveSceneToSmoothPLY(const char* fileName, uint32_t minTriangles, uint32_t steps) {
    itm_mesh_smooth_config cfg;
    check(itm_mesh_smooth_default_config(sceneParams.voxelSize, &cfg), "itm_mesh_smooth_default_config");
    cfg.steps = steps;
    SaveCleanPLY(fileName, minTriangles, &cfg);
  }
  // A lower level of detail of SaveSceneToIndexedPLY: the scene is resampled into one of twice the voxel size that the engine owns
  // (created by the first call with the same mu, maxW and index configuration; reset and refilled by every call), and THAT scene is
  // meshed (itm_mesh_volume), indexed and written with the attributes read from it
  void SaveSceneToCoarsePLY(const char* fileName) {
    const bool colour = TVoxel::kType == ITM_VOXEL_S_RGB || TVoxel::kType == ITM_VOXEL_F_RGB;
    if (!coarseScene) coarseScene = new ITMScene<TVoxel, TIndex>(&coarseParams, localBlockNum_);
    ITMSceneReconstructionEngine_HIP<TVoxel, TIndex>().ResetScene(coarseScene);
    CoarsenSceneInto(coarseScene);
    if (!coarseMesh) check(itm_mesh_create(coarseScene->handle, 0, &coarseMesh), "itm_mesh_create");
    check(itm_mesh_volume(coarseScene->handle, coarseMesh, nullptr), "MeshVolume");
    check(itm_mesh_index(coarseMesh, nullptr), "itm_mesh_index");
    check(itm_mesh_indexed_attributes(coarseScene->handle, coarseMesh, ITM_MESH_NORMALS | (colour ? ITM_MESH_COLOURS : 0), nullptr), "itm_mesh_indexed_attributes");
    check(itm_mesh_write_ply_indexed(coarseMesh, fileName, nullptr), "WriteIndexedPLY");
  }

 private:
  // the clean export; smooth given: itm_mesh_smooth between the second index and the indexed attributes
  void SaveCleanPLY(const char* fileName, uint32_t minTriangles, const itm_mesh_smooth_config* smooth) {
    const bool colour = TVoxel::kType == ITM_VOXEL_S_RGB || TVoxel::kType == ITM_VOXEL_F_RGB;
    MeshForExport(0);
    check(itm_mesh_index(exportMesh, nullptr), "itm_mesh_index");
    check(itm_mesh_components(exportMesh, nullptr), "itm_mesh_components");
    check(itm_mesh_filter_components(exportMesh, minTriangles, nullptr, 0, nullptr, nullptr, nullptr), "itm_mesh_filter_components");
    check(itm_mesh_index(exportMesh, nullptr), "itm_mesh_index");
    if (smooth) check(itm_mesh_smooth(exportMesh, smooth, nullptr, nullptr), "itm_mesh_smooth");
    check(itm_mesh_indexed_attributes(scene.handle, exportMesh, ITM_MESH_NORMALS | (colour ? ITM_MESH_COLOURS : 0), nullptr), "itm_mesh_indexed_attributes");
    check(itm_mesh_write_ply_indexed(exportMesh, fileName, nullptr), "WriteIndexedPLY");
  }
  void MeshForExport(int attributes) {
    if (!exportMesh) check(itm_mesh_create(scene.handle, 0, &exportMesh), "itm_mesh_create");
    check(itm_mesh_scene(scene.handle, exportMesh, nullptr), "MeshScene");
    if (attributes) check(itm_mesh_attributes(scene.handle, exportMesh, attributes, nullptr), "itm_mesh_attributes");
  }
};

// ITMMesh (Objects/ITMMesh.h:14-124): the triangle buffer lives in HBM; WriteOBJ / WriteSTL produce the reference's files.
// ComputeAttributes / WritePLY go beyond the reference's ITMMesh: per-vertex normals and colours of the buffer's triangles
// (itm_mesh_attributes: computeSingleNormalFromSDF and readFromSDF_color4u_interpolated at vertex / voxelSize) and a binary PLY.
class ITMMesh {
 public:
  itm_mesh* handle = nullptr;
  uint32_t noTotalTriangles = 0, noMaxTriangles = 0;
  float voxelSize = 0.0f;                // of the scene the mesh was created for: Smooth's default quantum
  itm_stream stream = nullptr;
  template <class TVoxel, class TIndex>
  explicit ITMMesh(const ITMScene<TVoxel, TIndex>* scene, uint32_t maxTriangles = 0) {
    check(itm_mesh_create(scene->handle, maxTriangles, &handle), "itm_mesh_create");
    check(itm_mesh_info(handle, nullptr, &noMaxTriangles, nullptr, nullptr), "itm_mesh_info");
    voxelSize = scene->sceneParams->voxelSize;
  }
  ~ITMMesh() { itm_mesh_destroy(handle); }
  ITMMesh(const ITMMesh&) = delete;
  ITMMesh& operator=(const ITMMesh&) = delete;
  const float* triangles() const { const float* p = nullptr; check(itm_mesh_info(handle, nullptr, nullptr, &p, stream), "itm_mesh_info"); return p; }   // device pointer
  void WriteOBJ(const char* fileName) const { check(itm_mesh_write_obj(handle, fileName, stream), "WriteOBJ"); }
  void WriteSTL(const char* fileName) const { check(itm_mesh_write_stl(handle, fileName, stream), "WriteSTL"); }
  // what: ITM_MESH_NORMALS, ITM_MESH_COLOURS or both; stale after the next MeshScene
  template <class TVoxel, class TIndex>
  void ComputeAttributes(const ITMScene<TVoxel, TIndex>* scene, int what) { check(itm_mesh_attributes(scene->handle, handle, what, stream), "ComputeAttributes"); }
  // host copies: 3 x float[3] / 3 x {r, g, b, 255} per triangle, buffer order
  void DownloadAttributes(float* normals, uint8_t* colours, uint32_t capacityTriangles) const {
    uint32_t n = 0;
    check(itm_mesh_download_attributes(handle, normals, colours, capacityTriangles, &n, stream), "DownloadAttributes");
  }
  void WritePLY(const char* fileName) const { check(itm_mesh_write_ply(handle, fileName, stream), "WritePLY"); }
  // the indexed form of the buffer's triangles (bit-equal positions are one vertex); stale after the next MeshScene
  uint32_t noVertices = 0;
  void Index() {
    check(itm_mesh_index(handle, stream), "Index");
    check(itm_mesh_index_info(handle, &noVertices, nullptr, nullptr, nullptr, nullptr, stream), "itm_mesh_index_info");
  }
  template <class TVoxel, class TIndex>
  void ComputeIndexedAttributes(const ITMScene<TVoxel, TIndex>* scene, int what) { check(itm_mesh_indexed_attributes(scene->handle, handle, what, stream), "ComputeIndexedAttributes"); }
  void WriteIndexedPLY(const char* fileName) const { check(itm_mesh_write_ply_indexed(handle, fileName, stream), "WriteIndexedPLY"); }
  void WriteIndexedOBJ(const char* fileName) const { check(itm_mesh_write_obj_indexed(handle, fileName, stream), "WriteIndexedOBJ"); }
  // the connected components of the present index; stale after the next MeshScene, Index or FilterComponents
  uint32_t noComponents = 0;
  void Components() {
    check(itm_mesh_components(handle, stream), "Components");
    check(itm_mesh_components_info(handle, &noComponents, nullptr, nullptr, nullptr, nullptr, stream), "itm_mesh_components_info");
  }
  // keeps the components with at least minTriangles triangles and, keep given (noKeep == noComponents entries), a non-zero entry there;
  // the kept triangles are packed to the front of the buffer.  Attributes, index and components are stale afterwards.
  void FilterComponents(uint32_t minTriangles, const uint8_t* keep = nullptr, uint32_t noKeep = 0) {
    check(itm_mesh_filter_components(handle, minTriangles, keep, noKeep, &noTotalTriangles, nullptr, stream), "FilterComponents");
    noVertices = 0; noComponents = 0;
  }
  // Fixed-point smoothing of the present index (itm_mesh_smooth): `steps` single passes with the factors lambda (even passes) and mu
  // (odd passes; mu == lambda: plain Laplacian) on positions quantised to `quantum` metres (0: voxelSize / 1024); pinIrregular keeps
  // border and non-manifold vertices where they are.  Vertices and triangle buffer move together, the index stays current; the
  // attributes (ComputeAttributes, ComputeIndexedAttributes) and the components are stale afterwards.
  itm_mesh_smooth_stats Smooth(uint32_t steps = 20, float lambda = 0.5f, float mu = -0.53f, float quantum = 0.0f, bool pinIrregular = true) {
    itm_mesh_smooth_config cfg;
    check(itm_mesh_smooth_default_config(voxelSize, &cfg), "itm_mesh_smooth_default_config");
    cfg.steps = steps;
    cfg.lambdaQ16 = (int32_t)std::lround((double)lambda * 65536.0);
    cfg.muQ16 = (int32_t)std::lround((double)mu * 65536.0);
    if (quantum != 0.0f) cfg.quantum = quantum;
    cfg.flags = pinIrregular ? ITM_MESH_SMOOTH_PIN_IRREGULAR : 0u;
    itm_mesh_smooth_stats stats;
    check(itm_mesh_smooth(handle, &cfg, &stats, stream), "Smooth");
    noComponents = 0;
    return stats;
  }
  // Incremental re-meshing (itm_mesh_touch / itm_mesh_update).  Touch marks the blocks that were rewritten since the mesh was last up to
  // date: the visible list of a render state (what a fused frame wrote), `n` table slots in device memory, or everything.  Update
  // (ITMMeshingEngine_HIP::UpdateMesh) re-meshes the marked blocks, those that appeared or vanished and their neighbours, and keeps every
  // other run; triangles() may answer with another address afterwards.  Attributes, index and components are stale after it.
  template <class TVoxel, class TIndex>
  void Touch(const ITMScene<TVoxel, TIndex>* scene, const ITMRenderState* renderState, const int32_t* slots = nullptr, int n = 0) {
    check(itm_mesh_touch(handle, scene->handle, renderState ? renderState->handle : nullptr, slots, n, stream), "Touch");
  }
  template <class TVoxel, class TIndex>
  void TouchEverything(const ITMScene<TVoxel, TIndex>* scene) { check(itm_mesh_touch(handle, scene->handle, nullptr, nullptr, -1, stream), "Touch (everything)"); }
  template <class TVoxel, class TIndex>
  itm_mesh_update_stats Update(const ITMScene<TVoxel, TIndex>* scene) {
    itm_mesh_update_stats stats;
    check(itm_mesh_update(scene->handle, handle, &stats, stream), "Update");
    noTotalTriangles = stats.trianglesAfter; noVertices = 0; noComponents = 0;
    return stats;
  }
  // the delta of the last Update on the host: the re-meshed blocks with their runs, the blocks that are gone
  void DownloadUpdate(std::vector<itm_mesh_changed_block>& changed, std::vector<itm_mesh_removed_block>& removed) const {
    uint32_t nc = 0, nr = 0;
    check(itm_mesh_update_info(handle, &nc, &nr, nullptr, nullptr, stream), "itm_mesh_update_info");
    changed.resize(nc); removed.resize(nr);
    check(itm_mesh_download_update(handle, changed.data(), nc, removed.data(), nr, nullptr, nullptr, stream), "DownloadUpdate");
  }
};

// ITMMeshingEngine<TVoxel,TIndex>::MeshScene (Engine/ITMMeshingEngine.h:19-26)
template <class TVoxel, class TIndex>
class ITMMeshingEngine_HIP {
 public:
  itm_stream stream = nullptr;
  void MeshScene(ITMMesh* mesh, const ITMScene<TVoxel, TIndex>* scene) {
    check(itm_mesh_scene(scene->handle, mesh->handle, stream), "MeshScene");
    check(itm_mesh_info(mesh->handle, &mesh->noTotalTriangles, nullptr, nullptr, stream), "itm_mesh_info");
  }
  // beyond the reference (its dense MeshScene is empty): itm_mesh_volume -- MeshScene for a hash scene, a dense scene brick by brick
  void MeshVolume(ITMMesh* mesh, const ITMScene<TVoxel, TIndex>* scene) {
    check(itm_mesh_volume(scene->handle, mesh->handle, stream), "MeshVolume");
    check(itm_mesh_info(mesh->handle, &mesh->noTotalTriangles, nullptr, nullptr, stream), "itm_mesh_info");
  }
  // beyond the reference: itm_mesh_update -- MeshScene at the cost of the blocks that ITMMesh::Touch marked (hash scenes)
  itm_mesh_update_stats UpdateMesh(ITMMesh* mesh, const ITMScene<TVoxel, TIndex>* scene) {
    const itm_stream keep = mesh->stream;
    mesh->stream = stream;
    const itm_mesh_update_stats stats = mesh->Update(scene);
    mesh->stream = keep;
    return stats;
  }
};

// One rank's end of the multi-stream exchange: the record of this stream goes out with every frame, the table of all
// streams comes back every `batch` frames.  Rank 0 creates the id, the host distributes it.
class ITMStreamExchange_HIP {
  itm_exchange* handle = nullptr;
  int world, maxIds, batch;

 public:
  static void UniqueId(unsigned char id[128]) { check(itm_exchange_unique_id(id), "itm_exchange_unique_id"); }
  ITMStreamExchange_HIP(int world_, int rank, const unsigned char id[128], int maxIds_ = 16384, int batch_ = 8) : world(world_), maxIds(maxIds_), batch(batch_) {
    check(itm_exchange_create(world, rank, id, maxIds, batch, &handle), "itm_exchange_create");
  }
  ~ITMStreamExchange_HIP() { itm_exchange_destroy(handle); }
  ITMStreamExchange_HIP(const ITMStreamExchange_HIP&) = delete;
  ITMStreamExchange_HIP& operator=(const ITMStreamExchange_HIP&) = delete;
  void Publish(const ITMRenderState* renderState, const ITMTrackingState* trackingState, itm_stream stream = nullptr) {
    check(itm_exchange_step(handle, renderState->handle, trackingState->pose_d.GetM(), stream), "itm_exchange_step");
  }
  size_t TableWords() const { return (size_t)world * (size_t)batch * (size_t)(17 + maxIds); }
  void Table(int32_t* hostTable) { check(itm_exchange_table(handle, hostTable, TableWords()), "itm_exchange_table"); }
};

}  // namespace itmhip
