/*
 * itm_hip.h -- C-ABI of the MI355X-native TSDF allocate / integrate / raycast path.
 *
 * This is the drop-in boundary: one flat `extern "C"` surface (plain pointers, sizes and POD
 * structs, no C++/torch types) that a fourth InfiniTAM back-end ("HIP", next to CPU/CUDA/Metal in
 * InfiniTAM/ITMLib/Engine/DeviceSpecific/) binds to.  Every entry point names the reference
 * method it replaces (paths relative to /root/reference/InfiniTAM/ITMLib).
 *
 * Conventions
 *  - All image / map pointers are DEVICE pointers for libitmhip.so (HBM), valid on `stream`'s
 *    device.  Nothing is synchronised implicitly except itm_get_counters / itm_download_* /
 *    itm_stream_synchronize; every other call only enqueues work on `stream` (a hipStream_t
 *    passed as void*; NULL = the default stream).
 *  - Matrices are 4x4 float, column-major `m[col*4+row]` exactly as ORUtils::Matrix4
 *    (ORUtils/Matrix.h:23-33,78); poses are world->camera.
 *  - Intrinsics are (fx, fy, cx, cy) = ITMIntrinsics::projectionParamsSimple.all
 *    (Objects/ITMIntrinsics.h:20-40).
 *  - Memory layouts of ITMHashEntry, ITMVoxel_{s,f,s_rgb,f_rgb}, Vector2f/4f/4u images are
 *    byte-identical to the reference (Utils/ITMLibDefines.h:71-199), so dumps compare 1:1.
 *  - Return value: 0 = ok, negative = ITM_ERR_*.  The reference's engines are `void` and
 *    exit(-1) on device errors (ORUtils/CUDADefines.h:27-36); the C++ adapter maps non-zero to
 *    std::runtime_error.  Pool exhaustion is NOT an error: blocks are silently skipped as in
 *    DeviceSpecific/CPU/ITMSceneReconstructionEngine_CPU.cpp:189,206.
 *
 * The same header is compiled with a different ITM_FN prefix by the test oracle (oracle/) so that
 * the parity tests can drive the oracle and the product through one binding; the product library
 * exports the `itm_` names only.
 */
#ifndef ITM_HIP_H_
#define ITM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifndef ITM_FN
#define ITM_FN(name) itm_##name
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes -------------------------------------------------------------------------- */
#define ITM_OK 0
#define ITM_ERR_INVALID -1      /* bad argument / unsupported configuration            */
#define ITM_ERR_DEVICE -2       /* HIP runtime error (message via itm_last_error)      */
#define ITM_ERR_UNSUPPORTED -3  /* valid in the reference, not available in this build */

/* ---- compile-time constants of the reference kept as defaults ---------------------------- */
#define ITM_SDF_BLOCK_SIZE 8            /* Utils/ITMLibDefines.h:37 */
#define ITM_SDF_BLOCK_SIZE3 512         /* :38 */
#define ITM_DEFAULT_LOCAL_BLOCK_NUM 0x10000 /* :40  (fork value; upstream 0x40000)     */
#define ITM_DEFAULT_BUCKET_NUM 0x100000 /* :51 */
#define ITM_DEFAULT_EXCESS_NUM 0x20000  /* :60 */
#define ITM_MAX_RENDERING_BLOCKS (65536 * 4) /* DeviceAgnostic/ITMVisualisationEngine.h:24 */

/* TVoxel / TIndex template parameters of the reference become runtime enums. */
enum itm_voxel_type {
  ITM_VOXEL_S = 0,     /* ITMVoxel_s      4 B  {i16 sdf; u8 w_depth; pad}           :153-174 */
  ITM_VOXEL_F = 1,     /* ITMVoxel_f      8 B  {f32 sdf; u8 w_depth; pad[3]}        :176-197 */
  ITM_VOXEL_S_RGB = 2, /* ITMVoxel_s_rgb  8 B  {i16 sdf; u8 w; u8 clr[3]; u8 w_color; pad}   */
  ITM_VOXEL_F_RGB = 3  /* ITMVoxel_f_rgb 12 B  {f32 sdf; u8 w; u8 clr[3]; u8 w_color; pad[3]} */
};
enum itm_index_type {
  ITM_INDEX_HASH = 0,  /* ITMVoxelBlockHash   Objects/ITMVoxelBlockHash.h:22-100  */
  ITM_INDEX_DENSE = 1  /* ITMPlainVoxelArray  Objects/ITMPlainVoxelArray.h:18-75  */
};
/* IITMVisualisationEngine::RenderImageType, Engine/ITMVisualisationEngine.h:21-26 */
enum itm_render_type {
  ITM_RENDER_SHADED_GREYSCALE = 0,
  ITM_RENDER_COLOUR_FROM_VOLUME = 1,
  ITM_RENDER_COLOUR_FROM_NORMAL = 2
};

/* ITMSceneParams, Objects/ITMSceneParams.h:14-70 (defaults Utils/ITMLibSettings.cpp:10). */
typedef struct itm_scene_params {
  float voxelSize;
  float mu;
  int32_t maxW;
  float viewFrustum_min;
  float viewFrustum_max;
  int32_t stopIntegratingAtMaxW;
} itm_scene_params;

/* What `new ITMScene<TVoxel,TIndex>(params, useSwapping=false, memoryType)` fixes at compile
 * time in the reference (Objects/ITMScene.h:37-43, ITMVoxelBlockHash.h:35-36,
 * ITMPlainVoxelArray.h:24-37) is a runtime configuration here.  0 = reference default. */
typedef struct itm_scene_config {
  int32_t voxelType;      /* enum itm_voxel_type */
  int32_t indexType;      /* enum itm_index_type */
  int32_t bucketNum;      /* SDF_BUCKET_NUM, power of two   */
  int32_t excessNum;      /* SDF_EXCESS_LIST_SIZE           */
  int32_t localBlockNum;  /* SDF_LOCAL_BLOCK_NUM            */
  int32_t denseSize[3];   /* ITMVoxelArrayInfo::size   (default 512^3)          */
  int32_t denseOffset[3]; /* ITMVoxelArrayInfo::offset (default -256,-256,0)    */
  int32_t denseOffsetSet; /* non-zero: use denseOffset even if it is all zero   */
  int32_t maxRenderingBlocks; /* MAX_RENDERING_BLOCKS (DeviceAgnostic/ITMVisualisationEngine.h:24);
                                 0 = 262144.  Runtime so that the cap path can be tested.       */
  int32_t useSwapping;        /* ITMScene(..., useSwapping, ...) Objects/ITMScene.h:37-43: the scene owns an ITMGlobalCache in host
                                 memory and AllocateSceneFromDepth keeps the swap states (hash index only)                          */
  int32_t transferBlockNum;   /* SDF_TRANSFER_BLOCK_NUM (Utils/ITMLibDefines.h): blocks moved per swapping call; 0 = 0x1000        */
} itm_scene_config;

/* The inputs an engine method takes from `const ITMView*` and `const ITMTrackingState*`:
 * view->depth, view->rgb, view->calib->{intrinsics_d, intrinsics_rgb, trafo_rgb_to_depth} and
 * trackingState->pose_d->GetM()  (Objects/ITMView.h:16-52, Objects/ITMTrackingState.h:18-75). */
typedef struct itm_view {
  const float* depth;      /* float[h*w] metres, <=0 invalid (ITMViewBuilder output)   */
  const uint8_t* rgb;      /* uchar4[h_rgb*w_rgb] RGBA; may be NULL for colourless voxels */
  int32_t w, h;            /* view->depth->noDims */
  int32_t w_rgb, h_rgb;    /* view->rgb->noDims   */
  float M_d[16];           /* trackingState->pose_d->GetM()             */
  float intr_d[4];         /* calib->intrinsics_d.projectionParamsSimple.all   */
  float intr_rgb[4];       /* calib->intrinsics_rgb.projectionParamsSimple.all */
  float rgb_to_depth[16];     /* calib->trafo_rgb_to_depth.calib      (Objects/ITMExtrinsics.h) */
  float rgb_to_depth_inv[16]; /* calib->trafo_rgb_to_depth.calib_inv                            */
} itm_view;

/* Host-visible scalars the reference keeps as members: ITMLocalVBA::lastFreeBlockId,
 * ITMVoxelBlockHash::lastFreeExcessListId, ITMRenderState_VH::noVisibleEntries,
 * ITMRenderState::noFwdProjMissingPoints, ITMPointCloud::noTotalPoints. */
typedef struct itm_counters {
  int32_t lastFreeBlockId;
  int32_t lastFreeExcessListId;
  int32_t noVisibleEntries;
  int32_t noFwdProjMissingPoints;
  int32_t noTotalPoints;
  int32_t noRenderingBlocks;   /* numRenderingBlocks of the last CreateExpectedDepths */
  int32_t noAllocRequests;     /* blocks requested by the last AllocateSceneFromDepth */
  int32_t statusFlags;         /* FATAL conditions: the scene is no longer what the reference would hold.  bit0: a depth pixel needed more ray
                                  steps than the allocation key can number (mu / voxelSize beyond ~2 000), blocks were not requested;
                                  bit1: a bounded wait between workgroups of the visible-list launch expired (a device that does not
                                  run what it was given), the frame was not fused.  Once raised, every call that names the scene
                                  returns ITM_ERR_DEVICE (itm_last_error says which) until itm_reset_scene; itm_get_counters still
                                  fills its output before it returns the error.  Never raised by a healthy frame. */
} itm_counters;

/* buffers addressable by itm_download / itm_upload (parity dumps, checkpoints) */
enum itm_buffer {
  ITM_BUF_HASH_ENTRIES = 0,     /* ITMHashEntry[bucketNum+excessNum]   scene->index.GetEntries() */
  ITM_BUF_EXCESS_LIST = 1,      /* int[excessNum]                      GetExcessAllocationList() */
  ITM_BUF_VOXEL_BLOCKS = 2,     /* TVoxel[localBlockNum*512 | sx*sy*sz] localVBA.GetVoxelBlocks() */
  ITM_BUF_ALLOCATION_LIST = 3,  /* int[localBlockNum]                  localVBA.GetAllocationList() */
  ITM_BUF_VISIBLE_IDS = 4,      /* int[localBlockNum]   renderState_vh->GetVisibleEntryIDs()   */
  ITM_BUF_VISIBLE_TYPE = 5,     /* uchar[noTotalEntries] renderState_vh->GetEntriesVisibleType() */
  ITM_BUF_RANGE_IMAGE = 6,      /* Vector2f[h*w]  renderState->renderingRangeImage  */
  ITM_BUF_RAYCAST_RESULT = 7,   /* Vector4f[h*w]  renderState->raycastResult        */
  ITM_BUF_RAYCAST_IMAGE = 8,    /* Vector4u[h*w]  renderState->raycastImage         */
  ITM_BUF_FORWARD_PROJECTION = 9, /* Vector4f[h*w] renderState->forwardProjection   */
  ITM_BUF_MISSING_POINTS = 10,  /* int[h*w]       renderState->fwdProjMissingPoints */
  ITM_BUF_SWAP_STATES = 11      /* uchar[noTotalEntries] globalCache->GetSwapStates(): ITMHashSwapState::state (scenes with useSwapping) */
};

typedef struct itm_scene itm_scene;               /* ITMScene<TVoxel,TIndex> + engine scratch */
typedef struct itm_render_state itm_render_state; /* ITMRenderState / ITMRenderState_VH       */
typedef void* itm_stream;                         /* hipStream_t */

/* ---- library ------------------------------------------------------------------------------ */
const char* ITM_FN(version)(void);
const char* ITM_FN(last_error)(void);
/* 1 for the product (device pointers), 0 for a host-memory implementation of this ABI. */
int ITM_FN(uses_device_memory)(void);
size_t ITM_FN(voxel_size_bytes)(int voxelType);

/* ---- device memory helpers (so a C / ctypes caller needs no other runtime) ---------------- */
int ITM_FN(dev_malloc)(void** ptr, size_t bytes);
int ITM_FN(dev_free)(void* ptr);
/* page-locked host memory (hipHostMalloc): the source of asynchronous uploads, see itm_depth_stager */
int ITM_FN(host_malloc)(void** ptr, size_t bytes);
int ITM_FN(host_free)(void* ptr);
/* Page-locks host memory the HOST owns (hipHostRegister): an image buffer of the reference (ORUtils::MemoryBlock allocates with `new`)
 * becomes a source / target of asynchronous copies at PCIe speed -- from pageable memory itm_memcpy_h2d is staged through the runtime's
 * bounce buffer and blocks the calling thread.  Registering a range that is registered already is not an error but is TOLD: the call
 * returns ITM_ALREADY_REGISTERED (> 0) and the caller does not own that registration -- it must not unregister it (someone else did the
 * registering, possibly for a different length).  Unregister what you registered before the memory is freed. */
#define ITM_ALREADY_REGISTERED 1
int ITM_FN(host_register)(void* ptr, size_t bytes);
int ITM_FN(host_unregister)(void* ptr);
int ITM_FN(memcpy_h2d)(void* dst_dev, const void* src_host, size_t bytes, itm_stream stream);
int ITM_FN(memcpy_d2h)(void* dst_host, const void* src_dev, size_t bytes, itm_stream stream);
int ITM_FN(stream_synchronize)(itm_stream stream);
/* A stream of the runtime THIS library runs on (hipStreamCreateWithFlags(hipStreamNonBlocking)), for hosts that have no HIP binding of
 * their own -- or whose process holds a second copy of the runtime (a framework that bundles one): a stream must come from the runtime
 * that launches on it.  Every `itm_stream` argument also accepts a hipStream_t the host created itself, or NULL (the null stream). */
int ITM_FN(stream_create)(itm_stream* out);
int ITM_FN(stream_destroy)(itm_stream stream);
int ITM_FN(set_device)(int device);

/* (Test hooks -- itm_debug_set and its keys, the division and cull probes -- are declared in itm_debug.h, which only tests include.) */

/* ---- scene -------------------------------------------------------------------------------- */
/* new ITMScene<TVoxel,TIndex>(sceneParams,false,memType)  Objects/ITMScene.h:37-43 ; also
 * allocates the engine scratch of ITMSceneReconstructionEngine_CPU ctor
 * (DeviceSpecific/CPU/ITMSceneReconstructionEngine_CPU.cpp:9-15). Does NOT reset. */
int ITM_FN(scene_create)(const itm_scene_config* cfg, const itm_scene_params* params,
                         itm_scene** out);
int ITM_FN(scene_destroy)(itm_scene* scene);
int ITM_FN(scene_get_config)(const itm_scene* scene, itm_scene_config* cfg,
                             itm_scene_params* params);

/* ITMSceneReconstructionEngine::ResetScene            Engine/ITMSceneReconstructionEngine.h:35
 * (CPU: DeviceSpecific/CPU/ITMSceneReconstructionEngine_CPU.cpp:24-45 hash, :301-312 dense) */
int ITM_FN(reset_scene)(itm_scene* scene, itm_stream stream);

/* ITMVisualisationEngine::CreateRenderState(imgSize)   Engine/ITMVisualisationEngine.h:79
 * (CPU: DeviceSpecific/CPU/ITMVisualisationEngine_CPU.cpp:18-32; ITMRenderState ctor fills the
 * range image with (vf_min, vf_max), Objects/ITMRenderState.h:51-75) */
int ITM_FN(render_state_create)(const itm_scene* scene, int w, int h, itm_render_state** out);
int ITM_FN(render_state_destroy)(itm_render_state* rs);

/* ---- the four calls of a frame ----------------------------------------------------------------------------------------------
 * ITMMainEngine::ProcessFrame reaches the engines as AllocateSceneFromDepth -> IntegrateIntoScene (Engine/ITMDenseMapper.cpp:50-57)
 * -> CreateExpectedDepths -> CreateICPMaps (Engine/ITMTrackingController.cpp:30-46).  By DEFAULT each of the entry points below
 * enqueues its kernels on `stream` before it returns (8 launches per frame), like the reference's CUDA engines on their stream.
 *
 * itm_scene_set_deferred_fusion(scene, 1) lets the library fuse the sequence (hash scenes): the first three calls then RECORD their
 * arguments (after checking everything they could be refused for) and return with NOTHING enqueued; itm_create_icp_maps for the same
 * view, pose and stream completes the sequence and launches the fused frame of itm_process_frame (5 launches instead of 8).  Any
 * other call of this library that names the scene or the render state, any copy / view-builder call of this library that writes an
 * image the recorded view reads, itm_stream_synchronize on the recording stream, itm_flush and itm_render_state_destroy launch what
 * was recorded first, call by call.  Results are identical either way.  The contract a host accepts by switching it on:
 *   - the images of the view are read when the sequence is LAUNCHED: they stay valid and unchanged until then -- a host that
 *     overwrites them with its OWN kernels or copies between AllocateSceneFromDepth and CreateICPMaps calls itm_flush first;
 *   - stream order only holds from the launching call on: before a hipEventRecord / hipStreamWaitEvent / kernel of the host's own
 *     that is meant to run behind one of the first three calls, and before it uses a raw pointer from itm_buffer_ptr, the host calls
 *     itm_flush;
 *   - the four calls of one frame come from one thread (calls for different scenes may come from different threads).
 * The reference's callers meet all three (the view is built before the tracker runs, Engine/ITMMainEngine.cpp:111-127, and results
 * are read through the engines), so the adapters (include/itm_hip_engines.hpp, integration/ITMEngines_HIP.h) switch it on.
 * Environment: ITM_DEFERRED_FUSION=1 switches it on for every new scene, ITM_NO_DEFERRED_FUSION=1 off whatever the host asked for. */
int ITM_FN(scene_set_deferred_fusion)(itm_scene* scene, int on);
int ITM_FN(flush)(itm_scene* scene, itm_render_state* rs, itm_stream stream);   /* scene == rs == NULL: everything recorded on `stream` */

/* ITMSceneReconstructionEngine::AllocateSceneFromDepth(scene, view, trackingState, renderState,
 * onlyUpdateVisibleList)                               Engine/ITMSceneReconstructionEngine.h:40
 * (CPU hash :116-291, dense :314-317 no-op)
 * The render state need not have the view's size, as in the reference: ITMMainEngine allocates from the depth image through the
 * render state of the TRACKED image, which is the colour camera's for TRACKER_COLOR (Engine/ITMMainEngine.cpp:50-52).  A call whose
 * sizes differ is always launched at once, never recorded for the fused frame (itm_scene_set_deferred_fusion). */
int ITM_FN(allocate_scene_from_depth)(itm_scene* scene, const itm_view* view,
                                      itm_render_state* rs, int onlyUpdateVisibleList,
                                      itm_stream stream);

/* ITMSceneReconstructionEngine::IntegrateIntoScene     Engine/ITMSceneReconstructionEngine.h:46
 * (CPU hash :47-114, dense :319-369) */
int ITM_FN(integrate_into_scene)(itm_scene* scene, const itm_view* view, itm_render_state* rs,
                                 itm_stream stream);

/* IITMVisualisationEngine::FindVisibleBlocks(pose, intrinsics, renderState)          :39
 * (CPU :39-77; dense: no-op :34-37) */
int ITM_FN(find_visible_blocks)(const itm_scene* scene, const float M[16], const float intr[4],
                                itm_render_state* rs, itm_stream stream);

/* IITMVisualisationEngine::CreateExpectedDepths(pose, intrinsics, renderState)       :45
 * (CPU hash :93-152, dense :79-91) */
int ITM_FN(create_expected_depths)(const itm_scene* scene, const float M[16],
                                   const float intr[4], itm_render_state* rs, itm_stream stream);

/* IITMVisualisationEngine::RenderImage(pose, intrinsics, renderState, outputImage, type) :49
 * (CPU :190-240, :356-368).  out_rgba: uchar4[h*w] device pointer; NULL = rs->raycastImage. */
int ITM_FN(render_image)(const itm_scene* scene, const float M[16], const float intr[4],
                         itm_render_state* rs, uint8_t* out_rgba, int type, itm_stream stream);

/* IITMVisualisationEngine::FindSurface(pose, intrinsics, renderState)               :53
 * (CPU :370-381): raycast only, result in rs->raycastResult. */
int ITM_FN(find_surface)(const itm_scene* scene, const float M[16], const float intr[4],
                         itm_render_state* rs, itm_stream stream);

/* IITMVisualisationEngine::CreatePointCloud(view, trackingState, renderState, skipPoints) :58
 * (CPU :242-264, :424-462).  locations/colours: Vector4f[h*w] = trackingState->pointCloud;
 * count is left in itm_counters::noTotalPoints. */
int ITM_FN(create_point_cloud)(const itm_scene* scene, const itm_view* view,
                               itm_render_state* rs, int skipPoints, float* locations,
                               float* colours, itm_stream stream);

/* IITMVisualisationEngine::CreateICPMaps(view, trackingState, renderState)          :63
 * (CPU :266-287).  points/normals: Vector4f[h*w] = trackingState->pointCloud->locations /
 * ->colours.  Grey rendering goes to rs->raycastImage. */
int ITM_FN(create_icp_maps)(const itm_scene* scene, const itm_view* view, itm_render_state* rs,
                            float* points, float* normals, itm_stream stream);

/* IITMVisualisationEngine::ForwardRender(view, trackingState, renderState)          :70
 * (CPU :289-354) */
int ITM_FN(forward_render)(const itm_scene* scene, const itm_view* view, itm_render_state* rs,
                           itm_stream stream);

/* The per-frame call sequence of ITMMainEngine::ProcessFrame after the view is built
 * (Engine/ITMMainEngine.cpp:123-126): ITMDenseMapper::ProcessFrame (Engine/ITMDenseMapper.cpp:
 * 50-65: AllocateSceneFromDepth + IntegrateIntoScene) followed by
 * ITMTrackingController::Prepare with requiresFullRendering (Engine/ITMTrackingController.cpp:
 * 31-35: CreateExpectedDepths + CreateICPMaps).  Results are identical to issuing the four calls
 * one after another; this entry point only removes launch overhead.  itm_process_frame and
 * itm_process_frame_ahead require view (and next view) and render state of the SAME size -- the
 * fused launches index the render state's per-pixel buffers by depth pixel -- and return
 * ITM_ERR_INVALID otherwise; the four separate calls have no such rule. */
int ITM_FN(process_frame)(itm_scene* scene, const itm_view* view, itm_render_state* rs,
                          float* points, float* normals, itm_stream stream);
/* The same frame, for a host that already HAS the next frame (an offline sequence, a buffered sensor): `next` (may be NULL) is the view
 * the next call will be made for.  Its per-pixel block requests -- the first stage of its AllocateSceneFromDepth, which only reads the
 * table as this frame's allocation leaves it -- ride in this frame's last launch, beside the ICP maps; the next frame then starts with
 * its visible-list launch (4 launches per frame instead of 5).  Results are identical to itm_process_frame, frame by frame.  Contract:
 * the next allocation on this render state (itm_process_frame[_ahead] or itm_allocate_scene_from_depth) must be for exactly that view
 * (same depth pointer, size, pose, intrinsics), and the scene must not be reset or have its table uploaded in between, else that
 * allocation returns ITM_ERR_INVALID (the render state's visible types then hold the marks of the abandoned requests: recreate it). */
int ITM_FN(process_frame_ahead)(itm_scene* scene, const itm_view* view, const itm_view* next, itm_render_state* rs,
                                float* points, float* normals, itm_stream stream);
/* While the requests of `next` are pending the render state's visible types carry their marks and the scene's request keys are in
 * use: a download / upload / save of the visible list, itm_find_visible_blocks on that render state and an allocation through ANOTHER
 * render state of the scene return ITM_ERR_INVALID.  itm_cancel_ahead abandons the requests: keys and counters return to "no
 * request", the marks are cleared and the entries of the visible list read 3 -- the state of the reference's AllocateSceneFromDepth
 * right after its "previous list -> 3" loop (CPU :160-161) -- so that any allocation may follow.  itm_reset_scene cancels by itself. */
int ITM_FN(cancel_ahead)(itm_scene* scene, itm_render_state* rs, itm_stream stream);

/* ---- frame de-integration: takes one fused depth frame back out of the TSDF ------------------------------------------------------
 * Not a reference operation: the reference can fuse a frame and cannot un-fuse it.  A host whose poses are corrected after the fact
 * (a loop closure, a batch optimisation, a pose verdict that turned out wrong) removes the frame's contribution with this call and
 * fuses it again under the new pose with the two calls above ("A pose update").
 *
 * The call visits exactly the voxels itm_integrate_into_scene visits for the same arguments: in a hash scene the blocks on the render
 * state's visible list with ptr >= 0, in a dense scene the whole array.  How the list got there is the caller's business:
 * itm_find_visible_blocks for the old pose, itm_allocate_scene_from_depth(..., onlyUpdateVisibleList = 1, ...), or the list as saved
 * when the frame was fused, uploaded again (ITM_BUF_VISIBLE_IDS + itm_set_counters).
 *
 * Per voxel (tests/defusion_terms.py transcribes this; the kernels reproduce it bit for bit).  The projection, the depth pixel, eta
 * and the exit eta < -mu are those of computeUpdatedVoxelDepthInfo, operation for operation: a voxel the integration would not write
 * is not touched.  stopIntegratingAtMaxW is not consulted (keepSaturated below stands for it).  For a voxel the integration would
 * write, with oldW = w_depth, oldF = SDF_valueToFloat(sdf), obs = MIN(1, eta / mu):
 *   oldW == 0                        untouched; counted in `unobserved`
 *   oldW >= maxW and keepSaturated   untouched, colour included; counted in `saturated` (its true count of observations is unknown)
 *   oldW == 1                        sdf = SDF_initialValue(), w_depth = 0; counted in `reset`
 *   otherwise                        F' = ((float)oldW * oldF - obs) / (float)(oldW - 1): product, difference and quotient each rounded
 *                                    once, IEEE division, nothing contracted; F' = MAX(-1, MIN(1, F')) with the reference's macros, a
 *                                    changed value counted in `clamped` (removing an observation that was never added can leave
 *                                    [-1, 1], which the short encoding cannot hold); sdf = SDF_floatToValue(F'), w_depth = oldW - 1.
 *                                    A saturated voxel without keepSaturated is treated as a count of oldW.
 *   `touched` counts the voxels whose depth part was written (the last two rows).
 * Colour voxel types: the gate is the integration's -- !(eta > mu || fabs(eta / mu) > 0.25) with the eta the depth part returned (-1
 * where it left early), then the colour image's bounds -- and a voxel kept as saturated above is skipped.  With oldWc = w_color,
 * m = the bilinear colour / 255, oc = clr / 255:  oldWc == 0, or oldWc >= (uchar)maxW with keepSaturated: untouched;  oldWc == 1:
 * clr = 0, w_color = 0 (`colourReset`);  otherwise c' = (oc * oldWc - m) / (oldWc - 1) per channel, x = c' * 255 rounded half away from
 * zero and clamped to [0, 255], w_color = oldWc - 1.  `coloured` counts the voxels whose colour part was written (resets included).
 *
 * cfg == NULL: keepSaturated = stopIntegratingAtMaxW of the scene.  keepSaturated is 0 or 1.
 * stats (host, may be NULL): integer sums, independent of order.  blocks: visible-list entries with a block (0 in a dense scene);
 * visited: voxels visited.  With `stats` the call synchronises `stream` once, at its end; without it nothing is read back.
 *
 * What the operation is NOT.  It is the exact inverse in the weights below saturation, and in the sdf only up to the stored encoding:
 * fuse-then-unfuse returns a short sdf within 4 steps of 1 / 32767 and a float sdf within 2^-20 (tests/test_defusion_terms.py derives
 * both), and colours within the rounding of a uchar times the weight.  A weight that was capped at maxW has forgotten how many
 * observations it stands for.  A block allocated AFTER the frame was fused but inside that frame's frustum and band loses an
 * observation it never got; a caller that minds passes the frame's saved visible list.
 *
 * Refusals, all before any launch, each ITM_ERR_INVALID with the scene unchanged: everything itm_integrate_into_scene refuses (a NULL
 * argument, a NULL depth image, a render state of another scene, colour voxels without an rgb image); keepSaturated outside {0, 1}.
 * Calls recorded for the fused frame (itm_scene_set_deferred_fusion) are launched first, as for every entry point naming the scene. */
typedef struct itm_deintegrate_config {
  int32_t keepSaturated;        /* 1: a voxel whose weight has reached maxW stays as it is */
  int32_t reserved[3];
} itm_deintegrate_config;       /* 16 bytes */
typedef struct itm_deintegrate_stats {
  int32_t blocks, visited, touched, reset, unobserved, saturated, clamped, coloured, colourReset;
  int32_t reserved[7];
} itm_deintegrate_stats;        /* 64 bytes */
int ITM_FN(deintegrate_from_scene)(itm_scene* scene, const itm_view* view, itm_render_state* rs, const itm_deintegrate_config* cfg,
                                   itm_deintegrate_stats* stats, itm_stream stream);

/* ---- view builder (the step before the path) -------------------------------- */
/* convertDepthAffineToFloat  DeviceAgnostic/ITMViewBuilder.h:22-28 */
int ITM_FN(convert_depth_affine)(const int16_t* raw, float* depth_out, int w, int h, float a,
                                 float b, itm_stream stream);
/* convertDisparityToDepth    DeviceAgnostic/ITMViewBuilder.h:7-20 */
int ITM_FN(convert_disparity)(const int16_t* raw, float* depth_out, int w, int h, float c0,
                              float c1, float fx_depth, itm_stream stream);

/* ITMViewBuilder::DepthFiltering  Engine/ITMViewBuilder.h:32, DeviceSpecific/CPU/ITMViewBuilder_CPU.cpp:119-130,
 * filterDepth DeviceAgnostic/ITMViewBuilder.h:30-52: one 5x5 bilateral pass; `out` is cleared, then pixels
 * 2 <= x < w-2, 2 <= y < h-2 are written (invalid input pixel -> -1).  in != out. */
int ITM_FN(filter_depth)(const float* in, float* out, int w, int h, itm_stream stream);
/* ITMViewBuilder::ComputeNormalAndWeights  Engine/ITMViewBuilder.h:33, ..._CPU.cpp:132-145, computeNormalAndWeight
 * DeviceAgnostic/ITMViewBuilder.h:55-117.  normals: float4[h*w], sigmaZ: float[h*w]; only the interior
 * (2-pixel border excluded) is written, as in the reference.  `intr` = projectionParamsSimple.all (fx,fy,cx,cy). */
int ITM_FN(compute_normal_and_weights)(const float* depth, float* normals, float* sigmaZ, int w, int h,
                                       const float intr[4], itm_stream stream);
/* ITMViewBuilder::UpdateView(view, rgb, rawDepth, useBilateralFilter, modelSensorNoise)  ..._CPU.cpp:14-63, for a raw
 * depth frame already in device memory: conversion by calibration type (0 = TRAFO_KINECT disparity, 1 = TRAFO_AFFINE,
 * Objects/ITMDisparityCalib.h:24-29), optionally the five bilateral passes (ping-pong with `scratch`, float[h*w]) and
 * the normal / uncertainty images (normals, sigmaZ may be NULL when modelSensorNoise == 0). */
int ITM_FN(update_view)(const int16_t* raw, int w, int h, int calibType, float c0, float c1, const float intr_d[4],
                        int useBilateralFilter, int modelSensorNoise, float* depth_out, float* scratch,
                        float* normals, float* sigmaZ, itm_stream stream);

/* ---- colour maps of the display path (ITMMainEngine::GetImage, Engine/ITMMainEngine.cpp:148-160) ----------------------
 * IITMVisualisationEngine::DepthToUchar4 / WeightToUchar4 / NormalToUchar4  Engine/ITMVisualisationEngine.cpp:7-57, :82-107,
 * :59-79 -- host loops there, kernels here.  All pointers are DEVICE pointers: src float[h*w], src4 float4[h*w], dst_rgba
 * uchar4[h*w].  The result is the reference's byte for byte; every output pixel is written (0 where the reference leaves its
 * cleared image untouched: the caller clears nothing).  Depth: the pixels > 0 are scaled between their minimum and maximum and
 * coloured by the reference's ramp, alpha 255; weight: red / green from min / value, alpha 0; normal: 0.3 + (c + 1) * 0.35 per
 * component where w >= 0, alpha 0.  Where the reference's float -> uchar conversion is undefined (a value outside [0, 256): a
 * normal component beyond +-1, garbage) the value saturates to 0 / 255 and NaN gives 0.
 * Stream-ordered like the view-builder calls, at most two launches, no allocation after the first call on a stream and nothing
 * returns to the host: the limits stay in device memory, in words that belong to the call's stream. */
int ITM_FN(depth_to_uchar4)(const float* src, uint8_t* dst_rgba, int w, int h, itm_stream stream);
int ITM_FN(weight_to_uchar4)(const float* src, uint8_t* dst_rgba, int w, int h, itm_stream stream);
int ITM_FN(normal_to_uchar4)(const float* src4, uint8_t* dst_rgba, int w, int h, itm_stream stream);

/* ---- raw frames from the host: the first statement of ITMViewBuilder_CUDA::UpdateView, shortImage->SetFrom(rawDepthImage, CPU_TO_CUDA)
 * (Engine/DeviceSpecific/CUDA/ITMViewBuilder_CUDA.cu:53), a synchronous copy there.  A stager owns `slots` device images of w x h
 * shorts and a copy stream: itm_depth_stager_upload puts a frame (PINNED host memory) on the copy stream and returns at once -- up to
 * slots - 1 frames ahead of the one being fused --, itm_depth_stager_acquire makes the frame's stream wait for the OLDEST uploaded frame
 * and returns its device image (the `raw` argument of itm_update_view), itm_depth_stager_release says that everything submitted to
 * that stream so far is what read it: the slot is overwritten only behind that work.  One acquire / release pair at a time, frames leave
 * in the order they were uploaded.  Host-side object, not thread safe. */
typedef struct itm_depth_stager itm_depth_stager;
int ITM_FN(depth_stager_create)(int w, int h, int slots, itm_depth_stager** out);
int ITM_FN(depth_stager_destroy)(itm_depth_stager* g);
int ITM_FN(depth_stager_upload)(itm_depth_stager* g, const int16_t* pinned_host);
int ITM_FN(depth_stager_acquire)(itm_depth_stager* g, itm_stream stream, const int16_t** device_image);
/* itm_depth_stager_upload returns BEFORE the copy stream has read the host buffer: a pinned buffer may be rewritten only once
 * *busy == 0 here (no upload still in flight; a query, never a wait), or after its frame has been acquired and the acquiring stream
 * synchronised.  *waiting = uploaded frames not acquired yet.  Either pointer may be NULL. */
int ITM_FN(depth_stager_pending)(itm_depth_stager* g, int* waiting, int* busy);
int ITM_FN(depth_stager_release)(itm_depth_stager* g, itm_stream stream);
/* The copy may also CONVERT: after itm_depth_stager_set_conversion (calibType, c0, c1 and fx = intr_d[0] as in itm_update_view; call it
 * while no frame waits in the ring) every uploaded frame is also turned into the float depth image of itm_update_view's first step
 * (convertDisparityToDepth / convertDepthAffineToFloat, DeviceAgnostic/ITMViewBuilder.h:7-28) by the copy itself, and
 * itm_depth_stager_acquire_depth hands out that image (and, if asked, the raw one) instead of itm_depth_stager_acquire.  For a view
 * without bilateral filter and noise model it IS view->depth -- no conversion launch on the frame's stream --; it stays valid until
 * the release, which therefore comes after the LAST launch that reads the frame's depth. */
int ITM_FN(depth_stager_set_conversion)(itm_depth_stager* g, int calibType, float c0, float c1, float fx);
int ITM_FN(depth_stager_acquire_depth)(itm_depth_stager* g, itm_stream stream, const int16_t** raw_image, const float** depth_image);

/* ---- on-disk input formats of the view builder's sources (host memory, no device work) -------------------------
 * Depth: PGM "P5" (or ASCII "P2") with maxval > 256: 16-bit samples stored BIG-endian, swapped on load
 * (Utils/FileUtils.cpp:377-421); colour: PPM "P6" / "P3" -> RGBA with alpha 255 (:324-375); writers :251-322
 * (the float writer stores millimetres WITHOUT the byte swap, as the reference does).  Calibration text:
 * ITMLib/Utils/ITMCalibIO.cpp:10-101 (rgb intrinsics, depth intrinsics, 3x4 rgb->depth extrinsics, disparity calib;
 * "0 0" selects affine 1/1000).  All pointers are host pointers.  Return ITM_OK or ITM_ERR_INVALID. */
typedef struct itm_rgbd_calib {
  float size_rgb[2], intr_rgb[4];          /* sizeX sizeY ; fx fy cx cy                                  */
  float size_d[2], intr_d[4];
  float rgb_to_depth[16];                  /* trafo_rgb_to_depth.calib, column-major                    */
  float rgb_to_depth_inv[16];              /* .calib_inv (transpose / -R^T t, Objects/ITMExtrinsics.h:32-42) */
  int32_t disparityType;                   /* 0 = TRAFO_KINECT, 1 = TRAFO_AFFINE                        */
  float disparityParams[2];
} itm_rgbd_calib;
int ITM_FN(read_depth_image)(const char* path, int16_t* dst, int capacityPixels, int* w, int* h);
int ITM_FN(read_rgb_image)(const char* path, uint8_t* dst_rgba, int capacityPixels, int* w, int* h);
int ITM_FN(write_depth_image)(const char* path, const int16_t* src, int w, int h);
int ITM_FN(write_rgb_image)(const char* path, const uint8_t* src_rgba, int w, int h);
int ITM_FN(write_float_depth_image)(const char* path, const float* src, int w, int h);
int ITM_FN(read_rgbd_calib)(const char* path, itm_rgbd_calib* out);

/* ---- ICP depth tracker (the step after the path) -------------------------------------
 * Consumes the points / normals maps CreateICPMaps writes.  Device-specific half of the reference tracker:
 *   ITMLowLevelEngine::FilterSubsampleWithHoles (float)  DeviceAgnostic/ITMLowLevelEngine.h:26-47,
 *                                                         DeviceSpecific/CPU/ITMLowLevelEngine_CPU.cpp:50-62
 *   ITMDepthTracker_CPU::ComputeGandH                     DeviceSpecific/CPU/ITMDepthTracker_CPU.cpp:15-79,
 *                                                         DeviceAgnostic/ITMDepthTracker.h:8-106
 * and the host Levenberg-Marquardt loop around it:
 *   ITMDepthTracker::TrackCamera                          Engine/ITMDepthTracker.cpp:149-200 (+ :79-147, ITMPose::Coerce) */
enum itm_tracker_iteration {               /* TrackerIterationType, Utils/ITMLibDefines.h:277-283 */
  ITM_TRACKER_ITERATION_ROTATION = 1,
  ITM_TRACKER_ITERATION_TRANSLATION = 2,
  ITM_TRACKER_ITERATION_BOTH = 3,
  ITM_TRACKER_ITERATION_NONE = 4
};
typedef struct itm_tracker_config {        /* ITMLibSettings fields the tracker factory passes on */
  int32_t noHierarchyLevels;               /* <= 8; default 5                                  */
  int32_t trackingRegime[8];               /* per level, level 0 = full resolution; default B B R R R */
  int32_t noICPRunTillLevel;               /* default 0                                        */
  float distThresh;                        /* depthTrackerICPThreshold, default 0.1*0.1        */
  float terminationThreshold;              /* depthTrackerTerminationThreshold, default 1e-3   */
} itm_tracker_config;
typedef struct itm_tracker_gh {
  float f;                                 /* sqrt(sum b^2)/n, or 1e5 when n <= 100            */
  float nabla[6];
  float hessian[36];                       /* r + c*6; entries outside the active block are 0  */
  int32_t noValidPoints;
} itm_tracker_gh;
/* out: float[(h_in/2)*(w_in/2)] */
int ITM_FN(filter_subsample_with_holes)(const float* in, int w_in, int h_in, float* out, itm_stream stream);
/* Synchronises `stream` (the host loop needs the sums).  Sums are accumulated by a fixed-order reduction
 * tree in double precision: deterministic, and within float rounding of the reference's sequential sum. */
int ITM_FN(tracker_compute_g_and_h)(const float* depth, int w, int h, const float viewIntr[4],
                                    const float* pointsMap, const float* normalsMap, int sceneW, int sceneH,
                                    const float sceneIntr[4], const float approxInvPose[16],
                                    const float scenePose[16], float distThresh, int iterationType,
                                    itm_tracker_gh* out, itm_stream stream);
/* ITMDepthTracker::TrackCamera: view->depth / intr_d / M_d (initial pose_d), the ICP maps of the previous
 * frame and the pose they were rendered from (pose_pointCloud); writes the refined pose_d to M_d_out. */
int ITM_FN(track_camera)(const itm_tracker_config* cfg, const itm_view* view, const float* pointsMap,
                         const float* normalsMap, const float scenePose[16], float M_d_out[16],
                         itm_stream stream);

/* The tracker as an object (ITMDepthTracker owns its hierarchy and reduction buffers, Engine/ITMDepthTracker.cpp:18-44): one
 * handle = the device partials, the pinned result records and the depth pyramid of ONE tracker.  Calls on a handle are
 * serialised by the handle; different handles (e.g. one per depth stream / HIP stream / host thread) are independent.  The
 * two handle-less entry points above use a handle private to the calling host thread.  A reduction that does not arrive
 * (hung or failed kernel) ends the call with ITM_ERR_DEVICE after a bounded wait instead of stalling the host. */
typedef struct itm_tracker itm_tracker;
int ITM_FN(tracker_create)(itm_tracker** out);
int ITM_FN(tracker_destroy)(itm_tracker* tracker);
int ITM_FN(tracker_g_and_h)(itm_tracker* tracker, const float* depth, int w, int h, const float viewIntr[4],
                            const float* pointsMap, const float* normalsMap, int sceneW, int sceneH,
                            const float sceneIntr[4], const float approxInvPose[16], const float scenePose[16],
                            float distThresh, int iterationType, itm_tracker_gh* out, itm_stream stream);
int ITM_FN(tracker_track_camera)(itm_tracker* tracker, const itm_tracker_config* cfg, const itm_view* view,
                                 const float* pointsMap, const float* normalsMap, const float scenePose[16],
                                 float M_d_out[16], itm_stream stream);

/* ---- weighted ICP tracker (this fork's ITMWeightedICPTracker, TRACKER_WICP) on the same handle -------------------------------------
 * The ICP evaluation with a per-pixel weight w = sigmaZ > 0 ? 0.0012f / sigmaZ * 0.5f + 0.5f : 0 from the view's uncertainty image
 * (ComputeNormalAndWeights: -1 where no normal, the 2-pixel border unwritten); b from the unweighted normal, f from sum b^2 w^2,
 * nabla = sum w b A, H = sum w^2 A A^T; a pixel of weight 0 still counts in noValidPoints.  Replaces:
 *   ITMWeightedICPTracker_CPU::ComputeGandH    DeviceSpecific/CPU/ITMWeightedICPTracker_CPU.cpp:14-86,
 *                                              DeviceAgnostic/ITMWeightedICPTracker.h:10-107 (computePerPointGH_wICP)
 *   ITMWeightedICPTracker::TrackCamera & co.   Engine/ITMWeightedICPTracker.cpp:10-45,57-100,102-191
 * The handle adds a sigmaZ pyramid (allocated on first use) to its depth pyramid and reduction records.
 * weighted_g_and_h: one level's sums, `weight` = that level's sigmaZ image (float[h*w], device).  Synchronises `stream`. */
int ITM_FN(tracker_weighted_g_and_h)(itm_tracker* tracker, const float* depth, const float* weight, int w, int h,
                                     const float viewIntr[4], const float* pointsMap, const float* normalsMap, int sceneW,
                                     int sceneH, const float sceneIntr[4], const float approxInvPose[16],
                                     const float scenePose[16], float distThresh, int iterationType, itm_tracker_gh* out,
                                     itm_stream stream);
/* TrackCamera: pyramids of view->depth and sigmaZ (the view's uncertainty image, float[h*w], device; its border must be <= 0),
 * coarse to fine from view->M_d, undamped Gauss-Newton steps (the 3x3 block on rotation- or translation-only levels); writes the
 * refined, coerced pose_d to M_d_out.  Where the weighted system is singular (e.g. every weight 0) the level ends without a step.
 * Synchronises `stream`. */
int ITM_FN(tracker_weighted_track_camera)(itm_tracker* tracker, const itm_tracker_config* cfg, const itm_view* view,
                                          const float* sigmaZ, const float* pointsMap, const float* normalsMap,
                                          const float scenePose[16], float M_d_out[16], itm_stream stream);

/* ---- colour (photometric) tracker ------------------------------------------------------------------
 * Aligns the rgb image of a view with the coloured point cloud CreatePointCloud wrote for the previous pose.  Device-specific half:
 *   ITMColorTracker::PrepareForEvaluation           Engine/ITMColorTracker.cpp:49-68 (CopyImage, FilterSubsample, GradientX / Y:
 *                                                   DeviceAgnostic/ITMLowLevelEngine.h:7-24,73-123, CPU/ITMLowLevelEngine_CPU.cpp:35-104)
 *   ITMColorTracker_CPU::F_oneLevel / G_oneLevel    DeviceSpecific/CPU/ITMColorTracker_CPU.cpp:14-101,
 *                                                   DeviceAgnostic/ITMColorTracker.h (getColorDifferenceSq, computePerPointGH_rt_Color)
 * and the host Levenberg-Marquardt loop around it:
 *   ITMColorTracker::TrackCamera / minimizeLM / ApplyDelta   Engine/ITMColorTracker.cpp:25-47,70-234
 * One handle owns the rgb pyramid, its gradients and the reduction buffers of ONE tracker; calls on a handle are serialised by the
 * handle, different handles are independent (as itm_tracker).  Sums are added in the fixed-order double-precision tree of the ICP
 * tracker: deterministic, within float rounding of the reference's sequential float sums, the valid count exact. */
typedef struct itm_colour_tracker itm_colour_tracker;
typedef struct itm_colour_eval {
  float f;                 /* F_oneLevel: sum of squared colour differences * noTotalPoints / noValidPoints; 0x7f800000 (MY_INF, read as
                              the float 2139095040) when nothing is valid                                                              */
  int32_t noValidPoints;   /* countedPoints_valid                                                                                    */
  int32_t numPara;         /* numParameters(): 3 for ROTATION, 6 for TRANSLATION and BOTH                                             */
  float nabla[6];          /* G_oneLevel gradient (numPara entries), scaled as f; zero unless asked for                             */
  float hessian[36];       /* G_oneLevel hessian, hessian[para + col * numPara] (numPara^2 entries, symmetric)                        */
} itm_colour_eval;
int ITM_FN(colour_tracker_create)(itm_colour_tracker** out);
int ITM_FN(colour_tracker_destroy)(itm_colour_tracker* tracker);
/* PrepareForEvaluation: level 0 = a copy of view->rgb (w_rgb x h_rgb), level i = FilterSubsample of level i-1 (floor halves),
 * gradients X / Y of every level (short4, borders 0).  levels: 1..8. */
int ITM_FN(colour_tracker_prepare)(itm_colour_tracker* tracker, const itm_view* view, int levels, itm_stream stream);
/* Synchronous read-back of one prepared level: rgb uchar4[h*w], gx / gy short4[h*w] (host pointers, each may be NULL). */
int ITM_FN(colour_tracker_read_level)(itm_colour_tracker* tracker, int level, uint8_t* rgb, int16_t* gx, int16_t* gy, int* w, int* h,
                                      itm_stream stream);
/* F_oneLevel (and G_oneLevel at the same pose when wantGH != 0, from the same pass) on a prepared level: locations / colours =
 * trackingState->pointCloud (Vector4f[noTotalPoints], device), pose = the rgb camera's world->camera matrix, intrinsics =
 * view->intr_rgb / 2^level of the last prepare.  Synchronises `stream`. */
int ITM_FN(colour_tracker_evaluate)(itm_colour_tracker* tracker, int level, const float* locations, const float* colours,
                                    int noTotalPoints, const float pose[16], int iterationType, int wantGH, itm_colour_eval* out,
                                    itm_stream stream);
/* ITMColorTracker::TrackCamera: prepares the pyramid from view->rgb (cfg->noHierarchyLevels levels, cfg->trackingRegime per level;
 * noICPRunTillLevel / distThresh / terminationThreshold are not used by this tracker), tracks from view->M_d through the
 * rgb -> depth extrinsics, writes the refined and coerced pose_d to M_d_out.  The point count is read on the device from rs
 * (itm_counters::noTotalPoints left by create_point_cloud; no extra host round trip), or is noTotalPoints when rs is NULL.
 * ITM_TRACKER_ITERATION_NONE is rejected (the reference leaves the step undefined).  Synchronises `stream`. */
int ITM_FN(colour_tracker_track_camera)(itm_colour_tracker* tracker, const itm_tracker_config* cfg, const itm_view* view,
                                        const itm_render_state* rs, const float* locations, const float* colours, int noTotalPoints,
                                        float M_d_out[16], itm_stream stream);
/* Evaluations (each one pass over the point cloud) of the last colour_tracker_track_camera call on this handle. */
int ITM_FN(colour_tracker_evaluations)(const itm_colour_tracker* tracker, int* out);

/* ---- Ren SDF tracker ----------------------------------------------------------------------------------------------
 * Registers the depth image of a view directly against the fused TSDF volume of a scene (any voxel type, hash or dense index).
 * Device-specific half: DeviceSpecific/CPU/ITMRenTracker_CPU.cpp (UnprojectDepthToCam, F_oneLevel, G_oneLevel) with
 * DeviceAgnostic/ITMRenTracker.h; host loop: ITMRenTracker::TrackCamera (Engine/ITMRenTracker.cpp).  One handle owns the point
 * image and the reduction buffers of ONE tracker; calls on a handle are serialised by the handle.  Sums are added in the
 * fixed-order double-precision tree of the ICP tracker: deterministic, within float rounding of the reference's sequential float
 * sums, the valid count exact.  The scene is read as the calls before left it: engine calls the library recorded but has not
 * launched yet (itm_scene_set_deferred_fusion) are launched first. */
typedef struct itm_ren_tracker itm_ren_tracker;
typedef struct itm_ren_eval {
  float f;                 /* F_oneLevel: minus the sum over points (w > -1) of 4 e / (e + 1)^2, e = exp(-6 dt); dt == 1 adds 0   */
  int32_t noValidPoints;   /* G_oneLevel: points with a Jacobian (sdf found and != 1 at the point and its six axis neighbours)     */
  float nabla[6];          /* G_oneLevel gradient: minus the sum of the Jacobians (translation, then MRP rotation)               */
  float hessian[36];       /* G_oneLevel hessian, hessian[r + c * 6] (symmetric); nabla / hessian / count zero unless asked for    */
} itm_ren_eval;
/* ITMRenTracker constructor / destructor (Engine/ITMRenTracker.cpp) */
int ITM_FN(ren_tracker_create)(itm_ren_tracker** out);
int ITM_FN(ren_tracker_destroy)(itm_ren_tracker* tracker);
/* PrepareForEvaluation, level 0 (Engine/ITMRenTracker.cpp): UnprojectDepthToCam of view->depth (w x h) with view->intr_d --
 * Vector4f (x z / fx - cx z / fx, y z / fy - cy z / fy, z, 1), (0, 0, 0, -1) where depth <= 0.  The coarser level the reference
 * builds is never read and is not built.  points_host (may be NULL): Vector4f[h*w] copied back synchronously. */
int ITM_FN(ren_tracker_prepare)(itm_ren_tracker* tracker, const itm_view* view, float* points_host, itm_stream stream);
/* ITMRenTracker_CPU::F_oneLevel (and G_oneLevel at the same pose when wantG != 0, from the same pass) on the prepared points at
 * the camera -> world matrix invM (column-major), voxels read nearest-neighbour at ROUND(invM p / voxelSize).  Synchronises
 * `stream`. */
int ITM_FN(ren_tracker_evaluate)(itm_ren_tracker* tracker, const itm_scene* scene, const float invM[16], int wantG,
                                 itm_ren_eval* out, itm_stream stream);
/* ITMRenTracker::TrackCamera: prepares the points from view->depth, runs the Levenberg-Marquardt loop from view->M_d (level 0 only;
 * the tracking regime is not used, as in the reference), writes the refined and coerced pose_d to M_d_out.  evaluations (may be
 * NULL): passes over the points the call made (each one energy + gradient + Hessian).  Synchronises `stream`. */
int ITM_FN(ren_tracker_track_camera)(itm_ren_tracker* tracker, const itm_scene* scene, const itm_view* view, float M_d_out[16],
                                     int* evaluations, itm_stream stream);

/* ---- state access ------------------------------------------------------------------------- */
/* Blocks until `stream` has drained, then reads the device-side counters. */
int ITM_FN(get_counters)(const itm_scene* scene, const itm_render_state* rs, itm_counters* out,
                         itm_stream stream);
/* Restores counters (checkpoint / test set-up).  Only lastFreeBlockId, lastFreeExcessListId,
 * noVisibleEntries are taken from `in`. */
int ITM_FN(set_counters)(itm_scene* scene, itm_render_state* rs, const itm_counters* in,
                         itm_stream stream);
size_t ITM_FN(buffer_bytes)(const itm_scene* scene, const itm_render_state* rs, int which);
/* Synchronous copies of whole buffers between host memory and the scene / render state.
 * Sentinel words: in a HASH scene two sdf words are no values -- the short -32768 (ITMVoxel_s, ITMVoxel_s_rgb) and the float word
 * 0xffffffff (ITMVoxel_f, ITMVoxel_f_rgb; one of the NaNs).  The integration never produces them, and the scene's sdf mirror keeps
 * them for "no block here".  An upload of ITM_BUF_VOXEL_BLOCKS into a hash scene that holds one in any voxel is refused with
 * ITM_ERR_INVALID before anything is written (the message names the first such voxel; the scene stays as it was); -32767 and
 * 0xfffffffe are values like any other.  Dense scenes have no mirror and accept every word, as the reference does. */
int ITM_FN(download)(const itm_scene* scene, const itm_render_state* rs, int which, void* dst_host,
                     size_t bytes, itm_stream stream);
int ITM_FN(upload)(itm_scene* scene, itm_render_state* rs, int which, const void* src_host,
                   size_t bytes, itm_stream stream);
/* Scene checkpoint: one file per memory block in the layout of ORUtils/MemoryBlockPersister.h:17-130
 * (int32 element count, then the raw elements): hash.dat (ITMHashEntry), excess.dat (int), alloc.dat (int),
 * voxel.dat (TVoxel), counters.dat (itm_counters as 8 ints), config.dat (itm_scene_config + itm_scene_params as bytes,
 * checked on load), and for a render state visible_ids.dat (int) / visible_type.dat (uchar).  A scene created with
 * useSwapping also writes swap_states.dat (uchar per table entry: 0, 1, 2), cache_flags.dat (uchar per table entry:
 * ITMGlobalCache::hasStoredData, 0 / 1) and cache_blocks.dat (TVoxel: the 512 voxels of every flagged entry's cached block,
 * flagged entries only, in entry order -- never the whole cache); entries with ptr == -1 have their voxels nowhere else.
 * Loading validates every file before anything of the scene is replaced (a refused load leaves scene, render state and host
 * cache untouched); a swapping scene refuses a checkpoint without those three files, states or flags out of range, and a
 * block count other than the number of flags set, and its host cache is replaced wholesale.  A hash scene also refuses, in
 * the same way and with ITM_ERR_INVALID, a voxel.dat or cache_blocks.dat that holds a sentinel word (see itm_upload) in any voxel;
 * itm_scene_save never writes one, because no scene holds one.  Loading into a scene of
 * the same configuration and continuing gives bit-identical results to the uninterrupted run.  `dir` must exist. */
int ITM_FN(scene_save)(const itm_scene* scene, const itm_render_state* rs, const char* dir, itm_stream stream);
int ITM_FN(scene_load)(itm_scene* scene, itm_render_state* rs, const char* dir, itm_stream stream);
/* ---- scene export: marching-cubes mesh ----------------------------------------------------------------
 * ITMMesh (Objects/ITMMesh.h:14-124): a triangle buffer of noMaxTriangles = SDF_LOCAL_BLOCK_NUM * 32 entries {p0, p1, p2} (nine
 * floats, metres) in device memory; max_triangles == 0 selects that default for the scene's pool size.
 * ITMMeshingEngine::MeshScene(mesh, scene) (Engine/ITMMeshingEngine.h:19-26, CPU: DeviceSpecific/CPU/ITMMeshingEngine_CPU.cpp:
 * 19-58): clears the buffer, then appends the triangles of every cell of every allocated block in table-slot order, voxels in
 * z, y, x order -- the same ORDER as the reference, and the same behaviour when the buffer is full (count stops at
 * noMaxTriangles - 1, the last slot holds the last triangle generated).  Dense scenes produce no triangles, as in the
 * reference (:70-72). */
typedef struct itm_mesh itm_mesh;
int ITM_FN(mesh_create)(const itm_scene* scene, uint32_t max_triangles, itm_mesh** out);
int ITM_FN(mesh_destroy)(itm_mesh* mesh);
int ITM_FN(mesh_scene)(const itm_scene* scene, itm_mesh* mesh, itm_stream stream);
/* The mesh of the scene's volume whatever its index (the reference has no dense mesher; this one is defined by its per-cell function).
 * Hash scenes: exactly itm_mesh_scene.  Dense scenes (ITMPlainVoxelArray: denseSize (sx, sy, sz), denseOffset, voxel (x, y, z) at
 * x + y * sx + z * sx * sy):
 *   bricks  the array is cut into bricks of 8^3 voxels by array index: brick (bx, by, bz) holds voxels 8b .. 8b + 7 clipped to the
 *           array, nb = ceil(s / 8) per axis; sizes need not be multiples of 8.
 *   order   bricks in ascending bx + by * nbx + bz * nbx * nby; inside a brick `for z for y for x` over the voxels it holds (the loop of
 *           ITMMeshingEngine_CPU.cpp:39 on one block).
 *   cell    buildVertList (DeviceAgnostic/ITMMeshingEngine.h:204-232) at the integer location L = (x, y, z) + denseOffset, the eight
 *           corners read through the dense readVoxel (ITMRepresentationAccess.h:129-142): a corner outside the array is not found; a
 *           corner that is not found or whose SDF_valueToFloat(sdf) == 1.0f kills the cell; corner positions are L + corner offset as
 *           floats; sdfInterp with its three `< 0.00001f` early returns; triangles in the case table's order; every vertex times
 *           voxelSize last.
 *   buffer  as itm_mesh_scene: cleared first, the count stops at noMaxTriangles - 1, the last slot holds the last triangle generated.
 * So a hash scene whose blocks hold the same voxels at the same global positions (default voxels where a brick sticks out of the array)
 * gives the same triangles, block run for block run.  Like itm_mesh_scene the call replaces the mesh, makes attributes and index stale,
 * and launches recorded engine calls first; itm_mesh_attributes, itm_mesh_index, itm_mesh_indexed_attributes, the downloads and the
 * writers serve the result.  The per-brick buffers belong to the mesh and are allocated by the first call on a dense scene.  Three
 * launches, no host round trip.  itm_mesh_scene itself stays empty for dense scenes, as in the reference. */
int ITM_FN(mesh_volume)(const itm_scene* scene, itm_mesh* mesh, itm_stream stream);
/* mesh->noTotalTriangles / noMaxTriangles / the triangle buffer; synchronises `stream`.  Any output pointer may be NULL.  The buffer's
 * address is fixed for the life of the mesh unless itm_mesh_update is used: an update that copies kept runs writes a second buffer and
 * the two change places, so ask again after every itm_mesh_update. */
int ITM_FN(mesh_info)(const itm_mesh* mesh, uint32_t* noTotalTriangles, uint32_t* noMaxTriangles,
                      const float** triangles, itm_stream stream);
/* copies min(noTotalTriangles, capacity) triangles (9 floats each) to host memory; synchronises `stream` */
int ITM_FN(mesh_download)(const itm_mesh* mesh, float* dst_host, uint32_t capacityTriangles,
                          uint32_t* noTotalTriangles, itm_stream stream);
/* ITMMesh::WriteOBJ (Objects/ITMMesh.h:34-62) and ITMMesh::WriteSTL (:64-110), byte-identical files */
int ITM_FN(mesh_write_obj)(const itm_mesh* mesh, const char* path, itm_stream stream);
int ITM_FN(mesh_write_stl)(const itm_mesh* mesh, const char* path, itm_stream stream);
/* Vertex attributes of the triangles the last itm_mesh_scene left in the buffer (the reference's ITMMesh has none; the two per-point
 * functions are the reference's).  For every vertex v, in buffer order (triangle i: p0, p1, p2), at p = v / voxelSize (three IEEE
 * divisions; a function of the stored vertex alone, so equal positions get equal attributes):
 *   ITM_MESH_NORMALS  g = computeSingleNormalFromSDF(p) (DeviceAgnostic/ITMRepresentationAccess.h:224-337), n = g * (1 / sqrt(g.g)),
 *                     (0, 0, 0) where the length is zero or n is not finite; n points from the surface into free space.
 *   ITM_MESH_COLOURS  readFromSDF_color4u_interpolated(p) (:187-222) converted as drawPixelColour does
 *                     (DeviceAgnostic/ITMVisualisationEngine.h:270-279): (uchar)(c * 255.0f) per channel, alpha 255.  Scenes whose
 *                     voxel type stores no colour: ITM_ERR_INVALID.
 * `what` is one of them or both (further calls add to what is current).  itm_mesh_scene / itm_mesh_volume make the attributes stale; their
 * buffers are allocated by the first call that needs them.  A dense scene after itm_mesh_scene: an empty mesh, empty attributes; after
 * itm_mesh_volume: the attributes of its triangles, read through the voxel array. */
#define ITM_MESH_NORMALS 1
#define ITM_MESH_COLOURS 2
int ITM_FN(mesh_attributes)(const itm_scene* scene, itm_mesh* mesh, int what, itm_stream stream);
/* copies the attributes of min(noTotalTriangles, capacity) triangles to host memory: normals_host 3 vertices x float[3] per triangle,
 * colours_host 3 vertices x {r, g, b, 255} per triangle; either may be NULL.  A non-NULL pointer whose attribute is stale or was
 * never computed: ITM_ERR_INVALID.  Synchronises `stream`. */
int ITM_FN(mesh_download_attributes)(const itm_mesh* mesh, float* normals_host, uint8_t* colours_host, uint32_t capacityTriangles,
                                     uint32_t* noTotalTriangles, itm_stream stream);
/* PLY, binary_little_endian 1.0: 3 vertices per triangle in buffer order -- float x, y, z, then float nx, ny, nz if the normals are
 * current, then uchar red, green, blue if the colours are -- and one face {3, 3i + 2, 3i + 1, 3i} per triangle (the winding of
 * ITMMesh::WriteOBJ, Objects/ITMMesh.h:34-62).  With neither attribute current the file holds positions only. */
int ITM_FN(mesh_write_ply)(const itm_mesh* mesh, const char* path, itm_stream stream);
/* Indexed mesh: the triangle soup welded into shared vertices (the reference has none; defined in terms of its triangle buffer).  With
 * s_j, j = 0 .. 3 * noTotalTriangles - 1, the buffer's vertices in buffer order: two of them are the same vertex iff their three floats
 * have the same 96 bits (no tolerance; -0.0f != +0.0f).  first[k] = the smallest j that holds the k-th distinct position, strictly
 * ascending -- unique vertices are numbered in the order of their first occurrence --, vertices[k] = s_first[k], faces[i] = the indices of
 * s_3i, s_3i+1, s_3i+2.  Every triangle is kept, also those whose corners coincide after welding: vertices[faces] is the soup bit for
 * bit.  The result is deterministic.  itm_mesh_index builds the three arrays for the present contents of the buffer in device memory
 * owned by the mesh (allocated / grown from the counts; the call synchronises `stream` to read them) and leaves the triangle buffer as
 * it is; itm_mesh_scene makes the index stale.  An empty buffer (dense scenes) gives an empty index. */
int ITM_FN(mesh_index)(itm_mesh* mesh, itm_stream stream);
/* number of unique vertices / of triangles of the index and its device arrays (float[3] per vertex, uint32[3] per triangle, uint32 per
 * vertex; NULL for an empty index); synchronises `stream`.  Any output pointer may be NULL.  Stale or missing index: ITM_ERR_INVALID. */
int ITM_FN(mesh_index_info)(const itm_mesh* mesh, uint32_t* noVertices, uint32_t* noTriangles, const float** vertices,
                            const uint32_t** faces, const uint32_t** first, itm_stream stream);
/* copies min(noVertices, capacityVertices) vertices (3 floats each) and entries of `first`, and min(noTriangles, capacityTriangles)
 * faces (3 uint32 each) to host memory; any pointer may be NULL.  Stale or missing index: ITM_ERR_INVALID.  Synchronises `stream`. */
int ITM_FN(mesh_download_indexed)(const itm_mesh* mesh, float* vertices_host, uint32_t* first_host, uint32_t capacityVertices,
                                  uint32_t* faces_host, uint32_t capacityTriangles, uint32_t* noVertices, uint32_t* noTriangles,
                                  itm_stream stream);
/* itm_mesh_attributes for the unique vertices of the index: normal[k], colour[k] = the attribute of s_first[k] (a function of the position
 * alone), evaluated once per unique vertex.  The same refusals as itm_mesh_attributes, and ITM_ERR_INVALID on a stale or missing index.
 * itm_mesh_scene and itm_mesh_index make them stale; they and the soup's attributes are independent of each other. */
int ITM_FN(mesh_indexed_attributes)(const itm_scene* scene, itm_mesh* mesh, int what, itm_stream stream);
/* copies the attributes of min(noVertices, capacity) unique vertices to host memory: normals_host float[3], colours_host {r, g, b, 255}
 * per vertex; either may be NULL.  A non-NULL pointer whose attribute is stale or was never computed: ITM_ERR_INVALID.  Synchronises. */
int ITM_FN(mesh_download_indexed_attributes)(const itm_mesh* mesh, float* normals_host, uint8_t* colours_host, uint32_t capacityVertices,
                                             uint32_t* noVertices, itm_stream stream);
/* The indexed mesh as a file.  PLY: the header lines and property order of itm_mesh_write_ply with `element vertex noVertices`, the
 * attributes written when the INDEXED attributes are current, one face {3, f2, f1, f0} per triangle.  OBJ: the format of
 * ITMMesh::WriteOBJ (Objects/ITMMesh.h:34-62), "v %f %f %f" per unique vertex, then "f c+1 b+1 a+1" per triangle (a, b, c).  Stale or
 * missing index: ITM_ERR_INVALID. */
int ITM_FN(mesh_write_ply_indexed)(const itm_mesh* mesh, const char* path, itm_stream stream);
int ITM_FN(mesh_write_obj_indexed)(const itm_mesh* mesh, const char* path, itm_stream stream);
/* Connected components of the indexed mesh (the reference has none; defined on the present index: noVertices unique vertices k,
 * noTriangles faces[i] = (a, b, c)).  Two vertices are LINKED iff some triangle names both -- degenerate triangles count like any other,
 * and nothing is linked by position: the index has decided which positions are one vertex, bit for bit.  A COMPONENT is a class of the
 * transitive closure; root(k) = the smallest vertex index of k's component.  Components are numbered c = 0 .. noComponents - 1 in
 * ascending order of their root (vertices are numbered by first occurrence, so this is the order in which the components first appear in
 * the triangle buffer).  Then
 *   vertexComponent[k]   = the number of vertex k's component
 *   triangleComponent[i] = vertexComponent[faces[i][0]]
 *   components[c]        = {firstVertex = the root, noVertices, noTriangles, reserved = 0, bbMin[3], bbMax[3]}: the box is the per-axis
 *                          minimum and maximum over the component's vertices in the total order of the IEEE bit patterns (sign-magnitude
 *                          mapped to a monotone unsigned: -0.0f < +0.0f); the stored floats are a vertex's own bits.
 * Everything is an integer or independent of order: no tolerance, deterministic, compared bit for bit.  (Surface area is not here: a
 * float sum over atomics depends on arrival order; a host that wants it computes it from the downloads.)
 * itm_mesh_components labels the present index in device memory owned by the mesh (sized from the counts; the call synchronises `stream`
 * to read them; a call that cannot get its memory keeps none of it).  It needs a current index (ITM_ERR_INVALID otherwise);
 * itm_mesh_scene, itm_mesh_volume, itm_mesh_index and itm_mesh_filter_components make the labelling stale.  An empty index gives zero
 * components and no error. */
typedef struct itm_mesh_component {
  uint32_t firstVertex;   /* the component's smallest vertex index */
  uint32_t noVertices;
  uint32_t noTriangles;
  uint32_t reserved;      /* 0 */
  float bbMin[3];
  float bbMax[3];
} itm_mesh_component;     /* 40 bytes */
int ITM_FN(mesh_components)(itm_mesh* mesh, itm_stream stream);
/* number of components, the number of union rounds the labelling took (1 unless its final check asked for more; 0 for an empty index)
 * and the three device arrays (uint32 per vertex, uint32 per triangle, itm_mesh_component per component; NULL where empty);
 * synchronises `stream`.  Any output pointer may be NULL.  Stale or missing labelling: ITM_ERR_INVALID. */
int ITM_FN(mesh_components_info)(const itm_mesh* mesh, uint32_t* noComponents, uint32_t* rounds, const uint32_t** vertexComponent,
                                 const uint32_t** triangleComponent, const itm_mesh_component** components, itm_stream stream);
/* copies min(count, capacity) entries of each array to host memory; any pointer may be NULL.  Stale or missing labelling:
 * ITM_ERR_INVALID.  Synchronises `stream`. */
int ITM_FN(mesh_download_components)(const itm_mesh* mesh, uint32_t* vertexComponent_host, uint32_t capacityVertices,
                                     uint32_t* triangleComponent_host, uint32_t capacityTriangles, itm_mesh_component* components_host,
                                     uint32_t capacityComponents, uint32_t* noComponents, itm_stream stream);
/* Drops fragments: component c is kept iff components[c].noTriangles >= minTriangles and (keep_host == NULL or keep_host[c] != 0);
 * noKeep must equal noComponents when keep_host is given (ITM_ERR_INVALID otherwise).  The call rewrites the TRIANGLE BUFFER: the kept
 * triangles, in their buffer order, packed to the front; keptTriangles / keptComponents (either may be NULL) receive the counts.  It
 * needs a current labelling (ITM_ERR_INVALID otherwise).  Afterwards the mesh behaves in every respect as if itm_mesh_scene /
 * itm_mesh_volume had generated exactly those triangles: itm_mesh_info reports the kept count, and the soup's attributes, the index, the
 * indexed attributes and the components are stale.  Keeping nothing leaves a valid empty mesh.  Synchronises `stream`. */
int ITM_FN(mesh_filter_components)(itm_mesh* mesh, uint32_t minTriangles, const uint8_t* keep_host, uint32_t noKeep,
                                   uint32_t* keptTriangles, uint32_t* keptComponents, itm_stream stream);
/* Mesh smoothing: lambda|mu (Taubin) or plain Laplacian passes over the present index, IN FIXED POINT (the reference has none; a float
 * umbrella sum over atomics or an unordered neighbour list would depend on arrival order, see the remark on surface area above).  The
 * topology does not change: faces, first, the per-block ranges, all counts and itm_mesh_info stay what they are; only positions move.
 * Defined on the present index, noVertices vertices v[k] (float[3]) and noTriangles faces (a, b, c), by this sequential definition:
 *   entries   a triangle whose three indices are pairwise distinct gives each of its corners one ENTRY for each of its other two
 *             corners; a triangle with two equal indices (welding produces them; they have no area) gives nothing.  L(k) = the multiset
 *             of the entries of vertex k, n(k) = |L(k)| = twice the number of its proper triangles.
 *   irregular k is irregular iff some vertex occurs in L(k) a number of times other than 2: k lies on an edge named by one triangle (a
 *             border) or by three or more (non-manifold).
 *   isolated  k is isolated iff n(k) == 0.
 *   moving    k is moving iff it is not isolated and not (ITM_MESH_SMOOTH_PIN_IRREGULAR set and k irregular).  On a moving vertex of a
 *             pinned run every neighbour has multiplicity 2: the operator there is exactly the uniform umbrella.  With the flag clear,
 *             border vertices move under the incidence-weighted umbrella.
 *   quantise  x[k] = (int32) rint((double) v[k] / (double) quantum) per coordinate, ties to even, for EVERY vertex.  A coordinate of any
 *             vertex that is not finite or has |rint(..)| > 2^30: ITM_ERR_INVALID, the mesh and its state exactly as before.
 *   pass      with factor f (Q16; pass i = 0 .. steps - 1 uses lambdaQ16 for even i, muQ16 for odd i), all vertices at once from the
 *             previous iterate (Jacobi).  For a moving k, per coordinate, in int64:
 *               S = sum over j in L(k) of x[j],  a = S - n * x[k]
 *               d = floor((2 a + n) / (2 n))                   the mean offset, rounded half up
 *               s = (f * d + 32768) >> 16                      an arithmetic shift: floor, half up
 *               x'[k] = clamp(x[k] + s, -2^30, 2^30)
 *             (no intermediate reaches 2^63 for any n < 2^32).  A vertex that is not moving keeps x.
 *   result    a moving vertex gets (float)((double) x * (double) quantum); every other vertex keeps its own 96 bits (-0.0f included).
 *             Then the triangle buffer is rewritten, soup[3 i + j] = vertices[faces[i][j]] for the noTriangles indexed triangles, so
 *             "vertices[faces] is the soup bit for bit" still holds.
 *   steps==0  the statistics only: positions are not read (no range check) and nothing is changed, the state included.
 * Everything is an integer or rounded once from one: the result does not depend on the order in which lanes ran, on the order inside an
 * adjacency row or on the kernel form, and is compared bit for bit.
 * stats (may be NULL): noVertices; noMoving, noIrregular, noIsolated = the numbers of vertices with that property (irregular counted
 * whether or not the flag pins them); maxEntries = max n(k); steps = the passes run.  An empty index: zero stats and no error.
 * Refusals (ITM_ERR_INVALID, the mesh untouched): steps > ITM_MESH_SMOOTH_MAX_STEPS (every pass is a launch queued before the call's
 * one wait: the cap keeps a garbage word from queueing billions); |lambdaQ16| or |muQ16| > 65536; a quantum that is not finite or not
 * > 0; non-zero reserved words; unknown flag bits; a stale or missing index.  A call that cannot get its memory (ITM_ERR_DEVICE) keeps
 * none of it and leaves vertices, triangle buffer and state as they were.  A call that fails on the device AFTER its passes were queued
 * (ITM_ERR_DEVICE) may have moved the positions: the state is then that of a call that succeeded.
 * State after a call with steps > 0 that succeeded: the index STAYS current -- it is the mesh's topology, and first[k] still names a
 * soup vertex that holds vertices[k] -- but two distinct vertices may now coincide in position, so a fresh itm_mesh_index could weld them
 * (and number the vertices anew).  The soup's attributes, the indexed attributes and the components (their boxes are no longer true)
 * are stale; whether the buffer holds a dense volume's mesh is unchanged.  itm_mesh_attributes / itm_mesh_indexed_attributes serve the
 * moved vertices (a vertex that has left its block's neighbourhood reads through the hash).  Synchronises `stream`, as itm_mesh_index. */
#define ITM_MESH_SMOOTH_PIN_IRREGULAR 1
#define ITM_MESH_SMOOTH_MAX_STEPS 65536
typedef struct itm_mesh_smooth_config {
  uint32_t steps;       /* single passes, at most ITM_MESH_SMOOTH_MAX_STEPS; pass i uses lambdaQ16 for even i, muQ16 for odd i */
  int32_t lambdaQ16;    /* factor * 65536, |factor| <= 1 */
  int32_t muQ16;        /* Taubin: negative, |mu| > lambda; plain Laplacian: muQ16 == lambdaQ16 */
  float quantum;        /* metres per fixed-point unit, > 0 and finite */
  uint32_t flags;       /* ITM_MESH_SMOOTH_PIN_IRREGULAR */
  uint32_t reserved[3]; /* 0 */
} itm_mesh_smooth_config; /* 32 bytes */
typedef struct itm_mesh_smooth_stats {
  uint32_t noVertices, noMoving, noIrregular, noIsolated, maxEntries, steps, reserved[2];
} itm_mesh_smooth_stats;  /* 32 bytes */
/* host only: steps 20, lambda 0.5 (32768), mu -0.53 (-34734), quantum = voxelSize / 1024, ITM_MESH_SMOOTH_PIN_IRREGULAR set.
 * voxelSize not finite or not > 0: ITM_ERR_INVALID. */
int ITM_FN(mesh_smooth_default_config)(float voxelSize, itm_mesh_smooth_config* out);
int ITM_FN(mesh_smooth)(itm_mesh* mesh, const itm_mesh_smooth_config* cfg, itm_mesh_smooth_stats* stats, itm_stream stream);
/* Incremental mesh: the triangle buffer follows the scene at the cost of the blocks a frame touched (the reference has none; defined in
 * terms of MeshScene, hash scenes only).
 * RUN TABLE, kept with the mesh: for every slot s that MeshScene listed (ptr >= 0, ascending) the block position pos_s it held then, the
 * first triangle of its run and the run's length.  It exists after a successful itm_mesh_scene on a hash scene (which records it: one
 * more launch, its results do not change) and after a successful itm_mesh_update; it is CURRENT only while the buffer is exactly what
 * those calls left and only if all generated triangles fitted (generated <= noMaxTriangles - 1).  itm_mesh_filter_components (once it
 * rewrites), itm_mesh_smooth (steps > 0) and itm_mesh_volume on a dense scene make it stale.
 * MARKS, kept with the mesh: a set of table slots, and the word "everything".  itm_mesh_touch adds to them, itm_mesh_update clears them.
 *
 * itm_mesh_touch(mesh, scene, rs, slots_dev, n): the blocks that were rewritten since the mesh was last brought up to date.
 *   rs != NULL          the slots visibleEntryIDs[0 .. noVisibleEntries) of the render state are marked -- a fused frame writes exactly
 *                       these blocks.  The count is read on the device.
 *   slots_dev != NULL   the n >= 0 table slots in device memory are marked.
 *   both NULL, n == -1  everything is marked: the next update is a full one.
 *   Both lists may be given in one call.  A value outside the table ([0, noTotalEntries)) is ignored and counted (ignoredMarks of the
 *   next update).  Recorded engine calls of the scene and of rs are launched first (the visible list is final only then); the call then
 *   only enqueues work on `stream` and does not synchronise.  Marks accumulate over any number of calls.
 *   Refusals (ITM_ERR_INVALID, the reason in itm_last_error, nothing changed): a NULL mesh or scene; a scene other than the mesh's; a
 *   dense scene; a render state of another scene; n < 0 with a list, or both NULL with n != -1.
 *
 * itm_mesh_update(scene, mesh, stats): brings the buffer up to date.  Sequential definition:
 *   0. Recorded calls are launched.  The call IS itm_mesh_scene (cap behaviour included) in three cases, stats->full naming which:
 *      ITM_MESH_UPDATE_NO_RUN_TABLE the run table is not current, ITM_MESH_UPDATE_ALL_MARKED everything is marked,
 *      ITM_MESH_UPDATE_OVERFLOW the triangles of step 5 number more than noMaxTriangles - 1.  Otherwise full = 0 and:
 *   1. A' = the slots with ptr >= 0 now, ascending; A = the run table's slots.  APPEARED: s in A' that is not in A or holds another
 *      position than pos_s.  VANISHED: s in A that is not in A' (swapped out, ptr == -1, included) or now holds another position.
 *   2. Seeds P = the present positions of the marked slots that are in A'  u  the positions of the appeared  u  the old positions of
 *      the vanished.
 *   3. Dirty D = { s in A' : pos_s + d in P for some d in {0, 1}^3 }: the cells of a block read its own voxels and one layer of the seven
 *      blocks at +d, and a missing corner kills a cell, so these are exactly the blocks whose cells can differ.
 *   4. Every s in D gets the triangles of MeshScene's loop over that block as the scene is now; every s in A' \ D keeps its old run,
 *      copied bit for bit.
 *   5. The buffer is the runs in ascending slot order, zero behind them; noTotalTriangles is their sum.  The run table is rewritten for A'.
 *   6. Delta (itm_mesh_update_info / itm_mesh_download_update): `changed` = D in ascending slot order, each {slot, pos, first triangle,
 *      count} in the NEW buffer; `removed` = {old slot, old position} of the vanished whose old position no entry of A' holds now, in
 *      ascending old slot order.  After a full path `changed` lists every listed block (runs as generated: with a full buffer the
 *      triangles from noMaxTriangles - 1 on are not in it) and `removed` is what steps 1-2 found, empty where the run table was not current.
 *   7. The marks are cleared.  The soup's attributes, the index, the indexed attributes and the components are stale, as after
 *      itm_mesh_scene.  The buffer's DEVICE POINTER may change (ask itm_mesh_info again): the copy of step 4 needs a second buffer of
 *      noMaxTriangles triangles, allocated by the first update that copies; the two change places.
 * PROPERTY: if every block whose stored sdf changed since the run table was made is marked or has appeared, the buffer after the call
 * equals a fresh itm_mesh_scene's bit for bit, order included.  Presence changes are found by the call itself, so itm_scene_prune,
 * swapping out and new allocations need no touch; a fused or de-integrated frame needs its render state; itm_scene_merge / _resample,
 * uploads and itm_scene_load change voxels in place and need their slots, or n == -1.
 * stats (may be NULL): full; allocated = |A'|; marked = distinct marked slots inside the table; ignoredMarks; appeared; vanished (both 0
 * where the run table was not current); remeshed = |D| and kept = |A' \ D| (allocated and 0 after a full path); trianglesBefore / After =
 * noTotalTriangles; trianglesCopied / Generated = the triangles of the kept / re-meshed runs; noChanged, noRemoved = the delta's lengths.
 * The call synchronises `stream` once to read the totals, which also decides the overflow fall-back (that path synchronises once more).
 * MI355X: one pass over the table (presence diff, eight slot-directory look-ups per seed), ordered compactions, marching cubes over D
 * only (the kernels of itm_mesh_scene on a list), a carry scan over A', one dword-granular coalesced copy of the kept runs.
 * Refusals as itm_mesh_touch.  A call that fails on the device leaves the run table stale: the next update is a full one. */
#define ITM_MESH_UPDATE_NO_RUN_TABLE 1
#define ITM_MESH_UPDATE_ALL_MARKED 2
#define ITM_MESH_UPDATE_OVERFLOW 3
typedef struct itm_mesh_update_stats {
  int32_t full, allocated, marked, ignoredMarks, appeared, vanished, remeshed, kept;
  uint32_t trianglesBefore, trianglesAfter, trianglesCopied, trianglesGenerated;
  uint32_t noChanged, noRemoved, reserved[2];
} itm_mesh_update_stats;   /* 64 bytes */
typedef struct itm_mesh_changed_block {
  int32_t slot;            /* table slot */
  int16_t pos[3];          /* block position */
  int16_t reserved;        /* 0 */
  uint32_t firstTriangle, noTriangles;
} itm_mesh_changed_block;  /* 20 bytes */
typedef struct itm_mesh_removed_block {
  int32_t slot;            /* the table slot it held */
  int16_t pos[3];
  int16_t reserved;        /* 0 */
} itm_mesh_removed_block;  /* 12 bytes */
int ITM_FN(mesh_touch)(itm_mesh* mesh, const itm_scene* scene, const itm_render_state* rs, const int32_t* slots_dev, int n, itm_stream stream);
int ITM_FN(mesh_update)(const itm_scene* scene, itm_mesh* mesh, itm_mesh_update_stats* stats, itm_stream stream);
/* the delta of the last itm_mesh_update: its lengths and device arrays (NULL where empty; owned by the mesh, rewritten by the next
 * update).  Any output pointer may be NULL.  No update since the mesh was created: ITM_ERR_INVALID.  Does not synchronise: the arrays
 * were complete when the update returned. */
int ITM_FN(mesh_update_info)(const itm_mesh* mesh, uint32_t* noChanged, uint32_t* noRemoved, const itm_mesh_changed_block** changed,
                             const itm_mesh_removed_block** removed, itm_stream stream);
/* copies min(count, capacity) entries of each array to host memory; any pointer may be NULL.  Synchronises `stream`. */
int ITM_FN(mesh_download_update)(const itm_mesh* mesh, itm_mesh_changed_block* changed_host, uint32_t capacityChanged,
                                 itm_mesh_removed_block* removed_host, uint32_t capacityRemoved, uint32_t* noChanged, uint32_t* noRemoved,
                                 itm_stream stream);

/* ---- multi-stream exchange (BASELINE configs[3]) ------------------------------------------------------------------
 * One depth stream per GPU; fusion needs no collective.  Per frame every rank publishes the record of itm_export_visible_record
 * ({M_d[16], noVisibleEntries, ids[max_ids]}); every `batch` frames the records are all-gathered with RCCL on a side stream owned by
 * the exchange, so that each rank holds the pose and the live block list of every stream (input of a shared-map merger).  The frame
 * stream never waits for a collective of the current batch, and the collectives are put on the side stream by a thread the exchange owns
 * (enqueueing an all-gather costs a host thread 60-80 us).  RCCL is loaded on first use (dlopen; ITM_RCCL_LIBRARY in the environment
 * names another collective library -- a site's own build, the tests' stand-in for several ranks on one GPU -- and says so on stderr).
 * Every world size, one rank included, gets an RCCL communicator and runs ncclAllGather.  Bootstrap: rank 0 calls itm_exchange_unique_id, the host hands the 128 bytes
 * to every rank; `id` may be NULL for world == 1 (the library then makes the id itself). */
typedef struct itm_exchange itm_exchange;
int ITM_FN(exchange_unique_id)(unsigned char id[128]);
int ITM_FN(exchange_create)(int world, int rank, const unsigned char id[128], int max_ids, int batch, itm_exchange** out);
int ITM_FN(exchange_destroy)(itm_exchange* exchange);
/* frame f of this rank's stream: record copy on `frame_stream`; on the last frame of a batch also the collective (side stream) */
int ITM_FN(exchange_step)(itm_exchange* exchange, const itm_render_state* rs, const float M_d[16], itm_stream frame_stream);
int ITM_FN(exchange_info)(const itm_exchange* exchange, int* world, int* rank, int* max_ids, int* batch, const void** gathered_device);
/* Hand-off of a gathered table to a DEVICE-side consumer (the per-GPU global visibility table of SURVEY 8e; a shared-map merger's kernel).
 * Every slot of the exchange's ring of eight has its own table.  itm_exchange_acquire makes `consumer_stream` wait for the newest
 * collective issued so far and returns its table (world x batch records, rank-major; *first_frame = the frame number of the batch's
 * first record; NULL / -1 before the first collective).  The table belongs to the consumer until itm_exchange_release -- or the next
 * itm_exchange_acquire, which releases first -- both given the stream the consumer's reads were put on: the ring skips a held slot,
 * and the collective that next writes a released slot waits (on the exchange's side stream) behind those reads.  One holder at a time.
 * Frames and collectives go on meanwhile; nothing here blocks the host.  Threads: the slot is chosen and marked as held under one lock,
 * so a consumer thread other than the one calling itm_exchange_step is safe; two consumer threads are not (one holder at a time). */
int ITM_FN(exchange_acquire)(itm_exchange* exchange, itm_stream consumer_stream, const int32_t** table, long long* first_frame);
int ITM_FN(exchange_release)(itm_exchange* exchange, itm_stream consumer_stream);
/* host copy of the gathered table, world x batch records of (17 + max_ids) int32 words, rank-major; synchronises the side stream */
int ITM_FN(exchange_table)(itm_exchange* exchange, int32_t* dst_host, size_t words);
/* Self-check, on by default at every world size (ITM_EXCHANGE_SELF_CHECK=0 in the environment switches it off): behind each collective,
 * on the side stream, this rank's own block of the gathered table is compared with the batch buffer it sent; words that differ make the
 * next itm_exchange_step / itm_exchange_table return ITM_ERR_DEVICE.  Here: collectives checked so far (-1 = self-check off) and words
 * found different; synchronises the side stream. */
int ITM_FN(exchange_self_check)(itm_exchange* exchange, int* collectives_checked, int* mismatched_words);

/* ---- swapping (Engine/ITMSwappingEngine.h:19-36, DeviceSpecific/CPU/ITMSwappingEngine_CPU.cpp, Objects/ITMGlobalCache.h) ----
 * Scenes created with useSwapping keep an ITMGlobalCache in HOST memory (one block slot + one `hasStoredData` flag per table entry) and
 * a swap state per entry on the device (0 host has the newest data / never loaded, 1 visible and still to be combined with the host's
 * copy, 2 the device has the newest data).  ITMDenseMapper::ProcessFrame calls the two methods after the integration
 * (Engine/ITMDenseMapper.cpp:59-64):
 *   IntegrateGlobalIntoLocal  the first transferBlockNum entries in state 1, in table order: the host's stored block (if any) is
 *                             combined voxel by voxel into the device block (weighted by w_depth / w_color), state -> 2
 *   SaveToGlobalMemory        the first transferBlockNum entries in state 2 that hold a block and are not visible: the block goes to
 *                             the host cache, the entry's ptr becomes -1, the voxel block returns to the allocation list, state -> 0
 * Both synchronise with the host (the reference's CUDA twin does, through cudaMemcpy).  Return ITM_ERR_INVALID for scenes without swapping. */
int ITM_FN(swap_integrate_global_into_local)(itm_scene* scene, itm_render_state* rs, itm_stream stream);
int ITM_FN(swap_save_to_global_memory)(itm_scene* scene, itm_render_state* rs, itm_stream stream);
/* ITMGlobalCache::HasStoredData / GetStoredVoxelBlock: copies the stored block of table entry `entry` (512 voxels) to dst_host if there
 * is one; *has = 1 / 0 */
int ITM_FN(global_cache_get)(const itm_scene* scene, int entry, void* dst_host, int* has);
/* hasStoredData[noTotalEntries] as bytes */
int ITM_FN(global_cache_flags)(const itm_scene* scene, uint8_t* dst_host, size_t bytes);

/* ---- scene merge: fuses scene `src` into scene `dst` on the same GPU (the shared-map merger the exchange above gathers for) ----------
 * Not a reference operation: assembled from the reference's two-phase block allocation (with src's block positions in the place of
 * ray steps) and its CombineVoxelInformation (src in the role of the stored block).  Requirements, else ITM_ERR_INVALID with the
 * reason in itm_last_error and dst untouched: dst != src, same device, same voxelType and indexType, bit-equal voxelSize (mu and maxW
 * may differ: dst's maxW is used); dense scenes: equal denseSize / denseOffset and srcSlots_dev == NULL.  Recorded calls of both
 * scenes are launched first.  srcSlots_dev: NULL = every table slot of src, else a DEVICE list of n slots of src's table in any order
 * (duplicates count once, an id outside the table is ITM_ERR_INVALID) -- a render state's visible list, a gathered exchange record.
 *
 * Hash index, sequential definition (the kernels reproduce it bit for bit):
 *  1. Participants: the selected entries of src with ptr >= 0, in ascending src slot order.  Selected entries with ptr == -1 count in
 *     srcWithoutBlock; empty slots are ignored.
 *  2. Rounds.  Request: every participant whose position is not in dst (a matching entry has ptr >= -1; walk from hashIndex(pos) along
 *     the offset chain) places a request -- ORDERED on the head if the head is empty (ptr < -1), else EXCESS on the chain's tail.
 *     Requests on one target overwrite each other, the highest src slot wins, the others ask again next round.  Sweep over dst's slots
 *     ascending: an ordered request is served iff lastFreeBlockId >= 0, an excess request iff also lastFreeExcessListId >= 0; a served
 *     request takes allocList[lastFreeBlockId--] (and excessList[lastFreeExcessListId--]) and writes {pos, offset 0, ptr} (the tail's
 *     offset = entry + 1) as AllocateSceneFromDepth does.  Unlike the frame sweep, a request that is not served consumes nothing and
 *     moves no counter; a counter below -1 counts as empty and stays.  Rounds end after the first round without a request, or the
 *     first that serves none: the participants still without a place then count in `unserved` (pool exhaustion is not an error).
 *     considered = participants, alreadyPresent = those found in round 1, allocated = requests served, rounds = rounds run.
 *  3. Combine: for every participant whose position is now in dst with ptr >= 0, all 512 voxels: dst = CombineVoxelInformation(src,
 *     dst, dst's maxW); counted in `combined`.  Those found with ptr == -1 (swapped out of dst) count in dstSwappedOut and are left.
 *  4. The occupancy bits, the directories and the sdf mirror of dst are what itm_upload of the same table and voxels would rebuild;
 *     the request keys are zero again.  dst's render states, visible lists and swap states are not touched (new entries are not
 *     visible until a frame sees them); src is never written.
 * Dense index: every voxel of dst is combined with the voxel of src at the same index; considered = combined = 1.
 * Synchronises `stream` once per round (the round's counts); the combine itself is enqueued.  `stats` (host) may be NULL. */
typedef struct itm_merge_stats {
  int32_t rounds, considered, alreadyPresent, allocated, combined, unserved, srcWithoutBlock, dstSwappedOut;
} itm_merge_stats;
int ITM_FN(scene_merge)(itm_scene* dst, const itm_scene* src, const int32_t* srcSlots_dev, int n, itm_merge_stats* stats, itm_stream stream);

/* ---- level of detail: resamples scene `src` into scene `dst` of TWICE the voxel size on the same GPU ---------------------------------
 * The reference has no counterpart (it has one resolution per scene and decimates nothing).  A TSDF is low-passed and every second
 * sample kept; whatever reads a scene -- meshing, ray cast, queries, the distance field, save, the exchange -- then works on the coarse
 * scene unchanged.  Defined on integers and a fixed tap order: the kernels reproduce it bit for bit.
 * Requirements, else ITM_ERR_INVALID with the reason in itm_last_error and dst untouched: neither scene NULL, dst != src, same device,
 * same voxelType and indexType, dst's voxelSize bit-equal to 2.0f * src's, mu bit-equal (sdf is stored as a fraction of mu: values carry
 * over only if it is the same; maxW may differ: dst's is used), dst not holding the block requests of a frame issued ahead, and the
 * slot-list rules of itm_scene_merge (srcSlots_dev: NULL = every table slot of src, else a DEVICE list of n slots in any order,
 * duplicates count once; an id outside src's table, n < 0, or a list with dense scenes: ITM_ERR_INVALID).  Dense scenes need NOT agree in
 * denseSize / denseOffset.  Recorded calls of both scenes are launched first; src is never written.
 *
 * Geometry.  A voxel at integer coordinate p stands for the point p * voxelSize, so coarse voxel q stands for fine voxel 2q, and fine
 * block b belongs to coarse block B = b >> 1 per component (arithmetic shift: -1 -> -1, -3 -> -2).
 *
 * The coarse voxel at q, for both index types.  Taps k = (kx, ky, kz) in {-1, 0, 1}^3, taken with kz outermost and kx innermost, each
 * ascending; c_k = (2 - |kx|)(2 - |ky|)(2 - |kz|) (they sum to 64); t_k = readVoxel(src, 2q + k) (DeviceAgnostic/
 * ITMRepresentationAccess.h:85-142) over the WHOLE of src, whatever the slot list selects; an absent voxel, an entry with ptr < 0 or a
 * block pointer outside src's pool reads as TVoxel() with weight 0.
 *   depth   a_k = c_k * w_depth(t_k), A = sum a_k.  A == 0: sdf = the initial value (32767 / 1.0f), w_depth = 0.  Otherwise
 *           w_depth' = min(dst maxW, 255, max(1, (A + 32) div 64)) and
 *             short sdf: S = sum a_k * sdf_k (fits int32: 64 * 255 * 32767 < 2^31), sdf' = sgn(S) * ((2|S| + A) div 2A) -- to nearest,
 *                        halves away from zero;
 *             float sdf: S = sum (double)a_k * (double)sdf_k, summed in double in the tap order above starting from +0.0 (every product
 *                        is exact, so contraction cannot change a bit), sdf' = (float)(S / (double)A).
 *   colour  (the two types that store it) b_k = c_k * w_color(t_k), Bc = sum b_k.  Bc == 0: clr = 0, w_color = 0.  Otherwise each channel
 *           is (2 * sum b_k * clr_k + Bc) div 2Bc and w_color' = min(dst maxW, 255, max(1, (Bc + 32) div 64)).
 * Property: where the 27 taps have equal weight and sdf is affine in the coordinates, sdf' = sdf(2q) and w' = w exactly.
 *
 * Hash index, sequential definition:
 *  1. Participants as in itm_scene_merge step 1: the selected entries of src with ptr >= 0, in ascending src slot order; selected entries
 *     with ptr == -1 count in srcWithoutBlock.
 *  2. Rounds: itm_scene_merge step 2 word for word, with the participant's COARSE position b >> 1 in the place of its position.  Up to
 *     eight participants share a position: one wins the target, the others find the entry in the next round.  rounds, considered,
 *     alreadyPresent, allocated and unserved mean what they mean there.
 *  3. D = the set of dst entries that hold the coarse position of at least one participant.  Those with ptr == -1 count in dstSwappedOut
 *     and are left alone; for the others all 512 voxels are OVERWRITTEN with the coarse voxel above, `written` is their number (an entry
 *     whose block pointer lies outside dst's pool -- only an uploaded table can name one -- is left alone and not counted).  Every other
 *     block of dst keeps its content.  Overwrite, not combine: CombineVoxelInformation with an empty partner is not the identity in
 *     float.  A coarse block is allocated only through b >> 1: coarse voxel 8B + 7 of a block reaches half a voxel into the fine blocks
 *     beyond, but a coarse block that no participant maps to is not created for that half voxel of dilation -- it is dropped.
 *  4. The occupancy bits, the directories and the sdf mirror of dst are what itm_upload of the same table and voxels would rebuild; the
 *     request keys are zero again.  dst's render states, visible lists and swap states are not touched.
 * Dense index: every cell of dst is overwritten with the coarse voxel at q = cell + dst's denseOffset; taps go through the dense
 * readVoxel of src, outside src's array a tap is absent; considered = written = 1.
 * Other factors: call it again through a third scene.  Synchronises `stream` once per round and once for the statistics; the resampling
 * launch itself is enqueued.  `stats` (host) may be NULL. */
typedef struct itm_coarsen_stats {
  int32_t rounds, considered, alreadyPresent, allocated, written, unserved, srcWithoutBlock, dstSwappedOut;
} itm_coarsen_stats;
int ITM_FN(scene_coarsen)(itm_scene* dst, const itm_scene* src, const int32_t* srcSlots_dev, int n, itm_coarsen_stats* stats, itm_stream stream);

/* ---- scene merge under a rigid transform: resamples scene `src` into the frame of scene `dst` and fuses it there, on the same GPU ----
 * itm_scene_merge needs one world frame, voxel for voxel; the maps of several sessions or robots have one each.  With the relative pose
 * (a relocalisation, the poses the exchange gathers) src is resampled at dst's voxels and combined into dst.  The reference has no
 * counterpart.  The transform is quantised once on the host; from there on everything is defined on integers and a fixed tap order,
 * so the kernels reproduce it bit for bit.
 *
 * itm_rigid_quantise.  dstFromSrc: column-major like every matrix here, in metres: x_dst = R x_src + t.  In double:
 *   fwd = llrint(R * 2^30)   fwdT = llrint(t / voxelSize * 2^30)   inv = llrint(R^T * 2^30)   invT = llrint(-(R^T t) / voxelSize * 2^30)
 * where R is the rotation next to the matrix's upper 3 x 3: three steps of R <- R (3 I - R^T R) / 2 in double.  A float matrix is
 * orthonormal to 1e-7 at best, some 50 units of Q30, and inv = R^T is the inverse of fwd only as far as R is orthonormal; after the
 * steps inv * fwd is within a few units of 2^60 I.  The identity and the turns by 90 degrees pass through bit for bit (+-2^30 and 0).
 * ITM_ERR_INVALID with the reason in itm_last_error: a null pointer, a voxelSize that is not positive and finite, a non-finite entry, a
 * bottom row other than (0, 0, 0, 1), an entry of R^T R - I above 1e-4 in magnitude, det R < 0, |t| / voxelSize >= 2^18 on an axis.
 * Q30, not Q16: block coordinates are shorts, voxel coordinates reach 2^18, where the rounding of fwd against inv stays below 1e-3 voxel. */
typedef struct itm_rigid_q {      /* Q30, row-major [3i + j]; voxel units */
  int32_t inv[9];  int64_t invT[3];   /* src voxel coordinate of dst voxel q:  p = inv * q + invT */
  int32_t fwd[9];  int64_t fwdT[3];   /* dst voxel coordinate of src voxel p:  q = fwd * p + fwdT */
} itm_rigid_q;
int ITM_FN(rigid_quantise)(const float dstFromSrc[16], float voxelSize, itm_rigid_q* out);

/* itm_scene_resample.  Requirements, else ITM_ERR_INVALID with the reason in itm_last_error and dst untouched: those of itm_scene_coarsen
 * (neither scene NULL, dst != src, same device, voxelType and indexType, dst not holding the block requests of a frame issued ahead, the
 * slot-list rules) with voxelSize bit-equal instead of doubled and mu bit-equal (maxW may differ: dst's is used); q not NULL; every row of
 * q->inv and of q->fwd has sum |entry| <= 1.75 * 2^30 (a rotation has at most sqrt(3)) and every |T| < 2^48.  The call does not ask q to
 * be a rotation: the definition below holds for whatever passes.  Recorded calls of both scenes are launched first; src is never written.
 *
 * The resampled voxel at dst voxel q, for both index types.  Per axis p = inv * q + invT (int64, Q30); P = (p + 2^23) >> 24 (arithmetic
 * shift: Q6, the position to the nearest 1/64 voxel, halves up); cell f = P >> 6, fraction u = P & 63.  Eight taps k in {0, 1}^3, taken
 * with kz outermost and kx innermost; c_k = prod_i (k_i ? u_i : 64 - u_i) (they sum to 2^18); t_k = readVoxel(src, f + k) over the WHOLE
 * of src, whatever the slot list selects; an absent voxel, an entry with ptr < 0 or a block pointer outside src's pool reads as TVoxel()
 * with weight 0, as in itm_scene_coarsen.
 *   depth   a_k = c_k * w_depth(t_k), A = sum a_k (int64; below 2^26).  A == 0: r carries no depth (w_depth 0) and dst's sdf and w_depth
 *           stay as they are.  Otherwise w' = min(255, max(1, (A + 2^17) >> 18)) and
 *             short sdf: S = sum a_k * sdf_k (int64), sdf' = sgn(S) * ((2|S| + A) div 2A) -- to nearest, halves away from zero;
 *             float sdf: S = sum (double)a_k * (double)sdf_k, summed in double in the tap order from +0.0 (every product is exact:
 *                        26 + 24 bits < 53), sdf' = (float)(S / (double)A).
 *   colour  (the two types that store it) b_k = c_k * w_color(t_k), Bc = sum b_k.  Bc == 0: r carries no colour (clr 0, w_color 0) and
 *           dst's stay as they are.  Otherwise each channel is (2 * sum b_k * clr_k + Bc) div 2Bc (int64) and
 *           w_color' = min(255, max(1, (Bc + 2^17) >> 18)).  The two parts are independent, as they are in the combine.
 *   fuse    dst = CombineVoxelInformation(r, dst, dst's maxW) with r = (sdf', w', clr', w_color') in the role of the stored block: the
 *           combine of itm_scene_merge step 3.  dst's maxW clamps there; r's own weights are clamped at 255 only.
 * Properties: inv the identity and invT whole voxels: u = 0, r is src's voxel at the shifted position (with zero translation every
 * voxel of dst comes out as itm_scene_merge leaves it; more BLOCKS exist, see below).  A rotation by a multiple of 90 degrees about an
 * axis with a whole-voxel translation permutes the voxels exactly.
 *
 * Hash index, sequential definition (box(M, T, [lo3, hi3]) is, per axis i, lo = T_i + sum_j min(M_ij lo3_j, M_ij hi3_j) and hi the same
 * with max; the voxels such a Q30 box can touch with a trilinear footprint are [(lo >> 30) - 1, (hi >> 30) + 2]):
 *  1. Participants as in itm_scene_merge step 1; `considered` is their number, selected entries with ptr == -1 count in srcWithoutBlock.
 *  2. Candidate list C.  The participants in ascending src slot order, each at block b: the forward box of its dilated cube
 *     box(fwd, fwdT, [8b - 1, 8b + 8]) gives a dst voxel range and, >> 3, a block range (at most 4 blocks per axis under the row bound).
 *     Its blocks B are walked with Bz outermost and Bx innermost, ascending; B is a candidate iff the voxel range of its inverse box
 *     box(inv, invT, [8B, 8B + 7]) meets [8b_i, 8b_i + 7] on every axis.  A candidate whose coordinates do not fit a short is dropped
 *     and counted in outOfRange; `candidates` = |C|.  One block is a candidate of every participant near it: C holds it that often.
 *     The two tests are the axis-aligned halves of a box-overlap check: what they over-allocate stays allocated and empty, as the
 *     blocks that ray-step allocation leaves beside a surface.
 *  3. Rounds: itm_scene_merge step 2 word for word, with C in the place of the participants and the index in C in the place of the
 *     src slot (the highest index wins a target).  alreadyPresent, allocated and unserved count candidates.
 *  4. D = the set of dst entries that hold the position of at least one candidate.  Those with ptr == -1 count in dstSwappedOut and
 *     are left alone; for the others all 512 voxels take the rule above, `resampled` is their number (an entry whose block pointer lies
 *     outside dst's pool -- only an uploaded table can name one -- is left alone and not counted).  Under the row bound every tap of
 *     a block of D lies in the 3 x 3 x 3 src blocks from ((lo >> 30) - 1) >> 3 of the block's inverse box on.
 *  5. Derived structures as in itm_scene_merge step 4.  A dst whose cubes nothing has placed yet gets them around the block that holds
 *     the image (fwd, fwdT, >> 30, >> 3) of the centre of src's.
 * Dense index: every cell of dst takes the voxel rule at q = cell + dst's denseOffset; taps go through the dense readVoxel of src, outside
 * src's array a tap is absent; denseSize / denseOffset need not agree; a slot list is refused; considered = resampled = 1, the rest 0.
 * Synchronises `stream` once for the candidate count (twice when the scratch has to grow), once per round and once for the statistics;
 * the resampling launch itself is enqueued.  `stats` (host) may be NULL. */
typedef struct itm_resample_stats {
  int32_t rounds, considered, candidates, alreadyPresent, allocated, resampled, unserved, srcWithoutBlock, dstSwappedOut, outOfRange;
} itm_resample_stats;
int ITM_FN(scene_resample)(itm_scene* dst, const itm_scene* src, const itm_rigid_q* q, const int32_t* srcSlots_dev, int n, itm_resample_stats* stats, itm_stream stream);

/* ---- scene pruning: returns the voxel blocks of a hash scene that carry no information to the pool --------------------------------------
 * Not a reference operation: a reference scene only gains blocks (AllocateSceneFromDepth allocates every block the band depth +- mu
 * touches; nothing but host swapping gives one back, and that keeps the entry).  A block without an observed voxel, or whose observed
 * voxels all sit at "free", reads exactly as an absent one does (readVoxel of a missing block: sdf 1, w 0), so removing it changes no
 * read while it frees a block of the pool, a table slot, its directory cells and its mirror values.
 * Refusals, each ITM_ERR_INVALID with the reason in itm_last_error and the scene untouched: a NULL scene or config; a dense scene; a scene
 * created with useSwapping (its host cache and swap states are keyed by table slot, and swapping is that scene's own way of getting
 * blocks back); a scene that holds the block requests of a frame issued ahead (itm_cancel_ahead first); classes == 0 or with a bit
 * outside the four; a freeSdf that is not finite or lies outside [-1, 1]; weakMaxW < 1 with ITM_PRUNE_WEAK selected; a box with
 * min > max in a component when it is used (ITM_PRUNE_BOX selected, or boxOnly).  Recorded calls of the scene are launched first.
 *
 * Sequential definition (the kernels reproduce it bit for bit; tests/scene_prune_terms.py transcribes it):
 *  1. Classes.  For every entry that holds a voxel block of the pool (ptr >= 0), in ascending slot order, over its 512 voxels: a voxel
 *     is OBSERVED if w_depth > 0 (colour weights play no part).  EMPTY: no observed voxel.  SURFACE: an observed voxel BELOW the
 *     threshold -- short voxels: stored word < (short)(freeSdf * 32767.0f), the threshold computed once; float voxels: not
 *     (sdf >= freeSdf).  FREE: an observed voxel and not SURFACE.  WEAK: an observed voxel and the largest w_depth <= weakMaxW.  INBOX
 *     (only when the box is used): boxMin <= pos <= boxMax in every component, block coordinates.  `considered` counts these entries;
 *     entries with ptr == -1 (or a pointer outside the pool, which only an uploaded table can hold) count in withoutBlock, take part
 *     in nothing and are left as they are; empty slots have the decision byte 0.
 *  2. Candidates.  An entry is a FIRST candidate if it shows a selected class among EMPTY, FREE, WEAK (with boxOnly: and is INBOX);
 *     with ITM_PRUNE_BOX selected every INBOX entry is a first candidate and FORCED, whatever it holds -- this is how a region is
 *     erased.  With `protect`, a first candidate that is not forced STAYS if one of its 26 neighbours (found by walking from
 *     hashIndex(pos) along the offset chain, as step 2 of itm_scene_merge does) holds a block, is SURFACE and is not a first candidate
 *     itself: it counts in protectedByNeighbour.  The trilinear reads and the marching-cubes cells at the surface (meshing skips a cell
 *     whose corner block is missing) are then unchanged.  The others are the CANDIDATES.
 *  3. Buckets, ascending; the head, then its chain in chain order.  A candidate excess entry is DROPPED and its predecessor's offset
 *     becomes its offset.  A candidate head is DROPPED only if no entry of its chain stays (entries with ptr == -1 included);
 *     otherwise it is PINNED (pinnedHeads) and keeps its block and voxels: the allocation takes an ordered slot with ptr < -1 without
 *     looking at its offset and would cut the chain off, and moving a chain entry into the head would change table slots that other
 *     structures hold.  candidates = dropped + pinnedHeads.
 *  4. Release, the dropped entries in ascending slot order.  A counter below -1 counts as -1 (as in SaveToGlobalMemory above).
 *     allocList[++lastFreeBlockId] = ptr; for an excess entry also excessList[++lastFreeExcessListId] = slot - bucketNum; a write past
 *     either list (only an uploaded, inconsistent counter can ask for one) is left out and the counter stops at the list's last index.
 *     The 512 voxels of every dropped block take the initial value (blocks on the allocation list are handed out unreset) and the
 *     entry becomes the one ResetScene writes.
 *  5. The occupancy bits, both directories and the sdf mirror read as itm_upload of the same table and voxels would leave them (in the
 *     paged form a page whose blocks have all gone stays mapped with every cell "absent" until the cubes are next emptied, as after a
 *     swap-out).  The request keys stay zero.  In EVERY render state of the scene: entriesVisibleType of a dropped slot becomes 0, the
 *     dropped slots leave visibleEntryIDs with the order of the rest kept, noVisibleEntries is lowered; visibleRemoved counts the list
 *     entries removed over all render states.  No later call finds a listed slot without a block.
 *  6. dryRun: steps 1 - 3 only.  The decision bytes and the statistics are those of the real run (the two counters as they would
 *     become); nothing in the scene or in a render state changes.
 * decisions_dev (DEVICE, uchar[noTotalEntries], may be NULL) receives per entry the ITM_PRUNE_IS_* bits.  `stats` (host, may be NULL):
 * with it the call synchronises `stream` once, at its end; without it everything is enqueued. */
enum { ITM_PRUNE_EMPTY = 1, ITM_PRUNE_FREE = 2, ITM_PRUNE_WEAK = 4, ITM_PRUNE_BOX = 8 };
enum { ITM_PRUNE_IS_EMPTY = 1, ITM_PRUNE_IS_FREE = 2, ITM_PRUNE_IS_WEAK = 4, ITM_PRUNE_IS_SURFACE = 8, ITM_PRUNE_IS_INBOX = 16,
       ITM_PRUNE_IS_CANDIDATE = 64, ITM_PRUNE_IS_DROPPED = 128 };
typedef struct itm_prune_config {
  int32_t classes;              /* OR of ITM_PRUNE_*: which kinds of block are candidates (default EMPTY | FREE) */
  float freeSdf;                /* FREE: every observed voxel has sdf >= freeSdf (default 1.0) */
  int32_t weakMaxW;             /* WEAK: the block's largest w_depth is in 1 .. weakMaxW (default 1) */
  int32_t protect;              /* 1: a candidate with a surface-bearing 26-neighbour stays (default 1) */
  int32_t boxMin[3], boxMax[3]; /* block coordinates, inclusive */
  int32_t boxOnly;              /* 1: EMPTY / FREE / WEAK apply inside the box only */
  int32_t dryRun;               /* 1: decide and count, change nothing */
} itm_prune_config;             /* 48 bytes */
typedef struct itm_prune_stats {
  int32_t considered, empty, free_, weak, inBox, candidates, protectedByNeighbour, pinnedHeads, dropped, droppedHeads, droppedExcess,
          withoutBlock, visibleRemoved, lastFreeBlockId, lastFreeExcessListId;
  int32_t reserved;
} itm_prune_stats;              /* 64 bytes */
int ITM_FN(prune_default_config)(itm_prune_config* out);
int ITM_FN(scene_prune)(itm_scene* scene, const itm_prune_config* cfg, uint8_t* decisions_dev, itm_prune_stats* stats, itm_stream stream);

/* ---- scene queries: the volume asked at caller-supplied points and along caller-supplied rays -------------------------------------
 * The reference makes these reads only from inside its engines, per pixel; here the work item is the caller's.  Both calls launch the
 * scene's recorded calls first, read the scene only, take DEVICE pointers and enqueue one launch on `stream` (no synchronisation).
 *
 * itm_scene_query_points, sequential definition.  For point i with x = points_dev[3i .. 3i + 2]:
 *   p = x / voxelSize (three IEEE divisions, as itm_mesh_attributes: a mesh's vertices reproduce its attributes bit for bit) for
 *   ITM_QUERY_METRES, p = x for ITM_QUERY_VOXELS.  Voxels are read as readVoxel reads them (DeviceAgnostic/ITMRepresentationAccess.h:
 *   85-142): an absent voxel is TVoxel() -- sdf 1, weight 0, colour 0.  Outputs, each written only where its pointer is not NULL:
 *     sdf          readFromSDF_float_interpolated(p)                                               :160-185
 *     sdf_nearest  readFromSDF_float_uninterpolated(p): the voxel at ROUND(p)                      :144-158
 *     gradient     computeSingleNormalFromSDF(p) as it returns it, not normalised                  :224-337
 *     normal       gradient * (1 / sqrt(g.g)), (0, 0, 0) where that is not finite (the normal of itm_mesh_attributes)
 *     colour       readFromSDF_color4u_interpolated(p) (:187-222) as drawPixelColour's bytes (DeviceAgnostic/ITMVisualisationEngine.h:
 *                  270-279), alpha 255; a scene whose voxel type stores no colour: ITM_ERR_INVALID, as itm_mesh_attributes
 *     weight       w_depth of the voxel at ROUND(p), 0 if absent
 *     flags        bit 0: the voxel at ROUND(p) exists; bits 8-15: which corners of the trilinear cell floor(p) + (dx, dy, dz) exist
 *                  (corner dx + 2 dy + 4 dz); bit 1: all eight do; bit 31 ITM_QUERY_INVALID: a coordinate of p is not finite or
 *                  !(|c| < 262136) -- then nothing is read at p (floor(p) - 1 .. floor(p) + 2 stays inside the table's short block
 *                  coordinates for every other p) and the outputs are the defaults: sdf and sdf_nearest 1, the others 0.
 *   n == 0: success, nothing launched.
 *
 * itm_scene_cast_rays, sequential definition.  Ray i is rays_dev[8i .. 8i + 7] = (sx, sy, sz, t0, ex, ey, ez, t1), metres: the segment
 * to search and the ray parameter at its two ends.  The result is castRay's (DeviceAgnostic/ITMVisualisationEngine.h:92-158) from the
 * statement that follows its camera preamble, with oneOverVoxelSize = 1.0f / voxelSize and stepScale = mu * oneOverVoxelSize:
 *   pt_block_s = s * oneOverVoxelSize, pt_block_e = e * oneOverVoxelSize, totalLength = t0 * oneOverVoxelSize, totalLengthMax = t1 *
 *   oneOverVoxelSize, rayDirection = (pt_block_e - pt_block_s) * (1 / sqrt(d.d)) as :117-121 form it, then the loop :126-156.
 * A camera ray fed this way -- s, e = invM * pt_camera_f of the range image's minimum / maximum depth, t = length(pt_camera_f) -- goes
 * through exactly the float operations of castRay.  hits_dev[4i .. 4i + 3] = (x, y, z, w) in voxel units as raycastResult holds them:
 * w = 1 a hit (feed xyz to itm_scene_query_points with ITM_QUERY_VOXELS for normals and colours), w = 0 a miss with xyz unspecified.
 * A ray is invalid, takes no step and gives (0, 0, 0, 0) when a value is not finite, when pt_block_s == pt_block_e, when a coordinate
 * of pt_block_s or pt_block_e has !(|c| < 131072), when !(|totalLength| < 4194304) or !(|totalLengthMax| < 4194304) (voxels: beyond
 * 2^24 the loop's `totalLength += stepLength` no longer moves and castRay would not end), or when the normalised direction is not
 * finite.  The limits bound the ray parameter, not the position: a ray whose t1 - t0 far exceeds |e - s| marches on past e, up to
 * ~8.4 M voxels from s, through space that reads "no block" (8 voxels a step: about a million steps for that lane and the wave it is
 * in) -- safe, but the caller pays for it; give t1 - t0 = |e - s| unless that is what is wanted.  hits_dev is 16-byte aligned.
 * n == 0: success, nothing launched. */
#define ITM_QUERY_METRES 0
#define ITM_QUERY_VOXELS 1
#define ITM_QUERY_INVALID 0x80000000u
typedef struct itm_query_out {      /* device pointers, NULL = not wanted */
  float* sdf;           /* [n]  */
  float* sdf_nearest;   /* [n]  */
  float* gradient;      /* [3n] */
  float* normal;        /* [3n] */
  uint8_t* colour;      /* [4n] */
  uint8_t* weight;      /* [n]  */
  uint32_t* flags;      /* [n]  */
} itm_query_out;
int ITM_FN(scene_query_points)(const itm_scene* scene, const float* points_dev, uint32_t n, int units, const itm_query_out* out, itm_stream stream);
int ITM_FN(scene_cast_rays)(const itm_scene* scene, const float* rays_dev, uint32_t n, float* hits_dev, itm_stream stream);

/* ---- distance field: Euclidean distance transform of a box of the volume ------------------------------------------------------------
 * What a planner asks: how far is this voxel from the nearest surface, how far from space nobody has seen.  The TSDF answers within
 * +-mu of a surface only; here every cell of a box gets the exact Euclidean distance, in voxels squared, to the nearest SITE of the box.
 * The reference has no counterpart.  Read-only on the scene; DEVICE pointers; launches on `stream`, nothing is synchronised.
 *
 * Sequential definition.  The box has a first voxel o = origin (voxel units, any alignment, may be negative) and a size (nx, ny, nz).
 * Cell (i, j, k) is voxel p = o + (i, j, k) and lies at linear index i + nx * (j + ny * k).
 *  1. Classification, one byte per cell (`state`).  Voxels are read as readVoxel reads them (DeviceAgnostic/ITMRepresentationAccess.h:
 *     85-142): an absent voxel is TVoxel().
 *       ITM_ESDF_STORED    a voxel exists at p
 *       ITM_ESDF_OBSERVED  stored and w_depth >= min_weight (min_weight >= 1)
 *       ITM_ESDF_INSIDE    observed and SDF_valueToFloat(sdf) <= 0
 *       ITM_ESDF_SITE      the cell is a site under one of the rules `sites` selects:
 *         ITM_ESDF_SITE_SURFACE  p is observed and has a 6-neighbour q that is observed with INSIDE(q) != INSIDE(p).  Neighbours are
 *                                read from the scene also where they lie outside the box: the classification of a sub-box is the crop
 *                                of a larger box's classification
 *         ITM_ESDF_SITE_UNKNOWN  p is not observed
 *     `sites` has at least one of the two bits and no others.
 *  2. Transform.  R = max_distance in voxels, 0 = unbounded.
 *       dist2[c]    min over the sites s of the box of |c - s|^2 (int32); ITM_ESDF_NONE where that exceeds R^2 (R > 0) or the box holds
 *                   no site
 *       nearest[c]  linear index of the site that attains the minimum, the smallest such index among ties; -1 with ITM_ESDF_NONE
 *     A separable transform meets this exactly: per axis, x then y then z, the candidates along the line taken in ascending order
 *     with a strict `<`; along every axis the smaller position is the smaller linear index of the site it stands for.  A window of
 *     +-R per axis loses nothing (a site within R has every axis offset within R) and every candidate is a real site.
 *  3. distance[c] = voxelSize * sqrtf((float)dist2[c]), negated where the cell is INSIDE; +-INFINITY (same sign rule) with
 *     ITM_ESDF_NONE.  dist2 < 2^24 at the allowed sizes, so the conversion is exact; sqrt and the product are IEEE, each rounded once.
 * Limits, refused with ITM_ERR_INVALID before anything is launched: each of nx, ny, nz in [1, 1024]; nx * ny * nz <= 2^27;
 * max_distance in [0, 1023]; every coordinate of the box with its one-voxel halo (o - 1 .. o + n) has |p| < 262136 (the limit of
 * itm_scene_query_points: block coordinates stay short).  out->dist2 is required: it is also the passes' working storage.
 *
 * itm_scene_esdf classifies the box of the scene (recorded calls are launched first) and transforms it.  itm_esdf_transform is the
 * scene-free half: it reads the SITE and INSIDE bits of a caller-supplied byte grid [nx * ny * nz], runs the same passes and ignores
 * out->state. */
#define ITM_ESDF_STORED 1
#define ITM_ESDF_OBSERVED 2
#define ITM_ESDF_INSIDE 4
#define ITM_ESDF_SITE 8
#define ITM_ESDF_SITE_SURFACE 1
#define ITM_ESDF_SITE_UNKNOWN 2
#define ITM_ESDF_NONE 0x7fffffff
typedef struct itm_esdf_box { int32_t origin[3]; int32_t size[3]; } itm_esdf_box;
typedef struct itm_esdf_out {      /* device pointers, [nx * ny * nz] each; NULL = not wanted, except dist2 */
  int32_t* dist2;                  /* required: also the passes' working storage */
  int32_t* nearest;
  float* distance;
  uint8_t* state;
} itm_esdf_out;
int ITM_FN(scene_esdf)(const itm_scene* scene, const itm_esdf_box* box, int sites, int min_weight, int max_distance, const itm_esdf_out* out,
                       itm_stream stream);
int ITM_FN(esdf_transform)(const uint8_t* state_dev, const int32_t size[3], int max_distance, float voxel_size, const itm_esdf_out* out,
                           itm_stream stream);

/* ---- keyframe relocaliser: "where have I seen this depth image before?" -------------------------------------------------------------
 * Randomised ferns over a small, smoothed depth image (Glocker et al., Real-Time RGB-D Camera Relocalization via Randomized Ferns
 * for Keyframe Encoding): a code of numFerns bytes per frame, a database of keyframe codes (device memory) with their poses (host),
 * a nearest-code search.  The reference at this revision has none; a host that has lost the pose takes the nearest keyframe's pose,
 * ray-casts from there and lets a tracker refine (ITMMainEngine_HIP::Relocalise).  The handle touches no scene.
 *
 * Sequential definition (the kernels reproduce it bit for bit; every product and sum is rounded separately, division is IEEE).
 *  1. Image.  I_0 is the float depth image, w x h, metres; a pixel <= 0 is a hole.  For l = 1 .. levels: I_l =
 *     FilterSubsampleWithHoles(I_{l-1}) (itm_filter_subsample_with_holes), sizes (w >> l, h >> l).  Then, for blurRadius R > 0, a
 *     hole-aware separable blur with taps t[0 .. R], the pass along x first, then the pass along y on its output.  A pass, for an
 *     output pixel: s = 0, n = 0; for i = -R .. R ascending, v the input at offset i along the axis: if that position is inside the
 *     image and v > 0 then s = s + t[|i|] * v, n = n + t[|i|]; the output is n > 0 ? s / n : 0.  R = 0: no blur, S = I_levels.  The
 *     result S has ws x hs = (w >> levels) x (h >> levels) pixels.
 *  2. Code.  numFerns F ferns of numDecisions D decisions (1 <= D <= 8, 1 <= F <= ITM_RELOC_MAX_FERNS); decision (f, d) has a pixel
 *     index pixel[f * D + d] in [0, ws * hs) and a threshold threshold[f * D + d]:
 *     code[f] = sum_d (S[pixel[f * D + d]] > threshold[f * D + d] ? 1 << d : 0), one byte per fern.
 *  3. Search.  The database holds `count` rows.  sim_i = #{f < F : row_i[f] == q[f]}.  Rows ordered by sim descending, then i
 *     ascending; for j < k (1 <= k <= ITM_RELOC_MAX_K): ids[j] the j-th row, dist[j] = (float)(F - sim) / (float)F; for j >= count:
 *     ids[j] = -1, dist[j] = 1.0f.
 *  4. Harvest (itm_reloc_process_frame).  The search result is that of the database BEFORE the call.  If harvest != 0 and (count ==
 *     0 or dist[0] > harvestThreshold) and count < capacity: the code becomes row `count`, M_d its pose, *added = the old count.  If
 *     only count < capacity fails: *added = -2.  Otherwise *added = -1.
 *  5. Defaults (host only).  levels: the smallest L with (w >> L) <= 40.  blurRadius 6, blurTaps[i] = (float)exp(-(double)(i * i) /
 *     (2 * 2.5 * 2.5)).  numFerns 500, numDecisions 4, capacity 65536.  Default ferns from a seed by splitmix64 (x += 0x9E3779B97F4A7C15;
 *     z = x; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; result z ^ z >> 31): for decision index
 *     0 .. F * D - 1 in order, pixel = (next() >> 32) % (ws * hs), u = (float)(next() >> 40) * (1.0f / 16777216.0f), threshold =
 *     lo + (hi - lo) * u in float (the metres a decision compares against: 0.2 and 3.0 span the default view frustum).
 *
 * Calls.  encode / find / process_frame enqueue on `stream`; encode never synchronises, find and process_frame synchronise `stream`
 * exactly once, to read their result.  A handle is used from one host thread at a time; work it has pending on another stream is
 * waited for first.  The calls without a stream (read, download, upload, save, load) wait for what the handle has pending.
 *   encode         image and code of depth_dev (device float[h * w]); both stay in the handle
 *   find           nearest rows of code_host (numFerns bytes), or of the last encoded code when NULL
 *   process_frame  encode + find + harvest; M_d (world -> camera, as itm_view) may be NULL when harvest == 0
 *   read           the last encode's small image (float[hs * ws]) and code (numFerns bytes); either may be NULL
 *   download       codes_host[count * numFerns], poses_host[count * 16]; either may be NULL
 *   upload         replaces the database by n rows
 *   save / load    one file, relocaliser.dat, in an existing directory (beside a scene checkpoint): configuration, ferns, codes and
 *                  poses.  Loading into a handle whose configuration (capacity apart) or ferns differ: ITM_ERR_INVALID.
 * ITM_ERR_INVALID with the handle untouched: a size that does not survive `levels` halvings, F, D, k or blurRadius (0 .. 8) out of
 * range, a pixel index outside the small image, an id outside the database, more rows than the capacity. */
#define ITM_RELOC_MAX_K 8
#define ITM_RELOC_MAX_FERNS 1024
typedef struct itm_reloc itm_reloc;
typedef struct itm_reloc_config {
  int32_t w, h, levels, blurRadius;
  float blurTaps[9];
  int32_t numFerns, numDecisions, capacity;
} itm_reloc_config;
int ITM_FN(reloc_default_config)(int w, int h, itm_reloc_config* cfg);
int ITM_FN(reloc_default_ferns)(const itm_reloc_config* cfg, uint64_t seed, float lo, float hi, int32_t* pixel, float* threshold);
int ITM_FN(reloc_create)(const itm_reloc_config* cfg, const int32_t* pixel_host, const float* threshold_host, itm_reloc** out);
int ITM_FN(reloc_destroy)(itm_reloc* reloc);
int ITM_FN(reloc_encode)(itm_reloc* reloc, const float* depth_dev, itm_stream stream);
int ITM_FN(reloc_find)(itm_reloc* reloc, const uint8_t* code_host, int k, int32_t* ids_host, float* dist_host, itm_stream stream);
int ITM_FN(reloc_process_frame)(itm_reloc* reloc, const float* depth_dev, const float M_d[16], int harvest, float harvestThreshold, int k,
                                int32_t* ids_host, float* dist_host, int32_t* added, itm_stream stream);
int ITM_FN(reloc_info)(const itm_reloc* reloc, int32_t* count, itm_reloc_config* cfg);
int ITM_FN(reloc_get_pose)(const itm_reloc* reloc, int32_t id, float M[16]);
int ITM_FN(reloc_read)(itm_reloc* reloc, float* image_host, uint8_t* code_host);
int ITM_FN(reloc_download)(itm_reloc* reloc, uint8_t* codes_host, float* poses_host);
int ITM_FN(reloc_upload)(itm_reloc* reloc, int32_t n, const uint8_t* codes_host, const float* poses_host);
int ITM_FN(reloc_save)(itm_reloc* reloc, const char* dir);
int ITM_FN(reloc_load)(itm_reloc* reloc, const char* dir);

/* ---- pose quality: "does this depth image, under this pose, agree with the fused volume?" -------------------------------------------
 * The judgement later InfiniTAM releases attach to a tracker's result (GOOD / POOR / FAILED), made here against the TSDF itself and
 * not against a tracker's residuals: it holds for every tracker type (an external pose source included), voxel type and index type,
 * and a tracker's own outlier rejection cannot flatter it.  The reference at this revision has none; this definition is the
 * specification and tests/pose_quality_terms.py its restatement.  ITMMainEngine_HIP acts on the verdict when
 * ITMLibSettings::useTrackingVerdict is set (include/itm_hip_engines.hpp).
 *
 * Sequential definition (float32, every product and sum rounded on its own, division IEEE).  For pixel (x, y) of view->depth (w x h,
 * intr_d = (fx, fy, cx, cy), pose M_d):
 *   d = depth[y * w + x].  !(d > 0) (negative, zero, NaN): the pixel is NONE.
 *   pc = (d * ((float(x) - cx) / fx), d * ((float(y) - cy) / fy), d)                 (the ICP tracker's back-projection order)
 *   pw = invM * (pc, 1), invM = Matrix4::inv of M_d as AllocateSceneFromDepth forms it, the product left to right as ORUtils'
 *        Matrix4 * Vector4: pw[r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r]
 *   (sdf, weight, flags) = itm_scene_query_points at pw with ITM_QUERY_METRES: the interpolated sdf, the weight and the flags
 *   KNOWN    flags has bit 0 (the voxel at ROUND(p) exists), not ITM_QUERY_INVALID, and weight >= cfg.minWeight
 *   UNKNOWN  every other pixel that is not NONE; a block that is swapped out reads as absent
 *   r = sdf * mu (metres; the sdf is clamped, so |r| <= mu)
 *   INLIER   KNOWN and fabsf(r) <= cfg.inlierDistance
 * itm_pose_quality: noPixels = w * h, noValid = pixels that are not NONE, noKnown, noInliers; sumSqKnown / sumSqInliers = the sum of
 * (double)r * (double)r (an exact product) over the KNOWN / INLIER pixels, added in a fixed order: the same call gives the same bits.
 * The optional residual image float[h * w] holds r for KNOWN pixels, ITM_POSE_QUALITY_UNKNOWN for UNKNOWN, ITM_POSE_QUALITY_NONE for
 * NONE.
 *
 * Verdict (itm_pose_quality_verdict: host only, a pure function of counts and configuration, compared in double):
 *   ITM_TRACKING_FAILED  noValid < minValidFraction * noPixels, or noKnown < failOverlap * noValid, or noInliers < failInliers *
 *                        noKnown, or noKnown == 0
 *   ITM_TRACKING_POOR    not failed, and noKnown < poorOverlap * noValid or noInliers < goodInliers * noKnown
 *   ITM_TRACKING_GOOD    otherwise
 * Defaults (itm_pose_quality_default_config(mu): host only): inlierDistance 0.5f * mu, minWeight 1, minValidFraction 0.05,
 * failOverlap 0.10, poorOverlap 0.30, failInliers 0.50, goodInliers 0.90.  The thresholds are POLICY: they separate the true pose from
 * shifted and rotated ones on the synthetic sphere-and-wall scene of the tests; nobody has tuned them on sensor data.
 * ITM_ERR_INVALID: !(0 < inlierDistance), a fraction outside [0, 1], failOverlap > poorOverlap, failInliers > goodInliers,
 * minWeight < 1, a null argument, w * h <= 0.
 *
 * Calls.  A handle owns its reduction records and serialises its own calls (two host threads use two handles).  evaluate launches the
 * scene's recorded calls first, only reads the scene, enqueues ONE launch on `stream` and returns with *out filled: the result
 * arrives through tagged records in page-locked host memory, no stream synchronise.  residuals_dev (device float[h * w]) may be
 * NULL. */
#define ITM_TRACKING_FAILED 0
#define ITM_TRACKING_POOR 1
#define ITM_TRACKING_GOOD 2
#define ITM_POSE_QUALITY_UNKNOWN 1e30f
#define ITM_POSE_QUALITY_NONE (-1e30f)
typedef struct itm_pose_quality_handle itm_pose_quality_handle;
typedef struct itm_pose_quality_config {
  float inlierDistance;      /* metres */
  int32_t minWeight;         /* w_depth a voxel needs to count as KNOWN */
  float minValidFraction, failOverlap, poorOverlap, failInliers, goodInliers;
} itm_pose_quality_config;
typedef struct itm_pose_quality { int32_t noPixels, noValid, noKnown, noInliers; double sumSqKnown, sumSqInliers; } itm_pose_quality;
int ITM_FN(pose_quality_default_config)(float mu, itm_pose_quality_config* cfg);
int ITM_FN(pose_quality_verdict)(const itm_pose_quality* stats, const itm_pose_quality_config* cfg, int32_t* result);
int ITM_FN(pose_quality_create)(itm_pose_quality_handle** out);
int ITM_FN(pose_quality_destroy)(itm_pose_quality_handle* handle);
int ITM_FN(pose_quality_evaluate)(itm_pose_quality_handle* handle, const itm_scene* scene, const itm_view* view, const itm_pose_quality_config* cfg,
                                  itm_pose_quality* out, float* residuals_dev, itm_stream stream);

/* ---- scene alignment: refines the rigid pose between sdf samples and a TSDF scene ------------------------------------------------------
 * itm_scene_resample fuses src into dst under a transform that something has to supply to the accuracy the resampling works at; a
 * relocalisation or the exchange's poses are centimetres and degrees off.  Here a coarse dstFromSrc is refined by registering SAMPLES
 * against dst: a sample is (p, d), a point p in metres in the source frame and the signed distance d in metres it should read there.
 * d = 0 everywhere: plain surface points (mesh vertices, a lidar sweep).  Samples taken from the voxels of a scene src
 * (itm_scene_band_samples): sdf-to-sdf registration of two scenes.  The reference has no counterpart; this definition is the
 * specification and tests/scene_align_terms.py its restatement.
 *
 * itm_scene_band_samples, sequential definition.  A stored voxel of src at global voxel coordinates (x, y, z) is KEPT when
 *   w_depth >= cfg->minWeight,  fabsf(SDF_valueToFloat(sdf)) < cfg->maxAbsSdf (0 < maxAbsSdf <= 1; strict: a truncated +-1 is never
 *   kept)  and  x, y and z are multiples of cfg->stride (>= 1).
 * Its sample is the float4 ((float)x * voxelSize, (float)y * voxelSize, (float)z * voxelSize, SDF_valueToFloat(sdf) * mu): one rounding
 * each.  Order: hash scenes in ascending table slot -- the slot list as in itm_scene_merge (NULL: every slot; duplicates count once; a
 * slot outside the table: ITM_ERR_INVALID), entries with ptr < 0 (swapped out, free) and block pointers outside the pool skipped --
 * and inside a block in ascending x + 8 y + 64 z; dense scenes in ascending linear index (a slot list is refused).  *count_out
 * receives the number of kept voxels, samples_dev (device, 16-byte aligned, may be NULL when capacity is 0) the first `capacity` of
 * them: a caller asks twice, or sizes from the voxel count.  Recorded calls of src are launched first; src is only read; `stream` is
 * synchronised once, for the count (and once before, for the check of a slot list).
 *
 * itm_aligner_evaluate, sequential definition (float32, every product and sum rounded on its own, division IEEE; no transcendental
 * function anywhere).  M = dstFromSrc (column-major, metres: x_dst = R x_src + t), sample i = (p, d):
 *   x_k = ((R_k0 p_0 + R_k1 p_1) + R_k2 p_2) + t_k;   q = x / voxelSize  (as itm_scene_query_points forms it)
 *   q is not finite or has !(|c| < 262136) (ITM_QUERY_INVALID's rule): the sample is invalid and nothing is read.
 *   The eight corners of the cell floor(q) are read as readVoxel reads them.  The sample is VALID iff all eight voxels exist and none
 *   converts to 1.0f: an absent, an unobserved and a front-truncated voxel all read 1, the rule the Ren tracker uses.  No weight is read
 *   (minWeight acts where the samples are made).
 *   s = readFromSDF_float_interpolated(q);  g = the derivative of that same interpolant per voxel, c = q - floor(q), v the raw corners:
 *     g_x = (1-c_z) ((1-c_y) (v100 - v000) + c_y (v110 - v010)) + c_z ((1-c_y) (v101 - v001) + c_y (v111 - v011))
 *     g_y = (1-c_z) ((1-c_x) (v010 - v000) + c_x (v110 - v100)) + c_z ((1-c_x) (v011 - v001) + c_x (v111 - v101))
 *     g_z = (1-c_y) ((1-c_x) (v001 - v000) + c_x (v101 - v100)) + c_y ((1-c_x) (v011 - v010) + c_x (v111 - v110))
 *   each blended on raw values and then converted by SDF_valueToFloat, as s is.
 *   r = mu * s - d;   n = g * (mu / voxelSize), the quotient formed once as a float;   J = (n, x cross n), the cross product as
 *   (x_1 n_2 - x_2 n_1, x_2 n_0 - x_0 n_2, x_0 n_1 - x_1 n_0): the derivative of r for a twist (v, w) applied on the left of M.
 *   Huber, delta = cfg->huberDelta (metres): a = |r|;  a <= delta: w = 1, rho = (0.5f * r) * r;  else w = delta / a,
 *   rho = delta * (a - 0.5f * delta).
 *   Over the valid samples, added in double in a fixed order (the same call gives the same bits):
 *     f = sum rho,   nabla_k = sum (w r) J_k,   hessian[r + c * 6] = sum (w J_r) J_c      (the products are float)
 *   each rounded to float once at the end; noValid is exact.  No sample set, or n == 0: nothing is launched, the result is zeros.
 *
 * itm_aligner_align: Levenberg-Marquardt over the pose, kept in double and rounded to float once per evaluation.
 *   The linear part of dstFromSrc_in is first brought to the rotation next to it (the steps of itm_rigid_quantise).  lambda = 1.
 *   A step solves (H + lambda diag(H)) step = -nabla in double (a diagonal entry below 1e-15 in magnitude is replaced by
 *   lambda * 1e-10); the trial pose is exp(step) o pose, the twist (v, w) on the left.  It is accepted when its noValid >= cfg->minValid
 *   and its MEAN cost f / noValid is below the current one (the valid set changes with the pose: raw sums do not compare): lambda *= 0.1.
 *   Otherwise lambda *= 10.  A system that is not positive definite counts as a rejected step without an evaluation.
 *   The loop ends when max |step_k| < cfg->minStep (metres / radians: ITM_ALIGN_CONVERGED), when lambda > 1e8 (ITM_ALIGN_STALLED) or after
 *   cfg->maxEvaluations evaluations (ITM_ALIGN_MAX_EVALUATIONS).  There is no relative-decrease test: with the step size as the only
 *   criterion the last iterate lies within about a step of the fixed point.
 *   First evaluation with noValid < cfg->minValid: ITM_ALIGN_TOO_FEW_SAMPLES and dstFromSrc_out = dstFromSrc_in, bit for bit.
 *   conditioning = the smallest eigenvalue of S H S at the final pose, S = diag(a, a, a, b, b, b), 1 / a^2 = the largest of the three
 *   translational and 1 / b^2 = the largest of the three rotational diagonal entries of H (cyclic Jacobi in double; 0 when a block has
 *   no positive diagonal entry).  Metres against radians do not matter: the value does not change when either unit is rescaled.  Those
 *   two factors are all the units account for; scaling each parameter by its OWN diagonal entry (D^-1/2 H D^-1/2, D = diag(H)) reads
 *   0.69 -- well posed -- on the fused sphere-and-wall scene of the tests, whose free rotation happens to be about a coordinate axis:
 *   its diagonal entry is discretisation noise, four orders below the other two rotations, and its own square root turns it into a 1.
 *   Below cfg->minConditioning the status becomes ITM_ALIGN_DEGENERATE: the geometry does not determine the pose (a sphere in front of
 *   a wall leaves the rotation about the wall's normal through the sphere free).  The pose is still returned, its determined directions
 *   refined; the caller decides.
 * itm_align_default_config(voxelSize, mu) (host only): minWeight 1, maxAbsSdf 1, stride 1, huberDelta mu / 4, minStep 1e-5,
 * maxEvaluations 60, minValid 100, minConditioning 1e-3.  minConditioning is POLICY chosen on analytic scenes -- it lies between the
 * 4e-6 of a sphere in front of a wall and the 7e-2 of a room corner -- nobody has tuned it on sensor data.
 * ITM_ERR_INVALID with nothing changed: a null argument, a matrix entry that is not finite, an entry of R^T R - I above 1e-3 in
 * magnitude, det R < 0, huberDelta <= 0, minStep <= 0, and for itm_aligner_align no samples set.  The matrix and the configuration are
 * checked before anything else is looked at.
 *
 * Calls.  A handle owns its reduction records and serialises its own calls.  set_samples keeps the DEVICE pointer (float4 (p, d), 16-byte
 * aligned) and does not copy: the samples stay the caller's and stay alive while the handle uses them.  evaluate launches dst's recorded
 * calls first, reads dst only, enqueues ONE launch on `stream` and returns with *out filled through tagged records in page-locked host
 * memory (no stream synchronise); align is a sequence of evaluations.  itm_align_step and itm_align_apply_step are the loop's two host
 * steps on their own (host only): the step of an evaluation for a lambda (0 where the system is not positive definite), and
 * exp(step) o pose rounded to float. */
#define ITM_ALIGN_CONVERGED 0
#define ITM_ALIGN_MAX_EVALUATIONS 1
#define ITM_ALIGN_STALLED 2
#define ITM_ALIGN_TOO_FEW_SAMPLES 3
#define ITM_ALIGN_DEGENERATE 4
typedef struct itm_aligner itm_aligner;
typedef struct itm_align_config {
  int32_t minWeight;         /* band samples: w_depth a voxel needs */
  float maxAbsSdf;           /* band samples: |sdf| below this, float sdf units */
  int32_t stride;            /* band samples: every stride-th voxel per axis */
  float huberDelta;          /* metres */
  float minStep;             /* metres / radians */
  int32_t maxEvaluations, minValid;
  float minConditioning;
} itm_align_config;          /* 32 bytes */
typedef struct itm_align_eval { float f; int32_t noValid; float nabla[6]; float hessian[36]; } itm_align_eval;      /* 176 bytes */
typedef struct itm_align_result {
  int32_t status, evaluations, noValid, reserved;
  double initialCost, finalCost;      /* mean cost f / noValid at the first and at the final pose */
  double conditioning;
} itm_align_result;          /* 40 bytes */
int ITM_FN(align_default_config)(float voxelSize, float mu, itm_align_config* cfg);
int ITM_FN(align_step)(const itm_align_eval* eval, double lambda, float step[6]);
int ITM_FN(align_apply_step)(const float pose[16], const float step[6], float out[16]);
int ITM_FN(scene_band_samples)(const itm_scene* src, const int32_t* srcSlots_dev, int n, const itm_align_config* cfg, float* samples_dev, int32_t capacity,
                               int32_t* count_out, itm_stream stream);
int ITM_FN(aligner_create)(itm_aligner** out);
int ITM_FN(aligner_destroy)(itm_aligner* aligner);
int ITM_FN(aligner_set_samples)(itm_aligner* aligner, const float* samples_dev, int32_t n, itm_stream stream);
int ITM_FN(aligner_evaluate)(itm_aligner* aligner, const itm_scene* dst, const float dstFromSrc[16], const itm_align_config* cfg, itm_align_eval* out,
                             itm_stream stream);
int ITM_FN(aligner_align)(itm_aligner* aligner, const itm_scene* dst, const float dstFromSrc_in[16], const itm_align_config* cfg, float dstFromSrc_out[16],
                          itm_align_result* res, itm_stream stream);

/* The acceleration structures a hash scene carries beside the reference's table (none of them part of the reference's state, all
 * derived from it): a block directory and a slot directory over a cube of 512^3 blocks, an sdf mirror over 256^3 blocks for the
 * short voxel types.  The cubes are NOT tied to the world origin: the first frame places them around its camera (the reference's
 * table has no spatial limit, Objects/ITMVoxelBlockHash.h:22-100, and an external pose source chooses the world frame), a frame
 * whose view leaves a cube moves it (emptied and refilled from the table on the frame's stream, O(allocated blocks)).  Blocks outside
 * a cube are found through the table as the reference finds them.  origin_*: block coordinates of cell (0, 0, 0); moves: cube moves
 * since creation; *_bytes: device memory of each structure (0 = absent). */
typedef struct itm_accel_info {
  int64_t directory_bytes, slot_directory_bytes, mirror_bytes;
  int32_t origin_directory[3], origin_mirror[3];
  int32_t placed;
  int64_t moves;
  int32_t mirror_pages, mirror_pages_mapped;   /* PAGED mirror (ITM_MIRROR=paged in the environment, or a device without 3 x 17 GB to spare): 4 MB pages (16 x 16 x 16 blocks of
                                                  int16 sdf) the pool holds / has handed out (reading this synchronises the device); both 0 for the DENSE form, whose
                                                  mirror_bytes are the whole cube's 17 GB */
} itm_accel_info;
int ITM_FN(scene_accel_info)(const itm_scene* scene, itm_accel_info* out);

/* Device address of a buffer (zero-copy hand-off to e.g. a collective); NULL if absent. */
void* ITM_FN(buffer_ptr)(const itm_scene* scene, const itm_render_state* rs, int which);

/* ---- per-kernel timers (the reference wraps ProcessFrame in a stopwatch: Engine/CLIEngine.cpp:44-86,
 * Utils/NVTimer.h; here hipEvents bracket individual kernels on their stream) ------------------- */
enum itm_timed_kernel {
  ITM_TK_REQUEST = 0,       /* per-pixel block requests (buildHashAllocAndVisibleTypePP)   */
  ITM_TK_ALLOC_SWEEP = 1,   /* ordered allocation sweep                                    */
  ITM_TK_VISIBLE_LIST = 2,  /* frustum re-test + ordered compaction (2 launches)           */
  ITM_TK_INTEGRATE = 3,     /* IntegrateIntoScene kernel                                   */
  ITM_TK_RANGE = 4,         /* CreateExpectedDepths kernels                                */
  ITM_TK_RAYCAST = 5,       /* GenericRaycast kernel                                       */
  ITM_TK_ICP_MAPS = 6,      /* processPixelICP kernel                                      */
  ITM_TK_EMPTY = 7,         /* itm_profile_calibrate: event pairs with nothing between them          */
  ITM_TK_COUNT = 8
};
typedef struct itm_profile {
  int32_t calls[ITM_TK_COUNT];
  double total_ms[ITM_TK_COUNT];
} itm_profile;
/* kernel_mask: bit i enables timing of kernel i (0 disables everything).  Each timed launch costs
 * two hipEventRecord calls on the frame stream. */
int ITM_FN(profile_enable)(itm_scene* scene, uint32_t kernel_mask);
/* Time only every `every`-th launch of each enabled kernel (1 = every launch, the default): the
 * event pair costs a few microseconds of stream time, which a throughput run should not pay on
 * every frame.  The average launch duration is over the sampled launches. */
int ITM_FN(profile_sample)(itm_scene* scene, int every);
/* Records n EMPTY brackets on `stream` (slot ITM_TK_EMPTY of itm_profile): the interval an event pair measures when nothing lies
 * between the two records, i.e. what the pair itself adds to every timed kernel's figure on this machine. */
int ITM_FN(profile_calibrate)(itm_scene* scene, int n, itm_stream stream);
/* Waits for the recorded events, accumulates and returns the totals; reset != 0 clears them. */
int ITM_FN(profile_read)(itm_scene* scene, itm_profile* out, int reset);

/* Fixed-size record for the multi-stream exchange: writes
 * {float M_d[16]; int32 noVisibleEntries; int32 ids[max_ids]} (padded with -1) to `dst`
 * (device memory, (17+max_ids)*4 bytes) on `stream`, without a host round-trip. */
int ITM_FN(export_visible_record)(const itm_render_state* rs, const float M_d[16], int max_ids,
                                  void* dst, itm_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* ITM_HIP_H_ */
