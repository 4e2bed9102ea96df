/*
 * itm_debug.h -- test hooks of libitmhip.so.  NOT part of the drop-in boundary (include/itm_hip.h): nothing here changes a result;
 * the keys select alternative code paths of the library so that every one of them has a parity test, and the probes expose device
 * routines (the reduced division sequences, the dense cull) and the tracker's host iteration to tests that check them in isolation.
 * Hosts do not include this header.
 */
#ifndef ITM_DEBUG_H_
#define ITM_DEBUG_H_

#include "itm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test hooks (no effect on results): select alternative code paths so that they can be covered. */
#define ITM_DEBUG_FORCE_GLOBAL_RANGE_ATOMICS 1 /* range image via global atomics even if it fits LDS */
#define ITM_DEBUG_EXPLICIT_MARK_PREVIOUS 2     /* always run the separate mark-previous-list launch   */
#define ITM_DEBUG_INTEGRATE_WORKGROUPS 3      /* tuning: persistent workgroups of the hash integration (0 = default); the dense strip kernel's grid reads it too */
#define ITM_DEBUG_NO_FUSED_PROJECTION 4       /* process_frame: keep integration and projection as two launches */
#define ITM_DEBUG_NO_DIRECTORY 5              /* ray casting / free-view reads walk the hash table instead of the block directory */
#define ITM_DEBUG_NO_FUSED_RANGE_REDUCE 6     /* process_frame: reduce the partial range images in their own launch, not in the ray cast */
#define ITM_DEBUG_TWO_PASS_VISIBLE_LIST 7     /* AllocateSceneFromDepth: visible list by a count launch and a compaction launch */
#define ITM_DEBUG_SINGLE_PASS_RAYCAST 8       /* ray casting: every ray start to finish in one launch (no parked-ray pass) */
#define ITM_DEBUG_DENSE_GROUP_CULL 9          /* dense integration: frustum test per 4-voxel group instead of the per-column row interval */
#define ITM_DEBUG_TRACKER_LAUNCH_PER_EVALUATION 10 /* TrackCamera: one launch per cost evaluation instead of one resident kernel per call */
#define ITM_DEBUG_TRACKER_HOST_COMMAND 11     /* TrackCamera session: commands through pinned host memory even where the device has a large BAR (set before the tracker's first call) */
#define ITM_DEBUG_NO_SDF_MIRROR 12            /* ray casting: voxels through the directory / table although the scene has an sdf mirror; set before itm_scene_create: no mirror is allocated */
#define ITM_DEBUG_SEPARATE_SWEEP 13           /* AllocateSceneFromDepth: allocation sweep as its own launch, not inside the visible-list launch */
#define ITM_DEBUG_NO_SIDE_PROJECTION 14       /* itm_process_frame on large images: projection of the visible blocks after the integration on the frame's stream, not beside it on the render state's own */
#define ITM_DEBUG_DENSE_RANGE_REFILL 15       /* dense scenes: write the constant expected-depth image on every frame, as the reference does, although it already holds it */
#define ITM_DEBUG_DENSE_CLASSIFY 16            /* dense integration: 0 = 4-voxel groups classified against the depth tiles before the fetch (default), 1 = no classification, 2 = classified after the fetch, 3 = check mode (itm_debug_dense_classify_check) */
#define ITM_DEBUG_DENSE_NO_STRIPS 17           /* dense integration: the launch shape of rounds 1-2 (four groups per lane, 131 072 short waves) instead of the strip kernel */
#define ITM_DEBUG_TRACKER_SESSION_UNUSABLE 18  /* TrackCamera: the resident evaluation kernel reports itself unusable at the n-th evaluation of a handle (n = value): the call must finish through one launch per evaluation with the same pose */
#define ITM_DEBUG_NO_DEFERRED_FUSION 19         /* the four per-frame engine calls launch at once, one by one, instead of being recorded and fused (see "the four calls" below) */
#define ITM_DEBUG_FORCE_LIST_STUCK 20           /* AllocateSceneFromDepth, one-launch visible list: chunk n - 1 behaves as if its bounded wait for another workgroup had expired (0 = off): the scene must raise statusFlags bit 1 and refuse further calls */
#define ITM_DEBUG_EXCHANGE_DEVICE_COPY 24        /* exchanges created while it is set: a ONE-rank exchange performs its collective as a device copy instead of ncclAllGather (a test pins both to the same table) */
#define ITM_DEBUG_EXCHANGE_CORRUPT_WORD 25       /* exchanges created while it is >= 0: the self-check behind every collective sees this word of the rank's own block flipped (the check must fire); -1 = off */
#define ITM_DEBUG_MESH_ATTR_PER_VERTEX 26        /* itm_mesh_attributes: one lane per vertex reading through the hash instead of one workgroup per block reading from LDS */
#define ITM_DEBUG_MESH_INDEX_WEAK_HASH 27        /* itm_mesh_index: the hash cut to 8 bits (256 start slots spread over the table, the last 64 slots before its end): probe chains hundreds of slots long and the wrap-around on small meshes */
#define ITM_DEBUG_FAIL_ALLOCATION 28             /* n > 0: the n-th allocation the library attempts from now on (device or pinned memory) fails with out-of-memory before the runtime is called, then the key clears itself; 0 = off */
#define ITM_DEBUG_POSE_QUALITY_ROWS 29            /* itm_pose_quality_evaluate: a wave covers 64 x 1 pixels of a row instead of an 8 x 8 tile (same counts and residual image; the sums are added in another order) */
#define ITM_DEBUG_MESH_COMPONENTS_PER_LANE 30      /* itm_mesh_components: the statistics with one atomic per lane instead of one per wave segment (lanes of a wave that share a component aggregate first) */
#define ITM_DEBUG_MESH_SMOOTH_SCATTER 31            /* itm_mesh_smooth: every pass as a scatter -- one lane per proper triangle adds its corners into per-vertex int64 accumulators with 64-bit integer atomics, a second kernel applies the step -- instead of the gather over the adjacency rows (same bits by construction) */
#define ITM_DEBUG_KEY_COUNT 32                      /* every key is below it; 0 and 21-23 are not keys */
/* itm_debug_set stores a key's value, itm_debug_get reads it back into *value (what FAIL_ALLOCATION still has to count down): every
 * key starts at 0, EXCHANGE_CORRUPT_WORD at -1.  A number that is not a key is refused with ITM_ERR_INVALID.  Host only. */
int ITM_FN(debug_set)(int key, int value);
int ITM_FN(debug_get)(int key, int* value);
/* The forward-only 32-bit counters behind the tagged granules (DESIGN.md "Forward-only counters"): reads one counter of one handle into
 * *get (may be NULL) and then, when set is not NULL, replaces it with *set -- so that a test can place a handle a few steps before the
 * roll-over that 2^32 frames of uptime would reach.  Only the number changes: no buffer is touched, no result depends on where a counter
 * stands, and a process that never calls this runs the code it always ran.  The caller keeps the handle idle during the call (no engine
 * call of another thread, nothing recorded and unflushed).  Host only, but for the image maps' first use of a stream (below).
 *   handle            counter
 *   itm_scene*        LIST_EPOCH    epoch of the last one-launch visible list (stamps of chunkGran / chunkSweepDone / chunkKeptGran)
 *                     FRAME_PARITY  allocations so far; its lowest bit selects the half of the request counters (set a value of the same parity)
 *                     TABLE_EPOCH   resets / replacements of the hash table
 *   itm_tracker*      TRACKER_SEQ   sequence number of the last evaluation (tag of commands and records); NULL = the calling thread's own
 *                     TRACKER_SESSION  number of the last resident evaluation kernel; where the handle has had a session, the pinned
 *                                   "exited" word with it, as if that kernel had run and left
 *                     TRACKER_FALLBACKS, TRACKER_RELAUNCHES  read only: sessions given up for one launch per evaluation / sessions
 *                                   replaced because the previous one seemed to have left without an answer
 *   itm_colour_tracker*, itm_ren_tracker*, itm_pose_quality_handle*, itm_aligner*   COLOUR_SEQ, REN_SEQ, POSE_QUALITY_SEQ, ALIGN_SEQ: as TRACKER_SEQ
 *   itm_stream        IMAGE_MAP_EPOCH  epoch of the last image-map call on this stream of the current device (the slot is created if
 *                                   the stream has none yet; that allocates and zeroes a block of slots exactly as a first GetImage would) */
#define ITM_COUNTER_LIST_EPOCH 1
#define ITM_COUNTER_FRAME_PARITY 2
#define ITM_COUNTER_TABLE_EPOCH 3
#define ITM_COUNTER_TRACKER_SEQ 4
#define ITM_COUNTER_TRACKER_SESSION 5
#define ITM_COUNTER_TRACKER_FALLBACKS 6
#define ITM_COUNTER_TRACKER_RELAUNCHES 7
#define ITM_COUNTER_COLOUR_SEQ 8
#define ITM_COUNTER_REN_SEQ 9
#define ITM_COUNTER_POSE_QUALITY_SEQ 10
#define ITM_COUNTER_IMAGE_MAP_EPOCH 11
#define ITM_COUNTER_ALIGN_SEQ 12
int ITM_FN(debug_counter)(int which, void* handle, const uint32_t* set, uint32_t* get);
/* Everything the library allocates passes through one pair of functions (csrc/device_memory.h): out = {live allocations, live bytes,
 * allocations attempted since the library was loaded}, device and pinned memory together, process-wide.  Memory handed out by
 * itm_dev_malloc / itm_host_malloc is the host's and is not counted.  Host only: touches no GPU state. */
int ITM_FN(debug_memory)(int64_t out[3]);
/* A stand-in for a device-side consumer of the exchange's table (tests of itm_exchange_acquire): dst[0] = sum over `rounds` passes of a
 * position-weighted checksum of src[0 .. words), computed by ONE workgroup on `stream` -- slow on purpose, so that collectives of later
 * batches run while it reads. */
int ITM_FN(debug_checksum)(const int32_t* src, size_t words, int rounds, unsigned long long* dst, itm_stream stream);
/* dense integration, check mode of key 16: {free groups, shadow groups, mixed groups, violations}; reset != 0 clears */
int ITM_FN(debug_dense_classify_check)(int32_t out[4], int reset);
/* Test hook (host only): rows [rlo, rhi] of the column of 4-voxel groups (x0 .. x0 + 3, slice z) that the dense integration visits for
 * a volume of `size` voxels at `offset` seen from M_d; every voxel of the column outside that interval must fail the exact
 * projection test of computeUpdatedVoxelDepthInfo.  Returns 1 when no cull planes can be formed (the kernel then tests per group). */
int ITM_FN(debug_column_cull_rows)(const float M_d[16], const float intr[4], int w, int h, float voxelSize, const int size[3],
                                   const int offset[3], int x0, int z, int* rlo, int* rhi);
/* out[i] = SDF_valueToFloat(in[i]) of the short voxel types, i.e. in[i] / 32767.0f, through the same
 * device routine the kernels use (a 3-instruction correctly rounded division; test hook). */
int ITM_FN(debug_div32767)(const float* in, float* out, int n, itm_stream stream);
/* out[i] = a[i] / b[i] through the reduced division sequences of the integration kernel (mode 1: shared
 * refined reciprocal; 2: small-integer divisor; 3: the refined reciprocal of b; 4: reciprocal given in r). */
int ITM_FN(debug_divide)(int mode, const float* a, const float* b, const float* r, float* out, int n, itm_stream stream);
/* The ordered compaction behind the visible list, FindVisibleBlocks, the mesher's slot list and the forward projection, in isolation:
 * the n flags (HOST memory, elemBytes = 1: bytes as the hash callers pass them, n a multiple of 8; elemBytes = 4: int32 as the pixel
 * callers do, any n) are copied to the device, counted per chunk of 2048 by a kernel of the hook's own and listed by the product
 * launcher.  ids_host holds cap + ITM_DEBUG_ORDERED_GUARD entries: all of them are uploaded as the device list's contents before the
 * launch and downloaded after it, so the caller sees every word the launch wrote -- the first min(total, cap) indices of the non-zero
 * flags, ascending, and its own pattern everywhere else, also in the guard words past cap.  counts = {total, min(total, cap)}. */
#define ITM_DEBUG_ORDERED_GUARD 8
int ITM_FN(debug_ordered_compact)(const void* flags_host, int elemBytes, int n, int cap, int32_t* ids_host, int32_t counts[2], itm_stream stream);
/* The labelling of itm_mesh_components on a caller-supplied face array (the triangle buffer cannot be uploaded): faces_host holds
 * noTriangles x 3 vertex indices < noVertices (an index >= noVertices: ITM_ERR_INVALID); the product's union / check / numbering / count
 * kernels run on it.  vertexComponent_host receives noVertices numbers, components_host min(noComponents, capComponents) entries with
 * the box left zero (it needs positions); a vertex no triangle names is a component of its own with 0 triangles.  *rounds = the union
 * rounds taken.  All pointers are HOST memory; vertexComponent_host and components_host may be NULL. */
int ITM_FN(debug_mesh_components)(const uint32_t* faces_host, uint32_t noTriangles, uint32_t noVertices, uint32_t* vertexComponent_host,
                                  itm_mesh_component* components_host, uint32_t capComponents, uint32_t* noComponents, uint32_t* rounds,
                                  itm_stream stream);
/* itm_mesh_smooth on caller-supplied arrays (the triangle buffer cannot be uploaded): vertices_host holds noVertices x float[3],
 * faces_host noTriangles x 3 vertex indices < noVertices (an index >= noVertices: ITM_ERR_INVALID); the product's adjacency / topology /
 * quantise / pass / dequantise kernels run on them.  vertices_out_host receives the noVertices smoothed positions, flags_out_host (may be
 * NULL) one byte per vertex: bit 0 irregular, bit 1 isolated.  A refused call (also a coordinate out of range or not finite) writes
 * nothing into either.  With cfg->steps == 0 vertices_out_host receives the input.  All pointers are HOST memory.
 * Cost: the multiplicity count of a row of n entries is n^2 comparisons, by one lane up to 128 entries and by one wave (n^2 / 64 per
 * lane) above.  Marching-cubes meshes stay at or below 40 entries; a hand-made apex of 10 000 entries is 10^8 comparisons, some
 * milliseconds, and the time grows with the square: keep the rows handed to this hook below some 10^5 entries. */
int ITM_FN(debug_mesh_smooth)(const float* vertices_host, uint32_t noVertices, const uint32_t* faces_host, uint32_t noTriangles,
                              const itm_mesh_smooth_config* cfg, float* vertices_out_host, uint8_t* flags_out_host,
                              itm_mesh_smooth_stats* stats, itm_stream stream);

/* Read-only probes of the acceleration cubes of a hash scene (block directory, slot directory, sdf mirror: itm_types.h).  Both launch
 * the scene's recorded, unflushed engine calls first, as a download does, and only read; a scene without directories, without a mirror
 * or with a dense index reports "nothing" (no cube covers anything, every count is 0).  All pointers are HOST memory.
 * itm_debug_accel_probe: for each of the n block positions (int32[n][3]) cells[i] = {the directory cube covers it, its dirPtr cell, its
 * dirSlot cell (-1 where not covered), the mirror cube covers it, its page-table entry (paged form; -1 otherwise), the block has NO place
 * in the mirror (outside the cube, page unmapped or unmappable, no mirror)} and values[i] = the 512 mirror values of the block in the
 * block's own voxel order x + 8 y + 64 z as stored: int16 for the short voxel types, uint32 for the float types ("absent" -- -32768 /
 * 0xffffffff -- where the block has no place). */
#define ITM_ACCEL_PROBE_CELLS 6
int ITM_FN(debug_accel_probe)(const itm_scene* scene, const int32_t* positions, int n, int32_t* cells, void* values, itm_stream stream);
/* itm_debug_accel_census: a full pass over the cubes on the device.  mirror_blocks counts the blocks with at least one cell that is not
 * "absent": over the whole cube (dense form) or over every page of the pool, mapped or not (paged form).  pageTable (may be null)
 * receives the 4096 entries of the page table (-1 everywhere unless the mirror is paged); page_counter is the pool's raw counter. */
typedef struct itm_accel_census {
  int64_t directory_cells;       /* dirPtr cells != -1 */
  int64_t slot_directory_cells;  /* dirSlot cells != -1 */
  int64_t mirror_blocks;
  int32_t page_counter;
  int32_t mirror_form;           /* 0 none, 1 dense, 2 paged */
  int32_t has_directory;
  int32_t reserved;
} itm_accel_census;
int ITM_FN(debug_accel_census)(const itm_scene* scene, itm_accel_census* out, int32_t* pageTable, itm_stream stream);

/* Test hook (host only, no device work): the tracker's host-side iteration (level schedule, accept / reject damping, SE(3)
 * update) driven by a caller-supplied evaluator of cost / gradient / Hessian, so that it can be checked on a machine without
 * a GPU against ITMDepthTracker::TrackCamera with the same evaluator.  `evaluate` returns 0 on success. */
typedef int (*itm_icp_evaluate_fn)(void* user, int level, int iterationType, const float approxInvPose[16],
                                   float distThresh, itm_tracker_gh* out);
int ITM_FN(debug_icp_track)(const itm_tracker_config* cfg, const float M_d[16], itm_icp_evaluate_fn evaluate,
                            void* user, float M_d_out[16]);
/* Test hook (host only, no device work): the weighted ICP tracker's host iteration (ITMWeightedICPTracker::TrackCamera: level
 * schedule, undamped step, SE(3) update) driven by a caller-supplied evaluator of the weighted sums -- the WICP twin of
 * itm_debug_icp_track. */
int ITM_FN(debug_wicp_track)(const itm_tracker_config* cfg, const float M_d[16], itm_icp_evaluate_fn evaluate,
                             void* user, float M_d_out[16]);

/* Measurement hook of the keyframe relocaliser (tools/reloc_bench.py): enable != 0 brackets the two search launches of every later
 * itm_reloc_find / itm_reloc_process_frame on this handle with device events (two event records per call; off by default).  *ms, when
 * not NULL, receives the device time of the last bracketed search, -1 if there is none. */
int ITM_FN(debug_reloc_search_ms)(struct itm_reloc* reloc, int enable, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* ITM_DEBUG_H_ */
