// debug.hip -- the test hooks of include/itm_debug.h that own no kernel: the table of switches (debug.h), the forward-only counters of
// every handle type, the memory statistics.  Host code only.
#include "itm_internal.h"
#include "gh_reduce.h"

namespace itm {

DebugSwitches g_debug;

// the three counters of a scene
static int scene_counter(int which, itm_scene* s, const uint32_t* set, uint32_t* get) {
  if (!s) return set_error(ITM_ERR_INVALID, "null scene");
  if (which == ITM_COUNTER_FRAME_PARITY && set && ((*set ^ s->frameParity) & 1u)) return set_error(ITM_ERR_INVALID, "the frame count keeps its parity");
  uint32_t& c = which == ITM_COUNTER_LIST_EPOCH ? s->listEpoch : which == ITM_COUNTER_FRAME_PARITY ? s->frameParity : s->tableEpoch;
  if (get) *get = c;
  if (set) c = *set;
  return ITM_OK;
}

// the sequence number of a handle that is a GHHandle and nothing more to this hook
static int seq_counter(GHHandle* h, const uint32_t* set, uint32_t* get) {
  return h ? h->seq_counter(set, get) : set_error(ITM_ERR_INVALID, "null handle");
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_debug_set(int key, int value) {
  if (!DebugSwitches::known(key)) return set_error(ITM_ERR_INVALID, "unknown debug key");
  if (key == ITM_DEBUG_FAIL_ALLOCATION) memory_stats().failAt.store(value > 0 ? value : 0);      // the countdown lives where the allocations pass
  else g_debug.value[key] = value;
  return ITM_OK;
}

int itm_debug_get(int key, int* value) {
  if (!DebugSwitches::known(key)) return set_error(ITM_ERR_INVALID, "unknown debug key");
  if (!value) return set_error(ITM_ERR_INVALID, "null argument");
  *value = key == ITM_DEBUG_FAIL_ALLOCATION ? (int)memory_stats().failAt.load() : g_debug.value[key];
  return ITM_OK;
}

int itm_debug_counter(int which, void* handle, const uint32_t* set, uint32_t* get) {
  switch (which) {
    case ITM_COUNTER_LIST_EPOCH: case ITM_COUNTER_FRAME_PARITY: case ITM_COUNTER_TABLE_EPOCH:
      return scene_counter(which, (itm_scene*)handle, set, get);
    case ITM_COUNTER_TRACKER_SEQ: case ITM_COUNTER_TRACKER_SESSION: case ITM_COUNTER_TRACKER_FALLBACKS: case ITM_COUNTER_TRACKER_RELAUNCHES:
      return tracker_counter(which, (itm_tracker*)handle, set, get);
    case ITM_COUNTER_COLOUR_SEQ: return seq_counter(gh_handle((itm_colour_tracker*)handle), set, get);
    case ITM_COUNTER_REN_SEQ: return seq_counter(gh_handle((itm_ren_tracker*)handle), set, get);
    case ITM_COUNTER_POSE_QUALITY_SEQ: return seq_counter(gh_handle((itm_pose_quality_handle*)handle), set, get);
    case ITM_COUNTER_ALIGN_SEQ: return seq_counter(gh_handle((itm_aligner*)handle), set, get);
    case ITM_COUNTER_IMAGE_MAP_EPOCH: return image_map_counter((itm_stream)handle, set, get);
  }
  return set_error(ITM_ERR_INVALID, "unknown counter");
}

int itm_debug_memory(int64_t out[3]) {
  if (!out) return set_error(ITM_ERR_INVALID, "null argument");
  const MemoryStats& m = memory_stats();
  out[0] = m.live.load(); out[1] = m.liveBytes.load(); out[2] = m.attempted.load();
  return ITM_OK;
}

}  // extern "C"
