// mesh_update.hip -- itm_mesh_touch / itm_mesh_update: the triangle buffer follows the scene at the cost of the blocks a frame touched
// (include/itm_hip.h "Incremental mesh", DESIGN.md "Incremental mesh").
//
// No reference engine re-meshes a part of the scene; the definition rests on one that exists:
//   MeshScene     the loop over a block and the order of the buffer (meshing.hip, mesh_cells.h, mc_device.h)
//
// MI355X design.  Everything on one stream, one read-back in the middle (the totals, which also decide the fall-back):
//   diff          one pass over the table, one 256-lane workgroup per chunk of 2048 slots, eight slots per lane: each entry against the run
//                 table's key of its slot gives present / appeared / vanished; a seed (marked and present, appeared, vanished) looks up
//                 the eight blocks at -d through the slot directory (the table walk outside its cube) and sets their dirty bytes.
//   lists         three ordered compactions (ordered_device.h): A' into the mesh's slot list, the removed, the dirty.
//   count         mesh_cells_kernel<COUNT> over the dirty list only.
//   prefixes      per listed block the new count (dirty: counted; kept: the run table's), the carry scan of itm_mesh_scene over A', the new
//                 run table; the dirty blocks learn where they write.
//   -- read-back: statistics and totals --
//   write         mesh_cells_kernel<WRITE> over the dirty list into the second buffer.
//   copy          one wave per kept block: its run moves as dwords, consecutive lanes on consecutive dwords (a run of 36-byte triangles
//                 is only 4-byte aligned at either end), from the old buffer at the old prefix to the new one at the new prefix.
//   delta         the changed blocks from the dirty list and the new run table.
// Cost: O(entries) of 16-byte loads for the diff, O(|D|) marching cubes, O(triangles) plain copy.
#include <algorithm>
#include <utility>

#include "itm_internal.h"
#include "mesh_cells.h"
#include "mesh_types.h"
#include "scene_ops.h"

namespace itm {

// the statistics in device memory: itm_mesh_update_stats word for word, then the words that outlive a call
enum { kUsFull, kUsAllocated, kUsMarked, kUsIgnored, kUsAppeared, kUsVanished, kUsRemeshed, kUsKept, kUsBefore, kUsAfter, kUsCopied, kUsGenerated,
       kUsChanged, kUsRemoved, kUsPerCall = 16, kUsIgnoredSoFar = 16 /* by the touches since the last update */,
       kUsRunFitted /* every triangle of the recorded run table is in the buffer */, kUsCount = 32 };
static_assert(sizeof(itm_mesh_update_stats) == 16 * 4, "itm_mesh_update_stats layout");
static_assert(sizeof(itm_mesh_changed_block) == 20 && sizeof(itm_mesh_removed_block) == 12, "delta layouts");

// statistics | run table x 2 | marks | dirty bytes | removed flags | their chunk counts | count by slot | dirty list | its counts, then
// bases | removed slots | the dirty list's length | the delta.  N: table entries, padded: chunks * kSweepChunk, cap: blocks of the pool.
struct UpdateArena {
  ScratchLayout L; ScratchPart<int32_t> stats; ScratchPart<Bytes16> run0, run1; ScratchPart<uint8_t> marks, dirty, removedFlags;
  ScratchPart<int32_t> chunkRemoved, chunkDirty, slotCount, dirtyList, dirtyTri, removedSlots; ScratchPart<RenderCounters> dirtyCount;
  ScratchPart<itm_mesh_changed_block> changed; ScratchPart<itm_mesh_removed_block> removed;
  UpdateArena(size_t N, size_t padded, size_t chunks, size_t cap)
      : stats(L.take<int32_t>(kUsCount)), run0(L.take<Bytes16>(N)), run1(L.take<Bytes16>(N)), marks(L.take<uint8_t>(padded)), dirty(L.take<uint8_t>(padded)),
        removedFlags(L.take<uint8_t>(padded)), chunkRemoved(L.take<int32_t>(chunks)), chunkDirty(L.take<int32_t>(chunks)), slotCount(L.take<int32_t>(N)),
        dirtyList(L.take<int32_t>(cap)), dirtyTri(L.take<int32_t>(cap)), removedSlots(L.take<int32_t>(cap)), dirtyCount(L.take<RenderCounters>(1)),
        changed(L.take<itm_mesh_changed_block>(cap)), removed(L.take<itm_mesh_removed_block>(cap)) {}
};
static UpdateArena arena_of(const itm_mesh* m) {
  const itm_scene* s = m->scene;
  return UpdateArena((size_t)s->noTotalEntries, (size_t)s->numChunks * kSweepChunk, (size_t)s->numChunks, (size_t)m->capBlocks);
}

// a run table entry: {px | py << 16, pz | listed << 16, first triangle, count}
__device__ inline uint4 run_entry(const HashEntry& he, uint32_t first, uint32_t count) {
  return make_uint4(((uint32_t)he.px & 0xffffu) | ((uint32_t)he.py << 16), ((uint32_t)he.pz & 0xffffu) | 0x10000u, first, count);
}
__device__ inline bool run_listed(const uint4& r) { return (r.y >> 16) != 0u; }
__device__ inline void run_position(const uint4& r, int& px, int& py, int& pz) {
  px = (int)(int16_t)(r.x & 0xffffu); py = (int)(int16_t)(r.x >> 16); pz = (int)(int16_t)(r.y & 0xffffu);
}

struct UpdateTable {      // the scene's table as the diff reads it
  const uint4* hash; const int32_t* dirSlot; AccelOrigin org; uint32_t mask; int bucketNum, noTotalEntries;
};

// the slot of the entry that holds block (bx, by, bz) with ptr >= 0, or -1: one load inside the slot directory's cube (its cells are
// exactly those entries), a bounded table walk that stays inside the table elsewhere
__device__ inline int find_block_slot(const UpdateTable& t, int bx, int by, int bz) {
  if ((int)(int16_t)bx != bx || (int)(int16_t)by != by || (int)(int16_t)bz != bz) return -1;      // beyond the table's short coordinates
  if (t.dirSlot) {
    const uint32_t ux = (uint32_t)(bx - t.org.dx), uy = (uint32_t)(by - t.org.dy), uz = (uint32_t)(bz - t.org.dz);
    if (dir_covers(ux, uy, uz)) {
      const int slot = t.dirSlot[dir_cell(ux, uy, uz)];
      return slot >= 0 && slot < t.noTotalEntries ? slot : -1;
    }
  }
  int idx = hash_index(bx, by, bz, t.mask);
  HashEntry e = unpack_entry(t.hash[idx]);
  for (int steps = 0; steps <= t.noTotalEntries - t.bucketNum; ++steps) {
    if (e.px == bx && e.py == by && e.pz == bz && e.ptr >= 0) return idx;
    if (e.offset < 1) return -1;
    idx = t.bucketNum + e.offset - 1;
    if (idx >= t.noTotalEntries) return -1;
    e = unpack_entry(t.hash[idx]);
  }
  return -1;
}

// marks[ids[i]] = 1 for i < n, where n = the list's own count on the device (rc) clamped to `cap`, or `cap` itself
__global__ void __launch_bounds__(256) mesh_touch_kernel(const int32_t* __restrict__ ids, const RenderCounters* __restrict__ rc, int cap, int nEntries,
                                                         uint8_t* __restrict__ marks, int32_t* __restrict__ stats) {
  const int n = rc ? min(max(rc->noVisibleEntries, 0), cap) : cap;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int slot = ids[i];
    if (slot < 0 || slot >= nEntries) atomicAdd(&stats[kUsIgnoredSoFar], 1);
    else marks[slot] = 1;                                  // (duplicates count once)
  }
}

// The diff.  present / removedFlags: a byte per slot; their per-chunk counts.  HAVE_RUN false (the run table is not current): presence
// and marks only.  runNew is cleared where no block is listed now (the listed ones are written once the prefixes are known).
template <bool HAVE_RUN>
__global__ void __launch_bounds__(256) mesh_diff_kernel(UpdateTable tb, const uint4* __restrict__ runOld, uint4* __restrict__ runNew, const uint8_t* __restrict__ marks,
                                                        uint8_t* __restrict__ present, int32_t* __restrict__ chunkPresent, uint8_t* __restrict__ removedFlags,
                                                        int32_t* __restrict__ chunkRemoved, uint8_t* dirty, int32_t* __restrict__ stats,
                                                        const uint32_t* __restrict__ totals) {
  __shared__ int lds[4];
  const int slot0 = blockIdx.x * kSweepChunk + threadIdx.x * 8;
  SlotBytes pb, rb;
  int nMarked = 0, nAppeared = 0, nVanished = 0;
  // every block whose cells read block (px, py, pz): the eight at -d
  auto seed = [&](int px, int py, int pz) {
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const int s = find_block_slot(tb, px - (d & 1), py - ((d >> 1) & 1), pz - (d >> 2));
      if (s >= 0) dirty[s] = 1;
    }
  };
  if (slot0 < tb.noTotalEntries) {
    const SlotBytes mk = SlotBytes::load(marks + slot0);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int slot = slot0 + k;
      if (slot >= tb.noTotalEntries) break;
      const HashEntry he = unpack_entry(tb.hash[slot]);
      const bool now = he.ptr >= 0, marked = mk.get(k) != 0u;
      nMarked += marked ? 1 : 0;
      if (now) pb.set(k, 1u);
      if (HAVE_RUN) {
        const uint4 r = runOld[slot];
        const uint4 key = run_entry(he, 0u, 0u);
        const bool was = run_listed(r), same = was && now && r.x == key.x && r.y == key.y;
        const bool appeared = now && !same, vanished = was && !same;
        nAppeared += appeared ? 1 : 0; nVanished += vanished ? 1 : 0;
        if (now && (marked || appeared)) seed(he.px, he.py, he.pz);
        if (vanished) {
          int ox, oy, oz;
          run_position(r, ox, oy, oz);
          seed(ox, oy, oz);
          if (find_block_slot(tb, ox, oy, oz) < 0) rb.set(k, 1u);
        }
      }
      if (!now) runNew[slot] = make_uint4(0u, 0u, 0u, 0u);
    }
    pb.store(present + slot0);
    rb.store(removedFlags + slot0);
  }
  const int nPresent = block_reduce_sum<4>(pb.count(), lds), nRemoved = block_reduce_sum<4>(rb.count(), lds);
  nMarked = block_reduce_sum<4>(nMarked, lds); nAppeared = block_reduce_sum<4>(nAppeared, lds); nVanished = block_reduce_sum<4>(nVanished, lds);
  if (threadIdx.x == 0) {
    chunkPresent[blockIdx.x] = nPresent; chunkRemoved[blockIdx.x] = nRemoved;
    if (nMarked) atomicAdd(&stats[kUsMarked], nMarked);
    if (nAppeared) atomicAdd(&stats[kUsAppeared], nAppeared);
    if (nVanished) atomicAdd(&stats[kUsVanished], nVanished);
    if (blockIdx.x == 0) { stats[kUsBefore] = (int32_t)totals[1]; stats[kUsIgnored] = stats[kUsIgnoredSoFar]; }
  }
}

// the dirty bytes as flags (0 / 1) with their per-chunk counts
__global__ void __launch_bounds__(256) mesh_dirty_flag_kernel(int nEntries, uint8_t* flags, int32_t* __restrict__ chunkCount) {
  flag_chunk(nEntries, flags, chunkCount, [&](int slot) { return flags[slot] != 0; });
}

// removed[j] = the slot and the old position of the j-th removed block
__global__ void __launch_bounds__(256) mesh_removed_kernel(const int32_t* __restrict__ removedSlots, const int32_t* __restrict__ count, int cap, const uint4* __restrict__ runOld,
                                                           itm_mesh_removed_block* __restrict__ removed) {
  const int n = min(*count, cap);
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    const int slot = removedSlots[j];
    int px, py, pz;
    run_position(runOld[slot], px, py, pz);
    itm_mesh_removed_block out;
    out.slot = slot; out.pos[0] = (int16_t)px; out.pos[1] = (int16_t)py; out.pos[2] = (int16_t)pz; out.reserved = 0;
    removed[j] = out;
  }
}

// slotCount[slot of dirty block j] = its counted triangles
__global__ void __launch_bounds__(256) mesh_dirty_counts_kernel(const int32_t* __restrict__ dirtyList, const RenderCounters* __restrict__ dirtyCount,
                                                                const int32_t* __restrict__ dirtyTri, int32_t* __restrict__ slotCount) {
  const int n = dirtyCount->noVisibleEntries;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) slotCount[dirtyList[j]] = dirtyTri[j];
}

__device__ inline void tally_words(int32_t* __restrict__ stats, int which, int v) {      // one atomic per wave; every lane of the wave calls
  const int n = wave_reduce_sum(v);
  if (n && lane_id() == 0) atomicAdd(&stats[which], n);
}

// blockTriangles[i] = the triangles of listed block i in the new buffer: counted where dirty, the old run's elsewhere
__global__ void __launch_bounds__(256) mesh_new_counts_kernel(const int32_t* __restrict__ slots, const RenderCounters* __restrict__ lc, const uint8_t* __restrict__ dirty,
                                                              const int32_t* __restrict__ slotCount, const uint4* __restrict__ runOld,
                                                              int32_t* __restrict__ blockTriangles, int32_t* __restrict__ stats) {
  const int n = lc->noVisibleEntries;
  const int rounds = (n + gridDim.x * blockDim.x - 1) / (gridDim.x * blockDim.x);
  for (int r = 0; r < rounds; ++r) {                       // (whole waves go round: the tallies are wave reductions)
    const int i = (r * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    int isDirty = 0, isKept = 0, copied = 0, generated = 0;
    if (i < n) {
      const int slot = slots[i];
      isDirty = dirty[slot] != 0; isKept = !isDirty;
      const int c = isDirty ? slotCount[slot] : (int)runOld[slot].w;
      blockTriangles[i] = c;
      if (isDirty) generated = c; else copied = c;
    }
    tally_words(stats, kUsRemeshed, isDirty); tally_words(stats, kUsKept, isKept);
    tally_words(stats, kUsCopied, copied); tally_words(stats, kUsGenerated, generated);
  }
}

// After the scan: the new run table for A', and where each dirty block writes.
__global__ void __launch_bounds__(256) mesh_new_runs_kernel(const uint4* __restrict__ hash, const int32_t* __restrict__ slots, const RenderCounters* __restrict__ lc,
                                                            const uint8_t* __restrict__ dirty, const int32_t* __restrict__ slotCount, const uint4* __restrict__ runOld,
                                                            const int32_t* __restrict__ blockTriangles, uint4* __restrict__ runNew,
                                                            const int32_t* __restrict__ dirtyList, const RenderCounters* __restrict__ dirtyCount,
                                                            int32_t* __restrict__ dirtyTri) {
  const int n = lc->noVisibleEntries, nDirty = dirtyCount->noVisibleEntries;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int slot = slots[i];
    const bool isDirty = dirty[slot] != 0;
    const uint32_t first = (uint32_t)blockTriangles[i], c = isDirty ? (uint32_t)slotCount[slot] : runOld[slot].w;
    runNew[slot] = run_entry(unpack_entry(hash[slot]), first, c);
    if (isDirty) {
      const uint32_t j = lower_bound(dirtyList, (uint32_t)nDirty, (uint32_t)slot);
      if (j < (uint32_t)nDirty) dirtyTri[j] = (int32_t)first;
    }
  }
}

// The run table of the buffer itm_mesh_scene has just written: blockTriangles holds the prefixes, totals[0] closes the last run.  `run`
// was cleared before.
__global__ void __launch_bounds__(256) mesh_record_kernel(const uint4* __restrict__ hash, const int32_t* __restrict__ slots, const RenderCounters* __restrict__ lc,
                                                          const int32_t* __restrict__ blockTriangles, const uint32_t* __restrict__ totals, uint32_t maxTriangles,
                                                          uint4* __restrict__ run, int32_t* __restrict__ stats) {
  const int n = lc->noVisibleEntries;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int slot = slots[i];
    const uint32_t first = (uint32_t)blockTriangles[i], next = i + 1 < n ? (uint32_t)blockTriangles[i + 1] : totals[0];
    run[slot] = run_entry(unpack_entry(hash[slot]), first, next - first);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) stats[kUsRunFitted] = totals[0] <= maxTriangles - 1u ? 1 : 0;
}

// changed[j] = listed block j of `list` with its run in `run`
__global__ void __launch_bounds__(256) mesh_changed_kernel(const int32_t* __restrict__ list, const RenderCounters* __restrict__ count, const uint4* __restrict__ run,
                                                           itm_mesh_changed_block* __restrict__ changed) {
  const int n = count->noVisibleEntries;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    const int slot = list[j];
    const uint4 r = run[slot];
    int px, py, pz;
    run_position(r, px, py, pz);
    itm_mesh_changed_block out;
    out.slot = slot; out.pos[0] = (int16_t)px; out.pos[1] = (int16_t)py; out.pos[2] = (int16_t)pz; out.reserved = 0;
    out.firstTriangle = r.z; out.noTriangles = r.w;
    changed[j] = out;
  }
}

// One wave per kept block: its run, nine dwords per triangle, from src at the old prefix to dst at the new one.
__global__ void __launch_bounds__(256) mesh_copy_runs_kernel(const int32_t* __restrict__ slots, const RenderCounters* __restrict__ lc, const uint8_t* __restrict__ dirty,
                                                             const uint4* __restrict__ runOld, const uint4* __restrict__ runNew, const uint32_t* __restrict__ src,
                                                             uint32_t* __restrict__ dst) {
  const int n = lc->noVisibleEntries, lane = lane_id();
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / kWave, waves = gridDim.x * blockDim.x / kWave;
  for (int i = wave; i < n; i += waves) {
    const int slot = slots[i];
    if (dirty[slot]) continue;                             // (uniform)
    const uint4 from = runOld[slot], to = runNew[slot];
    const uint32_t words = from.w * 9u;
    const uint32_t* p = src + (size_t)from.z * 9u;
    uint32_t* q = dst + (size_t)to.z * 9u;
    for (uint32_t k = (uint32_t)lane; k < words; k += (uint32_t)kWave) q[k] = p[k];
  }
}

constexpr int kListGrid = 256;            // workgroups of the launches that stride over a list whose length is on the device

hipError_t alloc_update_arena(const itm_scene* s, itm_mesh* m) {
  const UpdateArena a = arena_of(m);
  hipError_t e = m->update.alloc(a.L.bytes());
  if (e == hipSuccess) e = hipMemset(m->update.get(), 0, a.L.bytes());
  (void)s;
  return e;
}

static UpdateTable update_table(const itm_scene* s) {
  return UpdateTable{s->hash, debug_value(ITM_DEBUG_NO_DIRECTORY) ? nullptr : s->dirSlot.get(), s->org, (uint32_t)(s->cfg.bucketNum - 1), s->cfg.bucketNum, s->noTotalEntries};
}

int record_run_table(const itm_scene* s, itm_mesh* m, hipStream_t st) {
  const UpdateArena a = arena_of(m);
  void* base = m->update.get();
  uint4* run = (m->runCurrentHalf ? a.run1 : a.run0).at<uint4>(base);
  ITM_HIP(hipMemsetAsync(run, 0, (size_t)s->noTotalEntries * sizeof(uint4), st));
  mesh_record_kernel<<<kListGrid, 256, 0, st>>>(s->hash, m->slots, m->listCounters, m->blockTriangles, m->totals, m->maxTriangles, run, a.stats.at(base));
  ITM_LAUNCH_CHECK();
  m->run_table_recorded();
  return ITM_OK;
}

// the refusals the two entry points share
static int check_update_pair(const itm_scene* s, const itm_mesh* m, const char* what) {
  if (!s || !m) return refuse(what, "null scene or mesh");
  if (m->scene != s) return refuse(what, "mesh belongs to another scene");
  if (s->cfg.indexType != ITM_INDEX_HASH) return refuse(what, "a dense scene has no blocks to follow (itm_mesh_volume meshes it)");
  return ITM_OK;
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_mesh_touch(itm_mesh* m, const itm_scene* s, const itm_render_state* rs, const int32_t* slots_dev, int n, itm_stream stream) {
  { const int rc = check_update_pair(s, m, "mesh touch"); if (rc) return rc; }
  if (rs && (rs->scene != s || !rs->hash || !rs->visibleIds)) return refuse("mesh touch", "the render state belongs to another scene");
  if (slots_dev && n < 0) return refuse("mesh touch", "negative slot count");
  if (!rs && !slots_dev && n != -1) return refuse("mesh touch", "no list: n must be -1 (everything)");
  { const int rc = enter_scene(s, rs); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  const UpdateArena a = arena_of(m);
  void* base = m->update.get();
  if (!rs && !slots_dev) { m->allMarked = true; return ITM_OK; }
  if (rs) {
    const int cap = std::min(rs->capIds, s->cfg.localBlockNum);
    if (cap > 0) mesh_touch_kernel<<<std::min((cap + 255) / 256, 1024), 256, 0, st>>>(rs->visibleIds, rs->counters, cap, s->noTotalEntries, a.marks.at(base), a.stats.at(base));
  }
  if (slots_dev && n > 0) mesh_touch_kernel<<<std::min((n + 255) / 256, 1024), 256, 0, st>>>(slots_dev, nullptr, n, s->noTotalEntries, a.marks.at(base), a.stats.at(base));
  ITM_LAUNCH_CHECK();
  return ITM_OK;
}

int itm_mesh_update(const itm_scene* s, itm_mesh* m, itm_mesh_update_stats* stats, itm_stream stream) {
  { const int rc = check_update_pair(s, m, "mesh update"); if (rc) return rc; }
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  const UpdateArena a = arena_of(m);
  void* base = m->update.get();
  int32_t* dStats = a.stats.at(base);
  uint4* runOld = (m->runCurrentHalf ? a.run1 : a.run0).at<uint4>(base);
  uint4* runNew = (m->runCurrentHalf ? a.run0 : a.run1).at<uint4>(base);
  uint8_t* marks = a.marks.at(base); uint8_t* dirty = a.dirty.at(base); uint8_t* removedFlags = a.removedFlags.at(base);
  int32_t* chunkRemoved = a.chunkRemoved.at(base); int32_t* chunkDirty = a.chunkDirty.at(base); int32_t* slotCount = a.slotCount.at(base);
  int32_t* dirtyList = a.dirtyList.at(base); int32_t* dirtyTri = a.dirtyTri.at(base); int32_t* removedSlots = a.removedSlots.at(base);
  RenderCounters* dirtyCount = a.dirtyCount.at(base);
  itm_mesh_changed_block* changed = a.changed.at(base); itm_mesh_removed_block* removed = a.removed.at(base);
  const int N = s->noTotalEntries, nChunks = s->numChunks, padded = nChunks * kSweepChunk;
  const bool haveRun = m->run_table_current();
  int full = !haveRun ? ITM_MESH_UPDATE_NO_RUN_TABLE : m->allMarked ? ITM_MESH_UPDATE_ALL_MARKED : 0;
  m->deltaValid = false;

  // the diff and the lists
  ITM_HIP(hipMemsetAsync(dStats, 0, kUsPerCall * sizeof(int32_t), st));
  ITM_HIP(hipMemsetAsync(dirty, 0, (size_t)padded, st));
  const UpdateTable tb = update_table(s);
  if (haveRun) mesh_diff_kernel<true><<<nChunks, 256, 0, st>>>(tb, runOld, runNew, marks, m->flags, m->chunkCount, removedFlags, chunkRemoved, dirty, dStats, m->totals);
  else mesh_diff_kernel<false><<<nChunks, 256, 0, st>>>(tb, runOld, runNew, marks, m->flags, m->chunkCount, removedFlags, chunkRemoved, dirty, dStats, m->totals);
  ITM_LAUNCH_CHECK();
  { const int rc = launch_ordered_compaction(removedFlags, chunkRemoved, nChunks, padded, removedSlots, m->capBlocks, (int32_t*)nullptr, dStats + kUsRemoved, st); if (rc) return rc; }
  mesh_removed_kernel<<<kListGrid, 256, 0, st>>>(removedSlots, dStats + kUsRemoved, m->capBlocks, runOld, removed);
  ITM_LAUNCH_CHECK();

  int32_t hs[kUsCount] = {};
  uint32_t totals[2] = {0u, 0u};
  auto read_back = [&]() -> int {
    ITM_HIP(hipMemcpyAsync(hs, dStats, sizeof hs, hipMemcpyDeviceToHost, st));
    ITM_HIP(hipMemcpyAsync(totals, m->totals, 8, hipMemcpyDeviceToHost, st));
    ITM_HIP(hipStreamSynchronize(st));
    return ITM_OK;
  };
  const VolumeView vol = make_volume(s);
  if (!full) {
    // A' replaces the slot list; the dirty list; the counts of the dirty blocks; the prefixes over A' and the new run table
    { const int rc = launch_ordered_compaction(m->flags.get(), m->chunkCount, nChunks, N, m->slots, m->capBlocks, &m->listCounters->rawVisibleCount,
                                                &m->listCounters->noVisibleEntries, st); if (rc) return rc; }
    mesh_dirty_flag_kernel<<<nChunks, 256, 0, st>>>(N, dirty, chunkDirty);
    ITM_LAUNCH_CHECK();
    { const int rc = launch_ordered_compaction(dirty, chunkDirty, nChunks, N, dirtyList, m->capBlocks, &dirtyCount->rawVisibleCount, &dirtyCount->noVisibleEntries, st); if (rc) return rc; }
    const int rc = dispatch_voxel(s->cfg.voxelType, [&](auto vx) {
      using VX = decltype(vx);
      mesh_cells_kernel<VX, false><<<kMeshCellsGrid, 512, 0, st>>>(vol, dirtyList, dirtyCount, dirtyTri, nullptr, m->maxTriangles, m->totals, s->prm.voxelSize);
      return ITM_OK;
    });
    if (rc) return rc;
    ITM_LAUNCH_CHECK();
    m->soup_remeshed();                                         // the slot list and the counts describe the old buffer no more
    mesh_dirty_counts_kernel<<<kListGrid, 256, 0, st>>>(dirtyList, dirtyCount, dirtyTri, slotCount);
    mesh_new_counts_kernel<<<kListGrid, 256, 0, st>>>(m->slots, m->listCounters, dirty, slotCount, runOld, m->blockTriangles, dStats);
    mesh_scan_kernel<<<1, 1024, 0, st>>>(m->blockTriangles, m->listCounters, m->totals, m->maxTriangles);
    mesh_new_runs_kernel<<<kListGrid, 256, 0, st>>>(s->hash, m->slots, m->listCounters, dirty, slotCount, runOld, m->blockTriangles, runNew, dirtyList, dirtyCount, dirtyTri);
    ITM_LAUNCH_CHECK();
    { const int rb = read_back(); if (rb) return rb; }
    if (!hs[kUsRunFitted]) full = ITM_MESH_UPDATE_NO_RUN_TABLE;
    else if (totals[0] > m->maxTriangles - 1u) full = ITM_MESH_UPDATE_OVERFLOW;
  }

  uint32_t noChanged = 0;
  if (full) {
    // the call is itm_mesh_scene (which records the run table); the delta lists every block
    const int rc = itm_mesh_scene(s, m, stream);
    if (rc) return rc;
    mesh_changed_kernel<<<kListGrid, 256, 0, st>>>(m->slots, m->listCounters, runOld, changed);      // (recorded into the half that was current)
    ITM_LAUNCH_CHECK();
    RenderCounters lc;
    ITM_HIP(hipMemcpyAsync(&lc, m->listCounters, sizeof lc, hipMemcpyDeviceToHost, st));
    { const int rb = read_back(); if (rb) return rb; }
    hs[kUsAllocated] = lc.noVisibleEntries; hs[kUsRemeshed] = lc.noVisibleEntries; hs[kUsKept] = 0;
    hs[kUsCopied] = 0; hs[kUsGenerated] = (int32_t)totals[0]; hs[kUsAfter] = (int32_t)totals[1];
    if (full == ITM_MESH_UPDATE_NO_RUN_TABLE) { hs[kUsAppeared] = 0; hs[kUsVanished] = 0; hs[kUsRemoved] = 0; }
    noChanged = (uint32_t)lc.noVisibleEntries;
  } else {
    const uint32_t before = (uint32_t)hs[kUsBefore], after = totals[1];
    if (!m->spare) {
      ITM_HIP(m->spare.alloc((size_t)m->maxTriangles * 9));
      ITM_HIP(hipMemsetAsync(m->spare, 0, (size_t)m->maxTriangles * 36, st));
      m->spareHigh = 0;
    }
    if (m->spareHigh > after) ITM_HIP(hipMemsetAsync(m->spare + (size_t)after * 9, 0, (size_t)(m->spareHigh - after) * 36, st));
    const int rc = dispatch_voxel(s->cfg.voxelType, [&](auto vx) {
      using VX = decltype(vx);
      mesh_cells_kernel<VX, true><<<kMeshCellsGrid, 512, 0, st>>>(vol, dirtyList, dirtyCount, dirtyTri, m->spare, m->maxTriangles, m->totals, s->prm.voxelSize);
      return ITM_OK;
    });
    if (rc) return rc;
    mesh_copy_runs_kernel<<<1024, 256, 0, st>>>(m->slots, m->listCounters, dirty, runOld, runNew, (const uint32_t*)m->triangles.get(), (uint32_t*)m->spare.get());
    mesh_changed_kernel<<<kListGrid, 256, 0, st>>>(dirtyList, dirtyCount, runNew, changed);
    ITM_LAUNCH_CHECK();
    std::swap(m->triangles, m->spare);
    m->spareHigh = before;
    m->runCurrentHalf ^= 1;
    m->run_table_recorded();
    hs[kUsAllocated] = hs[kUsRemeshed] + hs[kUsKept];
    hs[kUsAfter] = (int32_t)after;
    noChanged = (uint32_t)hs[kUsRemeshed];
  }
  // the marks are consumed
  ITM_HIP(hipMemsetAsync(marks, 0, (size_t)padded, st));
  ITM_HIP(hipMemsetAsync(dStats + kUsIgnoredSoFar, 0, sizeof(int32_t), st));
  m->allMarked = false;
  m->lastFull = full;
  m->noChanged = noChanged;
  m->noRemoved = (uint32_t)std::min(hs[kUsRemoved], m->capBlocks);
  m->deltaValid = true;
  if (stats) {
    memcpy(stats, hs, sizeof *stats);
    stats->full = full;
    stats->noChanged = m->noChanged; stats->noRemoved = m->noRemoved;
    stats->reserved[0] = stats->reserved[1] = 0;
  }
  return ITM_OK;
}

int itm_mesh_update_info(const itm_mesh* m, uint32_t* noChanged, uint32_t* noRemoved, const itm_mesh_changed_block** changed_dev,
                         const itm_mesh_removed_block** removed_dev, itm_stream stream) {
  (void)stream;
  if (!m) return set_error(ITM_ERR_INVALID, "null mesh");
  if (!m->deltaValid) return set_error(ITM_ERR_INVALID, "no delta for this mesh: itm_mesh_update has not succeeded on it");
  const UpdateArena a = arena_of(m);
  if (noChanged) *noChanged = m->noChanged;
  if (noRemoved) *noRemoved = m->noRemoved;
  if (changed_dev) *changed_dev = m->noChanged ? a.changed.at(m->update.get()) : nullptr;
  if (removed_dev) *removed_dev = m->noRemoved ? a.removed.at(m->update.get()) : nullptr;
  return ITM_OK;
}

int itm_mesh_download_update(const itm_mesh* m, itm_mesh_changed_block* changed_host, uint32_t capacityChanged, itm_mesh_removed_block* removed_host,
                             uint32_t capacityRemoved, uint32_t* noChanged, uint32_t* noRemoved, itm_stream stream) {
  uint32_t nc = 0, nr = 0;
  const itm_mesh_changed_block* c = nullptr;
  const itm_mesh_removed_block* r = nullptr;
  const int rc = itm_mesh_update_info(m, &nc, &nr, &c, &r, stream);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  ITM_HIP(copy_out(changed_host, c, nc, capacityChanged, sizeof(itm_mesh_changed_block), st));
  ITM_HIP(copy_out(removed_host, r, nr, capacityRemoved, sizeof(itm_mesh_removed_block), st));
  ITM_HIP(hipStreamSynchronize(st));
  if (noChanged) *noChanged = nc;
  if (noRemoved) *noRemoved = nr;
  return ITM_OK;
}

}  // extern "C"
