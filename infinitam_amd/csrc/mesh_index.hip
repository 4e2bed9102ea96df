// mesh_index.hip -- the indexed form of the marching-cubes mesh: the triangle soup of itm_mesh_scene welded into shared vertices.
//
// The reference's ITMMesh is a buffer of independent triangles (Objects/ITMMesh.h:14-124); it has no indexed mesh.  This one is
// defined in terms of that buffer: with s_j, j = 0 .. 3n - 1, the soup's vertices in buffer order,
//   * two soup vertices are the same vertex iff their three floats have the same 96 bits (no tolerance, -0.0f != +0.0f);
//   * first[k] = the smallest j that holds the k-th distinct position, first strictly ascending (unique vertices are numbered in the
//     order of their first occurrence); vertices[k] = s_first[k];
//   * faces[j] = the k with the position of s_j.  Every triangle is kept, also those whose corners coincide after welding, so
//     vertices[faces] reproduces the soup bit for bit.
// Nothing in the result depends on the order in which lanes ran.
//
// MI355X design: a hash set of uint32 representatives in HBM, open addressing with linear probing, at least two slots per soup
// vertex (a power of two), so it cannot fill.
//   1. mesh_index_insert_kernel: lane j hashes its 96 position bits; an empty slot is claimed with atomicCAS(slot, EMPTY, j); on a
//      claimed slot the lane compares its position with the representative's (read from the triangle buffer): equal -> atomicMin
//      (slot, j), different -> next slot.  The POSITION of a slot never changes once it is claimed, only its representative falls, so
//      a stale read of a slot can at worst cause an atomicMin that changes nothing, and the table ends with min j per position
//      whatever the order: that is `first`.
//   2. mesh_index_resolve_kernel: every lane looks its position up again -> rep[j]; j is the first occurrence iff rep[j] == j; one
//      count per chunk of 1024 soup vertices.
//   3. mesh_index_scan_kernel: exclusive scan of the chunk counts by one workgroup; the sum is nV (read by the host: the vertex
//      buffers are sized from it).
//   4. mesh_index_compact_kernel: ordered compaction (workgroup scans, as the slot list of meshing.hip): the k-th first occurrence
//      writes first[k], vertices[k] and its own faces[j] = k.
//   5. mesh_index_faces_kernel: every other soup vertex takes faces[j] = faces[rep[j]].
//   6. mesh_index_blocks_kernel: blockVertex[b] = the number of unique vertices first seen before block b's triangles, so that the
//      vertices first seen in block b are the range [blockVertex[b], blockVertex[b + 1]) (itm_mesh_indexed_attributes stages per block).
// ITM_DEBUG_MESH_INDEX_WEAK_HASH cuts the hash to 8 bits (256 start slots spread over the table, the last one 64 slots before its
// end), so that probe chains hundreds of slots long and the wrap-around are exercised on small scenes.
#include "itm_internal.h"
#include "mesh_types.h"
#include "ordered_device.h"
#include "wave_utils.h"

namespace itm {


constexpr uint32_t kIndexEmpty = 0xffffffffu;
constexpr int kIndexChunk = 1024;                 // soup vertices per workgroup of the counting and compacting passes
constexpr size_t kIndexMinTable = 1024;

__device__ inline uint32_t index_start_slot(uint32_t x, uint32_t y, uint32_t z, uint32_t mask, int weak) {
  uint32_t h = x * 0x9E3779B1u ^ y * 0x85EBCA77u ^ z * 0xC2B2AE3Du;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
  if (weak) h = ((h & 0xffu) + 1u) * ((mask + 1u) >> 8) - 64u;      // 256 start slots; value 255 starts 64 slots before the table's end
  return h & mask;
}

__device__ inline bool same_position(const uint32_t* __restrict__ soup, uint32_t r, uint32_t x, uint32_t y, uint32_t z) {
  const uint32_t* q = soup + 3 * (size_t)r;
  return q[0] == x && q[1] == y && q[2] == z;
}

__global__ void __launch_bounds__(256) mesh_index_insert_kernel(const uint32_t* __restrict__ soup, uint32_t nSoup, uint32_t* table, uint32_t mask, int weak) {
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < nSoup; j += gridDim.x * 256u) {
    const uint32_t x = soup[3 * (size_t)j], y = soup[3 * (size_t)j + 1], z = soup[3 * (size_t)j + 2];
    uint32_t slot = index_start_slot(x, y, z, mask, weak);
    // the table has at least twice as many slots as there are soup vertices: an empty slot is met before the probe comes round
    for (uint32_t probe = 0; probe <= mask; ++probe, slot = (slot + 1u) & mask) {
      uint32_t r = table[slot];
      if (r == kIndexEmpty) {
        r = atomicCAS(table + slot, kIndexEmpty, j);
        if (r == kIndexEmpty) break;                                   // claimed for this position
      }
      if (r == j) break;
      if (same_position(soup, r, x, y, z)) {
        if (r > j) atomicMin(table + slot, j);
        break;
      }
    }
  }
}

// the representative of position (x, y, z) in the finished table
__device__ inline uint32_t index_lookup(const uint32_t* __restrict__ soup, const uint32_t* __restrict__ table, uint32_t mask, int weak,
                                        uint32_t x, uint32_t y, uint32_t z, uint32_t self) {
  uint32_t slot = index_start_slot(x, y, z, mask, weak);
  for (uint32_t probe = 0; probe <= mask; ++probe, slot = (slot + 1u) & mask) {
    const uint32_t r = table[slot];
    if (r == kIndexEmpty) break;                                       // (cannot happen: every position was inserted)
    if (r == self || same_position(soup, r, x, y, z)) return r;
  }
  return self;
}

__global__ void __launch_bounds__(256) mesh_index_resolve_kernel(const uint32_t* __restrict__ soup, uint32_t nSoup, const uint32_t* __restrict__ table,
                                                                 uint32_t mask, int weak, uint32_t* __restrict__ rep, uint32_t* __restrict__ chunkCount) {
  __shared__ int lds[4];
  int n = 0;
#pragma unroll
  for (int i = 0; i < kIndexChunk / 256; ++i) {
    const uint32_t j = blockIdx.x * (uint32_t)kIndexChunk + i * 256u + threadIdx.x;
    if (j < nSoup) {
      const uint32_t r = index_lookup(soup, table, mask, weak, soup[3 * (size_t)j], soup[3 * (size_t)j + 1], soup[3 * (size_t)j + 2], j);
      rep[j] = r;
      n += (r == j) ? 1 : 0;
    }
  }
  const int sum = block_reduce_sum<4>(n, lds);
  if (threadIdx.x == 0) chunkCount[blockIdx.x] = (uint32_t)sum;
}

// exclusive scan of the chunk counts (in place) by one workgroup; chunks[slotOfTotal] = their sum = nV
__global__ void __launch_bounds__(1024) mesh_index_scan_kernel(uint32_t* __restrict__ chunks, int nChunks, int slotOfTotal) {
  const uint32_t nV = carry_scan<16, uint32_t>(nChunks, [&](int i) { return chunks[i]; }, [&](int i, uint32_t before) { chunks[i] = before; });
  if (threadIdx.x == 0) chunks[slotOfTotal] = nV;
}

__global__ void __launch_bounds__(256) mesh_index_compact_kernel(const uint32_t* __restrict__ soup, uint32_t nSoup, const uint32_t* __restrict__ rep,
                                                                 const uint32_t* __restrict__ chunkOffset, uint32_t nUnique, uint32_t* __restrict__ first,
                                                                 uint32_t* __restrict__ vertices, uint32_t* __restrict__ faces) {
  __shared__ int lds[5];
  uint32_t base = chunkOffset[blockIdx.x];
#pragma unroll
  for (int i = 0; i < kIndexChunk / 256; ++i) {
    const uint32_t j = blockIdx.x * (uint32_t)kIndexChunk + i * 256u + threadIdx.x;
    const int flag = (j < nSoup && rep[j] == j) ? 1 : 0;
    int total;
    const int ex = block_exclusive_scan<4>(flag, lds, &total);
    const uint32_t k = base + (uint32_t)ex;
    if (flag && k < nUnique) {                                         // (k < nUnique always: nUnique is the sum of the flags)
      first[k] = j;
      vertices[3 * (size_t)k] = soup[3 * (size_t)j]; vertices[3 * (size_t)k + 1] = soup[3 * (size_t)j + 1]; vertices[3 * (size_t)k + 2] = soup[3 * (size_t)j + 2];
      faces[j] = k;
    }
    base += (uint32_t)total;
  }
}

// reads faces[] of first occurrences only (written by the launch before), writes faces[] of the others only
__global__ void __launch_bounds__(256) mesh_index_faces_kernel(uint32_t nSoup, const uint32_t* __restrict__ rep, uint32_t* faces) {
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < nSoup; j += gridDim.x * 256u) {
    const uint32_t r = rep[j];
    if (r != j && r < nSoup) faces[j] = faces[r];
  }
}

__global__ void __launch_bounds__(256) mesh_index_blocks_kernel(const RenderCounters* __restrict__ lc, const int32_t* __restrict__ blockTriangles,
                                                                const uint32_t* __restrict__ totals, int capBlocks, const uint32_t* __restrict__ first,
                                                                uint32_t nUnique, int32_t* __restrict__ blockVertex) {
  const int nBlocks = lc->noVisibleEntries < capBlocks ? lc->noVisibleEntries : capBlocks;
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b > nBlocks) return;
  uint32_t lo = nUnique;
  if (b < nBlocks) {
    const uint32_t count = totals[1];
    uint32_t t0 = (uint32_t)blockTriangles[b];
    t0 = t0 < count ? t0 : count;
    lo = lower_bound(first, nUnique, 3u * t0);                         // the unique vertices first seen before soup vertex 3 t0
  }
  blockVertex[b] = (int32_t)lo;
}

// the indexed mesh on the host, with the attributes of the unique vertices that are current where the writer carries them
int fetch_indexed(const itm_mesh* m, bool withAttributes, FetchedMesh& out, itm_stream stream) {
  int rc;
  if ((rc = m->require_index()) || (rc = enter_scene(m->scene, nullptr))) return rc;
  uint32_t nv = m->noVertices, nt = m->noIndexedTriangles;
  const uint32_t have = withAttributes ? m->attributes(true) : 0u;
  out.resize(nv, nt, true, have & ITM_MESH_NORMALS, have & ITM_MESH_COLOURS);
  if ((rc = itm_mesh_download_indexed(m, out.positions.data(), nullptr, nv, out.faces.data(), nt, nullptr, nullptr, stream)) || !have) return rc;
  return itm_mesh_download_indexed_attributes(m, out.normals_or_null(), out.colours_or_null(), nv, &nv, stream);
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_mesh_index(itm_mesh* m, itm_stream stream) {
  if (!m) return set_error(ITM_ERR_INVALID, "null mesh");
  hipStream_t st = as_stream(stream);
  uint32_t n = 0;
  int rc = itm_mesh_info(m, &n, nullptr, nullptr, stream);
  if (rc) return rc;
  m->index_rebuilding();                                               // its attributes and components belong to the index that is replaced
  m->noVertices = 0; m->noIndexedTriangles = n;
  if (n == 0) { m->index_current(); return ITM_OK; }                   // nothing meshed, or a dense scene: an empty index
  const size_t nSoup = (size_t)n * 3;                                  // < 2^32: the buffer holds less than 2^32 / 36 triangles
  if (nSoup >= 0x7fffffffull) return set_error(ITM_ERR_INVALID, "mesh too large to index");
  size_t tableSize = kIndexMinTable;
  while (tableSize < 2 * nSoup) tableSize <<= 1;                       // at least two slots per soup vertex: it cannot fill
  const int nChunks = (int)((nSoup + kIndexChunk - 1) / kIndexChunk);
  hipError_t e;
  // an index that cannot get its memory keeps none of it: every buffer is scratch or a result of this call
  auto fail = [&](hipError_t err, const char* what) {
    m->indexTable.reset(); m->rep.reset(); m->faces.reset(); m->indexChunks.reset(); m->first.reset(); m->vertices.reset();
    return hip_fail(err, what, __FILE__, __LINE__);
  };
  if ((e = m->indexTable.reserve(tableSize)) != hipSuccess) return fail(e, "mesh index table");
  if ((e = m->rep.reserve(nSoup)) != hipSuccess) return fail(e, "mesh index representatives");
  if ((e = m->faces.reserve(nSoup)) != hipSuccess) return fail(e, "mesh faces");
  if ((e = m->indexChunks.reserve((size_t)nChunks + 1)) != hipSuccess) return fail(e, "mesh index chunk counts");
  const uint32_t* soup = (const uint32_t*)m->triangles.get();
  const uint32_t mask = (uint32_t)(tableSize - 1);
  const int weak = debug_value(ITM_DEBUG_MESH_INDEX_WEAK_HASH);
  const int grid = 256 * 8;
  ITM_HIP(hipMemsetAsync(m->indexTable, 0xff, tableSize * 4, st));
  mesh_index_insert_kernel<<<grid, 256, 0, st>>>(soup, (uint32_t)nSoup, m->indexTable, mask, weak);
  mesh_index_resolve_kernel<<<nChunks, 256, 0, st>>>(soup, (uint32_t)nSoup, m->indexTable, mask, weak, m->rep, m->indexChunks);
  mesh_index_scan_kernel<<<1, 1024, 0, st>>>(m->indexChunks, nChunks, nChunks);
  ITM_LAUNCH_CHECK();
  uint32_t nV = 0;
  ITM_HIP(hipMemcpyAsync(&nV, m->indexChunks + nChunks, 4, hipMemcpyDeviceToHost, st));
  ITM_HIP(hipStreamSynchronize(st));
  if (nV == 0 || nV > nSoup) return set_error(ITM_ERR_DEVICE, "mesh index: impossible vertex count");
  if ((e = m->first.reserve(nV)) != hipSuccess) return fail(e, "mesh first occurrences");
  if ((e = m->vertices.reserve((size_t)nV * 3)) != hipSuccess) return fail(e, "mesh vertices");
  mesh_index_compact_kernel<<<nChunks, 256, 0, st>>>(soup, (uint32_t)nSoup, m->rep, m->indexChunks, nV, m->first, (uint32_t*)m->vertices.get(), m->faces);
  mesh_index_faces_kernel<<<grid, 256, 0, st>>>((uint32_t)nSoup, m->rep, m->faces);
  if (m->capBlocks > 0) {
    if (!m->blockVertex && (e = m->blockVertex.alloc((size_t)m->capBlocks + 1)) != hipSuccess) return fail(e, "mesh block vertices");
    mesh_index_blocks_kernel<<<(m->capBlocks + 1 + 255) / 256, 256, 0, st>>>(m->listCounters, m->blockTriangles, m->totals, m->capBlocks, m->first, nV, m->blockVertex);
  }
  ITM_LAUNCH_CHECK();
  m->noVertices = nV;
  m->index_current();
  return ITM_OK;
}

int itm_mesh_index_info(const itm_mesh* m, uint32_t* noVertices, uint32_t* noTriangles, const float** vertices_dev, const uint32_t** faces_dev,
                        const uint32_t** first_dev, itm_stream stream) {
  if (!m) return set_error(ITM_ERR_INVALID, "null mesh");
  { const int rc = m->require_index(); if (rc) return rc; }
  ITM_HIP(hipStreamSynchronize(as_stream(stream)));
  if (noVertices) *noVertices = m->noVertices;
  if (noTriangles) *noTriangles = m->noIndexedTriangles;
  if (vertices_dev) *vertices_dev = m->noVertices ? m->vertices : nullptr;
  if (faces_dev) *faces_dev = m->noIndexedTriangles ? m->faces : nullptr;
  if (first_dev) *first_dev = m->noVertices ? m->first : nullptr;
  return ITM_OK;
}

int itm_mesh_download_indexed(const itm_mesh* m, float* vertices_host, uint32_t* first_host, uint32_t capacityVertices, uint32_t* faces_host,
                              uint32_t capacityTriangles, uint32_t* noVertices, uint32_t* noTriangles, itm_stream stream) {
  if (!m) return set_error(ITM_ERR_INVALID, "null mesh");
  { const int rc = m->require_index(); if (rc) return rc; }
  if (noVertices) *noVertices = m->noVertices;
  if (noTriangles) *noTriangles = m->noIndexedTriangles;
  hipStream_t st = as_stream(stream);
  ITM_HIP(copy_out(vertices_host, m->vertices, m->noVertices, capacityVertices, 12, st));
  ITM_HIP(copy_out(first_host, m->first, m->noVertices, capacityVertices, 4, st));
  ITM_HIP(copy_out(faces_host, m->faces, m->noIndexedTriangles, capacityTriangles, 12, st));
  ITM_HIP(hipStreamSynchronize(st));
  return ITM_OK;
}

// the PLY and OBJ of the triangle buffer (mesh_files.h) with one vertex per distinct position and the faces through the index
int itm_mesh_write_ply_indexed(const itm_mesh* m, const char* path, itm_stream stream) {
  if (!m || !path) return set_error(ITM_ERR_INVALID, "null argument");
  FetchedMesh h;
  const int rc = fetch_indexed(m, true, h, stream);
  return rc ? rc : file_status(write_ply(h.view, path));
}

int itm_mesh_write_obj_indexed(const itm_mesh* m, const char* path, itm_stream stream) {
  if (!m || !path) return set_error(ITM_ERR_INVALID, "null argument");
  FetchedMesh h;
  const int rc = fetch_indexed(m, false, h, stream);
  return rc ? rc : file_status(write_obj(h.view, path));
}

}  // extern "C"
