// mesh_attributes.hip -- per-vertex normals and colours of the marching-cubes mesh, and the PLY writer that carries them.
//
// Reference behaviour (the reference's ITMMesh holds positions only; the two per-point functions are the reference's own):
//   computeSingleNormalFromSDF            DeviceAgnostic/ITMRepresentationAccess.h:224-337   (sample_device.h: gradient_axis)
//   readFromSDF_color4u_interpolated      DeviceAgnostic/ITMRepresentationAccess.h:187-222   (sample_device.h: colour_from)
//   drawPixelColour (float -> uchar)      DeviceAgnostic/ITMVisualisationEngine.h:270-279
// evaluated at p = vertex / voxelSize (three IEEE divisions) for every vertex of the triangles the last itm_mesh_scene left in
// the buffer, in buffer order.  The normal is the gradient times 1 / sqrt(g.g) (as normal_from_sdf forms it, no light test) and
// (0, 0, 0) where that is not finite; it points from the surface into free space.
//
// MI355X design: the triangles of one voxel block lie together in the buffer (meshing.hip: base(block) from the scan that
// itm_mesh_scene leaves in blockTriangles), and every vertex of the block's cells samples voxels within two of the block.  So
// mesh_attr_block_kernel runs one 256-lane workgroup per listed block that has triangles: the 13^3 raw sdf values (and packed
// colours) of planes -2 .. +10 of the block are staged in LDS once through the block directory -- 27 block look-ups per block
// instead of 40 per vertex -- and the lanes then work through the block's vertices from LDS with the reference's float
// operations.  floor(p) may sit one voxel under the cell's corner (a lattice coordinate that `* voxelSize / voxelSize` returned
// one ulp low): planes -2 and +10 are there for those.  A vertex whose floor(p) leaves [-1, 8] takes the global path, which is
// also the whole of mesh_attr_vertex_kernel (one lane per vertex; ITM_DEBUG_MESH_ATTR_PER_VERTEX).
//
// itm_mesh_indexed_attributes runs the same kernel over the unique vertices of the indexed mesh (mesh_index.hip): `first` ascends,
// so the unique vertices whose first occurrence lies in block b's triangles are one contiguous range [blockVertex[b], blockVertex
// [b + 1]) -- vertices of that block's cells, for which the staged planes hold as they do for the soup.  One evaluation per distinct
// position instead of one per occurrence.
#include "itm_internal.h"
#include "mesh_types.h"
#include "sample_device.h"
#include "shading_device.h"

namespace itm {


constexpr int kHaloLow = 2;                       // planes below the block
constexpr int kHaloSide = kBlockSide + 5;         // -2 .. +10
constexpr int kHaloCells = kHaloSide * kHaloSide * kHaloSide;

// the attributes of vertex v through the hash (directory / mirror where they cover) or, DENSE, the voxel array: the reference's
// functions as the renders use them (forced inline: out of line, the colour instances of the per-vertex kernel take scratch for the call)
template <class VX, bool DENSE = false>
__device__ __forceinline__ void vertex_global(const VolumeView& vol, size_t v, float px, float py, float pz, uint32_t what,
                                     float* __restrict__ normals, uchar4* __restrict__ colours) {
  if (what & ITM_MESH_NORMALS) {
    float gx, gy, gz;
    sdf_gradient<VX, DENSE>(vol, px, py, pz, gx, gy, gz);
    store_normal(normals + 3 * v, gx, gy, gz);
  }
  if constexpr (VX::kColor) {
    if (what & ITM_MESH_COLOURS) colours[v] = colour_bytes(colour_at<VX, DENSE>(vol, px, py, pz));
  }
}

// one lane per vertex: the soup's (totals: three per triangle in the buffer) or, totals == nullptr, `nFixed` unique vertices
template <class VX, bool DENSE>
__global__ void __launch_bounds__(256) mesh_attr_vertex_kernel(VolumeView vol, const float* __restrict__ triangles, const uint32_t* __restrict__ totals, uint32_t nFixed,
                                                               float voxelSize, uint32_t what, float* __restrict__ normals, uchar4* __restrict__ colours) {
  const size_t nVertices = totals ? (size_t)totals[1] * 3 : (size_t)nFixed;
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < nVertices; v += (size_t)gridDim.x * 256) {
    const float* p = triangles + 3 * v;
    vertex_global<VX, DENSE>(vol, v, p[0] / voxelSize, p[1] / voxelSize, p[2] / voxelSize, what, normals, colours);
  }
}

// INDEXED: `blockTriangles` is blockVertex (per listed block its first unique vertex, one entry past the last block = nV), `triangles`
// the unique vertices, and the attributes are stored per unique vertex
template <class VX, bool INDEXED>
__global__ void __launch_bounds__(256) mesh_attr_block_kernel(VolumeView vol, const int32_t* __restrict__ slots, const RenderCounters* __restrict__ lc,
                                                              const int32_t* __restrict__ blockTriangles, const float* __restrict__ triangles,
                                                              const uint32_t* __restrict__ totals, int capBlocks, float voxelSize, uint32_t what,
                                                              float* __restrict__ normals, uchar4* __restrict__ colours) {
  __shared__ float sdf[kHaloCells];                          // raw sdf; the default voxel's where none is stored (readVoxel)
  __shared__ uint32_t clr[VX::kColor ? kHaloCells : 1];      // r | g << 8 | b << 16; 0 where none is stored
  __shared__ int nbBase[27];
  const uint32_t generated = totals[0], count = totals[1];
  if (count == 0u) return;                                   // nothing meshed (yet): the block list may never have been written
  const int nBlocks = lc->noVisibleEntries < capBlocks ? lc->noVisibleEntries : capBlocks;
  const int t = threadIdx.x;
  const bool wantColour = VX::kColor && (what & ITM_MESH_COLOURS);
  for (int b = blockIdx.x; b < nBlocks; b += gridDim.x) {
    // the block's triangles: [prefix(b), prefix(b + 1)), cut at the count a full buffer stops at
    uint32_t t0, t1;
    if constexpr (INDEXED) {                                 // the unique vertices first seen in the block: [t0, t1)
      t0 = (uint32_t)blockTriangles[b]; t1 = (uint32_t)blockTriangles[b + 1];
    } else {
      t0 = (uint32_t)blockTriangles[b]; t1 = (b + 1 < nBlocks) ? (uint32_t)blockTriangles[b + 1] : generated;
      t0 = t0 < count ? t0 : count; t1 = t1 < count ? t1 : count;
    }
    if (t0 == t1) continue;                                  // (uniform) no surface in this block: nothing is staged
    const HashEntry he = unpack_entry(vol.hash[slots[b]]);
    __syncthreads();                                         // previous block's LDS contents are no longer needed
    if (t < 27) nbBase[t] = (t == 13) ? he.ptr * kBlockVoxels : block_base(vol, he.px + t % 3 - 1, he.py + (t / 3) % 3 - 1, he.pz + t / 9 - 1);
    __syncthreads();
    for (int i = t; i < kHaloCells; i += 256) {
      const int x = i % kHaloSide - kHaloLow, y = (i / kHaloSide) % kHaloSide - kHaloLow, z = i / (kHaloSide * kHaloSide) - kHaloLow;
      const int base = nbBase[((x + 8) >> 3) + 3 * ((y + 8) >> 3) + 9 * ((z + 8) >> 3)];
      float v = VX::kShort ? 32767.0f : 1.0f;
      uint32_t c = 0u;
      if (base >= 0) {
        const size_t a = (size_t)(base + (x & 7) + ((y & 7) << 3) + ((z & 7) << 6));
        if constexpr (VX::kColor) {
          if (wantColour) {
            const typename VX::Reg r = VX::load(vol.vba, a);
            int rgb[3], wc;
            VX::get_color(r, rgb, wc);
            v = VX::raw_sdf(r);
            c = (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16);
          } else v = VX::load_raw_sdf(vol.vba, a);
        } else v = VX::load_raw_sdf(vol.vba, a);
      }
      sdf[i] = v;
      if constexpr (VX::kColor) clr[i] = c;
    }
    __syncthreads();
    const int ox = he.px * kBlockSide, oy = he.py * kBlockSide, oz = he.pz * kBlockSide;
    const uint32_t nV = INDEXED ? t1 - t0 : (t1 - t0) * 3u;
    for (uint32_t k = t; k < nV; k += 256) {
      const size_t v = (INDEXED ? (size_t)t0 : (size_t)t0 * 3) + k;
      const float* p = triangles + 3 * v;
      const float px = p[0] / voxelSize, py = p[1] / voxelSize, pz = p[2] / voxelSize;
      const float bx = floorf(px), by = floorf(py), bz = floorf(pz);
      const float fx = px - bx, fy = py - by, fz = pz - bz;
      const int lx = (int)bx - ox, ly = (int)by - oy, lz = (int)bz - oz;
      // reads reach floor(p) - 1 .. floor(p) + 2: staged for floor(p) in [-1, 8] per axis
      if ((uint32_t)(lx + 1) > 9u || (uint32_t)(ly + 1) > 9u || (uint32_t)(lz + 1) > 9u) {
        vertex_global<VX>(vol, v, px, py, pz, what, normals, colours);
        continue;
      }
      const int at = (lx + kHaloLow) + (ly + kHaloLow) * kHaloSide + (lz + kHaloLow) * kHaloSide * kHaloSide;
      if (what & ITM_MESH_NORMALS) {
        auto raw = [&](int dx, int dy, int dz) { return sdf[at + dx + dy * kHaloSide + dz * kHaloSide * kHaloSide]; };
        const float gx = gradient_axis<VX, 0>(raw, fx, fy, fz);
        const float gy = gradient_axis<VX, 1>(raw, fy, fx, fz);
        const float gz = gradient_axis<VX, 2>(raw, fz, fx, fy);
        store_normal(normals + 3 * v, gx, gy, gz);
      }
      if constexpr (VX::kColor) {
        if (wantColour) {
          auto packed = [&](int dx, int dy, int dz) { return clr[at + dx + dy * kHaloSide + dz * kHaloSide * kHaloSide]; };
          colours[v] = colour_bytes(colour_from(packed, fx, fy, fz));
        }
      }
    }
  }
}

// what both attribute entry points ask of their arguments
static int check_attribute_request(const itm_scene* s, const itm_mesh* m, int what) {
  if (!s || !m) return set_error(ITM_ERR_INVALID, "null argument");
  if (m->scene != s) return set_error(ITM_ERR_INVALID, "mesh belongs to another scene");
  if (what <= 0 || (what & ~(ITM_MESH_NORMALS | ITM_MESH_COLOURS))) return set_error(ITM_ERR_INVALID, "what: ITM_MESH_NORMALS, ITM_MESH_COLOURS or both");
  if ((what & ITM_MESH_COLOURS) && !voxel_has_colour(s->cfg.voxelType))
    return set_error(ITM_ERR_INVALID, "the scene's voxel type stores no colour: the mesh has no colour attribute");
  return ITM_OK;
}

}  // namespace itm

using namespace itm;

extern "C" {

int itm_mesh_attributes(const itm_scene* s, itm_mesh* m, int what, itm_stream stream) {
  { const int rc = check_attribute_request(s, m, what); if (rc) return rc; }
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  const bool dense = s->cfg.indexType != ITM_INDEX_HASH;
  if (dense && !m->holds_volume_mesh()) { m->attributes_current(false, (uint32_t)what); return ITM_OK; }   // a dense scene that itm_mesh_volume has not meshed: nothing meshed, empty attributes
  const bool newNormals = (what & ITM_MESH_NORMALS) && !m->normals;
  if (newNormals) {
    const hipError_t e = m->normals.alloc((size_t)m->maxTriangles * 9);
    if (e != hipSuccess) return hip_fail(e, "mesh normals", __FILE__, __LINE__);
  }
  if ((what & ITM_MESH_COLOURS) && !m->colours) {
    const hipError_t e = m->colours.alloc((size_t)m->maxTriangles * 3);
    if (e != hipSuccess) { if (newNormals) m->normals.reset(); return hip_fail(e, "mesh colours", __FILE__, __LINE__); }      // what this call allocated, or nothing
  }
  const VolumeView vol = make_volume(s);
  const int grid = 256 * 8;
  const int rc = dispatch_volume(s, [&](auto vx, auto isDense) {
    using VX = decltype(vx);
    if (isDense.value || debug_value(ITM_DEBUG_MESH_ATTR_PER_VERTEX))      // the mesh of itm_mesh_volume: every vertex through the voxel array
      mesh_attr_vertex_kernel<VX, isDense.value><<<grid, 256, 0, st>>>(vol, m->triangles, m->totals, 0u, s->prm.voxelSize, (uint32_t)what, m->normals, m->colours);
    else
      mesh_attr_block_kernel<VX, false><<<grid, 256, 0, st>>>(vol, m->slots, m->listCounters, m->blockTriangles, m->triangles, m->totals, m->capBlocks, s->prm.voxelSize,
                                                      (uint32_t)what, m->normals, m->colours);
    return ITM_OK;
  });
  if (rc) return rc;
  ITM_LAUNCH_CHECK();
  m->attributes_current(false, (uint32_t)what);
  return ITM_OK;
}

int itm_mesh_download_attributes(const itm_mesh* m, float* normals_host, uint8_t* colours_host, uint32_t capacityTriangles,
                                 uint32_t* noTotalTriangles, itm_stream stream) {
  if (!m || !noTotalTriangles) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = m->require_attributes(normals_host != nullptr, colours_host != nullptr, false); if (rc) return rc; }
  { const int rc = enter_scene(m->scene, nullptr); if (rc) return rc; }
  int rc = itm_mesh_info(m, noTotalTriangles, nullptr, nullptr, stream);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  ITM_HIP(copy_out(normals_host, m->normals, *noTotalTriangles, capacityTriangles, 36, st));
  ITM_HIP(copy_out(colours_host, m->colours, *noTotalTriangles, capacityTriangles, 12, st));
  ITM_HIP(hipStreamSynchronize(st));
  return ITM_OK;
}

// the attributes of the unique vertices of the indexed mesh: one evaluation per distinct position, through the staged kernel
int itm_mesh_indexed_attributes(const itm_scene* s, itm_mesh* m, int what, itm_stream stream) {
  { const int rc = check_attribute_request(s, m, what); if (rc) return rc; }
  { const int rc = m->require_index(); if (rc) return rc; }
  { const int rc = enter_scene(s, nullptr); if (rc) return rc; }
  hipStream_t st = as_stream(stream);
  if (m->noVertices == 0) { m->attributes_current(true, (uint32_t)what); return ITM_OK; }   // an empty index (dense scenes, nothing meshed): empty attributes
  // (only a stale attribute's buffer can fail to grow: one that is current for this index already holds noVertices elements)
  hipError_t e;
  if ((what & ITM_MESH_NORMALS) && (e = m->vertexNormals.reserve((size_t)m->noVertices * 3)) != hipSuccess) return hip_fail(e, "vertex normals", __FILE__, __LINE__);
  if ((what & ITM_MESH_COLOURS) && (e = m->vertexColours.reserve((size_t)m->noVertices)) != hipSuccess) return hip_fail(e, "vertex colours", __FILE__, __LINE__);
  const VolumeView vol = make_volume(s);
  const int grid = 256 * 8;
  const int rc = dispatch_volume(s, [&](auto vx, auto isDense) {
    using VX = decltype(vx);
    if (isDense.value)                           // the mesh of itm_mesh_volume on a dense scene: one lane per unique vertex
      mesh_attr_vertex_kernel<VX, true><<<grid, 256, 0, st>>>(vol, m->vertices, nullptr, m->noVertices, s->prm.voxelSize, (uint32_t)what, m->vertexNormals, m->vertexColours);
    else
      mesh_attr_block_kernel<VX, true><<<grid, 256, 0, st>>>(vol, m->slots, m->listCounters, m->blockVertex, m->vertices, m->totals, m->capBlocks, s->prm.voxelSize,
                                                            (uint32_t)what, m->vertexNormals, m->vertexColours);
    return ITM_OK;
  });
  if (rc) return rc;
  ITM_LAUNCH_CHECK();
  m->attributes_current(true, (uint32_t)what);
  return ITM_OK;
}

int itm_mesh_download_indexed_attributes(const itm_mesh* m, float* normals_host, uint8_t* colours_host, uint32_t capacityVertices,
                                         uint32_t* noVertices, itm_stream stream) {
  if (!m || !noVertices) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = m->require_attributes(normals_host != nullptr, colours_host != nullptr, true); if (rc) return rc; }
  { const int rc = enter_scene(m->scene, nullptr); if (rc) return rc; }
  *noVertices = m->noVertices;
  hipStream_t st = as_stream(stream);
  ITM_HIP(copy_out(normals_host, m->vertexNormals, m->noVertices, capacityVertices, 12, st));
  ITM_HIP(copy_out(colours_host, m->vertexColours, m->noVertices, capacityVertices, 4, st));
  ITM_HIP(hipStreamSynchronize(st));
  return ITM_OK;
}

// binary_little_endian PLY of the soup with the attributes that are current (mesh_files.h)
int itm_mesh_write_ply(const itm_mesh* m, const char* path, itm_stream stream) {
  if (!m || !path) return set_error(ITM_ERR_INVALID, "null argument");
  { const int rc = enter_scene(m->scene, nullptr); if (rc) return rc; }
  FetchedMesh h;
  const int rc = fetch_soup(m, true, h, stream);
  return rc ? rc : file_status(write_ply(h.view, path));
}

}  // extern "C"
