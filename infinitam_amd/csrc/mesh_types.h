// mesh_types.h -- the mesh handle shared by meshing.hip (triangles), mesh_attributes.hip (per-vertex normals and colours) and
// mesh_index.hip (the indexed form: shared vertices and faces) and mesh_components.hip (its connected components, the fragment filter).
#pragma once

#include "itm_internal.h"
#include "volume_device.h"

namespace itm {

// What a labelling (mesh_components.hip) leaves in device memory, and its scratch: owned by the mesh, or by one call of the test hook.
struct ComponentBuffers {
  DeviceBuffer<uint32_t> parent;             // per vertex: the union-find link, always to a smaller index; the root once labelled
  DeviceBuffer<uint32_t> vertexComponent;    // per vertex: its component's number
  DeviceBuffer<uint32_t> triangleComponent;  // per triangle: the component of its first corner
  DeviceBuffer<itm_mesh_component> components;
  DeviceBuffer<uint8_t> flags;               // per vertex: a root?  (the filter: per triangle: kept?)
  DeviceBuffer<int32_t> chunkCount;          // flags per chunk of kSweepChunk
  DeviceBuffer<int32_t> ids;                 // the roots, ascending  (the filter: the kept triangles, ascending)
  DeviceBuffer<int32_t> counters;            // [0] flags set, [1] the same after the cap, [2] what the check launch found, [3] kept components
  void reset() {
    parent.reset(); vertexComponent.reset(); triangleComponent.reset(); components.reset(); flags.reset(); chunkCount.reset(); ids.reset();
    counters.reset();
  }
};

}  // namespace itm

struct itm_mesh {
  const itm_scene* scene = nullptr;
  uint32_t maxTriangles = 0;
  itm::DeviceBuffer<float> triangles;        // ITMMesh::Triangle[maxTriangles]: 9 floats (p0, p1, p2)
  itm::DeviceBuffer<int32_t> slots;          // allocated slots in ascending order
  itm::DeviceBuffer<int32_t> blockTriangles; // per listed block: triangle count, then exclusive prefix
  itm::DeviceBuffer<uint8_t> flags;          // per slot: allocated?
  itm::DeviceBuffer<int32_t> chunkCount;
  itm::DeviceBuffer<itm::RenderCounters> listCounters;   // noVisibleEntries = number of listed blocks
  itm::DeviceBuffer<uint32_t> totals;        // [0] triangles generated, [1] noTotalTriangles (after the cap)
  int capBlocks = 0;
  // itm_mesh_volume on a dense scene (mesh_dense.hip); allocated by the first such call
  itm::DeviceBuffer<int32_t> brickCount;     // per 8^3 brick of the array: triangle count
  itm::DeviceBuffer<unsigned long long> brickBase;   // per brick: triangles generated before it
  itm::DeviceBuffer<int32_t> brickList;      // the bricks that have triangles, ascending
  itm::DeviceBuffer<int32_t> brickCounters;  // [0] number of listed bricks; [2..3] triangles generated (64 bits)
  bool fromVolume = false;           // the buffer holds the mesh itm_mesh_volume made of a dense scene; itm_mesh_scene clears it
  // vertex attributes of the triangles the last itm_mesh_scene left in the buffer (mesh_attributes.hip); allocated on first use
  itm::DeviceBuffer<float> normals;          // 3 floats per vertex, 3 vertices per triangle, buffer order
  itm::DeviceBuffer<uchar4> colours;         // one per vertex
  uint32_t attrCurrent = 0;          // ITM_MESH_* bits computed for the buffer's present contents; itm_mesh_scene clears it
  // indexed form of the buffer's present contents (mesh_index.hip); allocated / grown by itm_mesh_index, sized from the counts
  itm::DeviceBuffer<float> vertices;         // 3 floats per unique vertex, in the order of first occurrence in the buffer
  itm::DeviceBuffer<uint32_t> faces;         // 3 vertex indices per triangle, buffer order
  itm::DeviceBuffer<uint32_t> first;         // per unique vertex: the smallest soup vertex index that holds its position (strictly ascending)
  itm::DeviceBuffer<uint32_t> rep;           // per soup vertex: first[] of its position (scratch of the build)
  itm::DeviceBuffer<uint32_t> indexTable;    // the hash set of representatives (scratch of the build)
  itm::DeviceBuffer<uint32_t> indexChunks;   // per chunk of soup vertices: unique vertices first seen there, then exclusive prefix, closed by nV
  itm::DeviceBuffer<int32_t> blockVertex;    // per listed block: its first unique vertex (the vertices first seen in block b are [b], [b + 1])
  uint32_t noVertices = 0, noIndexedTriangles = 0;
  bool indexCurrent = false;         // the index describes the buffer's present contents; itm_mesh_scene clears it
  // attributes of the unique vertices (itm_mesh_indexed_attributes), independent of the soup's
  itm::DeviceBuffer<float> vertexNormals;    // 3 floats per unique vertex
  itm::DeviceBuffer<uchar4> vertexColours;   // one per unique vertex
  uint32_t indexedAttrCurrent = 0;   // ITM_MESH_* bits computed for the present index; itm_mesh_scene and itm_mesh_index clear it
  // connected components of the present index (mesh_components.hip); allocated / grown by itm_mesh_components, sized from the counts
  itm::ComponentBuffers comp;
  itm::DeviceBuffer<uint8_t> componentKeep;  // per component: kept by itm_mesh_filter_components? (the host's mask, then the verdict)
  itm::DeviceBuffer<float> packed;           // the kept triangles, packed, before they replace the buffer's contents
  uint32_t noComponents = 0, componentRounds = 0;
  bool componentsCurrent = false;    // the labelling describes the present index; itm_mesh_scene, itm_mesh_index and the filter clear it
};

namespace itm {

int launch_mesh_volume_dense(const itm_scene* s, itm_mesh* m, hipStream_t st);   // mesh_dense.hip

}  // namespace itm
