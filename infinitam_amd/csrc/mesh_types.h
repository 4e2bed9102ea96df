// mesh_types.h -- the mesh handle shared by meshing.hip (triangles), mesh_attributes.hip (per-vertex normals and colours) and
// mesh_index.hip (the indexed form: shared vertices and faces), mesh_components.hip (its connected components, the fragment filter) and
// mesh_smooth.hip (fixed-point smoothing passes over the index).
// The handle's state -- which of those products are current -- is kept here and nowhere else.
#pragma once

#include "itm_internal.h"
#include "mesh_files.h"
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
  void reset() { *this = ComponentBuffers(); }
};

// The scratch of a smoothing call (mesh_smooth.hip), sized from the counts: owned by the mesh, or by one call of the test hook.
struct SmoothBuffers {
  DeviceBuffer<uint32_t> rowCount;           // per vertex: its neighbour entries n(k); the row's fill cursor while the rows are written
  DeviceBuffer<uint32_t> rowStart;           // per vertex: where its row starts in `entries` (exclusive prefix of rowCount)
  DeviceBuffer<uint32_t> chunkSum;           // entries per chunk of vertices, then their exclusive prefix
  DeviceBuffer<uint32_t> entries;            // the adjacency rows (CSR); the order inside a row is arbitrary
  DeviceBuffer<uint32_t> heavy;              // the vertices whose rows are long enough for a wave of their own, in no particular order
  DeviceBuffer<uint8_t> vertexFlags;         // per vertex: bit 0 irregular, bit 1 isolated, bit 2 moving
  DeviceBuffer<int4> xa, xb;                 // the two iterates: x, y, z in fixed point (w unused), 16 bytes per vertex
  DeviceBuffer<long long> sums;              // scatter form only: per vertex the sums S.x, S.y, S.z (and a word of padding)
  DeviceBuffer<uint32_t> counters;           // [0] moving [1] irregular [2] isolated [3] max entries [4] input out of range or not finite [5] listed long rows
  void reset() { *this = SmoothBuffers(); }
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
  // vertex attributes of the triangles in the buffer (mesh_attributes.hip); allocated on first use
  itm::DeviceBuffer<float> normals;          // 3 floats per vertex, 3 vertices per triangle, buffer order
  itm::DeviceBuffer<uchar4> colours;         // one per vertex
  // indexed form of the buffer's present contents (mesh_index.hip); allocated / grown by itm_mesh_index, sized from the counts
  itm::DeviceBuffer<float> vertices;         // 3 floats per unique vertex, in the order of first occurrence in the buffer
  itm::DeviceBuffer<uint32_t> faces;         // 3 vertex indices per triangle, buffer order
  itm::DeviceBuffer<uint32_t> first;         // per unique vertex: the smallest soup vertex index that holds its position (strictly ascending)
  itm::DeviceBuffer<uint32_t> rep;           // per soup vertex: first[] of its position (scratch of the build)
  itm::DeviceBuffer<uint32_t> indexTable;    // the hash set of representatives (scratch of the build)
  itm::DeviceBuffer<uint32_t> indexChunks;   // per chunk of soup vertices: unique vertices first seen there, then exclusive prefix, closed by nV
  itm::DeviceBuffer<int32_t> blockVertex;    // per listed block: its first unique vertex (the vertices first seen in block b are [b], [b + 1])
  uint32_t noVertices = 0, noIndexedTriangles = 0;
  // attributes of the unique vertices (itm_mesh_indexed_attributes), independent of the soup's
  itm::DeviceBuffer<float> vertexNormals;    // 3 floats per unique vertex
  itm::DeviceBuffer<uchar4> vertexColours;   // one per unique vertex
  // connected components of the present index (mesh_components.hip); allocated / grown by itm_mesh_components, sized from the counts
  itm::ComponentBuffers comp;
  itm::DeviceBuffer<uint8_t> componentKeep;  // per component: kept by itm_mesh_filter_components? (the host's mask, then the verdict)
  itm::DeviceBuffer<float> packed;           // the kept triangles, packed, before they replace the buffer's contents
  uint32_t noComponents = 0, componentRounds = 0;
  // scratch of itm_mesh_smooth (mesh_smooth.hip); allocated / grown by the call, sized from the counts
  itm::SmoothBuffers smooth;
  // incremental re-meshing (mesh_update.hip; hash scenes).  The RUN TABLE: per table slot {px | py << 16, pz | listed << 16, first
  // triangle, triangle count} of the block the slot held when the buffer was last generated, zero for a slot that was not listed.
  // `update` holds it twice (the one an update reads, the one it writes), the marks of itm_mesh_touch, the call's flags, lists and
  // statistics and the delta (UpdateArena); allocated with the mesh.
  itm::DeviceBuffer<void> update;
  int runCurrentHalf = 0;                    // which of the arena's two run tables describes the buffer
  bool allMarked = false;                    // itm_mesh_touch(everything) since the last update
  itm::DeviceBuffer<float> spare;            // the buffer an update writes while it copies from `triangles`; allocated by the first update that copies
  uint32_t spareHigh = 0;                    // triangles of `spare` that may not be zero
  int lastFull = 0;                          // the last update: its reason code, ...
  uint32_t noChanged = 0, noRemoved = 0;     // ... and the lengths of its delta
  bool deltaValid = false;

  // ---- which products describe the buffer's present contents ------------------------------------------------------------------------
  //   soup (the triangle buffer) -+- soup attributes (normals, colours)
  //                               +- index -+- indexed attributes
  //                               |         +- components
  //                               +- run table (which run of the buffer belongs to which block: itm_mesh_update)
  // A product is current once the call that computes it has succeeded (empty cases included: they need no device work) and stale from
  // the moment something above it is rewritten; a call that fails leaves its product stale.  Who rewrites what: itm_mesh_scene /
  // itm_mesh_volume and, once it starts rewriting, itm_mesh_filter_components the soup; itm_mesh_index the index; itm_mesh_components
  // the components.  Each function below clears its own row and calls the one for the rows beneath it.
  // itm_mesh_smooth moves positions and nothing else: vertices and soup are rewritten TOGETHER, through the faces, so the index goes on
  // describing the soup (vertices[faces] is the soup, first[k] names a soup vertex that holds vertices[k]) and stays current -- although
  // two distinct vertices may now hold one position, which a fresh itm_mesh_index would weld.  Everything computed FROM positions is stale.
  // The run table (itm_mesh_update) describes the buffer exactly as itm_mesh_scene on a hash scene or an update left it: current once one
  // of the two has recorded it, stale from the moment anything else writes the buffer (the filter, the smoothing, a dense volume's mesh).
  void vertices_moved() { attrCurrent = 0; indexedAttrCurrent = 0; runCurrent = false; components_recomputing(); }
  void soup_rewritten() { attrCurrent = 0; runCurrent = false; index_rebuilding(); }
  void soup_remeshed() { soup_rewritten(); fromVolume = false; }       // itm_mesh_scene: the buffer holds a dense volume's mesh no more
  void index_rebuilding() { indexCurrent = false; indexedAttrCurrent = 0; components_recomputing(); }
  void components_recomputing() { componentsCurrent = false; }
  void meshed_from_volume() { fromVolume = true; }                     // itm_mesh_volume has meshed a dense scene into the buffer
  void attributes_current(bool indexed, uint32_t what) { (indexed ? indexedAttrCurrent : attrCurrent) |= what; }
  void index_current() { indexCurrent = true; }
  void components_current() { componentsCurrent = true; }
  void run_table_recorded() { runCurrent = true; }
  bool run_table_current() const { return runCurrent; }
  bool holds_volume_mesh() const { return fromVolume; }
  uint32_t attributes(bool indexed) const { return indexed ? indexedAttrCurrent : attrCurrent; }   // the ITM_MESH_* bits that are current
  int require_index() const { return indexCurrent ? ITM_OK : itm::set_error(ITM_ERR_INVALID, "no index for this mesh: itm_mesh_index has not built it since the last itm_mesh_scene"); }
  int require_components() const {
    return indexCurrent && componentsCurrent ? ITM_OK : itm::set_error(ITM_ERR_INVALID, "no components for this mesh: itm_mesh_components has not labelled the present index");
  }
  // the attributes a download names (by a destination that is not null) are current: the soup's, or those of the present index
  int require_attributes(bool normals, bool colours, bool indexed) const {
    if (indexed) { const int rc = require_index(); if (rc) return rc; }
    const uint32_t missing = ((normals ? ITM_MESH_NORMALS : 0) | (colours ? ITM_MESH_COLOURS : 0)) & ~attributes(indexed);
    if (!missing) return ITM_OK;
    return itm::set_error(ITM_ERR_INVALID, std::string(missing & ITM_MESH_NORMALS ? "no normals" : "no colours") +
        (indexed ? " for the indexed mesh: itm_mesh_indexed_attributes has not computed them since the last itm_mesh_index"
                 : " for this mesh: itm_mesh_attributes has not computed them since the last itm_mesh_scene"));
  }
 private:
  bool fromVolume = false;           // the buffer holds the mesh itm_mesh_volume made of a dense scene
  uint32_t attrCurrent = 0;          // ITM_MESH_* bits computed for the soup
  bool indexCurrent = false;         // vertices / faces / first describe the soup
  uint32_t indexedAttrCurrent = 0;   // ITM_MESH_* bits computed for the index
  bool componentsCurrent = false;    // the labelling describes the index
  bool runCurrent = false;           // the run table describes the buffer (and, on the device, whether every generated triangle fitted)
};

namespace itm {

int launch_mesh_volume_dense(const itm_scene* s, itm_mesh* m, hipStream_t st);   // mesh_dense.hip
hipError_t alloc_update_arena(const itm_scene* s, itm_mesh* m);                    // mesh_update.hip: itm_mesh_create, hash scenes
int record_run_table(const itm_scene* s, itm_mesh* m, hipStream_t st);             // mesh_update.hip: the tail of itm_mesh_scene on a hash scene

// The clamped download: min(count, capacity) elements of `src` to the host, nothing where that is 0 or `dst` is null (the caller synchronises)
inline hipError_t copy_out(void* dst, const void* src, size_t count, size_t capacity, size_t bytesPerElement, hipStream_t st) {
  const size_t n = count < capacity ? count : capacity;
  return (n && dst) ? hipMemcpyAsync(dst, src, n * bytesPerElement, hipMemcpyDeviceToHost, st) : hipSuccess;
}

// The file writers' two fetchers (meshing.hip, mesh_index.hip; withAttributes: and the attributes that are current); a writer's answer as the library's
int fetch_soup(const itm_mesh* m, bool withAttributes, FetchedMesh& out, itm_stream stream);
int fetch_indexed(const itm_mesh* m, bool withAttributes, FetchedMesh& out, itm_stream stream);
inline int file_status(const std::string& error) { return error.empty() ? ITM_OK : set_error(ITM_ERR_INVALID, error); }

}  // namespace itm
