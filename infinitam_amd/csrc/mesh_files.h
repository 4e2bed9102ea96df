// mesh_files.h -- a mesh on the host and the three file formats, once each.  Plain C++: no device code, no runtime call, so the
// writers run (and are tested, tests/test_mesh_files.py) without a GPU.
//   write_obj   ITMMesh::WriteOBJ (Objects/ITMMesh.h:34-62): one "v" line per vertex, then the faces, 1-based, winding reversed
//   write_stl   ITMMesh::WriteSTL (:64-110): binary, 80 spaces of header, zero normals, corners p2 p1 p0, zero attribute word
//   write_ply   binary_little_endian PLY: positions, then the attributes the view has; faces with WriteOBJ's winding
// Each returns "" or the error's text ("cannot create <path>", "short write to <path>").
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace itm {

// The triangle soup (faces == nullptr: face i is (3i, 3i + 1, 3i + 2), noVertices == 3 noTriangles) or an indexed mesh.
struct HostMesh {
  const float* positions = nullptr;    // three floats per vertex
  size_t noVertices = 0, noTriangles = 0;
  const uint32_t* faces = nullptr;     // three vertex indices per triangle
  bool withNormals = false, withColours = false;
  const float* normals = nullptr;      // withNormals: three floats per vertex
  const uint8_t* colours = nullptr;    // withColours: four bytes per vertex, of which three are written
  uint32_t corner(size_t i, int k) const { return faces ? faces[3 * i + k] : (uint32_t)(3 * i + k); }
};

// Creates `path`, lets body(FILE*) write it and closes it; a write that failed shows in the stream's error flag or in the close.
template <class Body>
std::string write_file(const char* path, Body&& body) {
  FILE* f = fopen(path, "wb");
  if (!f) return std::string("cannot create ") + path;
  body(f);
  const bool failed = ferror(f) != 0;
  return (fclose(f) != 0 || failed) ? std::string("short write to ") + path : std::string();
}

// Face indices are printed with %u: a triangle buffer holds fewer than 2^32 / 36 triangles, so every index (and index + 1) is below
// 2^31, where %d and %u print the same digits.
inline std::string write_obj(const HostMesh& m, const char* path) {
  return write_file(path, [&](FILE* f) {
    for (size_t v = 0; v < m.noVertices; ++v) fprintf(f, "v %f %f %f\n", m.positions[v * 3], m.positions[v * 3 + 1], m.positions[v * 3 + 2]);
    for (size_t i = 0; i < m.noTriangles; ++i) fprintf(f, "f %u %u %u\n", m.corner(i, 2) + 1u, m.corner(i, 1) + 1u, m.corner(i, 0) + 1u);
  });
}

inline std::string write_stl(const HostMesh& m, const char* path) {
  return write_file(path, [&](FILE* f) {
    const uint32_t n = (uint32_t)m.noTriangles;
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const short attribute = 0;
    fwrite(std::string(80, ' ').data(), 1, 80, f);
    fwrite(&n, 4, 1, f);
    for (size_t i = 0; i < m.noTriangles; ++i) {
      fwrite(zero, 4, 3, f);
      for (int k = 2; k >= 0; --k) fwrite(m.positions + 3 * (size_t)m.corner(i, k), 4, 3, f);
      fwrite(&attribute, 2, 1, f);
    }
  });
}

inline std::string write_ply(const HostMesh& m, const char* path) {
  std::string head = "ply\nformat binary_little_endian 1.0\ncomment itm-hip mesh\nelement vertex " + std::to_string((unsigned long long)m.noVertices) +
                     "\nproperty float x\nproperty float y\nproperty float z\n";
  if (m.withNormals) head += "property float nx\nproperty float ny\nproperty float nz\n";
  if (m.withColours) head += "property uchar red\nproperty uchar green\nproperty uchar blue\n";
  head += "element face " + std::to_string((unsigned long long)m.noTriangles) + "\nproperty list uchar int vertex_indices\nend_header\n";
  const size_t vertexBytes = 12 + (m.withNormals ? 12 : 0) + (m.withColours ? 3 : 0);
  std::vector<uint8_t> body(m.noVertices * vertexBytes + m.noTriangles * 13);
  uint8_t* o = body.data();
  for (size_t v = 0; v < m.noVertices; ++v) {
    memcpy(o, m.positions + v * 3, 12); o += 12;
    if (m.withNormals) { memcpy(o, m.normals + v * 3, 12); o += 12; }
    if (m.withColours) { memcpy(o, m.colours + v * 4, 3); o += 3; }
  }
  for (size_t i = 0; i < m.noTriangles; ++i) {
    const int32_t idx[3] = {(int32_t)m.corner(i, 2), (int32_t)m.corner(i, 1), (int32_t)m.corner(i, 0)};
    *o++ = 3;
    memcpy(o, idx, 12); o += 12;
  }
  return write_file(path, [&](FILE* f) {
    fwrite(head.data(), 1, head.size(), f);
    if (!body.empty()) fwrite(body.data(), 1, body.size(), f);
  });
}

// A mesh fetched from the device, and the view of it the writers take.
struct FetchedMesh {
  std::vector<float> positions, normals;
  std::vector<uint32_t> faces;
  std::vector<uint8_t> colours;
  HostMesh view;
  // room for nV vertices, nT triangles (the soup: no faces) and the attributes asked for, and the view of it
  void resize(size_t nV, size_t nT, bool indexed, bool withNormals, bool withColours) {
    positions.resize(nV * 3); faces.resize(indexed ? nT * 3 : 0); normals.resize(withNormals ? nV * 3 : 0); colours.resize(withColours ? nV * 4 : 0);
    view = HostMesh{positions.data(), nV, nT, faces.empty() ? nullptr : faces.data(), withNormals, withColours, normals.data(), colours.data()};
  }
  float* normals_or_null() { return view.withNormals ? normals.data() : nullptr; }     // where a download puts them, if it is to fetch them
  uint8_t* colours_or_null() { return view.withColours ? colours.data() : nullptr; }
};

}  // namespace itm
