// Host-only exhaustive check of the block directory's index from voxel-unit coordinates (accel_device.h: dir_cell_voxel,
// dir_covers_voxel) against the block-unit form every writer and every other reader uses (dir_cell, dir_covers).  Own main, no device
// code runs and nothing is loaded into another process: built and run by tests/test_dir_index_exhaustive.py, and once by hand under
// -fsanitize=address,undefined.
//   1. every cube-relative block triple (2^27): the same cell from the triple and from a voxel of that block (the in-block offsets
//      cycle through all 8 x 8 x 8 combinations over the sweep), and the cell is the identity's image: below kDirCells, every cell once
//      per 64-cell brick position (checked through a checksum of the cells).
//   2. the ray cast's expressions, for the directory origins 0, negative and positive: a world voxel coordinate ix, origin d (blocks):
//      block form  u = (uint32)((ix >> 3) - d),  voxel form  t = (uint32)ix - 8 * (uint32)d  -- for every block of the cube and of a
//      band of 2 blocks around it on every side (516^3 triples per origin), in-block offsets cycling: the same coverage answer, and
//      where covered the same cell; where not covered the voxel form's cell is still a valid index (it is read, its value ignored).
//   3. per axis, EVERY voxel coordinate of the band (all 8 in-block offsets of all 516 blocks) with the other two axes at the cube's
//      corners, middle and just outside; and coordinates at the ends of the int range (never covered, always a valid cell).
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../infinitam_amd/csrc/accel_device.h"

using namespace itm;

static unsigned long long failures = 0;
static void fail(const char* what, long long a, long long b, long long c, long long d) {
  if (failures++ < 10) std::fprintf(stderr, "FAIL %s: %lld %lld %lld (origin %lld)\n", what, a, b, c, d);
}

// the two forms for world voxel (ix, iy, iz) and origin (dx, dy, dz), as raycast_device.h writes them
static inline void both(int ix, int iy, int iz, int dx, int dy, int dz, bool& covB, uint32_t& cellB, bool& covV, uint32_t& cellV) {
  const uint32_t ux = (uint32_t)((ix >> 3) - dx), uy = (uint32_t)((iy >> 3) - dy), uz = (uint32_t)((iz >> 3) - dz);
  covB = dir_covers(ux, uy, uz);
  cellB = covB ? dir_cell(ux, uy, uz) : 0u;
  const uint32_t tx = (uint32_t)ix - (uint32_t)dx * 8u, ty = (uint32_t)iy - (uint32_t)dy * 8u, tz = (uint32_t)iz - (uint32_t)dz * 8u;
  covV = dir_covers_voxel(tx, ty, tz);
  cellV = dir_cell_voxel(tx, ty, tz);
}

int main() {
  // ---- 1 ----
  unsigned long long sum = 0;
  for (uint32_t uz = 0; uz < (uint32_t)kDirSide; ++uz)
    for (uint32_t uy = 0; uy < (uint32_t)kDirSide; ++uy)
      for (uint32_t ux = 0; ux < (uint32_t)kDirSide; ++ux) {
        const uint32_t k = ux + 3u * uy + 5u * uz;                    // in-block offsets: all 512 combinations occur
        const uint32_t tx = ux * 8u + (k & 7u), ty = uy * 8u + ((k >> 3) & 7u), tz = uz * 8u + ((k >> 6) & 7u);
        const uint32_t want = dir_cell(ux, uy, uz), got = dir_cell_voxel(tx, ty, tz);
        if (want != got || !dir_covers_voxel(tx, ty, tz) || !dir_covers(ux, uy, uz) || got >= kDirCells) fail("cube triple", ux, uy, uz, 0);
        sum += got;
      }
  if (sum != (unsigned long long)kDirCells * (kDirCells - 1) / 2) fail("cells are not a permutation", (long long)sum, 0, 0, 0);
  // ---- 2 ----
  const int origins[][3] = {{0, 0, 0}, {-256, -256, -256}, {-37, -300, -1000}, {5, 255, 4000}, {-32768 - 256, 32767 - 256, 12}};
  const int band = 2;
  for (const auto& d : origins) {
    unsigned long long covered = 0;
    for (int bz = -band; bz < kDirSide + band; ++bz)
      for (int by = -band; by < kDirSide + band; ++by)
        for (int bx = -band; bx < kDirSide + band; ++bx) {
          const uint32_t k = (uint32_t)(bx + band) + 3u * (uint32_t)(by + band) + 5u * (uint32_t)(bz + band);
          const int ix = (d[0] + bx) * 8 + (int)(k & 7u), iy = (d[1] + by) * 8 + (int)((k >> 3) & 7u), iz = (d[2] + bz) * 8 + (int)((k >> 6) & 7u);
          bool cb, cv; uint32_t eb, ev;
          both(ix, iy, iz, d[0], d[1], d[2], cb, eb, cv, ev);
          const bool inside = bx >= 0 && bx < kDirSide && by >= 0 && by < kDirSide && bz >= 0 && bz < kDirSide;
          if (cb != inside || cv != inside || (inside && eb != ev) || ev >= kDirCells) fail("band triple", ix, iy, iz, d[0]);
          covered += inside;
        }
    if (covered != kDirCells) fail("covered count", (long long)covered, 0, 0, d[0]);
    // ---- 3 ----
    const int others[] = {-1, 0, 1, kDirSide / 2, kDirSide - 1, kDirSide};      // block coordinates of the other two axes
    for (int axis = 0; axis < 3; ++axis)
      for (int v = -band * 8; v < (kDirSide + band) * 8; ++v)
        for (int p : others)
          for (int q : others)
            for (int o = 0; o < 8; o += 7) {
              int b[3] = {p * 8 + o, q * 8 + (7 - o), 0};
              int w[3];
              w[axis] = v; w[(axis + 1) % 3] = b[0]; w[(axis + 2) % 3] = b[1];
              const int ix = d[0] * 8 + w[0], iy = d[1] * 8 + w[1], iz = d[2] * 8 + w[2];
              bool cb, cv; uint32_t eb, ev;
              both(ix, iy, iz, d[0], d[1], d[2], cb, eb, cv, ev);
              if (cb != cv || (cb && eb != ev) || ev >= kDirCells) fail("axis sweep", ix, iy, iz, d[0]);
            }
    const int far[] = {INT32_MIN, INT32_MIN + 1, -(1 << 30), (1 << 30), INT32_MAX - 7, INT32_MAX};
    for (int a : far)
      for (int axis = 0; axis < 3; ++axis) {
        int w[3] = {d[0] * 8 + 100, d[1] * 8 + 100, d[2] * 8 + 100};
        w[axis] = a;
        bool cb, cv; uint32_t eb, ev;
        both(w[0], w[1], w[2], d[0], d[1], d[2], cb, eb, cv, ev);
        if (cb || cv || ev >= kDirCells) fail("far coordinate", w[0], w[1], w[2], d[0]);
      }
  }
  if (failures) { std::fprintf(stderr, "%llu failures\n", failures); return 1; }
  std::printf("dir index check ok: %llu cube triples, %zu origins\n", (unsigned long long)kDirCells, sizeof(origins) / sizeof(origins[0]));
  return 0;
}
