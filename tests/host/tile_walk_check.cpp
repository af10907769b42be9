// Stand-alone check of barcode_amd/csrc/tile_walk.hpp on the CPU (tests/test_tile_walk_cpu.py builds it with g++ under
// AddressSanitizer / UndefinedBehaviorSanitizer and runs it): the threads of a workgroup are played out in a loop, every
// image cell must come exactly once, and every (LDS index, global cell index) pair must be what the formula gives that
// the tile kernels used before the walker:
//     cz = c % lz, cy = (c / lz) % ly, cx = c / (lz ly);  g = (o + c + n) % n per axis;  gz + n (gy + n gx).
// The visit counts live in a heap array of exactly the image's size and the global index is checked against [0, n^3)
// before it is compared, so an index outside either is a sanitizer report or a failure, never a silent pass.
#include <cstdio>
#include <vector>

#include "../../barcode_amd/csrc/tile_walk.hpp"

namespace {

long long g_failures = 0;

void fail(const char *what, int n, int tx, int ty, int tz, int halo, int tile, int nt, long long a, long long b) {
  if (g_failures++ < 20)
    std::printf("FAIL %s: n %d tile %d x %d x %d halo %d, tile index %d, %d threads: %lld vs %lld\n", what, n, tx, ty, tz,
                halo, tile, nt, a, b);
}

struct Case {
  int n, tx, ty, tz, halo;
};

// one tile's image, walked by nt threads; FIXED: through the compile-time instantiation of the 81-cell kernels
template <bool FIXED>
void check_tile(const Case &k, int txi, int tyi, int tzi, int nt) {
  const int n = k.n, lx = k.tx + 2 * k.halo, ly = k.ty + 2 * k.halo, lz = k.tz + 2 * k.halo;
  const int ox = txi * k.tx - k.halo, oy = tyi * k.ty - k.halo, oz = tzi * k.tz - k.halo;
  const int ncell = lx * ly * lz;
  const int tile = tzi + (n / k.tz) * (tyi + (n / k.ty) * txi);
  std::vector<int> seen(ncell, 0);
  int *seen_p = seen.data();  // plain pointer: an index outside the image is AddressSanitizer's to report
  const long long N = (long long)n * n * n;
  for (int tid = 0; tid < nt; tid++) {
    auto visit = [&](int lds, int cell) {
      if (lds < 0 || lds >= ncell) {
        fail("LDS index outside the image", n, k.tx, k.ty, k.tz, k.halo, tile, nt, lds, ncell);
        return;
      }
      seen_p[lds]++;
      if (cell < 0 || cell >= N) {
        fail("global index outside the grid", n, k.tx, k.ty, k.tz, k.halo, tile, nt, cell, N);
        return;
      }
      const int c = lds;
      const int cz = c % lz, cy = (c / lz) % ly, cx = c / (lz * ly);
      const int gx = (ox + cx + n) % n, gy = (oy + cy + n) % n, gz = (oz + cz + n) % n;
      const long long want = gz + (long long)n * (gy + (long long)n * gx);
      if (cell != want) fail("global index", n, k.tx, k.ty, k.tz, k.halo, tile, nt, cell, want);
    };
    if (FIXED)
      bchmc::tile_walk<12, 20, 256>(lx, 0, 0, ox, oy, oz, n, tid, 0, visit);
    else
      bchmc::tile_walk(lx, ly, lz, ox, oy, oz, n, tid, nt, visit);
  }
  for (int c = 0; c < ncell; c++)
    if (seen[c] != 1) fail("visits of an image cell", n, k.tx, k.ty, k.tz, k.halo, tile, nt, c, seen[c]);
}

long long check_case(const Case &k, int nt) {
  const int ntx = k.n / k.tx, nty = k.n / k.ty, ntz = k.n / k.tz;
  const bool is81 = nt == 256 && k.ty + 2 * k.halo == 12 && k.tz + 2 * k.halo == 20;
  long long tiles = 0;
  auto one = [&](int a, int b, int c) {
    check_tile<false>(k, a, b, c, nt);
    if (is81) check_tile<true>(k, a, b, c, nt);
    tiles++;
  };
  if (k.n <= 48) {
    for (int a = 0; a < ntx; a++)
      for (int b = 0; b < nty; b++)
        for (int c = 0; c < ntz; c++) one(a, b, c);
  } else {  // corners, edge midpoints, face centres and centre of the tile lattice
    const int px[3] = {0, ntx / 2, ntx - 1}, py[3] = {0, nty / 2, nty - 1}, pz[3] = {0, ntz / 2, ntz - 1};
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++)
        for (int c = 0; c < 3; c++) one(px[a], py[b], pz[c]);
  }
  return tiles;
}

}  // namespace

int main() {
  const Case cases[] = {{16, 8, 8, 16, 2}, {32, 8, 8, 16, 2}, {48, 8, 8, 16, 2}, {256, 8, 8, 16, 2},
                        {24, 8, 8, 8, 2},  {12, 4, 4, 4, 2},  {16, 8, 8, 16, 1}, {32, 8, 8, 16, 1},
                        // n = 4: ONE tile whose halo wraps onto the tile on every axis (halo 2: the image is (2 n)^3 and
                        // holds every cell 8 times); halo 1 (low-order kernels), 3 (the cube loop of h = 1.3 d), 4 = n
                        {4, 4, 4, 4, 2},   {4, 4, 4, 4, 1},   {4, 4, 4, 4, 3},   {4, 4, 4, 4, 4}};
  long long tiles = 0;
  for (const Case &k : cases) tiles += check_case(k, 256);
  // not what the kernels launch, but what the walker promises: other block sizes -- a row longer than the block
  // (several cells per lane), a block one row wide, one that is no multiple of anything, more rows per pass than ly --
  // and a halo as wide as the tile
  const Case extra[] = {{16, 8, 8, 16, 2}, {12, 4, 4, 4, 2}, {16, 8, 8, 16, 1}, {8, 4, 4, 4, 4}, {24, 8, 8, 8, 3},
                        {4, 4, 4, 4, 2},   {4, 4, 4, 4, 4}};
  const int blocks[] = {1, 7, 16, 20, 64, 100, 1024};
  for (const Case &k : extra)
    for (int nt : blocks) tiles += check_case(k, nt);
  if (g_failures) {
    std::printf("tile_walk_check: %lld failures\n", g_failures);
    return 1;
  }
  std::printf("tile_walk_check: ok (%lld tiles)\n", tiles);
  return 0;
}
