// launch_grid.hpp -- the grids of the engine's element-wise kernels over n elements (256 threads per workgroup): the
// capped grid of the grid-stride kernels and the full grid of the one-thread-per-element kernels.  One definition for
// the engine (bchmc.hip) and the kernel probes (fft_probe.hip), which thereby launch these kernels on the grid the
// engine gives them; and the workgroup -> row mapping of the two ALPT stencil passes, which a host program checks as it
// stands (tests/host/stencil_row_check.cpp).  Plain C++.
#pragma once

#include <algorithm>

#ifdef __HIPCC__
#define BCHMC_LAUNCH_GRID_FN __host__ __device__ __forceinline__
#else
#define BCHMC_LAUNCH_GRID_FN inline
#endif

namespace bchmc {

inline int nblk_stride(long long n) { return (int)std::min<long long>((n + 255) / 256, 2048); }
inline int nblk_full(long long n) { return (int)((n + 255) / 256); }

// Workgroup -> z-rows for the two stencil passes.  Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8
// share one), each XCD has its own L2, and the 4th-order stencils reach two rows (j) and two planes (i) either way: with
// consecutive rows on consecutive workgroups every XCD fetched every row of the array for its y neighbours.  Here the
// row slots a workgroup takes (b, b + gridDim, ...; gridDim a multiple of 8) all lie in ONE slab of n / 8 consecutive j
// -- the same slab for all workgroups of an XCD -- so the y and x neighbours of a row are rows of the same XCD, but for
// the two rows at each slab edge.  Pure scheduling: any mapping gives the same numbers.  (Measured: the two passes
// 0.70 -> 0.61 ms at 256^3.  Staging the rows of a group of 4 output rows in LDS instead -- 6 and 9 coalesced row loads
// per output row, neighbours read from LDS -- was measured too and ran 1.10 ms: 72 KB of LDS per workgroup leave two
// workgroups per CU and nothing to overlap their load phases with; profiles/r03_ab_alpt_rows.txt.)
BCHMC_LAUNCH_GRID_FN void stencil_row(int slot, int n, int &i, int &j) {
  if ((n & 7) == 0) {
    const int slab = n >> 3, x = slot & 7, loc = slot >> 3;
    j = x * slab + loc % slab;
    i = loc / slab;
  } else {
    j = slot % n;
    i = slot / n;
  }
}
inline int stencil_grid(int n) {  // workgroups of the stencil passes: a multiple of 8, at most one per row
  const long long rows = (long long)n * n;
  return (int)std::max<long long>(std::min<long long>(rows, 4096) / 8 * 8, 8);
}

}  // namespace bchmc
