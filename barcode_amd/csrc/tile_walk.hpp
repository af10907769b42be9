// tile_walk.hpp -- the one walk over a tile image (tile + halo) that the fills and flushes of the tile kernels share.
// Device code under hipcc, plain C++ otherwise (tests/host/tile_walk_check.cpp plays the threads out on the CPU).
#pragma once

#ifdef __HIPCC__
#define BCHMC_TILE_WALK_FN __host__ __device__ __forceinline__
#else
#define BCHMC_TILE_WALK_FN inline
#endif

namespace bchmc {

// The image of a work item is lx x ly x lz cells, LDS index cz + lz (cy + ly cx); its cell (0, 0, 0) is global cell
// (ox, oy, oz), which lies within one halo width below [0, n), and the grid is periodic: image cell (cx, cy, cz) is
// global cell gz + n (gy + n gx) with gx = (ox + cx) mod n, and so on.  tile_walk calls f(LDS index, global cell index)
// for the cells of thread `tid` of `nt`; over tid = 0 .. nt - 1 every image cell comes exactly once.
//
// Rows along z are contiguous in LDS and in global memory, so a thread keeps one lane (cz) of them and walks the rows
// r = cy + ly cx: nt / lz rows per pass, the nt % lz threads left over idle.  Row and lane are decoded once, with the
// only divisions; after that a step is adds and compares: (cx, cy) advance by the decoded row step with one carry,
// the row's global base n (oy + cy) + n^2 (ox + cx) advances with them, and the periodic wrap is one conditional
// add or subtract per axis (halo <= n).  The y and the x part of the base are kept apart: when the rows per pass are
// a multiple of ly -- 256 threads on the 12 x 12 x 20 image of the 81-cell kernels: 12 rows -- cy never changes, so
// everything that depends on the thread is loop-invariant, and cx is the same for the whole workgroup: the compiler
// keeps its wrap and base in scalar registers, and a cell costs one add for the index and the address arithmetic.
//
// LY, LZ, NT: compile-time ly, lz, nt (0 = take the run-time argument).
// Indices are 32-bit: n^2 (n + halo) < 2^31.  The tile path exists for N = n^3 < 2^30 only (bchmc.hip, where
// `tiled` is decided).
template <int LY = 0, int LZ = 0, int NT = 0, typename F>
BCHMC_TILE_WALK_FN void tile_walk(int lx, int ly_rt, int lz_rt, int ox, int oy, int oz, int n, int tid, int nt_rt,
                                  F &&f) {
  const int ly = LY ? LY : ly_rt, lz = LZ ? LZ : lz_rt, nt = NT ? NT : nt_rt;
  const int zl = lz < nt ? lz : nt;  // lanes along z; an image longer than the block takes several cells per row
  const int rpp = nt / zl;           // rows per pass
  const int r0 = tid / zl;
  if (r0 >= rpp) return;
  const int lane = tid - r0 * zl;
  const int sx = rpp / ly, sy = rpp - sx * ly;  // row step
  int cx = rpp <= ly ? 0 : r0 / ly;             // first row
  int cy = r0 - cx * ly;
  const int n2 = n * n, n3 = n2 * n;
  int lrow = lz * (cy + ly * cx);
  int yrow = n * (oy + cy), xrow = n2 * (ox + cx);  // before the wrap: may be negative or past the end
  const int lstep = lz * rpp, ystep = n * sy, xstep = n2 * sx, ycarry = n * ly;
  while (cx < lx) {
    const int gy = oy + cy, gx = ox + cx;
    const int ry = yrow + (gy < 0 ? n2 : (gy >= n ? -n2 : 0));
    const int rx = xrow + (gx < 0 ? n3 : (gx >= n ? -n3 : 0));
    if (lz <= nt) {
      int gz = oz + lane;
      if (gz < 0) gz += n;
      if (gz >= n) gz -= n;
      f(lrow + lane, rx + (ry + gz));
    } else {
      for (int cz = lane; cz < lz; cz += zl) {
        int gz = oz + cz;
        if (gz < 0) gz += n;
        if (gz >= n) gz -= n;
        f(lrow + cz, rx + (ry + gz));
      }
    }
    cx += sx;
    xrow += xstep;
    lrow += lstep;
    if (sy != 0) {
      cy += sy;
      yrow += ystep;
      if (cy >= ly) {
        cy -= ly;
        yrow -= ycarry;
        cx += 1;
        xrow += n2;
      }
    }
  }
}

}  // namespace bchmc
