// stencil_row_check.cpp -- the workgroup -> row mapping of the two ALPT stencil passes (barcode_amd/csrc/launch_grid.hpp:
// stencil_row, stencil_grid) as plain C++, for tests/test_rs_bounds.py.  For every n on the command line: every slot of
// [0, n^2) maps into the grid, no row is taken twice, every workgroup's slots lie in the slab of (workgroup & 7) where n is
// a multiple of 8, and marking rows the way the kernels' slot loop walks them leaves none unmarked.  Prints
// "n <n> grid <g>" and one line of "i j" pairs in slot order, which the test compares with its own restatement.
#include "../../barcode_amd/csrc/launch_grid.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
  for (int a = 1; a < argc; a++) {
    const int n = std::atoi(argv[a]);
    if (n < 1 || n > 512) return 2;
    const int grid = bchmc::stencil_grid(n), rows = n * n;
    if (grid % 8 || grid < 8 || grid > 4096 || (rows >= 8 && grid > rows)) return 3;
    std::vector<int> hits((size_t)rows, 0);  // the sanitizer sees an (i, j) outside the grid
    std::printf("n %d grid %d\n", n, grid);
    for (int slot = 0; slot < rows; slot++) {
      int i = -1, j = -1;
      bchmc::stencil_row(slot, n, i, j);
      if (i < 0 || i >= n || j < 0 || j >= n) return 4;
      std::printf("%d %d%c", i, j, slot + 1 < rows ? ' ' : '\n');
    }
    for (int b = 0; b < grid; b++)
      for (int slot = b; slot < rows; slot += grid) {  // the kernels' slot loop
        int i, j;
        bchmc::stencil_row(slot, n, i, j);
        hits[(size_t)i * n + j]++;
        if (n % 8 == 0 && j / (n / 8) != (b & 7)) return 5;
      }
    for (int h : hits)
      if (h != 1) return 6;
  }
  return 0;
}
