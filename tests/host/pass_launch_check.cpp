// Stand-alone check of the arithmetic part of barcode_amd/csrc/pass_launch.hpp on the CPU (tests/test_pass_launch_cpu.py
// builds it with g++ under AddressSanitizer / UndefinedBehaviorSanitizer and runs it): block sizes, template arguments,
// dynamic LDS sizes and grids of the engine's own FFT passes, against literals worked out by hand from the formulas the
// launch sites spelled out before the header existed:
//     KB = 128 / sizeof(complex);  NT_BIG = 256 (fp64) | 512 (fp32), NT_SMALL = NT_BIG / 4;
//     x pass: n = 32, 64 -> (NT_SMALL, 4 | 8); 128 -> (NT_BIG, 4); 256, 512 -> (2 NT_BIG, 4 | 8); two tiles: 128, 256 only;
//     y pass: n = 128 -> 256 threads, 256 and 512 -> 512 threads, PER = n KB / NT;  z rows: n threads, n = 128, 256, 512;
//     column LDS = (tiles n KB + n / 2) complex, row LDS = (6 n + n / 2) complex;
//     column grid = comps n (nhp / KB), row grid = (n / 2)^2.
// A wrong entry here is a kernel launched on the wrong tile: this is the proof that comes before any launch.
#include <cstdio>
#include <cstdlib>

#include "../../barcode_amd/csrc/fft_host.hpp"
#include "../../barcode_amd/csrc/pass_launch.hpp"

using namespace bchmc;

namespace {

int g_failures = 0;

void expect(const char *what, int esz, int n, long long got, long long want) {
  if (got != want && g_failures++ < 40) std::printf("FAIL %s (esz %d, n %d): %lld, expected %lld\n", what, esz, n, got, want);
}
void expect_shape(const char *what, int esz, int n, PassShape s, int nt, int per) {
  expect(what, esz, n, s.nt, nt);
  expect(what, esz, n, s.per, per);
}

struct Row {
  int n, nt, per;
};

void literals() {
  // ---- fp64 ----
  expect("KB", 8, 0, pass_kb(8), 8);
  expect("NT_BIG", 8, 0, pass_nt_big(8), 256);
  expect("NT_SMALL", 8, 0, pass_nt_small(8), 64);
  const Row x64[] = {{32, 64, 4}, {64, 64, 8}, {128, 256, 4}, {256, 512, 4}, {512, 512, 8}};
  for (const Row &r : x64) expect_shape("x pass", 8, r.n, x_shape(8, r.n), r.nt, r.per);
  const Row x2_64[] = {{32, 0, 0}, {64, 0, 0}, {128, 256, 4}, {256, 512, 4}, {512, 0, 0}};
  for (const Row &r : x2_64) expect_shape("two-tile x pass", 8, r.n, x2_shape(8, r.n), r.nt, r.per);
  const Row y64[] = {{32, 0, 0}, {64, 0, 0}, {128, 256, 4}, {256, 512, 4}, {512, 512, 8}};
  for (const Row &r : y64) expect_shape("y pass", 8, r.n, y_shape(8, r.n), r.nt, r.per);
  expect("column LDS", 8, 32, (long long)col_lds(8, 32), 4352);
  expect("column LDS", 8, 128, (long long)col_lds(8, 128), 17408);
  expect("column LDS", 8, 256, (long long)col_lds(8, 256), 34816);
  expect("column LDS", 8, 512, (long long)col_lds(8, 512), 69632);
  expect("column LDS, two tiles", 8, 128, (long long)col_lds(8, 128, 2), 33792);
  expect("column LDS, two tiles", 8, 256, (long long)col_lds(8, 256, 2), 67584);
  expect("row LDS", 8, 128, (long long)zrow_lds(8, 128), 13312);
  expect("row LDS", 8, 512, (long long)zrow_lds(8, 512), 53248);

  // ---- fp32 ----
  expect("KB", 4, 0, pass_kb(4), 16);
  expect("NT_BIG", 4, 0, pass_nt_big(4), 512);
  expect("NT_SMALL", 4, 0, pass_nt_small(4), 128);
  const Row x32[] = {{32, 128, 4}, {64, 128, 8}, {128, 512, 4}, {256, 1024, 4}, {512, 1024, 8}};
  for (const Row &r : x32) expect_shape("x pass", 4, r.n, x_shape(4, r.n), r.nt, r.per);
  const Row x2_32[] = {{32, 0, 0}, {64, 0, 0}, {128, 512, 4}, {256, 1024, 4}, {512, 0, 0}};
  for (const Row &r : x2_32) expect_shape("two-tile x pass", 4, r.n, x2_shape(4, r.n), r.nt, r.per);
  const Row y32[] = {{32, 0, 0}, {64, 0, 0}, {128, 256, 8}, {256, 512, 8}, {512, 512, 16}};
  for (const Row &r : y32) expect_shape("y pass", 4, r.n, y_shape(4, r.n), r.nt, r.per);
  expect("column LDS", 4, 32, (long long)col_lds(4, 32), 4224);
  expect("column LDS", 4, 512, (long long)col_lds(4, 512), 67584);
  expect("column LDS, two tiles", 4, 256, (long long)col_lds(4, 256, 2), 66560);
  expect("row LDS", 4, 512, (long long)zrow_lds(4, 512), 26624);

  // ---- both: z rows and grids (row stride: 17 unpadded at n = 32; 65 -> 72 | 80, 129 -> 136 | 144, 257 -> 264 | 272) ----
  for (int esz : {4, 8}) {
    const Row z[] = {{32, 0, 0}, {64, 0, 0}, {128, 128, 6}, {256, 256, 6}, {512, 512, 6}};
    for (const Row &r : z) expect_shape("z rows", esz, r.n, z_shape(esz, r.n), r.nt, r.per);
    for (int n : {16, 48, 1024})
      expect("not available", esz, n, x_shape(esz, n).nt + x2_shape(esz, n).nt + y_shape(esz, n).nt + z_shape(esz, n).nt, 0);
    expect("row grid", esz, 128, row_grid(128), 4096);
    expect("row grid", esz, 256, row_grid(256), 16384);
    expect("row grid", esz, 512, row_grid(512), 65536);
  }
  expect("row stride", 8, 256, fft_row_stride(256, 8), 136);
  expect("row stride", 4, 256, fft_row_stride(256, 4), 144);
  expect("column grid", 8, 32, col_grid(8, 32, fft_row_stride(32, 8)), 64);
  expect("column grid", 4, 32, col_grid(4, 32, fft_row_stride(32, 4)), 32);
  expect("column grid", 8, 128, col_grid(8, 128, fft_row_stride(128, 8)), 1152);
  expect("column grid", 4, 128, col_grid(4, 128, fft_row_stride(128, 4)), 640);
  expect("column grid", 8, 256, col_grid(8, 256, fft_row_stride(256, 8)), 4352);
  expect("column grid", 4, 256, col_grid(4, 256, fft_row_stride(256, 4)), 2304);
  expect("column grid", 8, 512, col_grid(8, 512, fft_row_stride(512, 8)), 16896);
  expect("column grid", 4, 512, col_grid(4, 512, fft_row_stride(512, 4)), 8704);
  expect("column grid, 3 components", 8, 256, col_grid(8, 256, fft_row_stride(256, 8), 3), 13056);
  expect("column grid, 3 components", 4, 256, col_grid(4, 256, fft_row_stride(256, 4), 3), 6912);
  expect("column grid, 3 components", 8, 512, col_grid(8, 512, fft_row_stride(512, 8), 3), 50688);
  expect("column grid, 3 components", 4, 512, col_grid(4, 512, fft_row_stride(512, 4), 3), 26112);
}

// every entry of every table: the tile is covered exactly, the block is one the hardware takes, the LDS fits the CU;
// every other n answers "not available"
void invariants() {
  const size_t kCuLds = 160 * 1024;
  for (int esz : {4, 8}) {
    const int kb = pass_kb(esz);
    int rows = 0;
    for (int n = 1; n <= 2048; n++) {
      const bool x_n = n == 32 || n == 64 || n == 128 || n == 256 || n == 512, big_n = n == 128 || n == 256 || n == 512;
      const PassShape x = x_shape(esz, n), x2 = x2_shape(esz, n), y = y_shape(esz, n), z = z_shape(esz, n);
      expect("x pass available", esz, n, x.nt != 0, x_n);
      expect("two-tile x pass available", esz, n, x2.nt != 0, n == 128 || n == 256);
      expect("y pass available", esz, n, y.nt != 0, big_n);
      expect("z rows available", esz, n, z.nt != 0, big_n);
      for (const PassShape &s : {x, x2, y}) {
        if (!s.nt) {
          expect("PER of an absent row", esz, n, s.per, 0);
          continue;
        }
        rows++;
        expect("PER * NT", esz, n, (long long)s.per * s.nt, (long long)n * kb);
        expect("NT <= 1024", esz, n, s.nt <= 1024 && s.nt % 64 == 0, 1);
      }
      if (x.nt) expect("column LDS fits", esz, n, col_lds(esz, n) <= kCuLds, 1);
      if (x2.nt) expect("two-tile column LDS fits", esz, n, col_lds(esz, n, 2) <= kCuLds, 1);
      if (z.nt) {
        rows++;
        expect("NZ == n", esz, n, z.nt, n);
        expect("NZ <= 1024", esz, n, z.nt <= 1024 && z.nt % 64 == 0, 1);
        expect("row LDS fits", esz, n, zrow_lds(esz, n) <= kCuLds, 1);
      }
    }
    expect("rows in the tables", esz, 0, rows, 5 + 2 + 3 + 3);
  }
}

}  // namespace

int main() {
  unsetenv("BCHMC_FFT_PAD");  // fft_row_stride's test switch: the literals are for the engine's default padding
  literals();
  invariants();
  if (g_failures) {
    std::printf("pass_launch_check: %d failures\n", g_failures);
    return 1;
  }
  std::printf("pass_launch_check: ok\n");
  return 0;
}
