// interp_plan_check.cpp -- barcode_amd/csrc/interp_plan.hpp as plain C++ against a table of cases worked out by hand:
// which kernel a bchmc_interp_particles call runs.  Run by tests/test_interp_plan_cpu.py under ASan / UBSan.
#include "../../barcode_amd/csrc/interp_plan.hpp"

#include <cstdio>
#include <initializer_list>

using namespace bchmc;

namespace {
int failures = 0;
void expect(bool ok, const char *what, int line) {
  if (!ok) {
    std::printf("interp_plan_check: line %d: %s\n", line, what);
    failures++;
  }
}
#define EXPECT(x) expect((x), #x, __LINE__)

InterpFacts facts(bool tiled, int n, int esz, int kernel, int n_fields, uint64_t n_part, int tx = 8, int ty = 8, int tz = 16) {
  InterpFacts f;
  f.tiled = tiled;
  f.tx = tiled ? tx : 0, f.ty = tiled ? ty : 0, f.tz = tiled ? tz : 0;
  f.ntiles = tiled ? (n / tx) * (n / ty) * (n / tz) : 0;
  f.esz = esz, f.kernel = kernel, f.n_fields = n_fields, f.n_part = n_part;
  return f;
}
}  // namespace

int main() {
  // the image: 10 x 10 x 18 cells per field
  EXPECT(interp_image_bytes(facts(true, 256, 8, 1, 1, 1)) == 14400);
  EXPECT(interp_image_bytes(facts(true, 256, 8, 2, 4, 1)) == 57600);
  EXPECT(interp_image_bytes(facts(true, 256, 4, 2, 4, 1)) == 28800);
  EXPECT(interp_tiles_possible(facts(true, 256, 8, 2, 4, 1)));
  EXPECT(!interp_tiles_possible(facts(false, 9, 8, 2, 1, 1)));
  // a tile shape whose four fp64 images pass 64 KiB cannot run the tile kernel; two of them (51840 bytes) can, and fp32 can
  EXPECT(interp_image_bytes(facts(true, 256, 8, 1, 4, 1, 8, 16, 16)) == 10 * 18 * 18 * 8 * 4);
  EXPECT(!interp_tiles_possible(facts(true, 256, 8, 1, 4, 1, 8, 16, 16)));
  EXPECT(!interp_tiles_possible(facts(true, 256, 8, 1, 3, 1, 8, 16, 16)));
  EXPECT(interp_tiles_possible(facts(true, 256, 8, 1, 2, 1, 8, 16, 16)));
  EXPECT(interp_tiles_possible(facts(true, 256, 4, 1, 4, 1, 8, 16, 16)));

  // what was asked is what runs, or a refusal
  for (int kernel = 1; kernel <= 2; kernel++)
    for (int K = 1; K <= 4; K++)
      for (uint64_t m : {uint64_t(0), uint64_t(1), uint64_t(1) << 16, uint64_t(1) << 20, uint64_t(1) << 24, uint64_t(2147483647)}) {
        const InterpFacts t = facts(true, 256, 8, kernel, K, m), o = facts(false, 9, 8, kernel, K, m);
        EXPECT(interp_path(t, 0) == kInterpDirect);
        EXPECT(interp_path(t, 1) == kInterpTile);
        EXPECT(interp_path(o, 0) == kInterpDirect);
        EXPECT(interp_path(o, 1) == kInterpNoTiles);
        EXPECT(interp_path(o, -1) == kInterpDirect);  // never a refusal, never the tile kernel without tiles
        const int p = interp_path(t, -1);
        EXPECT(p == kInterpDirect || p == kInterpTile);
        EXPECT(p == (interp_tiles_wanted(t) ? kInterpTile : kInterpDirect));
        EXPECT(interp_path(facts(true, 256, 8, kernel, 4, m, 8, 16, 16), 1) == kInterpNoTiles);
        EXPECT(interp_path(facts(true, 256, 8, kernel, 4, m, 8, 16, 16), -1) == kInterpDirect);
      }

  // the rule for path = -1, from the figures beside it in the header: TSC, three fields or more, 64 particles per tile in
  // the first batch, not the handle's own particles
  auto wanted = [](int kernel, int K, uint64_t m, bool own = false, int n = 256) {
    InterpFacts f = facts(true, n, 8, kernel, K, m);
    f.own_particles = own;
    return interp_path(f, -1) == kInterpTile;
  };
  EXPECT(facts(true, 256, 8, 2, 3, 0).ntiles == 16384);
  const uint64_t M16 = uint64_t(1) << 16, M20 = uint64_t(1) << 20, M24 = uint64_t(1) << 24;
  EXPECT(wanted(2, 3, M20) && wanted(2, 3, M24) && wanted(2, 4, M20) && wanted(2, 4, M24));  // measured 0.64
  EXPECT(!wanted(2, 3, M16) && !wanted(2, 4, M16));                                          // measured 4.6
  EXPECT(!wanted(2, 1, M20) && !wanted(2, 1, M24) && !wanted(2, 2, M24));                    // measured 1.4
  for (int K = 1; K <= 4; K++) EXPECT(!wanted(1, K, M16) && !wanted(1, K, M20) && !wanted(1, K, M24));  // CIC: 1.3 .. 6.9
  EXPECT(!wanted(2, 3, M24, true) && !wanted(2, 4, M24, true));                              // lattice order: 4.3
  EXPECT(wanted(2, 3, M20 - 1) == false);  // 16384 tiles x 64 is exactly a batch
  // a small grid: 4 tiles at n = 16, so 256 particles are 64 per tile
  EXPECT(facts(true, 16, 8, 2, 3, 0).ntiles == 4);
  EXPECT(wanted(2, 3, 256, false, 16) && !wanted(2, 3, 255, false, 16) && !wanted(2, 3, 50000, true, 16));
  // monotonic in the particle count, and a batch is the most that counts
  for (int K = 1; K <= 4; K++) {
    bool was = false;
    for (uint64_t m = 1; m <= (uint64_t(1) << 26); m *= 2) {
      const bool now = wanted(2, K, m);
      EXPECT(now || !was);
      was = now;
    }
    EXPECT(wanted(2, K, uint64_t(1) << 26) == wanted(2, K, M20));
  }
  EXPECT(!wanted(0, 4, M24) && !wanted(3, 4, M24));  // no such kernel: nothing is wanted

  if (failures) return 1;
  std::printf("interp_plan_check: ok\n");
  return 0;
}
