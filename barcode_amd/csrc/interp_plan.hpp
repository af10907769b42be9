// interp_plan.hpp -- which kernel a bchmc_interp_particles call runs: the tile kernel (LDS images, interp_particles.hpp)
// or the direct one.  The single statement of it, as pure functions of what the handle is and what the call asks.  Plain
// C++: no HIP types; tests/host/interp_plan_check.cpp proves it against a table of cases.
#pragma once

#include <cstddef>
#include <cstdint>

namespace bchmc {

struct InterpFacts {
  bool tiled = false;              // the handle has a tile partition (bchmc_tile_info)
  int tx = 0, ty = 0, tz = 0;      // its tile shape in cells
  int ntiles = 0;
  int esz = 8;                     // bytes of the storage type
  int kernel = 1;                  // 1 CIC, 2 TSC
  int n_fields = 1;
  uint64_t n_part = 0;
  bool own_particles = false;      // BCHMC_PART_FORWARD: the handle's particles, in lattice order
};

enum { kInterpDirect = 0, kInterpTile = 1, kInterpNoTiles = -1 };

constexpr uint64_t kInterpBatch = 1u << 20;        // the catalogue's batch (kCatBatch)
constexpr size_t kInterpLdsLimit = 64 * 1024;      // dynamic LDS a kernel gets without asking for more

// LDS of one work item: tile plus a halo of one cell, every field, in the storage type
constexpr size_t interp_image_bytes(const InterpFacts &f) {
  return (size_t)(f.tx + 2) * (size_t)(f.ty + 2) * (size_t)(f.tz + 2) * (size_t)f.esz * (size_t)f.n_fields;
}
constexpr bool interp_tiles_possible(const InterpFacts &f) {
  return f.tiled && f.ntiles > 0 && interp_image_bytes(f) <= kInterpLdsLimit;
}

// path = -1.  A work item pays for its whole image whatever its length, and a batch pays for count, scan and fill, so
// the tile kernel needs many reads per particle and enough particles per tile and batch to win.  Measured on an MI355X
// (256^3, fp64, 8 x 8 x 16 tiles, 16384 of them; profiles/interp_bench.json), event time of binning plus
// gather, tile kernel over direct kernel, uniform catalogue:
//     particles per tile and batch      4 (2^16)    64 (2^20)    64 (2^24, 16 batches)
//     CIC, 1 field                       6.4          1.80         1.80
//     TSC, 1 field                       5.8          1.44         1.40
//     CIC, 3 fields                      6.9          1.32         1.33
//     TSC, 3 fields                      4.6          0.64         0.64
// The binning costs 0.30 ns per particle at 64 per tile whatever the kernel; the gather falls from 0.87 to 0.26 ns per
// particle for TSC of three fields (81 reads) and by less than the binning costs everywhere else.  So: TSC, three fields
// or more, 64 particles per tile in the first batch.  Two and four fields, fp32 handles and occupancies between 4 and 64
// were not measured: two fields stay with the direct kernel, four go with three, and the threshold is the one occupancy
// seen to win.
// The handle's own particles arrive in lattice order, a batch of 2^20 is a slab of a few tile layers, and count and fill
// then contend on few tiles: 13.4 to 14.1 ms of binning for 2^24 particles against 5.0, and 4.2 to 4.3 times the direct
// kernel's time in all four cases.  They go to the direct kernel.  A host catalogue sorted the same way is as slow on the
// tile kernel and cannot be told from here; path = 0 is there for it.
constexpr int kInterpTileKernel = 2, kInterpTileMinFields = 3;
constexpr uint64_t kInterpTileMinPerTile = 64;
constexpr bool interp_tiles_wanted(const InterpFacts &f) {
  const uint64_t m = f.n_part < kInterpBatch ? f.n_part : kInterpBatch;
  return f.kernel == kInterpTileKernel && f.n_fields >= kInterpTileMinFields && !f.own_particles &&
         m >= kInterpTileMinPerTile * (uint64_t)f.ntiles;
}

// requested: opts->path.  kInterpNoTiles: path = 1 was asked where the tile kernel cannot run.
constexpr int interp_path(const InterpFacts &f, int requested) {
  if (requested == 0) return kInterpDirect;
  if (requested == 1) return interp_tiles_possible(f) ? kInterpTile : kInterpNoTiles;
  return interp_tiles_possible(f) && interp_tiles_wanted(f) ? kInterpTile : kInterpDirect;
}

}  // namespace bchmc
