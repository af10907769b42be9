// Stand-alone check of barcode_amd/csrc/tile_plan.hpp on the CPU (tests/test_tile_plan_cpu.py builds it with g++ under
// AddressSanitizer / UndefinedBehaviorSanitizer and runs it): the partition a handle gets at creation and what the
// record-slot policy does with a sequence of slot words.  Every expected value is a literal, worked out by hand from
// the rules (see the comments), never by calling the header: a mistake in this arithmetic is a record written past the
// array on the GPU, and this is the proof that comes before any launch.
#include <cstdio>
#include <initializer_list>

#include "../../barcode_amd/csrc/tile_plan.hpp"

using namespace bchmc;

namespace {

long long g_failures = 0, g_checks = 0;

void eq(const char *where, const char *what, long long got, long long want) {
  g_checks++;
  if (got != want && g_failures++ < 40) std::printf("FAIL %s: %s is %lld, expected %lld\n", where, what, got, want);
}
#define EQ(where, expr, want) eq(where, #expr, (long long)(expr), (long long)(want))

constexpr size_t kTotal288 = 288000000000ull;  // the device's memory, for the budget

struct Cfg {
  int n;
  int mk = 3;
  double min1 = 0., h_rel = 1.;
  size_t esz = 8, total = kTotal288;
};

// grid spacing 1250 / 256 (any would do: every rule depends on h / d only)
TilePlan plan(const Cfg &c, const TileSwitches &sw = TileSwitches()) {
  const double d = 1250. / 256.;
  const Hull hull = build_hull(c.h_rel * d, d);
  return plan_tiles(c.n, c.mk, c.min1, 0., 0., c.h_rel * d, d, (long long)c.n * c.n * c.n, c.esz, hull, sw, c.total);
}

TileSwitches with_cap(long long cap, bool fixed = false) {
  TileSwitches sw;
  sw.has_cap = true;
  sw.cap = cap;
  sw.cap_fixed = fixed;
  return sw;
}

void check_shape(const char *w, const TilePlan &p, int tx, int ty, int tz, int ntiles) {
  EQ(w, p.tiled, 1);
  EQ(w, p.tp.tx, tx);
  EQ(w, p.tp.ty, ty);
  EQ(w, p.tp.tz, tz);
  EQ(w, p.tp.ntx * tx, p.tp.nty * ty);  // cubic grid
  EQ(w, p.tp.ntiles, ntiles);
  EQ(w, p.tp.R, 2);
  EQ(w, p.tp.lx, tx + 4);
  EQ(w, p.tp.ly, ty + 4);
  EQ(w, p.tp.lz, tz + 4);
  EQ(w, p.tp.cap, p.slots.cap);
}

// h = d: (|i| - 1/2)^2 is 1/4 for |i| <= 1, 9/4 for |i| = 2, 25/4 for |i| = 3, in units of d^2, against (2h)^2 = 4.
// Columns with both |i|, |j| <= 1: 1/2 + z <= 4 admits |k| <= 2 (9 columns of 5 cells); one of them 2: 5/2 + z <= 4 admits
// |k| <= 1 (12 columns of 3 cells); both 2: 9/2 > 4.  21 columns, 81 cells, as hull81_zw says.  Outside it the nearest
// cells are (2, 2, 0) and (2, 0, 2) at 2 (3/2)^2 = 9/2 > 4 from any point of the home cell: the hull is exact.
void check_hull() {
  const char *w = "hull h = d";
  const Hull hull = build_hull(1., 1.);
  EQ(w, hull.cols.size(), 21);
  EQ(w, hull.reach, 3);
  EQ(w, hull.exact, 1);
  EQ(w, hull.maxlen, 5);
  EQ(w, hull.max_offset(), 2);
  int cells = 0;
  for (const HullCol &c : hull.cols) {
    const int a = c.x < 0 ? -c.x : c.x, b = c.y < 0 ? -c.y : c.y;
    const int zw = (a == 2 && b == 2) ? -1 : ((a == 2 || b == 2) ? 1 : 2);
    EQ(w, a <= 2 && b <= 2, 1);
    EQ(w, c.z, -zw);
    EQ(w, c.w, zw);
    EQ(w, hull81_zw(c.x + 2, c.y + 2), zw);
    cells += c.w - c.z + 1;
  }
  EQ(w, cells, 81);
  EQ(w, hull81_zw(0, 0), -1);
  EQ(w, hull81_zw(4, 0), -1);
  // h = 1.3 d: 2h / d = 2.6, reach 3; (2, 2, 1) lies at 9/4 + 9/4 + 1/4 = 4.75 <= 6.76
  const Hull wide = build_hull(1.3, 1.);
  EQ("hull h = 1.3 d", wide.reach, 3);
  EQ("hull h = 1.3 d", wide.cols.size() > 21, 1);
}

void check_partition() {
  {
    // 8 x 8 x 16 tiles: 4 x 4 x 2 = 32 of them; N = 2^15 < 2^20: chunk 256; mean occupancy 1024: 8x is the default
    // start, 16x the allocation, and without BCHMC_SORT_CAP all of it is in use; 16384 x 32 tiles = 524288 records
    const char *w = "n = 32";
    const TilePlan p = plan({32});
    check_shape(w, p, 8, 8, 16, 32);
    EQ(w, p.hull_n, 21);
    EQ(w, p.reach, 3);
    EQ(w, p.hull_exact, 1);
    EQ(w, p.hull_maxlen, 5);
    EQ(w, p.tp.lx, 12);
    EQ(w, p.tp.ly, 12);
    EQ(w, p.tp.lz, 20);
    EQ(w, p.tp.chunk, 256);
    EQ(w, p.std81, 1);
    EQ(w, p.slots.sort_direct, 1);
    EQ(w, p.slots.cap, 16384);
    EQ(w, p.slots.cap_alloc, 16384);
    EQ(w, p.slots.cap_pinned, 0);
    EQ(w, p.slots.cap_wanted, 0);
    EQ(w, p.slots.slot_watch, 0);
    EQ(w, p.nrec, 524288);
    // a quarter of 288e9 bytes over 32 tiles x 32 bytes per record
    EQ(w, p.slots.cap_budget, 70312500);
  }
  {
    const char *w = "n = 32, cap 64";
    const TilePlan p = plan({32}, with_cap(64));
    check_shape(w, p, 8, 8, 16, 32);
    EQ(w, p.slots.sort_direct, 1);
    EQ(w, p.slots.cap, 64);
    EQ(w, p.slots.cap_alloc, 16384);
    EQ(w, p.slots.slot_watch, 1);
    EQ(w, p.nrec, 524288);
    EQ(w, plan({32}, with_cap(70)).slots.cap, 64);  // whole octant segments only
  }
  {
    const char *w = "n = 32, cap 0";
    const TilePlan p = plan({32}, with_cap(0));
    EQ(w, p.tiled, 1);
    EQ(w, p.std81, 1);
    EQ(w, p.slots.sort_direct, 0);
    EQ(w, p.tp.cap, 0);
    EQ(w, p.nrec, 32768);
    EQ(w, plan({32}, with_cap(1ll << 30)).slots.sort_direct, 0);  // per-tile ranges are 32-bit
  }
  {
    // pinned: the allocation is the partition, 2048 x 32 = 65536 records
    const char *w = "n = 32, cap 2048 fixed";
    const TilePlan p = plan({32}, with_cap(2048, true));
    EQ(w, p.tiled, 1);
    EQ(w, p.slots.sort_direct, 1);
    EQ(w, p.slots.cap, 2048);
    EQ(w, p.tp.cap, 2048);
    EQ(w, p.slots.cap_alloc, 2048);
    EQ(w, p.slots.cap_pinned, 1);
    EQ(w, p.slots.slot_watch, 0);
    EQ(w, p.nrec, 65536);
  }
  {
    // one 4 x 4 x 4 tile (halo 2 <= n), mean occupancy 64: start max(512, 64), allocation max(512, 1024, 128)
    const char *w = "n = 4";
    const TilePlan p = plan({4});
    check_shape(w, p, 4, 4, 4, 1);
    EQ(w, p.std81, 0);
    EQ(w, p.slots.cap, 1024);
    EQ(w, p.slots.cap_alloc, 1024);
    EQ(w, p.nrec, 1024);
    EQ(w, p.tp.chunk, 256);
  }
  {
    const TilePlan p12 = plan({12}), p24 = plan({24});
    check_shape("n = 12", p12, 4, 4, 4, 27);
    EQ("n = 12", p12.std81, 0);
    EQ("n = 12", p12.slots.cap_alloc, 1024);
    check_shape("n = 24", p24, 8, 8, 8, 27);
    EQ("n = 24", p24.std81, 0);
    EQ("n = 24", p24.slots.cap, 8192);  // 16 x 512
    EQ("n = 24", p24.slots.cap_alloc, 8192);
  }
  for (int n : {5, 7, 9}) {
    const TilePlan p = plan({n});
    EQ("odd n", p.tiled, 0);
    EQ("odd n", p.std81, 0);
    EQ("odd n", p.slots.sort_direct, 0);
    EQ("odd n", p.tp.tx, 0);
    EQ("odd n", p.hull_n, 21);  // the hull is there for the direct kernels
  }
  EQ("n = 256", plan({256}).tp.chunk, 2048);  // N = 2^24 >= 2^23
  EQ("n = 256", plan({256}).tp.ntiles, 32 * 32 * 16);
  EQ("n = 256", plan({256}).std81, 1);
  EQ("n = 128", plan({128}).tp.chunk, 1024);  // 2^20 <= N = 2^21 < 2^23
  EQ("n = 1024", plan({1024}).tiled, 0);      // N = 2^30: past the 32-bit indices of the tile path
  {
    TileSwitches sw;
    sw.chunk = 64;
    EQ("chunk 64", plan({32}, sw).tp.chunk, 64);
    sw.chunk = 5000;
    EQ("chunk 5000", plan({32}, sw).tp.chunk, 2048);
    sw.chunk = 1;
    EQ("chunk 1", plan({32}, sw).tp.chunk, 64);
    EQ("chunk 1", plan({32}, sw).std81, 1);
  }
  {
    Cfg low{32};
    low.mk = 1;
    const TilePlan p = plan(low);
    check_shape("mk = 1", p, 8, 8, 16, 32);
    EQ("mk = 1", p.std81, 0);
    EQ("mk = 1", p.slots.cap, 16384);
    TileSwitches sw;
    sw.no_tiles_low = true;
    EQ("mk = 1, no_tiles_low", plan(low, sw).tiled, 0);
    EQ("mk = 3, no_tiles_low", plan({32}, sw).tiled, 1);
    low.min1 = 0.5;
    EQ("mk = 1, min1 = 0.5", plan(low).tiled, 0);
    Cfg sph{32};
    sph.min1 = 0.5;
    EQ("mk = 3, min1 = 0.5", plan(sph).std81, 1);
    TileSwitches off;
    off.no_tiles = true;
    EQ("no_tiles", plan({32}, off).tiled, 0);
    EQ("no_tiles", plan({32}, off).slots.sort_direct, 0);
  }
  {
    // h = 0.86 d: 2h / d = 1.72, reach 2, (2h)^2 = 2.9584: 1/2 + 9/4 and 5/2 + 1/4 fit, 5/2 + 9/4 and 9/2 do not -- the
    // same 21 columns, exact (9/2 > 2.9584), halo 2; only the h >= 0.8661 d rule keeps the unrolled kernels away
    Cfg c{32};
    c.h_rel = 0.86;
    const TilePlan p = plan(c);
    check_shape("h = 0.86 d", p, 8, 8, 16, 32);
    EQ("h = 0.86 d", p.hull_n, 21);
    EQ("h = 0.86 d", p.reach, 2);
    EQ("h = 0.86 d", p.hull_exact, 1);
    EQ("h = 0.86 d", p.std81, 0);
    c.h_rel = 0.87;
    EQ("h = 0.87 d", plan(c).std81, 1);
  }
  {
    // budget = max(cap_alloc, total / 4 / (ntiles x 4 x esz)): n = 32 fp64 divides by 1024, fp32 by 512
    Cfg c{32};
    c.total = 1u << 20;  // 2^18 / 2^10 = 256 < 16384
    EQ("budget, 1 MiB", plan(c).slots.cap_budget, 16384);
    c.total = 1u << 30;  // 2^28 / 2^10
    EQ("budget, 1 GiB", plan(c).slots.cap_budget, 262144);
    c.esz = 4;
    EQ("budget, 1 GiB fp32", plan(c).slots.cap_budget, 524288);
    c.total = kTotal288;
    EQ("budget, 288 GB fp32", plan(c).slots.cap_budget, 140625000);
    EQ("budget, 288 GB, n = 256", plan({256}).slots.cap_budget, 137329);  // 72e9 / (16384 x 32) = 137329.1
  }
}

#define ACT(where, a, k, c, o)        \
  do {                                \
    const SlotAction a_ = (a);        \
    EQ(where, a_.kind, k);            \
    EQ(where, a_.cap, c);             \
    EQ(where, a_.overflowed, o);      \
  } while (0)

void check_policy() {
  const int kNone = SlotAction::kNone, kRepartition = SlotAction::kRepartition, kRealloc = SlotAction::kRealloc;
  const SlotPolicy start = plan({32}, with_cap(64)).slots;  // cap 64 (segments of 8) of 16384, budget 70312500
  SlotPolicy s = start;
  // 1. a segment of 8 overflowed, 100 seen: 1.5 x 100 + 16 -> 168 per segment, 1344 per tile: the allocation holds that
  ACT("seq 1", s.observe(8, 100, true), kRepartition, 16384, 1);
  EQ("seq 1", s.cap, 16384);
  EQ("seq 1", s.slot_watch, 0);
  // 2. segments of 2048, 1700 seen: nothing to extend into
  ACT("seq 2", s.observe(0, 1700, true), kNone, 0, 0);
  EQ("seq 2", s.cap, 16384);
  EQ("seq 2", s.slot_watch, 0);
  // 3. a stamp of 8 predates the partition of 2048
  ACT("seq 3", s.observe(8, 0, true), kNone, 0, 0);
  ACT("seq 3", s.observe(8, 1700, true), kNone, 0, 0);
  EQ("seq 3", s.cap, 16384);
  const SlotPolicy full = s;
  // 4. 2048 overflowed, 3000 seen: (4500 + 23) / 8 * 8 = 4520 per segment, 36160 per tile, + 25 % = 45200
  ACT("seq 4", s.observe(2048, 3000, true), kRealloc, 45200, 1);
  EQ("seq 4", s.cap, 16384);
  EQ("seq 4", s.clamp_to_budget(45200), 45200);
  EQ("seq 4", s.rung(SlotGot::kWanted, 45200), 45200);
  EQ("seq 4", record_count(32768, 45200, 32), 1446400);
  s.after_realloc(SlotGot::kWanted, 45200);
  EQ("seq 4", s.cap, 45200);
  EQ("seq 4", s.cap_alloc, 45200);
  EQ("seq 4", s.cap_wanted, 0);
  EQ("seq 4", s.slot_watch, 0);
  EQ("seq 4", s.sort_direct, 1);
  ACT("seq 4, stale stamp", s.observe(2048, 3000, true), kNone, 0, 0);
  // 5. the same inside a trajectory: remembered, and the next synchronising call reallocates
  s = full;
  ACT("seq 5", s.observe(2048, 3000, false), kNone, 0, 0);
  EQ("seq 5", s.cap, 16384);
  EQ("seq 5", s.cap_alloc, 16384);
  EQ("seq 5", s.cap_wanted, 36160);
  EQ("seq 5", s.pending(), 45200);
  s.after_realloc(SlotGot::kWanted, s.clamp_to_budget(s.pending()));
  EQ("seq 5", s.cap, 45200);
  EQ("seq 5", s.cap_alloc, 45200);
  EQ("seq 5", s.cap_wanted, 0);
  EQ("seq 5", s.pending(), 0);
  EQ("seq 5, nothing pending", full.pending(), 0);
  // 6. the budget: at the allocation the array stays; above it, it is what the array grows to; 2^30 - 8 bounds it
  s = full;
  s.cap_budget = 16384;
  EQ("seq 6", s.clamp_to_budget(45200), 0);
  s.after_realloc(SlotGot::kOldSize, 0);
  EQ("seq 6", s.cap, 16384);
  EQ("seq 6", s.cap_alloc, 16384);
  EQ("seq 6", s.sort_direct, 1);
  s.cap_budget = 20000;
  EQ("seq 6", s.clamp_to_budget(45200), 20000);
  EQ("seq 6", s.clamp_to_budget(18000), 18000);
  EQ("seq 6", s.clamp_to_budget(16384), 0);
  s.cap_budget = 20005;
  EQ("seq 6", s.clamp_to_budget(45200), 20000);
  s.cap_budget = 1ll << 40;
  EQ("seq 6", s.clamp_to_budget(1ll << 30), (1ll << 30) - 8);
  EQ("seq 6", s.clamp_to_budget((1ll << 30) - 1), (1ll << 30) - 1);
  // 7. no memory for 45200: an array of the old size leaves everything as it was, N records only end the one-pass path
  s = full;
  ACT("seq 7", s.observe(2048, 3000, true), kRealloc, 45200, 1);
  EQ("seq 7", s.rung(SlotGot::kOldSize, 45200), 16384);
  s.after_realloc(SlotGot::kOldSize, 45200);
  EQ("seq 7", s.cap, 16384);
  EQ("seq 7", s.cap_alloc, 16384);
  EQ("seq 7", s.cap_wanted, 0);
  EQ("seq 7", s.sort_direct, 1);
  EQ("seq 7", s.rung(SlotGot::kRecordsOnly, 45200), 0);
  EQ("seq 7", record_count(32768, 0, 32), 32768);
  s.after_realloc(SlotGot::kRecordsOnly, 45200);
  EQ("seq 7", s.sort_direct, 0);
  EQ("seq 7", s.cap_alloc, 16384);
  ACT("seq 7, given up", s.observe(2048, 3000, true), kNone, 0, 0);
  // 8. pinned
  s = plan({32}, with_cap(2048, true)).slots;
  ACT("seq 8", s.observe(256, 3000, true), kNone, 0, 0);
  ACT("seq 8", s.observe(0, 250, false), kNone, 0, 0);
  EQ("seq 8", s.cap, 2048);
  EQ("seq 8", s.cap_wanted, 0);
  s = start;
  s.cap_pinned = true;
  ACT("seq 8", s.observe(8, 100, true), kNone, 0, 0);
  EQ("seq 8", s.cap, 64);
  // 9. segments of 1024, 1500 seen without a stamp: above 7/8 (896), so all of the allocation, and no more than that
  const SlotPolicy half = plan({32}, with_cap(8192)).slots;
  EQ("seq 9", half.cap, 8192);
  EQ("seq 9", half.cap_alloc, 16384);
  s = half;
  ACT("seq 9", s.observe(0, 1500, true), kRepartition, 16384, 0);
  EQ("seq 9", s.cap, 16384);
  EQ("seq 9", s.cap_wanted, 0);
  EQ("seq 9", s.slot_watch, 0);
  // 10. 800: above 3/4 (768), not above 7/8
  s = half;
  ACT("seq 10", s.observe(0, 800, false), kNone, 0, 0);
  EQ("seq 10", s.cap, 8192);
  EQ("seq 10", s.slot_watch, 1);
  ACT("seq 10", s.observe(0, 768, false), kNone, 0, 0);
  EQ("seq 10", s.slot_watch, 0);
  ACT("seq 10", s.observe(0, 896, false), kNone, 0, 0);
  EQ("seq 10", s.slot_watch, 1);
  ACT("seq 10", s.observe(0, 897, false), kRepartition, 16384, 0);
  // an overflow without a population figure: (0 + 23) / 8 * 8 = 16 per segment where that is more than now, else double
  // (2 x 2048 per segment, 32768 per tile, + 25 %)
  s = start;
  ACT("stamp only", s.observe(8, 0, false), kRepartition, 16384, 1);
  s = full;
  ACT("stamp only", s.observe(2048, 0, true), kRealloc, 40960, 1);
}

// The invariants, over every population up to 20000, with and without an overflow stamp, at a sync and inside a
// trajectory: the partition is whole segments, never shrinks, never passes the allocation, and an array is never asked
// for beyond 2^30 - 8 slots per tile or the budget.
void sweep() {
  struct Start {
    int n;
    long long cap;
    long long budget;  // 0: the device's
  };
  const Start starts[] = {{32, 64, 0}, {32, 8192, 0}, {32, 16384, 0}, {4, 1024, 0}, {32, 16384, 20005}, {32, 64, 16384}};
  for (const Start &st : starts) {
    SlotPolicy first = plan({st.n}, with_cap(st.cap)).slots;
    if (st.budget) first.cap_budget = st.budget;
    for (int maxc = 1; maxc <= 20000; maxc++)
      for (int stamped = 0; stamped < 2; stamped++)
        for (int sync = 0; sync < 2; sync++) {
          SlotPolicy s = first;
          const long long cap0 = s.cap, alloc0 = s.cap_alloc;
          SlotAction a = s.observe(stamped ? s.cap / kOct : 0, maxc, sync != 0);
          bool ok = true;
          if (a.kind == SlotAction::kRealloc) {
            const long long c = s.clamp_to_budget(a.cap);
            ok = ok && (c == 0 || (c > alloc0 && c <= (1ll << 30) - 8 && c <= a.cap && c <= s.cap_budget));
            ok = ok && sync && stamped;
            s.after_realloc(c ? SlotGot::kWanted : SlotGot::kOldSize, c);
            ok = ok && s.cap_alloc == (c ? c : alloc0);
          } else {
            ok = ok && s.cap_alloc == alloc0 && (a.kind == SlotAction::kNone || a.cap == s.cap);
          }
          ok = ok && s.cap % 8 == 0 && s.cap >= cap0 && s.cap <= s.cap_alloc && s.cap <= (1ll << 30) - 8;
          ok = ok && (s.cap_wanted == 0 || (!sync && stamped && s.cap_wanted > s.cap_alloc && s.cap_wanted % 8 == 0));
          g_checks++;
          if (!ok && g_failures++ < 40)
            std::printf("FAIL sweep: n %d cap %lld budget %lld, population %d, stamped %d, sync %d -> cap %d of %lld\n",
                        st.n, st.cap, st.budget, maxc, stamped, sync, s.cap, s.cap_alloc);
        }
  }
}

}  // namespace

int main() {
  check_hull();
  check_partition();
  check_policy();
  sweep();
  if (g_failures) {
    std::printf("tile_plan_check: %lld failures\n", g_failures);
    return 1;
  }
  std::printf("tile_plan_check: ok (%lld checks)\n", g_checks);
  return 0;
}
