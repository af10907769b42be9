// owned_check.cpp -- the owners of barcode_amd/csrc/owned.hpp against a stand-in runtime: the few HIP / rocFFT functions
// the header calls are defined here on malloc / free, with a knob that fails the next k allocations or creations.
// Built with -fsanitize=address,undefined and NOT linked against the HIP runtime (tests/test_owned_host.py): a double
// free, a leak or a fill past a buffer's end is AddressSanitizer's / LeakSanitizer's to report, the live counts are
// checked after every step here.
#include "../../barcode_amd/csrc/owned.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

using namespace owned;

namespace {
int g_fail_next = 0;  // the next k allocations / creations fail
int g_mallocs = 0, g_setups = 0, g_cleanups = 0;
hipStream_t g_fill_stream = nullptr;  // the stream of the last hipMemsetAsync

bool fail_now() { return g_fail_next > 0 && g_fail_next-- > 0; }
template <typename H>
hipError_t make_obj(H *out) {  // an opaque object is one heap byte: a missing destroy is a leak
  *out = nullptr;
  if (fail_now()) return hipErrorOutOfMemory;
  *out = reinterpret_cast<H>(std::malloc(1));
  return hipSuccess;
}
rocfft_status fake_plan_create(rocfft_plan *plan, int dims) {
  (void)dims;
  return make_obj(plan) == hipSuccess ? rocfft_status_success : rocfft_status_failure;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t n) {
  *p = nullptr;
  if (fail_now()) return hipErrorOutOfMemory;
  g_mallocs++;
  *p = std::malloc(n);
  return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return hipMalloc(p, n); }
hipError_t hipFree(void *p) {
  std::free(p);
  return hipSuccess;
}
hipError_t hipHostFree(void *p) { return hipFree(p); }
hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t s) {
  std::memset(dst, v, n);
  g_fill_stream = s;
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return make_obj(e); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return make_obj(s); }
hipError_t hipEventDestroy(hipEvent_t e) { return hipFree(e); }
hipError_t hipStreamDestroy(hipStream_t s) { return hipFree(s); }
rocfft_status rocfft_plan_destroy(rocfft_plan p) {
  std::free(p);
  return rocfft_status_success;
}
rocfft_status rocfft_execution_info_destroy(rocfft_execution_info i) {
  std::free(i);
  return rocfft_status_success;
}
rocfft_status rocfft_setup() {
  g_setups++;
  return rocfft_status_success;
}
rocfft_status rocfft_cleanup() {
  g_cleanups++;
  return rocfft_status_success;
}
}

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "owned_check:%d: %s is false\n", __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)
// the four live counts: device buffers, device bytes, pinned buffers, other objects
#define LIVE(bufs, bytes, pins, objs)                                                                          \
  CHECK(live.dev_bufs == (uint64_t)(bufs) && live.dev_bytes == (uint64_t)(bytes) && live.pinned == (uint64_t)(pins) && \
        live.other == (uint64_t)(objs))

int main() {
  hipStream_t raw_stream = nullptr;
  CHECK(hipStreamCreateWithFlags(&raw_stream, 0) == hipSuccess);  // not an owner's: stands for "the given stream"

  {  // empty owners are destroyed without a call into the runtime
    DevBuf<double> a;
    DevBytes b;
    PinnedBuf<int> p;
    Event e;
    Stream s;
    FftPlan plan;
    FftInfo info;
    RocfftUser user;
    CHECK(!a && !b && !p && !e && !s && !plan && !info && a.capacity() == 0);
    CHECK(a.release() == hipSuccess);
  }
  LIVE(0, 0, 0, 0);
  CHECK(g_cleanups == 0);

  {  // alloc: zero-filled on the given stream; byte form; pinned; release; free by the destructor
    DevBuf<double> a;
    CHECK(a.alloc(10, raw_stream) == hipSuccess && a && a.capacity() == 10 && g_fill_stream == raw_stream);
    for (int i = 0; i < 10; i++) CHECK(a[i] == 0.);
    LIVE(1, 80, 0, 0);
    DevBytes b;
    CHECK(b.alloc(100) == hipSuccess && b.capacity() == 100);
    LIVE(2, 180, 0, 0);
    PinnedBuf<int> p;
    CHECK(p.alloc(4) == hipSuccess && p.capacity() == 4);
    p[3] = 7;
    LIVE(2, 180, 1, 0);
    CHECK(b.release() == hipSuccess && !b && b.capacity() == 0);
    LIVE(1, 80, 1, 0);
    CHECK(a.alloc(3, raw_stream) == hipSuccess && a.capacity() == 3);  // alloc on a held buffer releases it first
    LIVE(1, 24, 1, 0);
  }
  LIVE(0, 0, 0, 0);

  {  // reserve: fits, grows, fails (empty, capacity 0, and fails again instead of handing out a null pointer)
    DevBuf<int> g;
    CHECK(g.reserve(8, raw_stream) == hipSuccess && g.capacity() == 8);
    int *const first = g;
    const int before = g_mallocs;
    CHECK(g.reserve(5, raw_stream) == hipSuccess && g == first && g.capacity() == 8 && g_mallocs == before);
    LIVE(1, 32, 0, 0);
    CHECK(g.reserve(20, raw_stream) == hipSuccess && g.capacity() == 20 && g_mallocs == before + 1);
    for (int i = 0; i < 20; i++) CHECK(g[i] == 0);
    LIVE(1, 80, 0, 0);
    g_fail_next = 2;
    CHECK(g.reserve(40, raw_stream) == hipErrorOutOfMemory && g.get() == nullptr && g.capacity() == 0);
    LIVE(0, 0, 0, 0);
    CHECK(g.reserve(1, raw_stream) == hipErrorOutOfMemory && g.get() == nullptr && g.capacity() == 0);
    LIVE(0, 0, 0, 0);
    CHECK(g.reserve(40, raw_stream) == hipSuccess && g.capacity() == 40);
    LIVE(1, 160, 0, 0);
  }
  LIVE(0, 0, 0, 0);

  {  // move construction, move assignment into a held buffer, std::swap (the handle swaps qk / qk2, gk / cg)
    DevBytes a, b;
    CHECK(a.alloc(16, raw_stream) == hipSuccess && b.alloc(32, raw_stream) == hipSuccess);
    void *const pa = a, *const pb = b;
    DevBytes c(std::move(a));
    CHECK(!a && a.capacity() == 0 && c == pa && c.capacity() == 16);
    LIVE(2, 48, 0, 0);
    std::swap(b, c);
    CHECK(b == pa && b.capacity() == 16 && c == pb && c.capacity() == 32);
    LIVE(2, 48, 0, 0);
    b = std::move(c);  // releases the 16 bytes
    CHECK(b == pb && b.capacity() == 32 && !c);
    LIVE(1, 32, 0, 0);
    b = std::move(b);  // self-assignment keeps the buffer
    CHECK(b == pb);
    PinnedBuf<double> p, q;
    CHECK(p.alloc(2) == hipSuccess);
    q = std::move(p);
    CHECK(!p && q.capacity() == 2);
    LIVE(1, 32, 1, 0);
  }
  LIVE(0, 0, 0, 0);

  {  // the rocFFT work buffer grows new-before-old: a failed allocation leaves the old one in place
    DevBytes work;
    CHECK(work.alloc(64) == hipSuccess);
    void *const old = work;
    {
      DevBytes nw;
      g_fail_next = 1;
      CHECK(nw.alloc(128) != hipSuccess && !nw);
      CHECK(work == old && work.capacity() == 64);
      LIVE(1, 64, 0, 0);
    }
    {
      DevBytes nw;
      CHECK(nw.alloc(128) == hipSuccess);
      LIVE(2, 192, 0, 0);  // both alive while the execution info is given the new one
      void *const fresh = nw;
      work = std::move(nw);
      CHECK(work == fresh && work.capacity() == 128);
    }
    LIVE(1, 128, 0, 0);
  }
  LIVE(0, 0, 0, 0);

  {  // realloc_slots: release, then { wanted, previous, minimum }; the first two allocations fail
    DevBytes srec;
    CHECK(srec.alloc(1000) == hipSuccess);
    (void)srec.release();
    LIVE(0, 0, 0, 0);
    g_fail_next = 2;
    size_t got = 0;
    for (size_t cap : {4000, 1000, 0}) {
      if (srec.alloc(std::max<size_t>(100, cap)) == hipSuccess) {
        got = cap + 1;
        break;
      }
      CHECK(!srec && srec.capacity() == 0);
      LIVE(0, 0, 0, 0);
    }
    CHECK(got == 1 && srec.capacity() == 100);
    LIVE(1, 100, 0, 0);
    g_fail_next = 1;  // and a reallocation that finds no memory at all leaves the owner empty
    CHECK(srec.alloc(200) != hipSuccess && !srec);
    LIVE(0, 0, 0, 0);
  }

  {  // events, streams, plans, infos: create, failed create, adopt, move through a pool as the profiling events do
    Event e;
    CHECK(e.create(hipEventDisableTiming) == hipSuccess && e);
    LIVE(0, 0, 0, 1);
    CHECK(e.create() == hipSuccess);  // re-creating destroys the held one
    LIVE(0, 0, 0, 1);
    g_fail_next = 1;
    Event bad;
    CHECK(bad.create() != hipSuccess && !bad);
    Stream s, masked;
    CHECK(s.create(hipStreamNonBlocking) == hipSuccess);
    hipStream_t raw = nullptr;
    CHECK(hipStreamCreateWithFlags(&raw, 0) == hipSuccess);
    masked.reset(raw);  // a stream made elsewhere (hipExtStreamCreateWithCUMask) is handed over
    CHECK(masked == raw);
    LIVE(0, 0, 0, 3);
    FftPlan plan;
    FftInfo info;
    CHECK(plan.create(fake_plan_create, 3) == rocfft_status_success && plan);
    g_fail_next = 1;
    FftPlan none;
    CHECK(none.create(fake_plan_create, 3) == rocfft_status_failure && !none);
    rocfft_execution_info raw_info = nullptr;
    CHECK(make_obj(&raw_info) == hipSuccess);
    info.reset(raw_info);
    LIVE(0, 0, 0, 5);
    plan.reset();
    LIVE(0, 0, 0, 4);
    std::vector<Event> pool;
    pool.push_back(std::move(e));
    CHECK(!e);
    for (int i = 0; i < 5; i++) {
      pool.emplace_back();
      CHECK(pool.back().create() == hipSuccess);
    }
    LIVE(0, 0, 0, 9);
    Event taken = std::move(pool.back());
    pool.pop_back();
    LIVE(0, 0, 0, 9);
  }
  LIVE(0, 0, 0, 0);

  {  // rocfft_setup once for the first user, rocfft_cleanup once after the last; a user that never acquired counts for none
    RocfftUser idle;
    {
      RocfftUser a, b;
      CHECK(a.acquire() == rocfft_status_success && b.acquire() == rocfft_status_success);
      CHECK(a.acquire() == rocfft_status_success && g_setups == 1 && g_cleanups == 0);
    }
    CHECK(g_setups == 1 && g_cleanups == 1);
    RocfftUser c;
    CHECK(c.acquire() == rocfft_status_success && g_setups == 2);
  }
  CHECK(g_cleanups == 2);

  {  // chains run in threads: the counts are atomic
    std::vector<std::thread> th;
    for (int t = 0; t < 4; t++)
      th.emplace_back([] {
        for (int i = 0; i < 2000; i++) {
          DevBytes b;
          PinnedBuf<int> p;
          if (b.alloc(24) != hipSuccess || p.alloc(2) != hipSuccess) std::exit(1);
        }
      });
    for (auto &t : th) t.join();
  }
  LIVE(0, 0, 0, 0);

  CHECK(hipStreamDestroy(raw_stream) == hipSuccess);
  std::puts("owned_check: ok");
  return 0;
}
