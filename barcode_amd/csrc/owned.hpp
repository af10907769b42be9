// owned.hpp -- move-only owners of the HIP and rocFFT resources a handle keeps: empty by default, released by the
// destructor, so a struct of them needs no hand-written teardown (members go in reverse declaration order).  Their
// functions return the API's own status.  Depends on the HIP runtime API, rocFFT and the standard library only:
// tests/host/owned_check.cpp builds it against stand-in runtime functions.
#pragma once

#include <hip/hip_runtime_api.h>
#include <rocfft/rocfft.h>

#include <atomic>
#include <cstdint>
#include <mutex>
#include <type_traits>
#include <utility>

namespace owned {

// What the owners of this process hold right now (bchmc_live_resources); atomic because chains run in threads.
struct Live {
  std::atomic<uint64_t> dev_bufs{0}, dev_bytes{0}, pinned{0}, other{0};  // other: events, streams, plans, infos
};
inline Live live;

// Elements of U in device memory (kDevice) or pinned host memory; U = void counts bytes.  Converts to its raw pointer.
template <typename U, bool kDevice>
class Buf {
  U *p_ = nullptr;
  size_t cap_ = 0;
  void tally(int sign) const {
    if (kDevice) live.dev_bufs += sign, live.dev_bytes += sign * (cap_ * kElem);
    else live.pinned += sign;
  }

 public:
  static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void_v<U>, char, U>);
  Buf() = default;
  Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) {
      (void)release();
      p_ = std::exchange(o.p_, nullptr), cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~Buf() { (void)release(); }
  operator U *() const { return p_; }
  U *get() const { return p_; }
  size_t capacity() const { return cap_; }  // elements

  hipError_t release() {  // empty afterwards, whatever the runtime answers
    if (!p_) return hipSuccess;
    tally(-1);
    cap_ = 0;
    void *p = std::exchange(p_, nullptr);
    return kDevice ? hipFree(p) : hipHostFree(p);
  }
  // Releases what is held, then allocates `count` elements with undefined contents; empty on failure.
  hipError_t alloc(size_t count) {
    (void)release();
    void *p = nullptr;
    const hipError_t e = kDevice ? hipMalloc(&p, count * kElem) : hipHostMalloc(&p, count * kElem, hipHostMallocDefault);
    if (e != hipSuccess || !p) return e;
    p_ = static_cast<U *>(p), cap_ = count;
    tally(+1);
    return hipSuccess;
  }
  // ... zero-filled ON `stream`: a null-stream memset could land after the first kernels that a non-blocking stream
  // runs on the buffer.  Device buffers only.
  hipError_t alloc(size_t count, hipStream_t stream) {
    hipError_t e = alloc(count);
    if (e == hipSuccess && p_) e = hipMemsetAsync(p_, 0, cap_ * kElem, stream);
    if (e != hipSuccess) (void)release();
    return e;
  }
  // The one grow idiom: nothing if `count` fits, else release THEN allocate (the largest buffers do not fit beside
  // their replacement).  Contents are not carried over; empty with capacity 0 on failure.
  hipError_t reserve(size_t count, hipStream_t stream) { return count <= cap_ ? hipSuccess : alloc(count, stream); }
};
template <typename U>
using DevBuf = Buf<U, true>;
template <typename U>
using PinnedBuf = Buf<U, false>;
using DevBytes = DevBuf<void>;

// An opaque API object (event, stream, rocFFT plan or execution info) and the call that destroys it.
template <typename H, auto kDestroy>
class Obj {
  H h_ = nullptr;

 public:
  Obj() = default;
  Obj(Obj &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Obj &operator=(Obj &&o) noexcept {
    if (this != &o) reset(std::exchange(o.h_, nullptr));
    return *this;
  }
  ~Obj() { reset(); }
  operator H() const { return h_; }
  void reset(H fresh = nullptr) {  // destroys what is held and takes over `fresh`
    if (h_) live.other--, (void)kDestroy(h_);
    h_ = fresh;
    if (h_) live.other++;
  }
  template <typename F, typename... A>
  auto create(F make, A... args) {  // make(&object, args...) is the API's create call; empty on failure
    H fresh = nullptr;
    const auto status = make(&fresh, args...);
    reset(status == decltype(status){} ? fresh : nullptr);  // success is 0 in both APIs
    return status;
  }
};
struct Event : Obj<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDefault) { return Obj::create(hipEventCreateWithFlags, flags); }
};
struct Stream : Obj<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) { return Obj::create(hipStreamCreateWithFlags, flags); }
};
using FftPlan = Obj<rocfft_plan, rocfft_plan_destroy>;                      // plan.create(rocfft_plan_create, ...)
using FftInfo = Obj<rocfft_execution_info, rocfft_execution_info_destroy>;  // info.create(rocfft_execution_info_create)

// One user of the process-wide rocfft_setup / rocfft_cleanup pair: the first acquire sets rocFFT up, the last
// destructor cleans it up.  A user counts from acquire on, whatever rocfft_setup answered.
class RocfftUser {
  static inline std::mutex mu_;
  static inline int users_ = 0;
  bool on_ = false;

 public:
  RocfftUser() = default;
  RocfftUser(const RocfftUser &) = delete;
  rocfft_status acquire() {
    std::lock_guard<std::mutex> lk(mu_);
    if (std::exchange(on_, true)) return rocfft_status_success;
    return users_++ == 0 ? rocfft_setup() : rocfft_status_success;
  }
  ~RocfftUser() {
    std::lock_guard<std::mutex> lk(mu_);
    if (on_ && --users_ == 0) (void)rocfft_cleanup();
  }
};

}  // namespace owned
