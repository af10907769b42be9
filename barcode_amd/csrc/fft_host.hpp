// fft_host.hpp -- host-side tables of the engine's own FFT passes (step_boundary_x.hpp, alpt_x.hpp, zpass.hpp): the
// half-complex row stride and the twiddle table.  One definition for the engine (bchmc.hip) and the pass probes
// (fft_probe.hip), so that the probes run the kernels on exactly the layout and the twiddles the engine gives them.
#pragma once
#include <cmath>
#include <cstdlib>
#include <vector>

namespace bchmc {

// Row stride nhp (complex elements) of the half-complex arrays for cells per axis n and a field element of esz bytes:
// n / 2 + 1 padded to whole 128-byte lines for n >= 128 (measured with scripts/fft_layout_bench.hip: batch-3 3-D
// transforms run 15-22 % faster in fp64 and ~30 % faster in fp32 than on contiguous n/2+1 rows; no gain below).
// BCHMC_FFT_PAD=0 / 1 forces the padding off / on at every n (tests run the small parity cases both ways).
inline int fft_row_stride(int n, int esz) {
  const int nh = n / 2 + 1;
  const int per_line = 128 / (2 * esz);
  const char *ev = std::getenv("BCHMC_FFT_PAD");
  const bool pad = ev ? (ev[0] == '1') : (n >= 128);
  return pad ? (nh + per_line - 1) / per_line * per_line : nh;
}

// Twiddles exp(-2 pi i r / n), r < n / 2, interleaved (re, im), from the host's libm in double and rounded once to T.
template <typename T> inline std::vector<T> fft_twiddles(int n) {
  std::vector<T> tw(n);
  for (int r = 0; r < n / 2; r++) {
    const double ang = -2. * M_PI * (double)r / (double)n;
    tw[2 * r] = (T)std::cos(ang);
    tw[2 * r + 1] = (T)std::sin(ang);
  }
  return tw;
}

}  // namespace bchmc
