// launch_grid.hpp -- the grid of the engine's grid-stride kernels over n elements (256 threads per workgroup).  One
// definition for the engine (bchmc.hip) and the kernel probes (fft_probe.hip), which thereby launch the element-wise
// k-space kernels on the grid the engine gives them.  Plain C++.
#pragma once

#include <algorithm>

namespace bchmc {

inline int nblk_stride(long long n) { return (int)std::min<long long>((n + 255) / 256, 2048); }

}  // namespace bchmc
