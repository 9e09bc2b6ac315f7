// Shared device/host helpers for the gfx950 (CDNA4, wave64) kernels of the geometry hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "crosslane.hpp"

#define VGG_OK 0
#define VGG_ERR_INVALID_ARGUMENT (-1)
#define VGG_ERR_HIP (-2)
#define VGG_ERR_WORKSPACE (-3)
#define VGG_ERR_UNSUPPORTED (-4)

#define VGG_HIP_CHECK(expr)                                    \
  do {                                                         \
    hipError_t e_ = (expr);                                    \
    if (e_ != hipSuccess) return VGG_ERR_HIP;                  \
  } while (0)

#define VGG_LAUNCH_CHECK()                                     \
  do {                                                         \
    if (hipGetLastError() != hipSuccess) return VGG_ERR_HIP;   \
  } while (0)

namespace vgg {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// (wave_sum, group_sum<W>, wave_max, wave_bcast on doubles: crosslane.hpp)
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// fixed-order reduction of Q quantities over the 256 threads: halving tree (t, t + 128), (t, t + 64), ...
template <int Q>
__device__ inline void block_tree_sum(double (*red)[256], const double* val, double* out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < Q; ++q) red[q][tid] = val[q];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
#pragma unroll
      for (int q = 0; q < Q; ++q) red[q][tid] = red[q][tid] + red[q][tid + st];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) out[q] = red[q][0];
  __syncthreads();
}

template <typename T>
__device__ __forceinline__ double load_f64(const T* p) { return (double)(*p); }

inline int div_up(long a, long b) { return (int)((a + b - 1) / b); }

// Overlap of the factorisation with the computation of the reduced system (ba.hip, ba_tiles.hip <-> chol.hip): contributions to
// columns >= first_col arrive in a second matrix S2 (same n x n layout) from work running on another stream; device flag k
// (set by a kernel behind each tile batch) says that every contribution to columns >= wait_col[k] (ascending) is in place.
// The dataflow factorisation is one launch, so it waits on the device: a tile waits for the last flag its columns need and
// adds S2 when it loads them.
struct CholOverlap {
  const double* S2;
  int first_col;
  int num_waits;
  int wait_col[8];
  const int32_t* dev_flags = nullptr;   // device [num_waits]
};
// by-value kernel argument of the dataflow factorisation
struct DfOverlap {
  const double* S2;
  const int32_t* flags;
  int first_col, num_waits;
  int wait_col[8];
};

}  // namespace vgg
