// Exclusive prefix sums over a workgroup of WAVES wavefronts in thread order: one copy, included by dense.hip,
// fuse/fuse.hip and tsdf/tsdf.hip.  Integer sums, so their order is free and the results are exact.
#pragma once
#include "common.hpp"

namespace vgg {

// a wavefront's share of both scans: the totals of the wavefronts before w, and *total = the sum of all
template <int WAVES>
__device__ __forceinline__ int scan_wave_totals(const int* wave_tot, int w, int* total) {
  int before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < WAVES; ++k) {
    before += k < w ? wave_tot[k] : 0;
    all += wave_tot[k];
  }
  *total = all;
  return before;
}

// exclusive prefix of `flag`; *total = number of set flags.  wave_cnt: WAVES ints of LDS, free for reuse on return only
// after the caller's next barrier; the leading barrier lets a loop call it again with the same array.
template <int WAVES>
__device__ __forceinline__ int block_scan_flag(bool flag, int* wave_cnt, int* total) {
  const unsigned long long b = __ballot(flag);
  const int lane = lane_id(), w = threadIdx.x / kWave;
  const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) wave_cnt[w] = __popcll(b);
  __syncthreads();
  return scan_wave_totals<WAVES>(wave_cnt, w, total) + in_wave;
}

// exclusive prefix of v; *total = the sum.  One barrier: wave_tot must not be in use when the workgroup arrives.
template <int WAVES>
__device__ __forceinline__ int block_scan_int(int v, int* wave_tot, int* total) {
  const int lane = lane_id(), w = threadIdx.x / kWave;
  int x = v;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int y = __shfl_up(x, d, kWave);
    if (lane >= d) x += y;
  }
  if (lane == kWave - 1) wave_tot[w] = x;
  __syncthreads();
  return scan_wave_totals<WAVES>(wave_tot, w, total) + x - v;
}

}  // namespace vgg
