// Device self-tests: the shared __device__ helpers of csrc/ run on a caller's data (vggsfm_amd_selftest.h).
#include "vggsfm_amd_selftest.h"
#include "../common.hpp"

namespace vgg {
namespace {

// the aligned group of W lanes around `lane` skips when the bit of its first lane is set
template <int W>
__device__ __forceinline__ bool group_skips(uint64_t word, int lane) { return ((word >> (lane & ~(W - 1))) & 1u) != 0; }

template <int NV>
__global__ __launch_bounds__(256) void crosslane_kernel(const double* __restrict__ in, const uint64_t* __restrict__ skip,
                                                        int bcast_src, const double* __restrict__ scatter_in,
                                                        double* __restrict__ out, double* __restrict__ scatter_out) {
  const size_t n = (size_t)gridDim.x * 256, e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t word = skip ? skip[(size_t)blockIdx.x * 4 + wave] : 0;
  const double v = in[e];
  // (per-group branches: the lanes of a skipping group are inactive while the others sum)
  if (!group_skips<8>(word, lane)) out[VGGS_GROUP_SUM_8 * n + e] = group_sum<8>(v);
  if (!group_skips<16>(word, lane)) out[VGGS_GROUP_SUM_16 * n + e] = group_sum<16>(v);
  if (!group_skips<32>(word, lane)) out[VGGS_GROUP_SUM_32 * n + e] = group_sum<32>(v);
  if (word != 0) return;                           // (wave-uniform: what follows needs all 64 lanes)
  out[VGGS_GROUP_SUM_64 * n + e] = group_sum<64>(v);
  out[VGGS_WAVE_SUM * n + e] = wave_sum(v);
  out[VGGS_WAVE_MAX * n + e] = wave_max(v);
  out[VGGS_WAVE_BCAST * n + e] = wave_bcast(v, bcast_src);
  if (scatter_in) {
    double a[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) a[i] = scatter_in[e * NV + i];
    wave_reduce_scatter<NV, 32>(a, lane, NV, 0, scatter_out + ((size_t)blockIdx.x * 4 + wave) * NV);
  }
}

}  // namespace
}  // namespace vgg

extern "C" {

const char* vggs_build_arch(void) { return "gfx950"; }

int vggs_crosslane(const double* in, const uint64_t* skip, int num_blocks, int bcast_src, const double* scatter_in,
                   int scatter_values, double* out, double* scatter_out, void* stream) {
  using namespace vgg;
  if (num_blocks < 0 || bcast_src < 0 || bcast_src > 63) return VGG_ERR_INVALID_ARGUMENT;
  if (num_blocks == 0) return VGG_OK;
  if (!in || !out || (scatter_in && !scatter_out)) return VGG_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
#define VGGS_LAUNCH(NV) crosslane_kernel<NV><<<num_blocks, 256, 0, st>>>(in, skip, bcast_src, scatter_in, out, scatter_out)
  if (!scatter_in) VGGS_LAUNCH(6);
  else {
    switch (scatter_values) {
      case 6: VGGS_LAUNCH(6); break;
      case 14: VGGS_LAUNCH(14); break;
      case 24: VGGS_LAUNCH(24); break;
      case 28: VGGS_LAUNCH(28); break;
      case 36: VGGS_LAUNCH(36); break;
      case 45: VGGS_LAUNCH(45); break;
      default: return VGG_ERR_INVALID_ARGUMENT;
    }
  }
#undef VGGS_LAUNCH
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
