// Cross-lane primitives on doubles for the gfx950 (wave64) kernels, on the VALU: DPP moves inside a row of 16 lanes,
// v_permlane16_swap / v_permlane32_swap across rows.  No LDS instruction: a 64-bit __shfl* is two ds_bpermute_b32 -- LDS-crossbar
// traffic that shares the LDS pipe and the lgkmcnt counter with real LDS reads.
//
// Every sum here is the xor butterfly "for (off = W / 2; off > 0; off >>= 1) v += value of lane (i ^ off)" to the last bit, in
// every lane: the same pairing tree, the same order of steps.  Two facts carry that:
//   * a + b and b + a are the same bits (likewise fmax on numbers: v_max_f64 orders -0 below +0 whichever operand holds it),
//     so the two lanes of a pair hold the same bits after a step, whichever of them is the first operand;
//   * hence after the step with offset h the partial sums have period h over the lanes of a group, and a lane that differs from
//     (i ^ h') in bits >= h holds the bits of lane (i ^ h').  Inside a row, row_ror:h' reads lane (i - h') mod 16, which differs
//     from i ^ h' at most in bits above h' -- so a rotation serves every in-row step of a group of 16 lanes or more.
//
// EXEC.  A DPP move reads nothing from an inactive lane (bound_ctrl: a zero instead) and the swaps exchange nothing with one,
// so every source lane of a step must be active.  All source lanes lie in the caller's aligned group of W lanes:
//   group_sum<8>, group_sum<16>: correct when all W lanes of the calling group are active, whatever the other groups do;
//   group_sum<32>: lanes 0..31 or lanes 32..63 -- all 32 of the calling half must be active (the xor-16 step swaps rows 0 <-> 1
//                  and rows 2 <-> 3 independently);
//   group_sum<64>, wave_sum, wave_max, wave_reduce_scatter_step: all 64 lanes of the wavefront must be active -- call them from
//                  wave-uniform control flow only.
#pragma once
#include <hip/hip_runtime.h>

namespace vgg {

// DPP controls
constexpr int kDppQuadXor1 = 0xB1;               // quad_perm:[1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;               // quad_perm:[2,3,0,1]
constexpr int kDppQuadXor3 = 0x1B;               // quad_perm:[3,2,1,0]
constexpr int kDppRowRor = 0x120;                // + n: row_ror:n (lane i reads lane (i - n) mod 16 of its row)
constexpr int kDppRowHalfMirror = 0x141;         // lane i reads lane i ^ 7

// v moved by one DPP control: both halves of the double, all rows and banks enabled.  (bound_ctrl with a zero `old` leaves the
// move without a tied source; none of the controls used here has an out-of-row source, so the zero never shows.)
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// value of lane (i ^ OFF), OFF = 1, 2, 4 or 8: the exact partner, for values without a period (wave_max's operands keep their
// order with it, the reduce-scatter sends a different value from each lane)
template <int OFF>
__device__ __forceinline__ double row_xor(double v) {
  static_assert(OFF == 1 || OFF == 2 || OFF == 4 || OFF == 8, "in-row xor offset");
  if constexpr (OFF == 8) return dpp_mov<kDppRowRor + 8>(v);                         // (i - 8) mod 16 = i ^ 8
  else if constexpr (OFF == 4) return dpp_mov<kDppQuadXor3>(dpp_mov<kDppRowHalfMirror>(v));   // i ^ 7 ^ 3
  else if constexpr (OFF == 2) return dpp_mov<kDppQuadXor2>(v);
  else return dpp_mov<kDppQuadXor1>(v);
}

// The two sides of a cross-row step.  v_permlane16_swap exchanges the odd rows of its first operand with the even rows of its
// second (rows 0 <-> 1, 2 <-> 3), v_permlane32_swap lanes 32..63 of the first with lanes 0..31 of the second.  With (a, b) in
// and L, U the lower and the upper lane of a pair (i, i ^ OFF):
//   lo = the first operand afterwards:   a_L in lane L, b_L in lane U
//   hi = the second operand afterwards:  a_U in lane L, b_U in lane U
// so with a = b = v both lanes hold (v_L, v_U).
struct LanePair { double lo, hi; };
template <int OFF>
__device__ __forceinline__ LanePair swap_rows(double a, double b) {
  static_assert(OFF == 16 || OFF == 32, "cross-row xor offset");
  const unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
  const unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
  if constexpr (OFF == 16) {
    const auto l = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
    return {__hiloint2double((int)h[0], (int)l[0]), __hiloint2double((int)h[1], (int)l[1])};
  } else {
    const auto l = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    const auto h = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    return {__hiloint2double((int)h[0], (int)l[0]), __hiloint2double((int)h[1], (int)l[1])};
  }
}

// one butterfly step of a sum: v + (value of lane i ^ OFF, or of a lane holding the same bits)
template <int OFF, int W>
__device__ __forceinline__ double sum_step(double v) {
  if constexpr (OFF >= 16) {
    // swap_rows(v, v): lo = the lower lane's v, hi = the upper lane's v, in both lanes -- the pair's sum needs no select
    const LanePair p = swap_rows<OFF>(v, v);
    return p.lo + p.hi;
  } else if constexpr (W >= 16) {
    return v + dpp_mov<kDppRowRor + OFF>(v);     // (a rotation would mix the two groups of 8 of a row)
  } else {
    return v + row_xor<OFF>(v);
  }
}

// sum over the aligned group of W lanes (W = 8, 16, 32, 64) this lane belongs to; every lane of the group gets the total
template <int W>
__device__ __forceinline__ double group_sum(double v) {
  static_assert(W == 8 || W == 16 || W == 32 || W == 64, "lanes per group");
  if constexpr (W >= 64) v = sum_step<32, W>(v);
  if constexpr (W >= 32) v = sum_step<16, W>(v);
  if constexpr (W >= 16) v = sum_step<8, W>(v);
  v = sum_step<4, W>(v);
  v = sum_step<2, W>(v);
  v = sum_step<1, W>(v);
  return v;
}

// full-wave (64 lanes) butterfly reductions; every lane ends with the total.  Wave-uniform call sites only.
__device__ __forceinline__ double wave_sum(double v) { return group_sum<64>(v); }

// (operand order as in the butterfly: fmax(own, partner's) in every lane)
__device__ __forceinline__ double wave_max(double v) {
  const int lane = threadIdx.x & 63;
  LanePair p = swap_rows<32>(v, v);
  v = fmax(v, (lane & 32) ? p.lo : p.hi);
  p = swap_rows<16>(v, v);
  v = fmax(v, (lane & 16) ? p.lo : p.hi);
  v = fmax(v, row_xor<8>(v));
  v = fmax(v, row_xor<4>(v));
  v = fmax(v, row_xor<2>(v));
  v = fmax(v, row_xor<1>(v));
  return v;
}

// value of lane `src` in every lane; src must be wave-uniform (v_readlane: the source lane need not be active)
__device__ __forceinline__ double wave_bcast(double v, int src) {
  const int s = __builtin_amdgcn_readfirstlane(src);
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), s), hi = __builtin_amdgcn_readlane(__double2hiint(v), s);
  return __hiloint2double(hi, lo);
}

// One step of the reduce-scatter butterfly (ba_obs.hpp, wave_reduce_scatter): a lane with bit OFF of its index clear keeps `low`
// and sends `up`, one with the bit set keeps `up` and sends `low`; returns keep + (what lane i ^ OFF sent).  Across rows the
// swap delivers both terms of the pair's sum to both lanes, in the in-row steps the sent value goes through the exact partner.
template <int OFF>
__device__ __forceinline__ double reduce_scatter_step(double low, double up, bool hi) {
  if constexpr (OFF >= 16) {
    // lower lane: low_L + low_U (keeps low, the upper lane sent its low); upper lane: up_L + up_U
    const LanePair p = swap_rows<OFF>(low, up);
    return p.lo + p.hi;
  } else {
    const double send = hi ? low : up, keep = hi ? up : low;
    return keep + row_xor<OFF>(send);
  }
}

// The wave sums of NV values per lane as a reduce-scatter butterfly: the same xor steps in the same order as wave_sum, but at
// each step a lane keeps one half of its values -- the low half where the step's lane bit is clear, the high half where it is
// set -- and sends the other half, so a step adds ceil(N / 2) values instead of N: 23 + 12 + 6 + 3 + 2 + 1 additions for 45
// values instead of 45 x 6.  The pairing tree of every value is wave_sum's (the keeper adds its partner's partial sum to its
// own, and a + b = b + a), so the sums are wave_sum's to the last bit; value i ends in ONE lane instead of in all.
// N: values this lane holds (capacity; the last may be padding where an odd count was halved), n: how many of them are real,
// base: index of v[0] among the NV values.  Start with <NV, 32>(v, lane, NV, 0, dst); all 64 lanes active.
template <int N, int OFF>
__device__ __forceinline__ void wave_reduce_scatter(double* v, int lane, int n, int base, double* dst) {
  if constexpr (OFF == 0) {
    static_assert(N == 1, "64 lanes hold at most 64 values");
    if (n > 0) dst[base] = v[0];
  } else {
    constexpr int H = (N + 1) / 2;
    const bool hi = (lane & OFF) != 0;
    double k[H];
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const double up = (H + i < N) ? v[H + i] : 0.0;
      k[i] = reduce_scatter_step<OFF>(v[i], up, hi);
    }
    wave_reduce_scatter<H, OFF / 2>(k, lane, hi ? max(n - H, 0) : min(n, H), base + (hi ? H : 0), dst);
  }
}

}  // namespace vgg
