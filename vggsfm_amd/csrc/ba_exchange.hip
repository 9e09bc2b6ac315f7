// Bundle adjustment, the exchange of the reduced system between the ranks of a sharded solve: packing its lower triangle
// for the collectives, in one piece or in the two parts of the split exchange.  The driver is ba.hip.
#include "ba_types.hpp"

namespace vgg {

// Multi-GPU payload of the reduced system: only the lower triangle is ever filled, so the all-reduce carries
// n(n+1)/2 + n doubles instead of n^2 + n (phases 4 / 5, called by the distributed host loop only).
// mode 0: S, rhs -> packed (+ the zero tail up to W equal slices, + this rank's gradient maximum behind its slice buffer);
// mode 1: packed -> S, rhs;  mode 2: the all-gather output -> S, rhs (slice r of ceil(count / W) elements sits at
// r (ceil(count / W) + 1), followed by rank r's gradient maximum) and the maximum over the ranks -> gmax_pts.
__global__ __launch_bounds__(256) void pack_lower_kernel(Ws w, int n, int mode) {
  if (w.ctl->done) return;
  const int i = blockIdx.x;                                   // row i, or row n = the right-hand side
  const size_t base = (i < n) ? (size_t)i * (i + 1) / 2 : (size_t)n * (n + 1) / 2;
  const int len = (i < n) ? i + 1 : n;
  double* full = (i < n) ? w.S + (size_t)i * n : w.rhs;
  const int W = w.ctl->world > 0 ? w.ctl->world : 1;
  const size_t chunk = (w.packed_count + W - 1) / W;
  if (mode == 0) {
    for (int j = threadIdx.x; j < len; j += 256) w.packed[base + j] = full[j];
    if (i == n) {
      for (size_t j = w.packed_count + threadIdx.x; j < (size_t)W * chunk; j += 256) w.packed[j] = 0.0;
      if (threadIdx.x == 0) w.pk_mine[chunk] = w.gmax_pts[0];
    }
  } else if (mode == 1) {
    for (int j = threadIdx.x; j < len; j += 256) full[j] = w.packed[base + j];
  } else {
    for (int j = threadIdx.x; j < len; j += 256) {
      const size_t e = base + j, r = e / chunk;
      full[j] = w.pk_gathered[r * (chunk + 1) + (e - r * chunk)];
    }
    if (i == n && threadIdx.x < 64) {
      double m = 0.0;
      for (int r = threadIdx.x; r < W; r += 64) m = fmax(m, w.pk_gathered[(size_t)r * (chunk + 1) + chunk]);
      m = wave_max(m);
      if (threadIdx.x == 0) w.gmax_pts[0] = m;
    }
  }
}

// SPLIT exchange of the sharded solve (round 6, phases 7..11): the packed lower triangle is cut into the part the OFF-DIAGONAL
// tile launch fills (A: elements whose row and column belong to cameras of different 16-camera groups) and the rest (B: the
// diagonal tiles' blocks, everything assemble_kernel adds, the shared-intrinsics border, the right-hand side), so that the
// reduce-scatter + all-gather of A can run on the communicator's stream while the diagonal tile launch is still computing B.
// Row r of S contributes up to three column ranges to A and two to B, in this order; a part is packed row by row.
struct RowParts { int a0[3], a1[3], b0[2], b1[2]; };   // fixed slots; a range with x1 <= x0 is empty
__device__ __forceinline__ RowParts row_parts(int r, int n, int C, int KD, int shared) {
  RowParts p;
  p.a0[0] = p.a1[0] = p.a0[1] = p.a1[1] = p.a0[2] = p.a1[2] = p.b0[0] = p.b1[0] = p.b0[1] = p.b1[1] = 0;
  const int P6 = 6 * C, GW = 6 * kGroup;
  if (r >= n) { p.b1[0] = n; }                                // the right-hand side
  else if (r < P6) { const int g = r / GW; p.a1[0] = GW * g; p.b0[0] = GW * g; p.b1[0] = r + 1; }
  else if (shared || KD == 0) { p.b1[0] = r + 1; }            // shared-intrinsics border: assemble_kernel's
  else {                                                      // intrinsics row of camera a (per-camera intrinsics)
    const int a = (r - P6) / KD, g = a / kGroup;
    const int pb0 = GW * g, pb1 = min(GW * (g + 1), P6), ib0 = P6 + kGroup * KD * g;
    p.a1[0] = pb0; p.b0[0] = pb0; p.b1[0] = pb1; p.a0[1] = pb1; p.a1[1] = P6; p.a0[2] = P6; p.a1[2] = ib0; p.b0[1] = ib0; p.b1[1] = r + 1;
  }
  return p;
}
__device__ __forceinline__ int parts_count(const RowParts& p, int part) {
  return part == 0 ? max(p.a1[0] - p.a0[0], 0) + max(p.a1[1] - p.a0[1], 0) + max(p.a1[2] - p.a0[2], 0)
                   : max(p.b1[0] - p.b0[0], 0) + max(p.b1[1] - p.b0[1], 0);
}
// mode 0: S, rhs -> the part's region of `packed` (zero tail up to W equal slices; part B: + this rank's gradient maximum behind
// its slice);  mode 2: the part's all-gather output -> S, rhs (part B: + the maximum over the ranks -> gmax_pts).
// Regions: packed = [A: W chunkA | B: W chunkB], pk_mine = [A: chunkA | B: chunkB + 1], pk_gathered = [A: W chunkA | B: W (chunkB + 1)].
// (the rows' offsets inside their part: one workgroup, once per workspace -- phase 12; the first version had every workgroup of
//  pack_split_kernel sum the rows above its own: 10 M row classifications per launch at n = 3200, 120 us)
__global__ __launch_bounds__(256) void split_offsets_kernel(Ws w, int n, int C, int KD, int shared) {
  __shared__ unsigned long long part_sum[2][256];
  const int per = (n + 1 + 255) / 256, r0 = threadIdx.x * per, r1 = min(r0 + per, n + 1);
  unsigned long long sa = 0, sb = 0;
  for (int r = r0; r < r1; ++r) { const RowParts p = row_parts(r, n, C, KD, shared); sa += parts_count(p, 0); sb += parts_count(p, 1); }
  part_sum[0][threadIdx.x] = sa; part_sum[1][threadIdx.x] = sb;
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long run = 0;
    for (int t = 0; t < 256; ++t) { const unsigned long long v = part_sum[threadIdx.x][t]; part_sum[threadIdx.x][t] = run; run += v; }
    w.split_off[(size_t)threadIdx.x * (n + 2) + n + 1] = run;
  }
  __syncthreads();
  sa = part_sum[0][threadIdx.x]; sb = part_sum[1][threadIdx.x];
  for (int r = r0; r < r1; ++r) {
    const RowParts p = row_parts(r, n, C, KD, shared);
    w.split_off[r] = sa; w.split_off[(size_t)(n + 2) + r] = sb;
    sa += parts_count(p, 0); sb += parts_count(p, 1);
  }
}
__global__ __launch_bounds__(256) void pack_split_kernel(Ws w, int n, int C, int KD, int shared, int part, int mode) {
  if (w.ctl->done) return;
  const int i = blockIdx.x;                                   // row i, or row n = the right-hand side
  const unsigned long long before = w.split_off[(size_t)part * (n + 2) + i], total = w.split_off[(size_t)part * (n + 2) + n + 1];
  const unsigned long long total_a = w.split_off[n + 1];
  const size_t W = w.ctl->world > 0 ? w.ctl->world : 1;
  const size_t chunk_a = (total_a + W - 1) / W, chunk_b = (w.packed_count - total_a + W - 1) / W;
  const size_t chunk = part == 0 ? chunk_a : chunk_b, gstride = chunk + (part == 0 ? 0 : 1);
  double* packed = w.packed + (part == 0 ? 0 : W * chunk_a);
  const double* gathered = w.pk_gathered + (part == 0 ? 0 : W * chunk_a);
  double* full = (i < n) ? w.S + (size_t)i * n : w.rhs;
  const RowParts p = row_parts(i, n, C, KD, shared);
  size_t e = before;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (part == 1 && k == 2) break;
    const int x0 = part == 0 ? p.a0[k] : p.b0[k < 2 ? k : 0], x1 = part == 0 ? p.a1[k] : p.b1[k < 2 ? k : 0];
    if (x1 <= x0) continue;
    if (mode == 0) {
      for (int j = x0 + threadIdx.x; j < x1; j += 256) packed[e + (size_t)(j - x0)] = full[j];
    } else {
      // (slice of the first element once per thread, then by increments: no 64-bit division per element)
      size_t ee = e + threadIdx.x, r = ee / chunk, off = ee - r * chunk;
      for (int j = x0 + threadIdx.x; j < x1; j += 256) {
        full[j] = gathered[r * gstride + off];
        off += 256;
        while (off >= chunk) { off -= chunk; ++r; }
      }
    }
    e += (size_t)(x1 - x0);
  }
  if (i == n) {
    if (mode == 0) {
      for (size_t j = total + threadIdx.x; j < W * chunk; j += 256) packed[j] = 0.0;
      if (part == 1 && threadIdx.x == 0) w.pk_mine[chunk_a + chunk_b] = w.gmax_pts[0];
    } else if (part == 1 && threadIdx.x < 64) {
      double m = 0.0;
      for (size_t r = threadIdx.x; r < W; r += 64) m = fmax(m, gathered[r * gstride + chunk]);
      m = wave_max(m);
      if (threadIdx.x == 0) w.gmax_pts[0] = m;
    }
  }
}
// (host: number of elements of part A -- the same sum)
size_t split_count_a(const Dims& d) {
  size_t c = 0;
  const int P6 = 6 * d.C, GW = 6 * kGroup;
  for (int r = 0; r < d.n_red; ++r) {
    if (r < P6) c += (size_t)GW * (r / GW);
    else if (!(d.shared || d.kd == 0)) {
      const int a = (r - P6) / d.kd, g = a / kGroup;
      const int pb0 = GW * g, pb1 = (GW * (g + 1) < P6) ? GW * (g + 1) : P6;
      c += (size_t)pb0 + (size_t)(P6 - pb1) + (size_t)kGroup * d.kd * g;
    }
  }
  return c;
}

// a workgroup per row of S, one more for the right-hand side
void launch_pack_lower(const Launch& L, int mode) {
  pack_lower_kernel<<<L.d.n_red + 1, 256, 0, L.st>>>(L.w, L.d.n_red, mode);
}
void launch_split_offsets(const Launch& L) {
  split_offsets_kernel<<<1, 256, 0, L.st>>>(L.w, L.d.n_red, L.d.C, L.d.kd, L.d.shared);
}
void launch_pack_split(const Launch& L, int part, int mode) {
  pack_split_kernel<<<L.d.n_red + 1, 256, 0, L.st>>>(L.w, L.d.n_red, L.d.C, L.d.kd, L.d.shared, part, mode);
}

}  // namespace vgg
