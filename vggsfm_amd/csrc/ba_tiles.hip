// Bundle adjustment, the reduced camera system: the Schur tile launches, the ordered sums of their chunks and the assembly
// (tile_reduce_kernel, assemble_kernel, or tile_assemble_kernel for all of it at once), and prep_kernel, whose body
// tile_assemble_kernel runs as well.  The driver is ba.hip.
#include "ba_obs.hpp"

namespace vgg {

#ifndef VGG_OFFDIAG_OCC
#define VGG_OFFDIAG_OCC 3   // wavefronts per SIMD of the off-diagonal Schur kernel (BD = 6): see DESIGN.md section 6
#endif
#ifndef VGG_DIAG_OCC
#define VGG_DIAG_OCC 4      // wavefronts per SIMD of the diagonal Schur kernel (BD = 6)
#endif
#ifndef VGG_DIAG_FULL_DEPTH
#define VGG_DIAG_FULL_DEPTH 2   // staging register sets of the full-factor diagonal tile launch
#endif
#ifndef VGG_OFF_FULL_DEPTH
#define VGG_OFF_FULL_DEPTH 2    // ... of the full-factor off-diagonal one
#endif
#ifndef VGG_TRF_ABLATE
#define VGG_TRF_ABLATE 0      // profiling builds, bits: 1 = no row products, 2 = no z loads, 4 = no store of the sums
#endif
#ifndef VGG_ABLATE
#define VGG_ABLATE 0
#endif

// ---------------------------------------------------------------------------------------------
// Block-sparse Schur complement on the matrix cores.
// Tile (gI,gJ) of the reduced system is the R x R matrix (R = 16 cameras x BD rows)
//     C = sum over entries  YA_e (R x 3) * YB_e^T (3 x R),
// where YA_e / YB_e are the two *segments* of the entry: the per-observation factors
// Y_i = s_c o ((F_i^T E_i) G_p) of one point inside one camera group, stored by point_pass at the slot of
// their camera in a zero-padded block of 16 slots (cameras of the group that do not see the point stay
// zero for the whole solve).  A segment is therefore one contiguous, 16-byte aligned run of 16*BD*3 doubles:
// staging is a pure linear copy global -> LDS (dwordx4, coalesced, no masks, no index arithmetic), double
// buffered against the MFMAs.  Four entries are packed along K (4 x 3 = 12 = three K=4 steps of
// v_mfma_f64_16x16x4_f64).  The 4 wavefronts form a 2x2 grid over the NT x NT sub-tiles, each keeps up to
// NH x NH accumulators in registers for the whole chunk; all MFMAs are unconditional (scalar loop bounds).
typedef double f64x4_t __attribute__((ext_vector_type(4)));

#ifndef VGG_TILE_TRACE
#define VGG_TILE_TRACE 0             // debug builds: per-wavefront phase cycle sums of the off-diagonal schur_tile launch
#endif
#if VGG_TILE_TRACE
__device__ long long g_tile_trace[2048 * 4 * 8];   // [workgroup][wave][batches, fetch+issue, matrix phase, LDS write phase, barrier wait, total]
#endif
#ifndef VGG_NO_SKIP
#define VGG_NO_SKIP 0               // profiling builds: 1 = every sub-tile of every batch runs (no presence skipping)
#endif
// bits of a segment's 16-slot presence mask whose cameras have rows in the 16-row block `blk` of a tile with BD rows per
// camera (0 for a block past the last one)
template <int BD>
__device__ __forceinline__ uint32_t block_slot_bits(int blk) {
  if (blk * 16 >= kGroup * BD) return 0u;
  const int s0 = (16 * blk) / BD, s1 = min(kGroup - 1, (16 * blk + 15) / BD);
  return ((2u << s1) - 1u) & ~((1u << s0) - 1u);
}

template <int BD, bool DIAG>
__device__ __forceinline__ void schur_tile_body(const Ws& w, const int32_t* __restrict__ chunk_desc,
                                                const int32_t* __restrict__ entries, int chunk, int zero_seg,
                                                double* __restrict__ ops) {
  constexpr int YS = BD * 3;                      // doubles per Y block
  constexpr int SEG = kGroup * YS;                // doubles per segment (16 slots)
  constexpr int R = kGroup * BD;                  // rows / cols of the tile
  constexpr int NT = R / 16;                      // 16x16 sub-tiles per side
  constexpr int NH = (NT + 1) / 2;                // sub-tile rows (cols) of one wavefront
  // [buffer][side][entry of the batch][component c][tile row]: a staged segment is a linear copy of the global
  // one, except that the tile rows of the odd entries are XOR-swizzled by 16 (double2 index ^ 8) when the entry
  // stride is a multiple of 256 bytes.  K step ks of the MFMAs takes component c = ks of the four entries
  // (lane group lk = entry), so the four 128-byte runs one operand fetch touches fall two and two into the
  // two halves of the LDS banks (conflict-free ds_read_b64).
  constexpr int SWZ = ((SEG * 8) % 256 == 0) ? 16 : 0;
  constexpr int SIDES = DIAG ? 1 : 2;             // LDS image: ops[buffer][side][entry of the batch][SEG]
  // BD = 6: the global segments are COMPRESSED (kYc = 12 doubles per slot: N row-major, 2 a; y_slot_doubles) and the six
  // rows of a slot -- [2 a]x N on top of N -- are rebuilt on the way into LDS.  The LDS image and everything behind it are
  // those of the full factors (without the Jacobi scales: tile_reduce_kernel applies them).
  constexpr bool CY = (BD == 6);
  constexpr int CSEG = kGroup * kYc;              // doubles per compressed segment
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: MFMAs only behind scalar control flow
  // chunk = the j-th of the J workgroups of tile (gI,gJ).  The tile's entry list [e0,e1) is sorted by point;
  // workgroup j takes the sub-chunks j, j+J, j+2J, ... of kSub entries, so all workgroups of all tiles sweep
  // the point range at the same relative rate and the (up to ~G) re-reads of one point's segments by
  // different tiles fall close together in time (they hit the L2 / Infinity Cache instead of HBM).
  const int e0 = chunk_desc[6 * chunk + 2], e1 = chunk_desc[6 * chunk + 3];
  const int cj = chunk_desc[6 * chunk + 4], cJ = chunk_desc[6 * chunk + 5];
  constexpr int BPS = kSub / 4;                   // batches of 4 entries per sub-chunk
  const int nsub = (e1 - e0 + kSub - 1) / kSub;
  const int nb = ((nsub - cj + cJ - 1) / cJ) * BPS;                          // batches of this workgroup
  auto ebase = [&](int b) -> int { return e0 + ((b / BPS) * cJ + cj) * kSub + (b % BPS) * 4; };
  f64x4_t acc[NH][NH];
#pragma unroll
  for (int i = 0; i < NH; ++i)
#pragma unroll
    for (int j = 0; j < NH; ++j) acc[i][j] = (f64x4_t){0.0, 0.0, 0.0, 0.0};

  // Staging of a batch = linear copy of its 8 (diagonal tile: 4) segments, 32 (64) threads per segment.  It is split so that
  // no wavefront ever waits on a dependent global load: the segment index of batch n+2 is loaded while
  // the segment data of batch n+1 is in flight, and that data is written to LDS only after the MFMAs of
  // batch n (async-stage split).
  // Compressed: a PAIR of lanes per slot, three double2 each (the even lane rows 0, 1 of N, the odd lane row 2 and 2 a);
  // the halves are exchanged with one DPP quad permute per register, the even lane then writes the rows 3..5 of the slot
  // (N itself), the odd lane the rows 0..2 (the cross products).  A diagonal tile stages 4 segments: waves 2, 3 idle here.
  constexpr int V = SEG / 2;                      // double2 per segment (full factors)
  constexpr int TPS = CY ? 32 : (DIAG ? 64 : 32); // threads per segment
  constexpr int NV = CY ? 3 : (V + TPS - 1) / TPS; // double2 per thread per batch
  const int sseg = tid / TPS, l32 = tid % TPS;
  const int se = DIAG ? (sseg & 3) : (sseg >> 1), sside = DIAG ? 0 : (sseg & 1);
  // tile_rhs (compressed diagonal tiles): every observation sits in exactly one segment and every segment is exactly one
  // diagonal entry, so  sum over the entries of a diagonal tile of  Y_seg (96 x 3) Z_p (3 x 3)  is, per camera, what
  // cam_pass<RHS> summed per observation: F^T E hs (column 0: Z = [z | y_0 | y_1], E hs = E G z) and F^T E Ms_m (columns
  // 1, 2) -- from operands that are in LDS anyway.  The wavefronts 2, 3 have no segment to stage here (four segments, 32
  // lanes each): they are the HELPERS -- they fetch the Z of the batch's four points through the same two-stage prefetch
  // (entry -> point index, point index -> Z: field 0 of an entry is the point) into a 96-double LDS image per buffer and,
  // while the other two wavefronts write the next batch's segments to LDS, add the products of their row (a lane per tile
  // row) for the four entries of the batch that has just been multiplied.  The two roles are two instantiations of the loop
  // (`run` below): the stagers carry the staging registers, the helpers the three sums, both within the 128 registers of four
  // wavefronts per SIMD.  Scales and constant-parameter masks are applied by assemble_kernel, like tile_reduce_kernel does
  // for the tile sums.
  constexpr bool TR = CY && DIAG;
  constexpr bool INTERLEAVE = !CY;   // full-factor tiles: LDS writes of the next batch between the K steps of the current one
  const bool trhs = TR && w.tile_rhs != 0;
  // tile_rhs with FULL factors (7 x 7 / 8 x 8 blocks: per-camera intrinsics, round 6).  All four wavefronts stage here, so
  // there are no helpers: once a batch is in LDS, thread t adds the products of tile row t % R for two of the batch's four
  // entries (t / R picks the pair) -- six LDS reads and six multiply-adds per batch beside 48 matrix instructions per wavefront.
  // Only z is needed (column 0 of Z: without a shared camera the intrinsics border has no per-point terms), and the factors
  // carry their Jacobi scales and constant-parameter masks: the sums go into the right-hand side as they are.  The 12
  // doubles of a batch's four z come in through threads 0..11 with the staging's own two-stage prefetch.
  constexpr bool TRF = !CY && DIAG;
  const bool trf = TRF && w.tile_rhs != 0;
  constexpr int ZS = 12;                              // doubles per entry of the Z image (9 used; 16-byte aligned rows)
  double* zs = ops + 2 * (DIAG ? 1 : 2) * 4 * SEG;    // [buffer][entry][col][k]
  auto run = [&](auto role) __attribute__((always_inline)) {
  constexpr bool HELPER = decltype(role)::value;      // (only with TR: wavefronts 2, 3)
  const bool zthread = HELPER && trhs && l32 < 9;
  double racc[3] = {0.0, 0.0, 0.0};
  // The segment index of a batch is loaded unconditionally (clamped entry) and only CONSUMED one iteration later;
  // entries past the end of the list are redirected to the all-zero segment behind the last real one.  Nothing in
  // the current iteration depends on the loaded value, so no s_waitcnt sits between the prefetch and the MFMAs.
  const int32_t* seg_field = entries + (HELPER ? 0 : 1 + sside);   // entries[e] = (point, segA, segB, masks)
  auto load_seg_index = [&](int eb) -> int { return seg_field[4 * (size_t)min(eb + se, e1 - 1)]; };
  auto seg_valid = [&](int eb) -> bool { return eb + se < e1; };
  // two staging register sets: the loads of batch b + 2 are issued while batch b is multiplied and batch b + 1 (loaded an
  // iteration earlier) is written to LDS -- twice the bytes in flight per workgroup for NV more double2 registers
  constexpr int DEPTH = (CY && !DIAG) ? 3 : ((!CY && DIAG) ? VGG_DIAG_FULL_DEPTH : ((!CY && !DIAG) ? VGG_OFF_FULL_DEPTH : 2));   // staging register sets = batches in flight ahead of the one being multiplied
  double2 sv[DEPTH][NV];
  // (full-factor tile_rhs) lane l of EVERY wavefront requests component l & 3 of z of entry (l >> 2) & 3 (16 distinct addresses
  //  per wavefront, four of them padding), unconditionally and without a validity select: an entry past the end of the list
  //  multiplies the all-zero segment, so any finite z will do there (the clamped last entry's).  The first formulation had
  //  the twelve lanes of wavefront 0 do it inside `if (tid < 12)`: the loop-carried point index then went through a copy at
  //  the join of that divergent region, which the compiler guards with s_waitcnt vmcnt(0) right behind the load -- wavefront 0
  //  waited for every load in flight, every batch (rocprofv3, one configs[3] shard: diagonal launch 293 -> 345 us from the z
  //  loads alone).  Threads 0..15 (minus the padding lanes) write the image to LDS.
  constexpr bool ZLOAD = TRF && !(VGG_TRF_ABLATE & 2);
  const int zte = (lane >> 2) & 3, ztc = lane & 3;
  const bool zt = ZLOAD && trf && tid < 16 && ztc < 3;
  auto z_point = [&](int eb) -> int { return entries[4 * (size_t)min(eb + zte, e1 - 1)]; };
  double zv[DEPTH];
  int zpt_next = 0;
  double rfull = 0.0;
  // compressed staging: the lane's two LDS targets inside a staged segment (see write_lds)
  const bool cy_top = (l32 & 1) != 0;
  const int cy_sw = (se & 1) * SWZ, cy_r0 = 6 * (l32 >> 1);
  const int cy_row16 = (cy_top ? cy_r0 : cy_r0 + 4) ^ cy_sw, cy_row8 = (cy_top ? cy_r0 + 2 : cy_r0 + 3) ^ cy_sw;
  auto issue_loads = [&](double2 (&sv)[NV], int seg_index, bool valid) __attribute__((always_inline)) {
    if constexpr (CY) {
      if constexpr (!HELPER) {
        // (no `if (stager)` here, and no `if (zthread)` / validity select around the helpers' load below: a load inside a
        //  conditional region is one the compiler cannot count on, so every s_waitcnt vmcnt(n) behind it is computed as if
        //  it had not been issued -- the stagers' wait for the batch loaded a step earlier came out as vmcnt(1) with four
        //  younger loads in flight, i.e. it waited for most of THIS step's loads, every step.  The non-helper loop only
        //  runs on staging wavefronts; a helper lane >= 9 fetches a ninth Z component nobody reads; an entry past the end
        //  of the list multiplies the all-zero segment, so the clamped entry's finite Z does no harm.)
        const double2* src = reinterpret_cast<const double2*>(w.Y) + (size_t)(valid ? seg_index : zero_seg) * (CSEG / 2) + 3 * l32;
#pragma unroll
        for (int i = 0; i < NV; ++i) sv[i] = src[i];
      } else {
        sv[0].x = w.Zp[9 * (size_t)seg_index + min(l32, 8)];   // (seg_index = the entry's point here)
      }
    } else {
      const double2* src = reinterpret_cast<const double2*>(w.Y) + (size_t)(valid ? seg_index : zero_seg) * V;
#pragma unroll
      for (int i = 0; i < NV; ++i) { const int off = l32 + TPS * i; sv[i] = (off < V) ? src[off] : make_double2(0.0, 0.0); }
    }
  };
  // (third k of 3 of a batch's LDS image: one component of the compressed factors, a third of the double2 of the full ones)
  auto write_lds_k = [&](const double2 (&sv)[NV], int buf, const int k) __attribute__((always_inline)) {
    if constexpr (CY && HELPER) {
      if (k == 0 && zthread) zs[(buf * 4 + se) * ZS + l32] = sv[0].x;
    } else if constexpr (CY) {
      {
        // odd lane:  mine = (N20 N21 N22, 2a0 2a1 2a2), other = (N00 N01 N02, N10 N11 N12) -> rows 0..2 = (2 a) x N[:, k]:
        //            16 bytes at row 0, 8 at row 2
        // even lane: mine = (N00 N01 N02, N10 N11 N12), other = (N20 N21 N22, ...)         -> rows 3..5 = N[:, k]:
        //            8 bytes at row 3, 16 at row 4
        // (the odd entries' tile rows are XOR-swizzled by 16; k R is a multiple of 32, so the swizzle acts on the row alone
        //  and the component enters the LDS address as an immediate offset)
        double* dst = ops + (size_t)((buf * SIDES + sside) * 4 + se) * SEG;
        const double m[6] = {sv[0].x, sv[0].y, sv[1].x, sv[1].y, sv[2].x, sv[2].y};
#if VGG_ABLATE == 4                               // (profiling build: the staging without its exchange / arithmetic)
        *reinterpret_cast<double2*>(dst + k * R + cy_row16) = make_double2(m[3 + k], m[k]);
        dst[k * R + cy_row8] = m[k];
#else
        const double ok = row_xor<1>(m[k]), o3k = row_xor<1>(m[3 + k]);   // the other half, one component at a time
        const double t0 = m[4] * m[k] - m[5] * o3k, t1 = m[5] * ok - m[3] * m[k], t2 = m[3] * o3k - m[4] * ok;
        *reinterpret_cast<double2*>(dst + k * R + cy_row16) = cy_top ? make_double2(t0, t1) : make_double2(m[3 + k], ok);
        dst[k * R + cy_row8] = cy_top ? t2 : m[k];
#endif
      }
    } else {
      double2* dst = reinterpret_cast<double2*>(ops + (size_t)((buf * SIDES + sside) * 4 + se) * SEG);
      constexpr int PER3 = (NV + 2) / 3;
#pragma unroll
      for (int i = k * PER3; i < (k + 1) * PER3 && i < NV; ++i) {
        const int off = l32 + TPS * i;
        if (off < V) dst[off ^ ((se & 1) * (SWZ / 2))] = sv[i];
      }
    }
  };
  auto write_lds = [&](const double2 (&sv)[NV], int buf) __attribute__((always_inline)) {
    write_lds_k(sv, buf, 0); write_lds_k(sv, buf, 1); write_lds_k(sv, buf, 2);
  };
  // operand addressing: entry e = lane >> 4 of the batch, component c = ks, tile row rr = 16 rb + (lane & 15)
  const int li = lane & 15, lk = lane >> 4;
  // (ks enters the address as a compile-time immediate: ks R doubles)
  const int kbase = lk * SEG, swz = (lk & 1) * SWZ;

  // presence of a batch (quad): field 3 of its first entry, wave-uniform (scalar load), fetched one batch ahead
  auto load_quad_mask = [&](int eb) -> uint32_t { return (uint32_t)entries[4 * (size_t)min(eb, e1 - 1) + 3]; };
  // DEPTH staging register sets (batch n lives in set n % DEPTH): the loads of batch b + DEPTH are issued while batch b is
  // multiplied and batch b + 1, requested DEPTH - 1 steps earlier, is written to LDS (round 3, off-diagonal launch with
  // compressed segments: with two sets the LDS write phase spent most of its ~1000 cycles per batch waiting for loads
  // issued one step -- ~2 us -- before; the other variants have no registers to spare for a third set)
#pragma unroll
  for (int u = 0; u < DEPTH; ++u) issue_loads(sv[u], load_seg_index(ebase(u)), seg_valid(ebase(u)));
  int seg_next = load_seg_index(ebase(DEPTH));
  bool valid_next = seg_valid(ebase(DEPTH));
  if constexpr (ZLOAD) {
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) zv[u] = w.Zp[9 * (size_t)z_point(ebase(u)) + ztc];
    zpt_next = z_point(ebase(DEPTH));
    if (zt) zs[(0 * 4 + zte) * ZS + ztc] = zv[0];
  }
  uint32_t qmask = load_quad_mask(ebase(0)), qmask_next = load_quad_mask(ebase(1));
  write_lds(sv[0], 0);
  __syncthreads();
  // software pipeline shared by the two sub-tile assignments below
  auto sweep = [&](auto&& mfma_batch) __attribute__((always_inline)) {
#if VGG_TILE_TRACE
    long long tr_issue = 0, tr_mfma = 0, tr_write = 0, tr_bar = 0;
    const long long tr_begin = __builtin_amdgcn_s_memtime(), tr_wall = (long long)wall_clock64();
#define VGG_TT(var) { const long long now_ = __builtin_amdgcn_s_memtime(); var += now_ - tr_last; tr_last = now_; }
#else
#define VGG_TT(var)
#endif
    auto step = [&](int b, int buf, double2 (&sv_load)[NV], const double2 (&sv_write)[NV], double& zv_load, const double& zv_write) __attribute__((always_inline)) {
#if VGG_TILE_TRACE
      long long tr_last = __builtin_amdgcn_s_memtime();
#endif
#if VGG_ABLATE != 2                               // (profiling builds only: 1 = no MFMA, 2 = no global loads)
      // (the index of batch b+DEPTH+1 is requested BEFORE the data of batch b+DEPTH: waiting for it next time round then
      //  leaves the younger data loads in flight -- vmcnt(3), not vmcnt(0))
      const int seg_after = load_seg_index(ebase(b + DEPTH + 1));
      // (full-factor tile_rhs: the point index and the z are requested IN FRONT of the segment data, like the segment index)
      if constexpr (ZLOAD) {
        const int zpt_after = z_point(ebase(b + DEPTH + 1));
        zv_load = w.Zp[9 * (size_t)zpt_next + ztc];
        zpt_next = zpt_after;
      }
      issue_loads(sv_load, seg_next, valid_next); // batch b+DEPTH (the zero segment past the end of the tile's list)
      seg_next = seg_after;
      valid_next = seg_valid(ebase(b + DEPTH + 1));
#endif
      VGG_TT(tr_issue)
#if VGG_ABLATE != 1
      // wave priority raised outside the matrix phase (staging, LDS writes, barrier): a wavefront gets back to its matrix
      // instructions sooner (round 3: off-diagonal launch 0.620 -> 0.606 ms)
      __builtin_amdgcn_s_setprio(0);
      auto rhs_rows = [&](int buf) __attribute__((always_inline)) {
        if (trf && tid < 2 * R && !(VGG_TRF_ABLATE & 1)) {
          const int rrow = tid % R, half = tid / R;
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const int e = 2 * half + q;
            const double* zz = zs + (buf * 4 + e) * ZS;
            const double* op = ops + (size_t)(buf * 4 + e) * SEG + (rrow ^ ((e & 1) * SWZ));
            rfull += op[0] * zz[0] + op[R] * zz[1] + op[2 * R] * zz[2];
          }
        }
      };
      // INTERLEAVE (full factors, 7 x 7 / 8 x 8 blocks): the LDS image of batch b + 1 is written in three pieces BETWEEN
      // the K steps of batch b instead of in a phase of its own behind the last matrix instruction -- the ds_writes issue
      // while the matrix pipe works.  Same-box A/B (round 4): configs[3] whole, off-diagonal launch 13.66 -> 13.18 ms,
      // iteration 21.1 -> 20.6; with the compressed 6 x 6 factors (whose write phase is arithmetic: exchanges and cross
      // products on the pipe the matrix instructions use) nothing for the off-diagonal launch and +6 % for the diagonal one
      mfma_batch(buf, qmask, [&](const int k) __attribute__((always_inline)) {
#if VGG_ABLATE != 5
        if constexpr (INTERLEAVE) write_lds_k(sv_write, buf ^ 1, k);
        if constexpr (INTERLEAVE && TRF) { if (k == 0 && zt) zs[((buf ^ 1) * 4 + zte) * ZS + ztc] = zv_write; }
#endif
        // (full-factor tile_rhs: the row's products are read and added BETWEEN K steps 1 and 2, under the matrix instructions
        //  of the batch -- behind the last one they were a tail of twelve exposed LDS reads per wavefront in front of the barrier)
        if constexpr (TRF) { if (k == 1) rhs_rows(buf); }
      });
      if constexpr (TR && HELPER) {
        if (trhs) {
          const int rrow = tid & 127;                 // (wavefront 2: tile rows 0..63, wavefront 3: 64..95)
          if (rrow < R) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const double* zz = zs + (buf * 4 + e) * ZS;
              const double2* z2 = reinterpret_cast<const double2*>(zz);
              const double2 za = z2[0], zb = z2[1], zc = z2[2], zd = z2[3];   // z0 z1 | z2 y00 | y01 y02 | y10 y11
              const double ze = zz[8];                                          // y12
              const double* op = ops + (size_t)(buf * 4 + e) * SEG + (rrow ^ ((e & 1) * SWZ));
              const double v0 = op[0], v1 = op[R], v2 = op[2 * R];
              racc[0] += v0 * za.x + v1 * za.y + v2 * zb.x;
              racc[1] += v0 * zb.y + v1 * zc.x + v2 * zc.y;
              racc[2] += v0 * zd.x + v1 * zd.y + v2 * ze;
            }
          }
        }
      }
      __builtin_amdgcn_s_setprio(3);
#endif
      VGG_TT(tr_mfma)
      qmask = qmask_next;
      qmask_next = load_quad_mask(ebase(b + 2));
#if VGG_ABLATE != 5                               // (profiling build: 5 = no LDS writes)
      if constexpr (!INTERLEAVE) write_lds(sv_write, buf ^ 1);   // batch b+1, in flight for two steps
      if constexpr (!INTERLEAVE && TRF) { if (zt) zs[((buf ^ 1) * 4 + zte) * ZS + ztc] = zv_write; }
#endif
      VGG_TT(tr_write)
#if VGG_ABLATE != 3
      __syncthreads();
#endif
      VGG_TT(tr_bar)
    };
    // (2 DEPTH steps per trip: the LDS buffers alternate, the register sets rotate)
    constexpr int TRIP = 2 * DEPTH;
    int b = 0;
    for (; b + TRIP - 1 < nb; b += TRIP) {
#pragma unroll
      for (int u = 0; u < TRIP; ++u) step(b + u, u & 1, sv[u % DEPTH], sv[(u + 1) % DEPTH], zv[u % DEPTH], zv[(u + 1) % DEPTH]);
    }
#pragma unroll
    for (int u = 0; u < TRIP - 1; ++u)
      if (b + u < nb) step(b + u, u & 1, sv[u % DEPTH], sv[(u + 1) % DEPTH], zv[u % DEPTH], zv[(u + 1) % DEPTH]);
#if VGG_TILE_TRACE
    if (!DIAG && lane == 0 && blockIdx.x < 2048) {
      long long* t = g_tile_trace + ((size_t)blockIdx.x * 4 + wave) * 8;
      t[0] = nb; t[1] = tr_issue; t[2] = tr_mfma; t[3] = tr_write; t[4] = tr_bar; t[5] = __builtin_amdgcn_s_memtime() - tr_begin;
      t[6] = (long long)wall_clock64() - tr_wall;
    }
#endif
  };
  // partial tile of this chunk, row-major R x R (f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 reg);
  // tile_reduce_kernel sums the chunks of a tile in a fixed order (deterministic, no atomics)
  double* part = w.tile_part + (size_t)chunk * R * R;
  auto store_subtile = [&](int rb, int cb, const f64x4_t& v) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) part[(size_t)(16 * rb + lk + 4 * reg) * R + 16 * cb + li] = v[reg];
  };
  if constexpr (!DIAG) {
    // off-diagonal tile: 2x2 wave grid, wave (wr,wc) owns the sub-tiles (wr + 2 i, wc + 2 j): strided, so that a run of
    // absent cameras (a track that starts or ends inside the group) thins out all four wavefronts alike.  A sub-tile is
    // skipped for the batch when none of its four entries has a camera in its 16 rows or in its 16 columns (scalar
    // branches on the quad mask; a block index >= NT has no rows and never runs).
    const int wr = wave >> 1, wc = wave & 1;
    int rowoffA[NH], rowoffB[NH];
    uint32_t bitsA[NH], bitsB[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      rowoffA[i] = kbase + ((16 * min(wr + 2 * i, NT - 1) + li) ^ swz);
      rowoffB[i] = kbase + ((16 * min(wc + 2 * i, NT - 1) + li) ^ swz);
      bitsA[i] = block_slot_bits<BD>(wr + 2 * i);
      bitsB[i] = block_slot_bits<BD>(wc + 2 * i) << 16;
    }
#if !VGG_ABLATE && !VGG_TILE_TRACE    // (ablation / trace builds take sweep(), which carries their hooks)
    if constexpr (CY) {
      // PIPELINED BARRIER (round 5, compressed 6 x 6 off-diagonal tiles): the LAST K step of a batch is issued BEHIND the
      // batch's barrier.  Per step:  [loads of b+DEPTH] [K steps 0, 1 of b; operands of K step 2 fetched] [LDS image of b+1]
      // [barrier] [operands of K step 0 of b+1 requested] [K step 2 of b].  The matrix instructions of K step 2 (their
      // operands sit in registers since before the barrier) cover the LDS round trip of the next batch's first operands,
      // which the plain order exposes on every wavefront right behind every barrier (profiles/r05_tile_diag_ablations.jsonl:
      // without LDS operand reads the launch is 8 % shorter).  Hazards: every read of buffer `buf` (K steps 0..2 of b) is
      // complete before barrier(b) -- the fetches are waited for by the `pin`s in front of it --, buffer buf is rewritten
      // (batch b + 2) in step b + 1's write phase, behind that barrier; buffer buf^1 (batch b + 1) is read behind barrier(b),
      // which follows its writes.  Same matrix instructions in the same order per accumulator: bit-identical sums.
      // Same-box A/B (profiles/r05_ab_tile_pipe_c3.jsonl): off-diagonal launch 0.578 -> 0.560 ms.  The same order for the
      // diagonal tiles (a second operand set at 128 registers) measured SLOWER (0.256 -> 0.269 ms), and so did the same order
      // for the 8 x 8 full-factor tiles with their interleaved LDS writes (configs[3] whole: 13.13 -> 13.35 ms,
      // profiles/r05_ab_tile_pipe_c4full.jsonl): neither is in the tree.
      double a[2][NH], bq[2][NH];
      auto fetch = [&](int set, int buf, int ks) __attribute__((always_inline)) {
        const double* As = ops + (size_t)(buf * SIDES) * 4 * SEG;
        const double* Bs = ops + (size_t)(buf * SIDES + 1) * 4 * SEG;
#pragma unroll
        for (int i = 0; i < NH; ++i) { a[set][i] = As[rowoffA[i] + ks * R]; bq[set][i] = Bs[rowoffB[i] + ks * R]; }
      };
      auto pin = [&](int set) __attribute__((always_inline)) {
        static_assert(NH == 3, "operand sets");
        asm volatile("" : "+v"(a[set][0]), "+v"(a[set][1]), "+v"(a[set][2]), "+v"(bq[set][0]), "+v"(bq[set][1]), "+v"(bq[set][2]));
      };
      uint32_t on = 0u;
      auto skip_bits = [&](uint32_t qm) -> uint32_t {
        uint32_t colm = 0u, o = 0u;
#pragma unroll
        for (int j = 0; j < NH; ++j) colm |= ((qm & bitsB[j]) != 0 ? 1u : 0u) << j;
#pragma unroll
        for (int i = 0; i < NH; ++i) o |= ((qm & bitsA[i]) != 0 ? colm : 0u) << (NH * i);
        return VGG_NO_SKIP ? 0xFFFFFFFFu : (uint32_t)__builtin_amdgcn_readfirstlane((int)o);
      };
      auto group = [&](int set) __attribute__((always_inline)) {
        uint32_t m = on;
        asm volatile("" : "+s"(m));
#pragma unroll
        for (int i = 0; i < NH; ++i)
#pragma unroll
          for (int j = 0; j < NH; ++j)
            if (m & (1u << (NH * i + j))) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[set][i], bq[set][j], acc[i][j], 0, 0, 0);
      };
      // step of batch b; P = the operand set that holds K step 0 of b on entry (alternates from step to step)
      auto pstep = [&](int b, int buf, const int P, double2 (&sv_load)[NV], const double2 (&sv_write)[NV]) __attribute__((always_inline)) {
        const int seg_after = load_seg_index(ebase(b + DEPTH + 1));
        issue_loads(sv_load, seg_next, valid_next);
        seg_next = seg_after;
        valid_next = seg_valid(ebase(b + DEPTH + 1));
        // the LDS image of batch b + 1 is written FIRST: buffer buf^1 is free since barrier(b - 1) -- its last readers fetched
        // K step 2 of batch b - 1 in front of that barrier -- so the writes have landed long before this step's barrier and
        // its lgkmcnt(0) costs nothing (same-box A/B profiles/r05_ab_tile_pipe_c3.jsonl: 0.531 -> 0.521 ms)
        write_lds(sv_write, buf ^ 1);
        __builtin_amdgcn_s_setprio(0);
        on = skip_bits(qmask);
        fetch(1 - P, buf, 1); pin(P);
        group(P);                                     // K step 0
        fetch(P, buf, 2); pin(1 - P);
        group(1 - P);                                 // K step 1
        pin(P);                                       // (the operands of K step 2 have landed: no read of `buf` is left)
        __builtin_amdgcn_s_setprio(3);
        qmask = qmask_next;
        qmask_next = load_quad_mask(ebase(b + 2));
        __syncthreads();
        fetch(1 - P, buf ^ 1, 0);                     // K step 0 of batch b + 1 (stale bytes behind the last batch: never used)
        __builtin_amdgcn_s_setprio(0);
        pin(P);                                       // (keeps the matrix instructions below behind the barrier)
        group(P);                                     // K step 2 of batch b
      };
      fetch(0, 0, 0);
      constexpr int TRIP = 2 * DEPTH;
      int b = 0;
      for (; b + TRIP - 1 < nb; b += TRIP) {
#pragma unroll
        for (int u = 0; u < TRIP; ++u) pstep(b + u, u & 1, u & 1, sv[u % DEPTH], sv[(u + 1) % DEPTH]);
      }
#pragma unroll
      for (int u = 0; u < TRIP - 1; ++u)
        if (b + u < nb) pstep(b + u, u & 1, u & 1, sv[u % DEPTH], sv[(u + 1) % DEPTH]);
    } else
#endif
    sweep([&](int buf, uint32_t qm, auto&& wr) {
      const double* As = ops + (size_t)(buf * SIDES) * 4 * SEG;
      const double* Bs = ops + (size_t)(buf * SIDES + 1) * 4 * SEG;
      // one scalar bit per sub-tile of this wavefront (bit NH i + j), built once per batch: every skip test below is a bit
      // test + branch.  (With the conditions kept as booleans the compiler built each of the 27 tests of a batch from 64-bit
      // lane masks -- six dependent scalar instructions and two branches per matrix instruction.)
      uint32_t colm = 0u, on = 0u;
#pragma unroll
      for (int j = 0; j < NH; ++j) colm |= ((qm & bitsB[j]) != 0 ? 1u : 0u) << j;
#pragma unroll
      for (int i = 0; i < NH; ++i) on |= ((qm & bitsA[i]) != 0 ? colm : 0u) << (NH * i);
      on = VGG_NO_SKIP ? 0xFFFFFFFFu : (uint32_t)__builtin_amdgcn_readfirstlane((int)on);
      // operands of K step ks + 1 are requested before the matrix instructions of step ks; `pin` keeps the compiler from
      // sinking the LDS reads to their first use (it then waited for each one right in front of its matrix instruction),
      // `opaque` from turning the bit tests into lane-mask booleans shared by the three K steps
      double a[2][NH], bq[2][NH];
      auto fetch = [&](int set, int ks) __attribute__((always_inline)) {
#if VGG_ABLATE == 6                               // (profiling build: no LDS operand reads)
#pragma unroll
        for (int i = 0; i < NH; ++i) { a[set][i] = 1.0 + ks; bq[set][i] = 2.0 + i; }
#else
#pragma unroll
        for (int i = 0; i < NH; ++i) { a[set][i] = As[rowoffA[i] + ks * R]; bq[set][i] = Bs[rowoffB[i] + ks * R]; }
#endif
      };
      auto pin = [&](int set) __attribute__((always_inline)) {
        static_assert(NH == 3 || NH == 4, "operand sets");
        if constexpr (NH == 3)
          asm volatile("" : "+v"(a[set][0]), "+v"(a[set][1]), "+v"(a[set][2]), "+v"(bq[set][0]), "+v"(bq[set][1]), "+v"(bq[set][2]));
        else
          asm volatile("" : "+v"(a[set][0]), "+v"(a[set][1]), "+v"(a[set][2]), "+v"(a[set][3]), "+v"(bq[set][0]), "+v"(bq[set][1]),
                       "+v"(bq[set][2]), "+v"(bq[set][3]));
      };
      auto group = [&](int set) __attribute__((always_inline)) {
        uint32_t m = on;
        asm volatile("" : "+s"(m));
#pragma unroll
        for (int i = 0; i < NH; ++i)
#pragma unroll
          for (int j = 0; j < NH; ++j)
            if (m & (1u << (NH * i + j))) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[set][i], bq[set][j], acc[i][j], 0, 0, 0);
      };
      fetch(0, 0);
      fetch(1, 1); pin(0);
      group(0);
      wr(0);
      fetch(0, 2); pin(1);
      group(1);
      wr(1);
      pin(0);
      group(0);
      wr(2);
    });
#pragma unroll
    for (int i = 0; i < NH; ++i)
#pragma unroll
      for (int j = 0; j < NH; ++j)
        if (wr + 2 * i < NT && wc + 2 * j < NT) store_subtile(wr + 2 * i, wc + 2 * j, acc[i][j]);
  } else {
    // diagonal tile (A == B, symmetric): only the NT (NT + 1) / 2 sub-tiles of the lower triangle are computed.  Round 4: a
    // wavefront owns a PARITY CLASS of them -- rows wr + 2 i, columns wc + 2 j, row block >= column block -- like the
    // off-diagonal variant, instead of every fourth one of the row-by-row enumeration: its sub-tiles then share their row
    // and column operands (3..6 LDS reads per K step for 3..6 matrix instructions; dealt round-robin every matrix instruction
    // fetched its own two: 10..12 reads), and the classes still thin out alike under a run of absent cameras.  The classes
    // (0,0), (1,1), (0,1), (1,0) hold 6, 6, 3 and 6 sub-tiles at NT = 6.
    // With the stager / helper split of the compressed tiles (TR) the class follows the role, so that each of the two loop
    // bodies needs the accumulators i >= j only (six: the 128-register budget of four wavefronts per SIMD): stagers 0, 1
    // take the classes (0,0), (1,1) -- column blocks = row blocks, ONE operand set --, the helpers (0,1) -- three sub-tiles,
    // the wavefront with the 64-row share of the right-hand side -- and (1,0).
    const int mrole = wave;
    const int wr = (mrole == 1 || mrole == 3) ? 1 : 0, wc = (mrole == 1 || mrole == 2) ? 1 : 0;   // (0,0), (1,1), (0,1), (1,0)
    constexpr bool SAME = TR && !HELPER;              // compile-time: column operands are the row operands
    const bool same_rt = !TR && wr == wc;             // (full factors: one loop body for the four classes)
    int rowoffA[NH], rowoffB[NH];
    uint32_t bitsA[NH], bitsB[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      rowoffA[i] = kbase + ((16 * min(wr + 2 * i, NT - 1) + li) ^ swz);
      rowoffB[i] = kbase + ((16 * min(wc + 2 * i, NT - 1) + li) ^ swz);
      bitsA[i] = block_slot_bits<BD>(wr + 2 * i);
      bitsB[i] = block_slot_bits<BD>(wc + 2 * i);
    }
    // bit NH i + j: sub-tile (wr + 2 i, wc + 2 j) exists and lies in the lower triangle (wave-uniform)
    uint32_t lower = 0u;
#pragma unroll
    for (int i = 0; i < NH; ++i)
#pragma unroll
      for (int j = 0; j < NH; ++j)
        if (wr + 2 * i < NT && wc + 2 * j < NT && wr + 2 * i >= wc + 2 * j) lower |= 1u << (NH * i + j);
    lower = (uint32_t)__builtin_amdgcn_readfirstlane((int)lower);
    sweep([&](int buf, uint32_t qm, auto&& wr_lds) {
      const double* As = ops + (size_t)(buf * SIDES) * 4 * SEG;
      uint32_t colm = 0u, on = 0u;
#pragma unroll
      for (int j = 0; j < NH; ++j) colm |= ((qm & bitsB[j]) != 0 ? 1u : 0u) << j;
#pragma unroll
      for (int i = 0; i < NH; ++i) on |= ((qm & bitsA[i]) != 0 ? colm : 0u) << (NH * i);
      on = (VGG_NO_SKIP ? 0xFFFFFFFFu : (uint32_t)__builtin_amdgcn_readfirstlane((int)on)) & lower;
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        uint32_t m = on;
        asm volatile("" : "+s"(m));                 // (keeps the tests scalar bit tests; see the off-diagonal variant)
        double a[NH], bq[NH];
#pragma unroll
        for (int i = 0; i < NH; ++i) a[i] = As[rowoffA[i] + ks * R];
        if (SAME || same_rt) {                      // (scalar branch)
#pragma unroll
          for (int i = 0; i < NH; ++i) bq[i] = a[i];
        } else {
#pragma unroll
          for (int i = 0; i < NH; ++i) bq[i] = As[rowoffB[i] + ks * R];
        }
#pragma unroll
        for (int i = 0; i < NH; ++i)
#pragma unroll
          for (int j = 0; j < NH; ++j) {
            if (TR && j > i) continue;                // (classes of the compressed tiles: i >= j only)
            if (m & (1u << (NH * i + j))) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bq[j], acc[i][j], 0, 0, 0);
          }
        wr_lds(ks);
      }
    });
#pragma unroll
    for (int i = 0; i < NH; ++i)
#pragma unroll
      for (int j = 0; j < NH; ++j) {
        if (TR && j > i) continue;
        if (lower & (1u << (NH * i + j))) store_subtile(wr + 2 * i, wc + 2 * j, acc[i][j]);
      }
    if constexpr (TR && HELPER) {
      if (trhs) {                                     // the chunk's 96 x 3 block, a lane per tile row
        const int rrow = tid & 127;
        if (rrow < R) {
          double* dst = w.rz_part + ((size_t)chunk * R + rrow) * 3;
          dst[0] = racc[0]; dst[1] = racc[1]; dst[2] = racc[2];
        }
      }
    }
    if constexpr (TRF) {                              // full factors: [chunk][pair of entries][tile row], 288 doubles per chunk
      if (trf && tid < 2 * R && !(VGG_TRF_ABLATE & 4)) w.rz_part[(size_t)chunk * (kGroup * 18) + tid] = rfull;
    }
  }
  };   // run
  if constexpr (TR) {
    if (wave < 2) run(std::false_type{}); else run(std::true_type{});
  } else {
    run(std::false_type{});
  }
}

// the two launches of a tile batch (off-diagonal tiles, diagonal tiles) ...
template <int BD, bool DIAG>
__global__ __launch_bounds__(256, (BD == 6 ? (DIAG ? VGG_DIAG_OCC : VGG_OFFDIAG_OCC) : 2)) void schur_tile_kernel(Ws w, const int32_t* __restrict__ chunk_desc,
                                                         const int32_t* __restrict__ entries, int chunk0, int zero_seg) {
  __shared__ __attribute__((aligned(16))) double ops[2 * (DIAG ? 1 : 2) * 4 * kGroup * BD * 3 + (DIAG ? 96 : 0)];
  if (w.ctl->done) return;
  const int chunk = chunk0 + blockIdx.x;
  schur_tile_body<BD, DIAG>(w, chunk_desc, entries, chunk, zero_seg, ops);
}
// ... or ONE launch for both (vgg_ba_problem::merged_tile_launch): the diagonal tiles then sweep the points together with the
// off-diagonal ones and find the segments those have just brought into the Infinity Cache
template <int BD>
__global__ __launch_bounds__(256, (BD == 6 ? VGG_OFFDIAG_OCC : 2)) void schur_tile_merged_kernel(Ws w, const int32_t* __restrict__ chunk_desc,
                                                         const int32_t* __restrict__ entries, int chunk0, int zero_seg) {
  __shared__ __attribute__((aligned(16))) double ops[2 * 2 * 4 * kGroup * BD * 3];
  if (w.ctl->done) return;
  const int chunk = chunk0 + blockIdx.x;
  if (chunk_desc[6 * chunk] == chunk_desc[6 * chunk + 1]) schur_tile_body<BD, true>(w, chunk_desc, entries, chunk, zero_seg, ops);
  else schur_tile_body<BD, false>(w, chunk_desc, entries, chunk, zero_seg, ops);
}

// S[(cI,a,i),(cJ,b,j)] = - sum over the chunks of tile (gI,gJ) of the partial tiles (plain stores: every
// element of S outside the per-camera diagonal terms belongs to exactly one (tile, element)).
// grid = (R*R/256, num_tiles): one element per thread, chunks summed in order.
template <int BD>
__global__ __launch_bounds__(256) void tile_reduce_kernel(Ws w, int n_red, int C, int KD,
                                                          const int32_t* __restrict__ tile_desc, int tile0,
                                                          double* __restrict__ dst, int want) {
  constexpr int R = kGroup * BD;
  if (w.ctl->done) return;
  const int tile = tile0 + blockIdx.y;
  const int gI = tile_desc[4 * tile], gJ = tile_desc[4 * tile + 1];
  // (want: -1 = every tile of the range; 0 / 1 = only its off-diagonal / diagonal tiles -- the split exchange of the sharded
  //  solve sums the off-diagonal launch's tiles while the diagonal launch has not run yet, phases 7 / 9)
  if (want >= 0 && (gI == gJ) != (want == 1)) return;
  const int c0 = tile_desc[4 * tile + 2], c1 = tile_desc[4 * tile + 3];
  const int n = n_red;
  if constexpr (BD == 6) {
    // tile_rhs: the blocks behind the R x R elements add up, for a diagonal tile, the chunks' 96 x 3 right-hand-side blocks
    // (schur_tile_body's helpers) in the same fixed order -- assemble_kernel then reads 18 numbers per camera instead of
    // walking ~80 chunks with 18 of its 64 threads (24 us of every iteration at configs[2])
    const int nb2 = (R * R + 255) / 256;
    if ((int)blockIdx.x >= nb2) {
      if (gI != gJ || !w.tile_rhs) return;
      const int e = ((int)blockIdx.x - nb2) * 256 + threadIdx.x;
      if (e >= R * 3) return;
      double s0 = 0.0, s1 = 0.0;
      int ch = c0;
      const double* src = w.rz_part + e;
      for (; ch + 7 < c1; ch += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(ch + u) * R * 3];
#pragma unroll
        for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
      }
      for (; ch + 1 < c1; ch += 2) { s0 += src[(size_t)ch * R * 3]; s1 += src[(size_t)(ch + 1) * R * 3]; }
      if (ch < c1) s0 += src[(size_t)ch * R * 3];
      w.rz[(size_t)gI * R * 3 + e] = s0 + s1;
      return;
    }
  }
  if constexpr (BD != 6) {
    // tile_rhs with full factors: the chunks' [pair of entries][tile row] right-hand-side sums of a diagonal tile, in chunk order
    const int nb2 = (R * R + 255) / 256;
    if ((int)blockIdx.x >= nb2) {
      if (gI != gJ || !w.tile_rhs) return;
      const int e = ((int)blockIdx.x - nb2) * 256 + threadIdx.x;
      if (e >= 2 * R) return;
      double s0 = 0.0, s1 = 0.0;
      int ch = c0;
      const double* src = w.rz_part + e;
      constexpr size_t STR = kGroup * 18;
      for (; ch + 7 < c1; ch += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(ch + u) * STR];
#pragma unroll
        for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
      }
      for (; ch + 1 < c1; ch += 2) { s0 += src[(size_t)ch * STR]; s1 += src[(size_t)(ch + 1) * STR]; }
      if (ch < c1) s0 += src[(size_t)ch * STR];
      w.rz[(size_t)gI * STR + e] = s0 + s1;
      return;
    }
  }
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= R * R) return;
  const int row = e / R, col = e - row * R;
  const int a = row / BD, i = row - a * BD, b = col / BD, j = col - b * BD;
  const int ca = gI * kGroup + a, cb = gJ * kGroup + b;
  if (ca >= C || cb >= C) return;
  if (gI == gJ && col > row) return;             // diagonal tile is symmetric: the lower half is the unique source
  const int ri = (i < 6) ? 6 * ca + i : 6 * C + KD * ca + (i - 6);
  const int cj = (j < 6) ? 6 * cb + j : 6 * C + KD * cb + (j - 6);
  // (eight loads in flight per thread; the order of the additions -- even chunks into s0, odd ones into s1 -- is fixed)
  double s0 = 0.0, s1 = 0.0;
  int ch = c0;
  const double* src = w.tile_part + e;
  for (; ch + 7 < c1; ch += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(ch + u) * R * R];
#pragma unroll
    for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
  }
  for (; ch + 1 < c1; ch += 2) { s0 += src[(size_t)ch * R * R]; s1 += src[(size_t)(ch + 1) * R * R]; }
  if (ch < c1) s0 += src[(size_t)ch * R * R];
  const int hi = ri > cj ? ri : cj, lo = ri > cj ? cj : ri;
  double v = -(s0 + s1);
  if constexpr (BD == 6) {
    // compressed factors carry neither the Jacobi scales nor the constant-parameter masks (y_slot_doubles): both act on
    // whole rows / columns of the sum
    const double mi = w.active[ri] ? w.scale_c[ri] : 0.0, mj = w.active[cj] ? w.scale_c[cj] : 0.0;
    v *= mi * mj;
  }
  dst[(size_t)hi * n + lo] = v;
}

// diagonal blocks, camera/intrinsics coupling, damping, right-hand side.  One workgroup (64) per camera,
// plus one extra for the shared-intrinsics block.  Only rank 0 adds the terms that were already summed
// over ranks (U, g, damping); the per-rank systems are then all-reduced.
// tile_rhs: the pose rows of T_c = F^T [r - E hs | -E Ms] are  [g_c | 0] - (sum over the chunks of the camera's diagonal
// tile, in order, of rz_part)  -- g_c from the linearisation pass, rz_part from schur_tile_body -- and the intrinsics rows
// of the shared block come from point_pass' per-workgroup sums part_Q; T and cam_pass<RHS> are not used.
template <int KD>
__global__ __launch_bounds__(64) void assemble_kernel(DevProblem pb, Ws w, const int32_t* __restrict__ tile_desc, int num_tiles,
                                                      int point_parts) {
  // (fp contraction off: tile_assemble_kernel computes the same bits, so where a product is fused into an addition is written
  //  down in both -- fma() below -- and not left to the optimiser)
#pragma clang fp contract(off)
  constexpr int BD = 6 + KD;
  __shared__ double rz[6][3];
  __shared__ double rzf[BD];                       // tile_rhs with full factors (per-camera intrinsics): BD rows, scaled and masked
  if (w.ctl->done) return;
  const int global_terms = (w.ctl->rank == 0);
  const Dims& d = pb.d;
  const int n = d.n_red, kdsh = d.kdsh, tw = 1 + kdsh;
  const int c = blockIdx.x, tid = threadIdx.x;
  const bool trhs = w.tile_rhs != 0;
  if (c < d.C) {
    const double* U = w.U + (size_t)c * BD * BD;
    const double* T = w.T + (size_t)c * BD * tw;
    const int ia = 6 * d.C + (d.shared ? 0 : KD * c);
    const bool full = trhs && !d.shared && KD > 0;     // full factors: rz carries scales and masks, one column, BD rows
    if (full) {
      if (tid < BD) {
        const int g = c / kGroup;
        const bool has_tile = pb.col_ptr[min((g + 1) * kGroup, d.C)] > pb.col_ptr[g * kGroup];
        const size_t base = (size_t)g * kGroup * 18 + (size_t)(c % kGroup) * BD + tid;
        rzf[tid] = has_tile ? w.rz[base] + w.rz[base + kGroup * BD] : 0.0;      // (the two entry pairs of a batch)
      }
      __syncthreads();
    } else if (trhs) {
      // (a group without observations has no diagonal tile: nothing was summed for it)
      if (tid < 18) {
        const int i = tid / 3, col = tid - 3 * i;
        const int g = c / kGroup;
        const bool has_tile = pb.col_ptr[min((g + 1) * kGroup, d.C)] > pb.col_ptr[g * kGroup];
        rz[i][col] = has_tile ? w.rz[(size_t)g * kGroup * 18 + ((size_t)(c % kGroup) * 6 + i) * 3 + col] : 0.0;
      }
      __syncthreads();
    }
    // (the compressed factors behind rz carry no constant-parameter masks -- cam_pass<RHS> evaluated MASKED Jacobians, so a
    //  constant pose / translation component contributed exact zeros: the mask acts on the row here, like in tile_reduce)
    auto Tc = [&](int i, int m) -> double {
      if (!trhs) return T[i * tw + m];
      if (!w.active[6 * c + i]) return 0.0;
      return (m == 0 ? (global_terms ? w.g[(size_t)c * BD + i] : 0.0) : 0.0) - rz[i][m];
    };
    // BD x BD block (lower part), rows/cols mapped to reduced indices
    for (int e = tid; e < BD * BD; e += 64) {
      const int i = e / BD, j = e - i * BD;
      const int ri = (i < 6) ? 6 * c + i : ia + (i - 6), cj = (j < 6) ? 6 * c + j : ia + (j - 6);
      if (cj > ri) continue;
      if (d.shared && i >= 6 && j >= 6) continue;           // intr-intr of the shared block: extra workgroup
      if (trhs && !full && !d.shared && (i >= 6 || j >= 6)) continue;   // (compressed tile_rhs without shared intrinsics: none are refined)
      double v = 0.0;
      if (global_terms) {
        v = w.scale_c[ri] * w.scale_c[cj] * U[i * BD + j];
        if (ri == cj) v += w.dsq_c[ri];
      }
      if (d.shared && i >= 6) v = fma(w.scale_c[cj], Tc(j, 1 + (i - 6)), v);   // -F_pose^T E M
      w.S[(size_t)ri * n + cj] += v;
    }
    if (full) {
      if (tid < BD) {
        const int ri = (tid < 6) ? 6 * c + tid : ia + (tid - 6);
        const double v = (global_terms ? w.scale_c[ri] * w.g[(size_t)c * BD + tid] : 0.0) - rzf[tid];
        w.rhs[ri] += w.active[ri] ? v : 0.0;
      }
    } else {
      if (tid < 6) w.rhs[6 * c + tid] = fma(w.scale_c[6 * c + tid], Tc(tid, 0), w.rhs[6 * c + tid]);
      if (!trhs && !d.shared && tid >= 6 && tid < BD) w.rhs[ia + tid - 6] = fma(w.scale_c[ia + tid - 6], T[tid * tw], w.rhs[ia + tid - 6]);
    }
  } else {
    if (trhs) {                                    // (rides along: max of the point passes' per-workgroup gradient norms,
      double m = 0;                                //  what cam_reduce_kernel<KD, 1> did)
      // (these loops run in ONE wavefront and each trip is a round trip to memory: unrolled, so that several are in flight --
      //  the extra workgroup was the long pole of the launch, ~20 of its 23 us at configs[2])
#pragma unroll 8
      for (int i = tid; i < point_parts; i += 64) m = fmax(m, w.part_B[i]);
      m = wave_max(m);
      if (tid == 0) w.gmax_pts[0] = m;
    }
    if (d.shared && KD > 0) {
      // shared-intrinsics block: sum the per-camera parts (one wavefront, lanes stride over cameras)
      const int ia = 6 * d.C;
      constexpr int NS = (KD > 0) ? KD * KD + KD : 1;
      double sums[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) sums[i] = 0.0;
#pragma unroll 4
      for (int cc = tid; cc < d.C; cc += 64) {
#pragma unroll
        for (int i = 0; i < KD; ++i) {
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            double v = trhs ? 0.0 : w.scale_c[ia + i] * w.T[((size_t)cc * BD + 6 + i) * tw + 1 + j];
            if (global_terms) v = fma(w.scale_c[ia + i] * w.scale_c[ia + j], w.U[(size_t)cc * BD * BD + (6 + i) * BD + 6 + j], v);
            sums[i * KD + j] += v;
          }
          sums[KD * KD + i] += trhs ? (global_terms ? w.g[(size_t)cc * BD + 6 + i] : 0.0) : w.T[((size_t)cc * BD + 6 + i) * tw];
        }
      }
      if (trhs) {
        // - sum_p Wa_p Ms_p^T (scaled like the T terms above) and - sum_p Wa_p hs_p, workgroup partials in launch order
#pragma unroll 8
        for (int b = tid; b < point_parts; b += 64) {
          const double* q = w.part_Q + 8 * (size_t)b;
#pragma unroll
          for (int i = 0; i < KD; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) sums[i * KD + j] = fma(-w.scale_c[ia + i], q[KD + i * KD + j], sums[i * KD + j]);
            sums[KD * KD + i] -= q[i];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NS; ++i) sums[i] = wave_sum(sums[i]);
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < KD; ++i) {
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            double v = sums[i * KD + j];
            if (global_terms && i == j) v += w.dsq_c[ia + i];
            w.S[(size_t)(ia + i) * n + ia + j] += v;
          }
          w.rhs[ia + i] = fma(w.scale_c[ia + i], sums[KD * KD + i], w.rhs[ia + i]);
        }
      }
    }
  }
}

// after (the all-reduce of) buffer 0: column norms, Jacobi scaling (first time), camera-side gradient max, cost
template <int KD>
__device__ __forceinline__ void prep_body(const DevProblem& pb, const Ws& w, const vgg_ba_options& opt, double* red) {
  constexpr int BD = 6 + KD;
  Ctl* ctl = w.ctl;
  const Dims& d = pb.d;
  const bool first = !ctl->scale_ready;
  double gmax = 0.0, cost = 0.0;
  constexpr int NS = 1 + 2 * (KD > 0 ? KD : 1);
  double sums[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) sums[k] = 0.0;
  for (int c = threadIdx.x; c < d.C; c += 256) {
    const double* U = w.U + (size_t)c * BD * BD;
    const double* g = w.g + (size_t)c * BD;
    cost += w.costc[c];
    if (d.shared && KD > 0) {                      // shared intrinsics: column norm and gradient are sums over all cameras
#pragma unroll
      for (int k = 0; k < KD; ++k) { sums[1 + k] += U[(6 + k) * BD + 6 + k]; sums[1 + KD + k] += g[6 + k]; }
    }
    for (int k = 0; k < 6; ++k) w.colsq_c[6 * c + k] = U[k * BD + k];
    if (!d.shared) for (int k = 0; k < KD; ++k) w.colsq_c[6 * d.C + KD * c + k] = U[(6 + k) * BD + 6 + k];
    // |Plus(x, -g) - x|_inf for this camera (Ceres projected-gradient norm)
    double dl[3], qn[4];
    for (int k = 0; k < 3; ++k) dl[k] = w.active[6 * c + k] ? -g[k] : 0.0;
    quat_plus(pb.cam_q + 4 * c, dl, qn);
    for (int k = 0; k < 4; ++k) gmax = fmax(gmax, fabs(qn[k] - pb.cam_q[4 * c + k]));
    for (int k = 3; k < 6; ++k) if (w.active[6 * c + k]) gmax = fmax(gmax, fabs(g[k]));
    if (!d.shared) for (int k = 0; k < KD; ++k) if (w.active[6 * d.C + KD * c + k]) gmax = fmax(gmax, fabs(g[6 + k]));
  }
  // one block reduction for everything (round 4: six 256-thread trees of eight barriers each took 15 us of every iteration):
  // wave sums (crosslane.hpp), then the four wavefronts' partials in a fixed order
  sums[0] = cost;
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const double v = wave_sum(sums[k]);
    if (ln == 0) red[wv * 8 + k] = v;
  }
  gmax = wave_max(gmax);
  if (ln == 0) red[32 + wv] = gmax;
  __syncthreads();
  const double cost_total = (red[0] + red[8]) + (red[16] + red[24]);
  double gm = fmax(fmax(red[32], red[33]), fmax(red[34], red[35]));
  if (d.shared && KD > 0) {
#pragma unroll
    for (int k = 0; k < KD; ++k) {
      const double cs = (red[1 + k] + red[9 + k]) + (red[17 + k] + red[25 + k]);
      const double gs = (red[1 + KD + k] + red[9 + KD + k]) + (red[17 + KD + k] + red[25 + KD + k]);
      if (threadIdx.x == 0) w.colsq_c[6 * d.C + k] = cs;
      if (w.active[6 * d.C + k]) gm = fmax(gm, fabs(gs));
    }
  }
  __syncthreads();                                 // (colsq_c is read below by other threads)
  if (first) {
    for (int j = threadIdx.x; j < d.n_red; j += 256)
      w.scale_c[j] = opt.jacobi_scaling ? 1.0 / (1.0 + sqrt(w.colsq_c[j])) : 1.0;
  }
  if (threadIdx.x == 0) {
    ctl->gmax_cams = gm;
    if (first) { ctl->x_cost = 0.5 * cost_total; ctl->initial_cost = ctl->x_cost; }
  }
}

// after (the all-reduce of) buffer 0: prep_body when a new linearisation is in place, then -- every iteration -- the LM
// damping of the reduced columns for the current radius (one launch: both are a few hundred elements)
template <int KD>
__global__ __launch_bounds__(256) void prep_kernel(DevProblem pb, Ws w, vgg_ba_options opt) {
  __shared__ double red[256];
  Ctl* ctl = w.ctl;
  if (ctl->done) return;
  if (ctl->need_lin) prep_body<KD>(pb, w, opt, red);       // (uniform branch: the body synchronises the workgroup)
  __syncthreads();
  const int n_red = pb.d.n_red;
  const double radius = ctl->radius;
#pragma unroll 4
  for (int j = threadIdx.x; j < n_red; j += 256) {
    const double sc = w.scale_c[j];
    double dd = w.colsq_c[j] * sc * sc;
    dd = fmin(fmax(dd, opt.min_lm_diagonal), opt.max_lm_diagonal);
    w.dsq_c[j] = dd / radius;
  }
}

// LM damping of reduced column j for the current radius (prep_kernel's loop body)
__device__ __forceinline__ double lm_damping(double colsq, double sc, double radius, const vgg_ba_options& opt) {
  double dd = colsq * sc * sc;
  dd = fmin(fmax(dd, opt.min_lm_diagonal), opt.max_lm_diagonal);
  return dd / radius;
}

// tile_reduce_kernel + assemble_kernel + prep_kernel in ONE launch (phase 1 with tile_rhs, one tile batch, every camera group
// with a diagonal tile; the three kernels stay for every other configuration and for vgg_ba_set_tile_rhs(| 4)).  assemble_kernel
// adds per-camera terms to elements that tile_reduce_kernel stored a few microseconds earlier and derives the right-hand side
// from the rz sums of the same launch: here the thread that sums an element of a camera's own block adds that camera's term
// and stores once, and the thread that sums an rz element writes the row of rhs / of the shared-intrinsics border made from it.
// KD: intrinsics unknowns per block; BD: rows of a tile block (6 = compressed factors: shared or constant intrinsics).
// grid = (tile_reduce_kernel's x, 1 + num_tiles): row y > 0 is tile y - 1; row 0 carries the two workgroups that need no tile sum,
//   x = 0: assemble_kernel's extra workgroup (gmax_pts; the shared-intrinsics block from part_Q and the per-camera parts),
//   x = 1: prep_body (column norms, gmax_cams) when a new linearisation is in place.  The FIRST linearisation's prep_body also
//          makes scale_c, which point_pass reads: that one stays prep_kernel, a launch in front of point_pass (phase_schur).
// dsq_c is computed where it is added, from U's diagonal (= colsq_c: prep_body copies it from there) -- and stored as well.
// Same sums in the same order as the three kernels, so the same bits: fp contraction is OFF in this function and the two
// places where the compiler contracts assemble_kernel's expressions are spelled fma() -- S = v; S += t rounds v and t first.
template <int KD, int BD>
__global__ __launch_bounds__(256) void tile_assemble_kernel(DevProblem pb, Ws w, vgg_ba_options opt,
                                                            const int32_t* __restrict__ tile_desc, int point_parts) {
#pragma clang fp contract(off)
  constexpr int R = kGroup * BD, UBD = 6 + KD;
  constexpr bool SH = (KD > 0 && BD == 6);          // shared intrinsics: border rows 6 C .. behind the poses
  constexpr int nb2 = (R * R + 255) / 256;
  static_assert(BD == 6 || 2 * R <= 256, "the two entry pairs of a full-factor rz row meet in one workgroup");
  __shared__ double red[256];
  const Ctl* ctl = w.ctl;
  if (ctl->done) return;
  const Dims& d = pb.d;
  const int C = d.C, n = d.n_red, tid = threadIdx.x;
  const int global_terms = (ctl->rank == 0);
  const double radius = ctl->radius;
  if (blockIdx.y == 0) {
    if (blockIdx.x == 1) {
      if (ctl->need_lin && ctl->scale_ready) prep_body<KD>(pb, w, opt, red);   // (uniform branch: the body synchronises)
      return;
    }
    if (blockIdx.x != 0) return;
    // the shared column norms: prep_body's sum over the cameras, same order (its workgroup may not have stored it yet)
    double cs[KD > 0 ? KD : 1] = {};
    if constexpr (SH) {
      double part[KD];
#pragma unroll
      for (int k = 0; k < KD; ++k) part[k] = 0.0;
      for (int c = tid; c < C; c += 256) {
#pragma unroll
        for (int k = 0; k < KD; ++k) part[k] += w.U[(size_t)c * UBD * UBD + (6 + k) * UBD + 6 + k];
      }
      const int wv = tid >> 6, ln = tid & 63;
#pragma unroll
      for (int k = 0; k < KD; ++k) {
        const double v = wave_sum(part[k]);
        if (ln == 0) red[wv * 8 + 1 + k] = v;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < KD; ++k) cs[k] = (red[1 + k] + red[9 + k]) + (red[17 + k] + red[25 + k]);
    }
    if (tid >= 64) return;
    {
      double m = 0;                                // (one wavefront, round trips to memory: unrolled, see assemble_kernel)
#pragma unroll 8
      for (int i = tid; i < point_parts; i += 64) m = fmax(m, w.part_B[i]);
      m = wave_max(m);
      if (tid == 0) { w.gmax_pts[0] = m; w.ctl->merged_glue_launches += 1; }
    }
    if constexpr (SH) {
      const int ia = 6 * C;
      constexpr int NS = KD * KD + KD;
      double sums[NS];
#pragma unroll
      for (int i = 0; i < NS; ++i) sums[i] = 0.0;
#pragma unroll 4
      for (int cc = tid; cc < C; cc += 64) {
#pragma unroll
        for (int i = 0; i < KD; ++i) {
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            if (global_terms) v += w.scale_c[ia + i] * w.scale_c[ia + j] * w.U[(size_t)cc * UBD * UBD + (6 + i) * UBD + 6 + j];
            sums[i * KD + j] += v;
          }
          sums[KD * KD + i] += global_terms ? w.g[(size_t)cc * UBD + 6 + i] : 0.0;
        }
      }
#pragma unroll 8
      for (int b = tid; b < point_parts; b += 64) {
        const double* q = w.part_Q + 8 * (size_t)b;
#pragma unroll
        for (int i = 0; i < KD; ++i) {
#pragma unroll
          for (int j = 0; j <= i; ++j) sums[i * KD + j] = fma(-w.scale_c[ia + i], q[KD + i * KD + j], sums[i * KD + j]);
          sums[KD * KD + i] -= q[i];
        }
      }
#pragma unroll
      for (int i = 0; i < NS; ++i) sums[i] = wave_sum(sums[i]);
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < KD; ++i) {
          const double dsq = lm_damping(cs[i], w.scale_c[ia + i], radius, opt);
          w.dsq_c[ia + i] = dsq;
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            double v = sums[i * KD + j];
            if (global_terms && i == j) v += dsq;
            w.S[(size_t)(ia + i) * n + ia + j] = 0.0 + v;
          }
          w.rhs[ia + i] = fma(w.scale_c[ia + i], sums[KD * KD + i], 0.0);
        }
      }
    }
    return;
  }
  const int tile = blockIdx.y - 1;
  const int gI = tile_desc[4 * tile], gJ = tile_desc[4 * tile + 1];
  const int c0 = tile_desc[4 * tile + 2], c1 = tile_desc[4 * tile + 3];
  if ((int)blockIdx.x >= nb2) {
    // the right-hand-side sums of a diagonal tile (tile_reduce_kernel), then what assemble_kernel makes of them
    if (gI != gJ) return;
    constexpr int NE = (BD == 6) ? R * 3 : 2 * R;              // elements, and the chunk stride
    constexpr size_t STR = (BD == 6) ? (size_t)R * 3 : (size_t)kGroup * 18;
    const int e = ((int)blockIdx.x - nb2) * 256 + tid;
    if (BD == 6 && e >= NE) return;
    const bool live = e < NE;
    double s0 = 0.0, s1 = 0.0;
    int ch = c0;
    const double* src = w.rz_part + (live ? e : 0);            // (a thread beyond the row walks element 0: loads stay unconditional)
    for (; ch + 7 < c1; ch += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(ch + u) * STR];
#pragma unroll
      for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
    }
    for (; ch + 1 < c1; ch += 2) { s0 += src[(size_t)ch * STR]; s1 += src[(size_t)(ch + 1) * STR]; }
    if (ch < c1) s0 += src[(size_t)ch * STR];
    const double rzv = s0 + s1;
    if (live) w.rz[(size_t)gI * STR + e] = rzv;
    if constexpr (BD == 6) {
      // compressed factors: element (camera slot a, pose row i, column col) -- column 0 is the right-hand side, 1 + k the border
      // of shared intrinsics k; rz carries neither scales nor masks
      const int a = e / 18, i = (e - 18 * a) / 3, col = e - 18 * a - 3 * i;
      const int c = gI * kGroup + a;
      if (c >= C) return;
      const int rj = 6 * c + i;
      const bool act = w.active[rj] != 0;
      const double sc = w.scale_c[rj];
      if (col == 0) {
        const double Tc = act ? ((global_terms ? w.g[(size_t)c * UBD + i] : 0.0) - rzv) : 0.0;
        w.rhs[rj] = fma(sc, Tc, 0.0);
      } else if (SH && col <= KD) {
        const int k = col - 1, ia = 6 * C;
        double v = 0.0;
        if (global_terms) v = w.scale_c[ia + k] * sc * w.U[(size_t)c * UBD * UBD + (6 + k) * UBD + i];
        const double Tc = act ? (0.0 - rzv) : 0.0;
        v = fma(sc, Tc, v);
        w.S[(size_t)(ia + k) * n + rj] = 0.0 + v;
      }
    } else {
      // full factors: rz carries scales and masks; a row is the sum of the batch's two entry pairs (elements e and e + R)
      red[tid] = rzv;
      __syncthreads();
      if (e >= R) return;
      const int a = e / BD, t = e - a * BD;
      const int c = gI * kGroup + a;
      if (c >= C) return;
      const double rzf = red[e] + red[e + R];
      const int ri = (t < 6) ? 6 * c + t : 6 * C + KD * c + (t - 6);
      const double v = (global_terms ? w.scale_c[ri] * w.g[(size_t)c * UBD + t] : 0.0) - rzf;
      w.rhs[ri] = 0.0 + (w.active[ri] ? v : 0.0);
    }
    return;
  }
  const int e = blockIdx.x * 256 + tid;
  if (e >= R * R) return;
  const int row = e / R, col = e - row * R;
  const int a = row / BD, i = row - a * BD, b = col / BD, j = col - b * BD;
  const int ca = gI * kGroup + a, cb = gJ * kGroup + b;
  if (ca >= C || cb >= C) return;
  if (gI == gJ && col > row) return;             // diagonal tile is symmetric: the lower half is the unique source
  const int ri = (i < 6) ? 6 * ca + i : 6 * C + KD * ca + (i - 6);
  const int cj = (j < 6) ? 6 * cb + j : 6 * C + KD * cb + (j - 6);
  // (eight loads in flight per thread; the order of the additions -- even chunks into s0, odd ones into s1 -- is fixed)
  double s0 = 0.0, s1 = 0.0;
  int ch = c0;
  const double* src = w.tile_part + e;
  for (; ch + 7 < c1; ch += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(ch + u) * R * R];
#pragma unroll
    for (int u = 0; u < 8; u += 2) { s0 += v[u]; s1 += v[u + 1]; }
  }
  for (; ch + 1 < c1; ch += 2) { s0 += src[(size_t)ch * R * R]; s1 += src[(size_t)(ch + 1) * R * R]; }
  if (ch < c1) s0 += src[(size_t)ch * R * R];
  const int hi = ri > cj ? ri : cj, lo = ri > cj ? cj : ri;
  double v = -(s0 + s1);
  if constexpr (BD == 6) {
    const double mi = w.active[ri] ? w.scale_c[ri] : 0.0, mj = w.active[cj] ? w.scale_c[cj] : 0.0;
    v *= mi * mj;
  }
  if (gI == gJ && a == b) {
    // the camera's own block (ri >= cj): + s_i s_j U_ij, + the damping on the diagonal -- rank 0 only, the other ranks' share is 0
    const double* U = w.U + (size_t)ca * UBD * UBD;
    double t = 0.0;
    if (global_terms) t = w.scale_c[ri] * w.scale_c[cj] * U[i * UBD + j];
    if (ri == cj) {
      const double dsq = lm_damping(U[i * UBD + i], w.scale_c[ri], radius, opt);
      w.dsq_c[ri] = dsq;
      if (global_terms) t += dsq;
    }
    v = v + t;
  }
  w.S[(size_t)hi * n + lo] = v;
}

// one batch of Schur tiles: the off-diagonal launch, the diagonal launch, and the ordered sum of their chunks into
// dst (S, or S2 for a batch that runs beside the factorisation)
template <int BD>
static void launch_schur_batch(const Launch& L, int batch, hipStream_t st, double* dst, int which = 0, bool sums = true) {
  // sums = false: the caller sums the chunks itself (tile_assemble_kernel)
  // which: 0 = the whole batch; 1 = the off-diagonal launch and the sums of its tiles; 2 = the diagonal launch and its sums
  // (1 / 2: the split exchange of the sharded solve; never with the merged launch)
  const int32_t* B = L.batches + 6 * batch;
  const int c0 = B[0], cm = B[1], c1 = B[2], t0 = B[3], t1 = B[4];
  if (L.merged_tile_launch && c1 > c0) {
    ProfScope ps(kProfSchurTile, st);
    schur_tile_merged_kernel<BD><<<c1 - c0, 256, 0, st>>>(L.w, L.chunk_desc, L.entries, c0, L.num_segments);
  } else if (cm > c0 && which != 2) {
    ProfScope ps(kProfSchurTile, st);
    schur_tile_kernel<BD, false><<<cm - c0, 256, 0, st>>>(L.w, L.chunk_desc, L.entries, c0, L.num_segments);
  }
  if (!L.merged_tile_launch && c1 > cm && which != 1) {
    ProfScope ps(kProfSchurTileDiag, st);
    schur_tile_kernel<BD, true><<<c1 - cm, 256, 0, st>>>(L.w, L.chunk_desc, L.entries, cm, L.num_segments);
  }
  if (t1 > t0 && sums)
    tile_reduce_kernel<BD><<<dim3(div_up(kGroup * BD * kGroup * BD, 256) + (L.w.tile_rhs ? (BD == 6 ? div_up(kGroup * BD * 3, 256) : div_up(2 * kGroup * BD, 256)) : 0),
                                  t1 - t0), 256, 0, st>>>(L.w, L.d.n_red, L.d.C, L.d.kd, L.tile_desc, t0, dst, which == 0 ? -1 : which - 1);
}

// tile blocks of 6 rows (compressed factors: shared or constant intrinsics), of 6 + kd with per-camera intrinsics
void launch_schur_batches(const Launch& L, int b0, int b1, hipStream_t st, double* dst, int32_t* done_flags, int which, bool sums) {
  for (int b = b0; b < b1; ++b) {
    if (L.d.shared || L.d.kd == 0) launch_schur_batch<6>(L, b, st, dst, which, sums);
    else if (L.d.kd == 1) launch_schur_batch<7>(L, b, st, dst, which, sums);
    else launch_schur_batch<8>(L, b, st, dst, which, sums);
    if (done_flags) dataflow_signal(done_flags + b, st);    // (the single-launch factorisation waits on the device)
  }
}

void launch_prep(const Launch& L) {
  dispatch_kd(L.d.kd, [&](auto kd) { prep_kernel<decltype(kd)::value><<<1, 256, 0, L.st>>>(L.dp, L.w, L.opt); });
}

void launch_assemble(const Launch& L) {
  dispatch_kd(L.d.kd, [&](auto kd) {
    assemble_kernel<decltype(kd)::value><<<L.d.C + 1, 64, 0, L.st>>>(L.dp, L.w, L.tile_desc, L.num_tiles, L.wgB);
  });
}

// tile sums, assembly and preparation in one launch (the caller sums no chunks: launch_schur_batches(..., sums = false))
void launch_tile_assemble(const Launch& L) {
  dispatch_kd(L.d.kd, [&](auto kd) {
    constexpr int KD = decltype(kd)::value;
    auto launch = [&](auto bd) {
      constexpr int BD = decltype(bd)::value;
      constexpr int R = kGroup * BD;
      const int gx = div_up(R * R, 256) + (BD == 6 ? div_up(R * 3, 256) : div_up(2 * R, 256));
      tile_assemble_kernel<KD, BD><<<dim3(gx, 1 + L.num_tiles), 256, 0, L.st>>>(L.dp, L.w, L.opt, L.tile_desc, L.wgB);
    };
    if (L.d.shared || KD == 0) launch(std::integral_constant<int, 6>{});
    else launch(std::integral_constant<int, 6 + KD>{});
  });
}

}  // namespace vgg

#if VGG_TILE_TRACE
extern "C" int vgg_debug_read_tile_trace(long long* host, size_t count) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(vgg::g_tile_trace), sizeof(long long) * count);
}
#endif
