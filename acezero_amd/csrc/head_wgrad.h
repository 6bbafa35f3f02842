// head_wgrad.h -- the weight-gradient K loop, shared by wgrad_kernel and wgrad_opt_kernel (head_optim.hip).
#pragma once
#include "head_kernels.h"

namespace acez {

// ---------------------------------------------------------------------------------------------------
// wgrad: dW_l[n][c] = sum_m dZ_l[m][n] * In_l[m][c] (the bias gradients are column sums taken where dZ is produced), all wide layers in one
// launch (grid.y = layer), split-K over rows (slab s = blockIdx.x / 16). Both operands are row-major with
// the reduction index m as the slow dimension, so the MFMA fragments (8 consecutive m for one column) are
// read with ds_read_b64_tr_b16 from an untransposed [64 m][128 cols] LDS tile (row pitch 320 B: the four
// rows a 32-lane group touches fall on disjoint banks).
// ---------------------------------------------------------------------------------------------------
// LDS stage = [64 m][128 cols] bf16 per operand (256-byte rows, no padding: the image is written by LDS-DMA in
// lane order). The four rows a 32-lane tr-read group touches would share banks, so the 32-byte segment index of a
// row is XOR-ed with (row & 3) << 1 -- applied to the per-lane DMA source chunk and, identically, to the reads.
// element offset, inside a [64][128] stage, of the first of the two transposed 8-byte reads lane l issues for the
// fragment tile[k0 + 8*(l>>5) + e][col0 + (l & 31)], e = 0..7, for k0 = 0 (other k0: + k0 * 128)
__device__ __forceinline__ int tr_base(int col0, int l) {
  const int q = l >> 4, i16 = l & 15;
  const int row = 8 * (q >> 1) + (i16 >> 2);                     // row & 3 == i16 >> 2 (also for row + 4)
  const int colb = (col0 + 16 * (q & 1) + 4 * (i16 & 3)) * 2;    // logical byte offset inside the 256-byte row
  const int phys = ((((colb >> 5) ^ ((i16 >> 2) << 1)) << 5) | (colb & 31)) >> 1;
  return row * 128 + phys;
}
template <class E = EltBf16>
__device__ __forceinline__ typename E::frag tr_frag(const uint16_t* p) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * 128));
  s16x8 r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return __builtin_bit_cast(typename E::frag, r);
}

// The K loop of one (layer, row slab, 128 x 128 tile) workgroup, shared by wgrad_kernel and wgrad_opt_kernel. Returns true in the
// loader waves (their loop is over: every stage has landed and every barrier of the loop has been passed), false in the four multiplier
// waves, whose accumulators then hold the slab's partial tile. KT = number of 64-row stages of this slab.
// PFN > 0: `prefetch()` issues exactly PFN vector-memory loads (wgrad_opt_kernel: the optimiser state of the workgroup's half tile) from
// inside the loader loop, about a dozen stages before its end, so that they travel beside the operand stream instead of after it; loads
// complete in order, so the counted waits of the stages requested BEFORE the prefetch allow PFN more instructions in flight.
template <class E, int PFN, class PF>
__device__ __forceinline__ bool wgrad_kloop(const WgradArgs& a, uint16_t (*smem)[2][64 * 128], const int layer, const int slab, const int tile,
                                            f32x16 (&acc)[2][2], int& KT_out, PF&& prefetch) {
  constexpr int RING = WGRAD_RING;
  static_assert(2 * (16 / WGRAD_LOADERS) * (RING - 1) + PFN <= 31, "wait_vmcnt_dyn covers 1 .. 31");
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  // Role split: waves 0..3 multiply (2 x 2 grid of 64 x 64 sub-tiles: 4 fragment reads feed 4 MFMAs), waves 4..11 only
  // issue the LDS-DMA. A wave's instruction stream is in-order: with every wave loading AND multiplying, the ~0.4 us a
  // stage's DMA instructions need to get through the memory pipeline was added to the MFMA time instead of hidden
  // behind it (ablation: 18 us loads-only + 23 us MFMA-only = 41 us). Waves w and w + 4 share a SIMD, so every SIMD
  // has one multiplier and two loaders.
  const bool loader = w >= 4;
  const int cw = w & 3, wn = cw >> 1, wc = cw & 1;
  const int lw = w - 4;                         // loader index
  constexpr int GPL = 16 / WGRAD_LOADERS;       // 4-row DMA groups (x 2 operands) per loader and stage
  const int n0 = (tile >> 2) * 128, c0 = (tile & 3) * 128;
  const uint16_t* __restrict__ Z = a.dZ[layer];
  const uint16_t* __restrict__ X = a.In[layer];
  const int M = a.M;
  // rows of this slab: [mb, me), multiple of 64 per slab except the tail
  const int rows_per_slab = ((M + a.nslabs * 64 - 1) / (a.nslabs * 64)) * 64;
  const int mb = slab * rows_per_slab;
  const int me = min(M, mb + rows_per_slab);
  const int KT = (me > mb) ? (me - mb + 63) >> 6 : 0;
  KT_out = KT;

  // DMA instruction j of loader wave lw covers stage rows (lw*GPL+j)*4 .. +3 of both operands; this lane: row + (l>>4),
  // physical 16-byte chunk l&15, which must receive the logical chunk whose 32-byte segment index is XOR-swizzled
  const int prow = l >> 4, pq = l & 15;
  auto issue = [&](int kt) {
    const int slot = kt % RING;
#pragma unroll
    for (int j = 0; j < GPL; ++j) {
      const int srow = (lw * GPL + j) * 4 + prow;
      const int lchunk = ((((pq >> 1) ^ ((srow & 3) << 1)) << 1) | (pq & 1)) * 8;  // element offset of the source chunk
      const int m = mb + kt * 64 + srow;
      const bool ok = m < me;
      // rows past the slab end must contribute zeros: they are fetched from a zero page
      const uint16_t* gz = ok ? Z + (size_t)m * 512 + n0 + lchunk : a.zeros + pq * 8;
      const uint16_t* gx = ok ? X + (size_t)m * 512 + c0 + lchunk : a.zeros + pq * 8;
      __builtin_amdgcn_global_load_lds((gvoid_t*)gz, (lvoid_t*)&smem[slot][0][(lw * GPL + j) * 4 * 128], 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gvoid_t*)gx, (lvoid_t*)&smem[slot][1][(lw * GPL + j) * 4 * 128], 16, 0, 0);
    }
  };

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // Two separate loops (one per role) with the same number of barriers: sharing one loop body makes the compiler
  // carry the 64 accumulator registers through the loader's control flow (moves on every iteration).
  if (loader) {
    for (int kt = 0; kt < RING && kt < KT; ++kt) issue(kt);
    // stage kt: wait until it has landed, meet the multipliers (they are done with stage kt - 1), refill the slot of stage kt - 1
    auto stage = [&](int kt, int extra) {
      // stages issued so far: 0..RING-1 at kt = 0, 0..kt+RING-2 afterwards; a loader wave has 2 * GPL DMA instructions per stage in flight
      const int later = (kt == 0) ? min(RING - 1, KT - 1) : min(RING - 2, KT - 1 - kt);
      wait_vmcnt_dyn(2 * GPL * later + extra);
      __builtin_amdgcn_s_barrier();
      if (kt >= 1 && kt + RING - 1 < KT) issue(kt + RING - 1);
    };
    if (PFN == 0) {
      for (int kt = 0; kt < KT; ++kt) stage(kt, 0);
    } else {
      // the prefetch goes out behind the issue of iteration P (P < 0: behind the first RING stages); the last stage requested before
      // it is S: stages kt <= S are older than the prefetch, their waits allow it to be in flight
      const int P = KT > 16 ? KT - 13 : -1;
      for (int kt = 0; kt <= P; ++kt) stage(kt, 0);
      prefetch();
      const int S = P < 0 ? min(RING, KT) - 1 : min(P + RING - 1, KT - 1);
      for (int kt = P + 1; kt < KT; ++kt) stage(kt, kt <= S ? PFN : 0);
    }
    return true;
  }
  const int offA[2] = {tr_base(wn * 64, l), tr_base(wn * 64 + 32, l)};
  const int offB[2] = {tr_base(wc * 64, l), tr_base(wc * 64 + 32, l)};
  for (int kt = 0; kt < KT; ++kt) {
    __builtin_amdgcn_s_barrier();
    const int slot = kt % RING;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      typename E::frag fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = tr_frag<E>(&smem[slot][0][offA[i] + kk * 16 * 128]);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = tr_frag<E>(&smem[slot][1][offB[j] + kk * 16 * 128]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = E::mfma32(fa[i], fb[j], acc[i][j]);
    }
  }
  return false;
}

}  // namespace acez
