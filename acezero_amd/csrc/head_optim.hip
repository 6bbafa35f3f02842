// head_optim.hip -- gfx950 kernels of the head's optimiser side: gather, weight gradients, gradient reduction, AdamW, schedule.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "head_kernels.h"
#include "gemm_common.h"
#include "head_gather.h"
#include "head_seq.h"
#include "head_wgrad.h"
#include "head_opt.h"
#include "head_sched.h"

namespace acez {

__global__ __launch_bounds__(256) void gather_kernel(const uint16_t* __restrict__ feat, const int64_t* __restrict__ idx,
                                                     uint16_t* __restrict__ out, int n, const TrainState* st, GatherMeta meta) {
  if (st && !st->active) return;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  gather_rows(feat, idx, out, n, wave, nwaves, lane, meta);
}

template <class E = EltBf16>
__global__ __launch_bounds__(WGRAD_THREADS) void wgrad_kernel(WgradArgs a) {
  const int active = a.st ? a.st->active : 1;  // tested before the stores only (see rowgemm80_body)
  __shared__ __attribute__((aligned(16))) uint16_t smem[WGRAD_RING][2][64 * 128];
  const int l = threadIdx.x & 63;
  const int cw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 3, wn = cw >> 1, wc = cw & 1;
  // XCD-aware decode: the 16 output tiles of one (layer, slab) group re-read the same dZ / In rows (4x each); they
  // are placed on ONE XCD (workgroup b runs on XCD b % 8) so that the re-reads hit that XCD's L2 instead of the
  // fabric. Placement only affects speed.
  const int b = blockIdx.x;
  const int xcd = b & 7, jx = b >> 3;
  const int group = xcd + 8 * (jx >> 4), tile = jx & 15;
  if (group >= a.n_layers * a.nslabs) return;
  const int layer = group / a.nslabs, slab = group - layer * a.nslabs;
  const int n0 = (tile >> 2) * 128, c0 = (tile & 3) * 128;
  f32x16 acc[2][2];
  int KT;
  if (wgrad_kloop<E, 0>(a, smem, layer, slab, tile, acc, KT, [] {})) return;

  if (!active) return;
  float* __restrict__ G = a.slabs + (size_t)slab * a.slab_stride;
  const int h = l >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = c0 + wc * 64 + j * 32 + (l & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wn * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        G[a.w_off[layer] + (size_t)n * 512 + c] = acc[i][j][r];
      }
    }
}

__global__ __launch_bounds__(256) void grad_reduce_kernel(GradReduceArgs a) { grad_reduce_body(a, (int)blockIdx.x); }

__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) {
  __shared__ uint16_t tileT[64][66];
  adamw_body(a, blockIdx.x, tileT);
}

// W^T of wide layers layer_lo .. from their 16-bit W (acez_trainer_import_weights16: the sharded data-parallel update receives the
// other ranks' layers as 16-bit copies and derives the transposed operand of the input-gradient GEMM locally). One 64 x 64 tile per block.
__global__ __launch_bounds__(256) void transpose16_kernel(const uint16_t* __restrict__ Wb, uint16_t* __restrict__ WbT, int layer_lo) {
  __shared__ uint16_t tileT[64][66];
  const int t = threadIdx.x, b = blockIdx.x;
  const int layer = layer_lo + b / 64, tl = b % 64;
  const int r0 = (tl >> 3) * 64, c0 = (tl & 7) * 64, cc = (t & 15) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = (t >> 4) + 16 * i;
    const uint2 pk = *reinterpret_cast<const uint2*>(Wb + (size_t)layer * 262144 + (size_t)(r0 + rr) * 512 + c0 + cc);
    tileT[cc + 0][rr] = (uint16_t)(pk.x & 0xffff);
    tileT[cc + 1][rr] = (uint16_t)(pk.x >> 16);
    tileT[cc + 2][rr] = (uint16_t)(pk.y & 0xffff);
    tileT[cc + 3][rr] = (uint16_t)(pk.y >> 16);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = (t >> 4) + 16 * i;
    uint2 pk;
    pk.x = (uint32_t)tileT[rr][cc + 0] | ((uint32_t)tileT[rr][cc + 1] << 16);
    pk.y = (uint32_t)tileT[rr][cc + 2] | ((uint32_t)tileT[rr][cc + 3] << 16);
    *reinterpret_cast<uint2*>(WbT + (size_t)layer * 262144 + (size_t)(c0 + rr) * 512 + r0 + cc) = pk;
  }
}

// recast only (no optimiser step): used after loading weights
// The sharded data-parallel update in ONE launch on the receiving side: every wide layer OUTSIDE [own_lo, own_hi) is taken from the
// all-gather buffer `src` ([L][512][512] 16-bit, all ranks' layers) into W and, transposed, into W^T (the rank's own layers were written
// by its optimiser launch). Replaces one copy + one transpose launch per peer (2 (G - 1) small launches per step at G ranks).
__global__ __launch_bounds__(256) void import16_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ Wb, uint16_t* __restrict__ WbT,
                                                       int own_lo, int own_hi) {
  __shared__ uint16_t tileT[64][66];
  const int t = threadIdx.x, b = blockIdx.x;
  const int layer = b / 64, tl = b % 64;
  if (layer >= own_lo && layer < own_hi) return;
  const int r0 = (tl >> 3) * 64, c0 = (tl & 7) * 64, cc = (t & 15) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = (t >> 4) + 16 * i;
    const size_t o = (size_t)layer * 262144 + (size_t)(r0 + rr) * 512 + c0 + cc;
    const uint2 pk = *reinterpret_cast<const uint2*>(src + o);
    *reinterpret_cast<uint2*>(Wb + o) = pk;
    tileT[cc + 0][rr] = (uint16_t)(pk.x & 0xffff);
    tileT[cc + 1][rr] = (uint16_t)(pk.x >> 16);
    tileT[cc + 2][rr] = (uint16_t)(pk.y & 0xffff);
    tileT[cc + 3][rr] = (uint16_t)(pk.y >> 16);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = (t >> 4) + 16 * i;
    uint2 pk;
    pk.x = (uint32_t)tileT[rr][cc + 0] | ((uint32_t)tileT[rr][cc + 1] << 16);
    pk.y = (uint32_t)tileT[rr][cc + 2] | ((uint32_t)tileT[rr][cc + 3] << 16);
    *reinterpret_cast<uint2*>(WbT + (size_t)layer * 262144 + (size_t)(c0 + rr) * 512 + r0 + cc) = pk;
  }
}

__global__ __launch_bounds__(256) void recast_kernel(AdamArgs a) {
  __shared__ uint16_t tileT[64][66];
  const int t = threadIdx.x, b = blockIdx.x;
  if (b < a.n_layers * 64) {
    const int layer = b / 64, tl = b % 64;
    const int r0 = (tl >> 3) * 64, c0 = (tl & 7) * 64;
    const int64_t woff = a.w_off[layer];
    const int cc = (t & 15) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = (t >> 4) + 16 * i;
      const float4 p = *reinterpret_cast<const float4*>(a.params + woff + (int64_t)(r0 + rr) * 512 + c0 + cc);
      const uint2 pk = a.f16 ? EltF16::pk4(p.x, p.y, p.z, p.w) : pack4(p.x, p.y, p.z, p.w);
      *reinterpret_cast<uint2*>(a.Wb + (size_t)layer * 262144 + (size_t)(r0 + rr) * 512 + c0 + cc) = pk;
      tileT[cc + 0][rr] = (uint16_t)(pk.x & 0xffff);
      tileT[cc + 1][rr] = (uint16_t)(pk.x >> 16);
      tileT[cc + 2][rr] = (uint16_t)(pk.y & 0xffff);
      tileT[cc + 3][rr] = (uint16_t)(pk.y >> 16);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = (t >> 4) + 16 * i;
      uint2 pk;
      pk.x = (uint32_t)tileT[rr][cc + 0] | ((uint32_t)tileT[rr][cc + 1] << 16);
      pk.y = (uint32_t)tileT[rr][cc + 2] | ((uint32_t)tileT[rr][cc + 3] << 16);
      *reinterpret_cast<uint2*>(a.WbT + (size_t)layer * 262144 + (size_t)(c0 + rr) * 512 + r0 + cc) = pk;
    }
  } else {
    const int64_t k = (int64_t)(b - a.n_layers * 64) * 256 + t;
    if (k < (int64_t)a.no * 512) a.W3b[k] = a.f16 ? EltF16::from_f(a.params[a.fc3_off + k]) : f2bf(a.params[a.fc3_off + k]);
  }
}

// after a rowseq fall-back (head_api.hip seq_fault_check): the fault handler had cleared `active`; restore what sched_prepare would set
__global__ void sched_reactivate_kernel(TrainState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) st->active = (st->iteration < st->max_iterations && !st->nan_flag) ? 1 : 0;
}

// initial state: lr as left by the torch scheduler constructors (ace_schedule.py:12-70)
__global__ void sched_init_kernel(TrainState* st, SchedConfig c) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st->active = 0; st->iteration = 0; st->max_iterations = c.iterations; st->in_cooldown = 0;
  st->warmup_epoch = 0; st->cooldown_epoch = 0; st->nan_flag = 0; st->opt_steps = 0; st->crit_count = 0; st->crit_pos = 0;
  st->calib_steps = 0; st->loss_weight = c.soft_clamp; st->last_loss = 0.f; st->last_inliers = 0.f;
  st->calib_g = 0.0; st->calib_m = 0.0; st->calib_v = 0.0; st->beta1_pow = 1.0; st->beta2_pow = 1.0;
  st->pose_enable = 0; st->pose_opt_steps = 0; st->pose_b1pow = 1.0; st->pose_b2pow = 1.0;
  st->grad_scale = c.f16 ? 64.f : 1.f; st->inv_grad_scale = 1.f / st->grad_scale;   // (fp16: adapted after every step, sched_post_wave)
  for (int i = 0; i < 64; ++i) st->dz_absmax_slots[i * 32] = 0u;
  if (c.schedule == SCHED_CONSTANT) st->lr = c.lr_min;
  else if (c.schedule == SCHED_1CYCLEPOLY) st->lr = c.lr_max * (c.warmup_lr / c.lr_max);  // LinearLR._initial_step
  else st->lr = onecycle_lr(c, 0);
  sched_prepare(st, c, 0.f);
}

__global__ __launch_bounds__(64) void sched_post_kernel(const TrainState* src, TrainState* st, SchedConfig c, const float* grad_stats, float inv_global_batch,
                                                        float* log_loss, float* log_inl, int log_cap, const int* fault, const float* stat_partials,
                                                        int n_loss_blocks) {
  sched_post_wave(src, st, c, grad_stats, inv_global_batch, log_loss, log_inl, log_cap, fault, stat_partials, n_loss_blocks);
}

// step_begin: the batch gather of iteration i + 1 and, in ONE extra single-wave workgroup, the schedule bookkeeping that
// closes iteration i (the two are independent: the gather does not look at the schedule state; a gather into the scratch
// rows of an inactive step is harmless). Saves a dependent single-thread launch per step.
__global__ __launch_bounds__(256) void step_begin_kernel(const uint16_t* __restrict__ feat, const int64_t* __restrict__ idx,
                                                         uint16_t* __restrict__ out, int n, PostArgs p, GatherMeta meta) {
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x < 64) sched_post_wave(p.src, p.st, p.c, p.grad_stats, p.inv_global_batch, p.log_loss, p.log_inl, p.log_cap, p.fault, p.stat_partials, p.n_loss_blocks);
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = ((gridDim.x - 1) * blockDim.x) >> 6;
  gather_rows(feat, idx, out, n, wave, nwaves, lane, meta);
}

// The optimiser of step k, the batch gather of step k + 1 and the schedule bookkeeping that closes step k in ONE launch (single-GPU
// step with the next batch's indices known: acez_train_step_next). The three do not depend on each other: the bookkeeping reads the
// loss kernel's statistic partials and the state slot of step k and writes the OTHER slot (sched_post_wave), which only later launches
// read. Saves the step_begin launch (5 us + a kernel boundary) of every step: the gather hides under the HBM-bound optimiser.
// (First version: one slot, bookkeeping in the workgroup that finished last, found with a ticket counter -- 1700 atomics on one word
// cost 20 us.)   Grid: the gather blocks, the schedule wave, then adamw_kernel's n_adam blocks (order: below)
__global__ __launch_bounds__(256, 4) void adamw_next_kernel(AdamArgs a, int n_adam, const uint16_t* __restrict__ feat, const int64_t* __restrict__ idx_next,
                                                         uint16_t* __restrict__ out, int n_next, PostArgs p, GatherMeta meta) {
  __shared__ uint16_t tileT[64][66];
  // Grid order (round 6): the gather workgroups FIRST, then the schedule wave, then the optimiser's. The gather is a chain of three dependent
  // load levels (~7 us) and used to sit at the END of the grid, where its workgroups started when optimiser workgroups retired: the launch
  // was adamw_kernel's 12.2 us + 5.2. In front, the chain runs under the optimiser's HBM traffic from the first cycle. <= 128 VGPRs
  // (launch bounds): all 1024 workgroups of the launch are resident at once.
  const int b = (int)blockIdx.x;
  const int gblocks = (int)gridDim.x - 1 - n_adam;
  if (b < gblocks) {
    const int lane = threadIdx.x & 63;
    const int wave = (b * (int)blockDim.x + (int)threadIdx.x) >> 6;
    const int nwaves = (gblocks * (int)blockDim.x) >> 6;
    gather_rows(feat, idx_next, out, n_next, wave, nwaves, lane, meta);
    return;
  }
  if (b == gblocks) {
    if (threadIdx.x < 64) {
      // fused flow (a.slabs): the statistics are being reduced by sibling workgroups of this launch, the wave reduces the loss kernel's
      // partials itself; split flow (acez_train_update_next): they are in the bucket, reduced by grad_reduce_kernel and all-reduced since
      // (two call sites: a run-time choice between &a.tail and null makes the kernel arguments addressable -- the compiler copies them to
      // scratch, 680 bytes per lane, and the launch takes 51 us instead of 22)
      if (a.slabs) {
        sched_post_wave(p.src, p.st, p.c, p.grad_stats, p.inv_global_batch, p.log_loss, p.log_inl, p.log_cap, p.fault, p.stat_partials, p.n_loss_blocks, &a.tail);
      } else {
        sched_post_wave(p.src, p.st, p.c, p.grad_stats, p.inv_global_batch, p.log_loss, p.log_inl, p.log_cap, p.fault, p.stat_partials, p.n_loss_blocks);
      }
    }
    return;
  }
  adamw_body(a, b - gblocks - 1, tileT);
}

// ---------------------------------------------------------------------------------------------------
// wgrad_opt: wgrad_kernel's product with the optimiser step of the wide layers as its epilogue (single-GPU fused step). wgrad + adamw
// as two launches round-trip both split-K slabs through HBM (16.8 MB written, 16.8 MB read), start the optimiser's 25 MB of state
// reads only when the gradients are complete, and pay a kernel boundary; here
//  * both row slabs of a 128 x 128 tile are placed on ONE XCD (layer = XCD, 32 workgroups each for the default head). A workgroup
//    finalises the 64 x 128 half tile of its slab index: its two multiplier waves of the OTHER half store their accumulators to the
//    partner's exchange tile (this XCD's L2), wait for the acknowledgement and bump the partner's counter (two senders per word, so a
//    counter and not rowseq_kernel's progress words: seq_bump, seq_poll_word_expired) --
//    L2-local atomic, bounded sc1 poll on the other side, no fence, nothing read before it is produced;
//  * the eight loader waves, idle once the last stage is requested, fetch p, m, v of the half tile a dozen stages before the K loop
//    ends, then poll, add own (through LDS) + partner partial in slab order (slab 0 + slab 1: the additions of grad_reduce_kernel /
//    adamw_body, so the parameters are bitwise those of backward + update), apply adamw_one and store p, m, v, W and -- through an
//    LDS transpose -- W^T.
// The guards are adamw_body's (schedule inactive, chain fault, NaN loss, fp16 overflow: nothing is stored); the exchange itself is
// unconditional, so the two partners never disagree about it. A poll that expires raises the trainer's fault word exactly like a
// rowseq hand-off (the host falls back to wgrad_kernel + adamw_kernel at its next state read); the stores of that wave are skipped.
// Host: only when the grid fits the CUs (every workgroup resident) and the placement probe has passed (head_api.hip).
// The four multiplier waves of a workgroup have nothing to do while its loader waves run the optimiser arithmetic (~3.5 us of VALU work
// per CU): in the first `nsmall` workgroups they are the small-parameter workgroups of the optimiser launch (adamw_small_columns: biases,
// fc3, statistics), and wave 0 of the last workgroup is the schedule wave that closes the step (do_post) -- with the next batch
// gathered beside the loss kernel (loss_gather_kernel), a step without pose refinement has no optimiser launch left at all.
// ---------------------------------------------------------------------------------------------------
constexpr int WGO_PF = 17;   // prefetch loads per loader lane: 4 x (p, m, v) float4 + the first five rows of the loss partials
#ifdef ACEZ_DIAG   // timeline of the epilogue (tools/wgo_trace.py): stamp i of this wave
#define WGO_STAMP(i) do { if (o.trace && (threadIdx.x & 63) == 0) o.trace[((size_t)blockIdx.x * 12 + (threadIdx.x >> 6)) * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define WGO_STAMP(i) do { } while (0)
#endif
template <class E = EltBf16>
__global__ __launch_bounds__(WGRAD_THREADS) void wgrad_opt_kernel(WgradArgs a, WgradOptArgs o, PostArgs post) {
  constexpr int RING = WGRAD_RING;
  static_assert(RING >= 3, "two free ring slots are used as staging areas after the K loop");
  __shared__ __attribute__((aligned(16))) uint16_t smem[RING][2][64 * 128];
  __shared__ uint32_t wsync[2];   // [0]: multiplier waves that have staged their accumulators, [1]: loader waves that have written their W^T rows
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  // workgroup b runs on XCD b % 8: both slabs of all 16 tiles of a layer on one XCD (placement affects speed AND the hand-off, hence the probe)
  const int b = blockIdx.x;
  const int xcd = b & 7, jx = b >> 3;
  const int layer = xcd + 8 * (jx >> 5), slab = (jx >> 4) & 1, tile = jx & 15;
  if (layer >= a.n_layers) return;
  if (t < 2) wsync[t] = 0;   // (ordered before its first use by the barriers of the K loop; a slab without rows has none)
  WGO_STAMP(0);   // kernel entry
  const int n0 = (tile >> 2) * 128, c0 = (tile & 3) * 128;
  const AdamArgs& ad = o.ad;
  // this lane's share of the workgroup's 64 x 128 half tile in the epilogue (loader waves): rows rb + 16 i, columns col4 .. col4 + 3
  const int e = t - 256, rb = e >> 5, col4 = (e & 31) * 4;
  const int64_t woff = ad.w_off[layer];
  const int nrow0 = n0 + 64 * slab;   // first row of the half tile this workgroup finalises
  float4 p4[4], m4[4], v4[4];
  float lp[5];   // the loss partials tail_output reads first (NaN guard)
  uint32_t amx = 0u, amxm = 0u;   // fp16: this lane's stripe of the step's largest propagated gradient (final before this launch), prefetched with p / m / v
  const int nlb = ad.tail.n_loss_blocks;
  auto prefetch = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t off = woff + (int64_t)(nrow0 + rb + 16 * i) * 512 + c0 + col4;
      p4[i] = *reinterpret_cast<const float4*>(ad.params + off);
      m4[i] = *reinterpret_cast<const float4*>(ad.m + off);
      v4[i] = *reinterpret_cast<const float4*>(ad.v + off);
    }
#pragma unroll
    for (int u = 0; u < 5; ++u) lp[u] = ad.tail.stat_partials[(size_t)min(l + 64 * u, max(nlb - 1, 0)) * 4];
    if (E::is_f16) amx = __builtin_nontemporal_load(&ad.st->dz_absmax_slots[l * 32]);
  };
  // the multiplier waves' small-parameter share (workgroups b < nsmall): requested once the accumulators are on their way. (In front of
  // the send it delayed every exchange by the 2.5 us the requests take to issue -- tools/wgo_trace.py; from inside the K loop, two or
  // eight stages before its end, it bought nothing or stalled the loop on the loaded registers one iteration later: measured, round 4.)
  SmallCols<8> sm;
  float lpm[5];
  const bool do_small = b < o.nsmall;
  auto mprefetch = [&]() {
    if (do_small) {
      sm.issue(ad.tail, small_opt(ad), b);
#pragma unroll
      for (int u = 0; u < 5; ++u) lpm[u] = ad.tail.stat_partials[(size_t)min(l + 64 * u, max(nlb - 1, 0)) * 4];
      if (E::is_f16) amxm = __builtin_nontemporal_load(&ad.st->dz_absmax_slots[l * 32]);
    }
  };
  // the sum of the loss partials from five prefetched rows per lane: ONLY its NaN-ness is used (the guard tail_output applies to the step;
  // the logged loss is tail_output's own fixed-order sum), so the cross-lane part is a DPP sum + one v_readlane instead of six ds_bpermute
  // rounds on every wave's path from the K loop to its epilogue (a NaN stays a NaN in any order; the partials are >= 0)
  auto loss_sum = [&](const float (&v5)[5]) {
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < 5; ++u)
      if (l + 64 * u < nlb) sum += v5[u];
    for (int r = l + 320; r < nlb; r += 64) sum += ad.tail.stat_partials[(size_t)r * 4];
    sum = wave_sum63(sum);
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(sum), 63));
  };
  f32x16 acc[2][2];
  int KT;
  const bool loader = wgrad_kloop<E, WGO_PF + (E::is_f16 ? 1 : 0)>(a, smem, layer, slab, tile, acc, KT, prefetch);   // (fp16: + the absmax stripe)
  if (KT == 0) __builtin_amdgcn_s_barrier();   // (wsync)
  WGO_STAMP(1);   // K loop done
  // Slot KT % RING was last written for stage KT - RING and slot (KT + 1) % RING for stage KT - RING + 1: every wave is past the barrier
  // of stage KT - 1, i.e. done with both; the slot of stage KT - 1 itself may still be read by a slower multiplier wave.
  float* const stage = reinterpret_cast<float*>(&smem[KT % RING][0][0]);                                  // [64][128] fp32: own partial
  uint16_t (*const tileT)[66] = reinterpret_cast<uint16_t (*)[66]>(&smem[(KT + 1) % RING][0][0]);         // [128][66]: W^T staging
  const int pair = layer * 16 + tile;
  const TrainState* st = ad.st;
  if (!loader) {
    const int cw = w & 3, wn = cw >> 1, wc = cw & 1, h = l >> 5;
    if (wn != slab) {
      float* __restrict__ X = o.xch + (size_t)(pair * 2 + (1 - slab)) * 8192;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            X[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 128 + wc * 64 + j * 32 + (l & 31)] = acc[i][j][r];
      ACEZ_VMCNT(0);   // acknowledged by the L2 both workgroups share
      if (l == 0) seq_bump(o.flags + (size_t)(pair * 2 + (1 - slab)) * 32, 1u);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            stage[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 128 + wc * 64 + j * 32 + (l & 31)] = acc[i][j][r];
      lds_bump(&wsync[0]);   // the own half is in LDS (two waves)
    }
    WGO_STAMP(2);   // multipliers: accumulators sent (acknowledged) / staged
    mprefetch();
    // from here on the multiplier waves are free: the small parameters and the schedule wave run beside the loader waves' arithmetic
    if (do_small) {   // this workgroup's share of the small parameters, under adamw_body's guards
      const int active = st->active;
      const AdamScalars sc = st->adam;
      const int fault_now = *ad.fault;
      sm.finish(ad.tail, small_opt(ad), b, sc, [&] {
        const float lossv = loss_sum(lpm);
        bool skip = !active || fault_now || lossv != lossv;
        if (E::is_f16) skip = skip || f16_overflow(absmax_reduce(amxm));
        return skip;
      });
    }
    WGO_STAMP(3);   // multipliers: small parameters done
    if (o.do_post && b == (int)gridDim.x - 1 && w == 0)
      sched_post_wave(post.src, post.st, post.c, post.grad_stats, post.inv_global_batch, post.log_loss, post.log_inl, post.log_cap, post.fault,
                      post.stat_partials, post.n_loss_blocks, &ad.tail);
    WGO_STAMP(4);   // multipliers: (schedule wave) done
    return;
  }
  // ------------------------------------------------------------------ loader waves: the optimiser step of the half tile
  const int active = st->active;
  const AdamScalars s = st->adam;
  const float inv_scale = st->inv_grad_scale;
  const int fault_now = *ad.fault;
  const float lossv = loss_sum(lp);
  bool skip = !active || fault_now || lossv != lossv;   // adamw_body's guards
  if (E::is_f16) skip = skip || f16_overflow(absmax_reduce(amx));
  const bool skip_by_guard = skip;   // (uniform over the launch: every wave evaluates the same words)
  const uint32_t* flag = o.flags + (size_t)(pair * 2 + slab) * 32;
  uint32_t wgo_target = o.target;
#ifdef ACEZ_DIAG   // fault injection in SOME workgroups (ACEZ_WGO_FAULT_MOD): a partially applied step
  if (o.fault_mod > 0 && b % o.fault_mod == 1) wgo_target += 1u << 20;
#endif
  if (seq_poll_word_expired(flag, wgo_target, o.spin_limit)) {   // the partner never arrived (the two slabs of a tile are not on one XCD after all): fault word, step switched off
    skip = true;
    if (l == 0) {
      // What the host needs to finish this step (wgo_recover, head_api.hip): which rows were not updated, and with what they would have
      // been. The small parameters and the schedule wave of this launch read the fault word long before it is raised and DO apply the
      // step; tiles whose exchange completed are updated too -- so the fall-back completes the step instead of undoing it. Every kernel
      // of the trainer that writes a step's buffers returns at entry while the word is set: the operands are still there.
      if (!skip_by_guard && o.status) {
        o.status[(size_t)b * WGRAD_LOADERS + (w - 4)] = o.epoch * 4u + 3u;
        o.rec->s = s; o.rec->inv_scale = inv_scale; o.rec->M = a.M; o.rec->in0 = a.In[0];
        __hip_atomic_store(&o.rec->epoch, o.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      seq_raise_fault(reinterpret_cast<uint32_t*>(ad.fault), st);
    }
  }
  WGO_STAMP(2);   // loaders: guards evaluated, partner's counter seen
  float4 oth[4];
  {
    const float* __restrict__ Xin = o.xch + (size_t)(pair * 2 + slab) * 8192;
#pragma unroll
    for (int i = 0; i < 4; ++i) oth[i] = *reinterpret_cast<const float4*>(Xin + (rb + 16 * i) * 128 + col4);
  }
  lds_wait_ge(&wsync[0], 2);   // the own half is in LDS
  WGO_STAMP(3);   // loaders: own half staged (the partner's half is still in flight)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = rb + 16 * i;
    const float4 own = *reinterpret_cast<const float4*>(stage + row * 128 + col4);
    // slab 0 + slab 1 (fp32 addition commutes: the same bits whichever of the two is `own`), then the un-scaling of the fp16 chain
    float4 g;
    g.x = (own.x + oth[i].x) * inv_scale; g.y = (own.y + oth[i].y) * inv_scale;
    g.z = (own.z + oth[i].z) * inv_scale; g.w = (own.w + oth[i].w) * inv_scale;
    float4 p = p4[i], m = m4[i], v = v4[i];
    p.x = adamw_one(p.x, g.x, m.x, v.x, s);
    p.y = adamw_one(p.y, g.y, m.y, v.y, s);
    p.z = adamw_one(p.z, g.z, m.z, v.z, s);
    p.w = adamw_one(p.w, g.w, m.w, v.w, s);
    const uint2 pk = E::pk4(p.x, p.y, p.z, p.w);
    if (!skip) {
      const int64_t off = woff + (int64_t)(nrow0 + row) * 512 + c0 + col4;
      *reinterpret_cast<float4*>(ad.params + off) = p;
      *reinterpret_cast<float4*>(ad.m + off) = m;
      *reinterpret_cast<float4*>(ad.v + off) = v;
      *reinterpret_cast<uint2*>(ad.Wb + (size_t)layer * 262144 + (size_t)(nrow0 + row) * 512 + c0 + col4) = pk;
    }
    tileT[col4 + 0][row] = (uint16_t)(pk.x & 0xffff);
    tileT[col4 + 1][row] = (uint16_t)(pk.x >> 16);
    tileT[col4 + 2][row] = (uint16_t)(pk.y & 0xffff);
    tileT[col4 + 3][row] = (uint16_t)(pk.y >> 16);
  }
  WGO_STAMP(4);   // loaders: optimiser arithmetic done, p / m / v / W stores issued
  lds_bump(&wsync[1]);
  lds_wait_ge(&wsync[1], WGRAD_LOADERS);   // every loader wave's rows of the transpose tile
  WGO_STAMP(5);   // loaders: all eight waves' transpose rows written
  {
    // W^T: row c0 + cl holds the 64 values n = nrow0 .. nrow0 + 63 of column cl: 128 contiguous bytes, 32 per lane
    const int cl = e >> 2, part = e & 3;
    uint32_t q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = (uint32_t)tileT[cl][part * 16 + 2 * k] | ((uint32_t)tileT[cl][part * 16 + 2 * k + 1] << 16);
    // skip_by_guard, not skip: a wave whose own poll timed out still stores its W^T COLUMNS -- they hold the rows of the waves of this
    // workgroup that did complete (their W / parameter rows were stored above); its own rows of every column are rewritten by
    // wgo_recover_kernel. (With `skip` here a partial time-out inside one workgroup left W^T old where W was new.)
    if (!skip_by_guard) {
      uint16_t* dst = ad.WbT + (size_t)layer * 262144 + (size_t)(c0 + cl) * 512 + nrow0 + part * 16;
      *reinterpret_cast<uint4*>(dst) = make_uint4(q[0], q[1], q[2], q[3]);
      *reinterpret_cast<uint4*>(dst + 8) = make_uint4(q[4], q[5], q[6], q[7]);
    }
  }
#ifdef ACEZ_DIAG
  if (o.trace) { ACEZ_VMCNT(0); WGO_STAMP(6); }   // loaders: every store of this wave acknowledged
#endif
}

// The rows of wgrad_opt_kernel's half tiles whose loader wave timed out in launch rec->epoch (WgradOptArgs::status), finished from the
// slabs wgrad_kernel has just recomputed on the faulted step's untouched buffers: slab 0 + slab 1, the step's own AdamW scalars and
// gradient scale, adamw_one -- the arithmetic of the wave that gave up, so the parameters end up bitwise those of the two-launch flow.
// Same grid decode and the same lane -> (row, column) map as wgrad_opt_kernel's loader waves; one 512-thread workgroup per half tile.
template <class E = EltBf16>
__global__ __launch_bounds__(512) void wgo_recover_kernel(AdamArgs ad, const float* __restrict__ slabs, int64_t slab_stride, const uint32_t* __restrict__ status,
                                                          const WgoFaultRec* __restrict__ rec, int n_layers) {
  const int t = threadIdx.x, l = t & 63, lw = t >> 6;
  const int b = blockIdx.x;
  const int xcd = b & 7, jx = b >> 3;
  const int layer = xcd + 8 * (jx >> 5), slab = (jx >> 4) & 1, tile = jx & 15;
  if (layer >= n_layers) return;
  if (status[(size_t)b * WGRAD_LOADERS + lw] != rec->epoch * 4u + 3u) return;
  const AdamScalars s = rec->s;
  const float inv_scale = rec->inv_scale;
  const int n0 = (tile >> 2) * 128, c0 = (tile & 3) * 128;
  const int e = t, rb = e >> 5, col4 = (e & 31) * 4;
  const int64_t woff = ad.w_off[layer];
  const int nrow0 = n0 + 64 * slab;
  (void)l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = rb + 16 * i;
    const int64_t off = woff + (int64_t)(nrow0 + row) * 512 + c0 + col4;
    const float4 s0 = *reinterpret_cast<const float4*>(slabs + off);
    const float4 s1 = *reinterpret_cast<const float4*>(slabs + slab_stride + off);
    float4 g;
    g.x = (s0.x + s1.x) * inv_scale; g.y = (s0.y + s1.y) * inv_scale; g.z = (s0.z + s1.z) * inv_scale; g.w = (s0.w + s1.w) * inv_scale;
    float4 p = *reinterpret_cast<const float4*>(ad.params + off), m = *reinterpret_cast<const float4*>(ad.m + off), v = *reinterpret_cast<const float4*>(ad.v + off);
    p.x = adamw_one(p.x, g.x, m.x, v.x, s);
    p.y = adamw_one(p.y, g.y, m.y, v.y, s);
    p.z = adamw_one(p.z, g.z, m.z, v.z, s);
    p.w = adamw_one(p.w, g.w, m.w, v.w, s);
    const uint2 pk = E::pk4(p.x, p.y, p.z, p.w);
    *reinterpret_cast<float4*>(ad.params + off) = p;
    *reinterpret_cast<float4*>(ad.m + off) = m;
    *reinterpret_cast<float4*>(ad.v + off) = v;
    *reinterpret_cast<uint2*>(ad.Wb + (size_t)layer * 262144 + (size_t)(nrow0 + row) * 512 + c0 + col4) = pk;
    uint16_t* wt = ad.WbT + (size_t)layer * 262144 + (size_t)(c0 + col4) * 512 + nrow0 + row;
    wt[0] = (uint16_t)(pk.x & 0xffff); wt[512] = (uint16_t)(pk.x >> 16); wt[1024] = (uint16_t)(pk.y & 0xffff); wt[1536] = (uint16_t)(pk.y >> 16);
  }
}

// the product's instantiations (head_kernels.h)
ACEZ_OPTIM_KERNELS(template __global__, EltBf16)
ACEZ_OPTIM_KERNELS(template __global__, EltF16)

}  // namespace acez

#include "pose_fused.hip"   // the pose network's launches: they call the bodies above
