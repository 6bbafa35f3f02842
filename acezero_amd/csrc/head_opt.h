// head_opt.h -- the optimiser bodies: the fixed-order reduction of a step's partials and AdamW, shared by grad_reduce_kernel, adamw_kernel,
// adamw_next_kernel, wgrad_opt_kernel (head_optim.hip) and the pose launches that carry them (pose_fused.hip).
#pragma once
#include "head_gather.h"

namespace acez {

// ---------------------------------------------------------------------------------------------------
// grad_reduce: flat gradient = fixed-order sum of the wgrad slabs (wide layers) and of the per-workgroup
// partials of the loss kernel (fc3 + statistics). Deterministic: no atomics anywhere in the step.
// ---------------------------------------------------------------------------------------------------
// tail outputs, one wavefront per output: the biases of the wide layers (column-sum partials written where each dZ is
// produced), fc3 weights/bias, then the 4 statistics. Lane-strided partial sums followed by the fixed butterfly order:
// deterministic; every lane returns the sum. (A two-level "32 outputs x 8 groups" variant with coalesced reads measured
// 2-4x slower: its 80-deep dependent add chains are latency bound.) Shared by grad_reduce_kernel and the fused adamw_kernel.
__device__ __forceinline__ float tail_output(const GradReduceArgs& a, int64_t k, int lane, int64_t& dst) {
  const int64_t n_bias = (int64_t)a.n_layers * 512;
  const int64_t n_fc3 = a.n_params - a.n_wide;
  float acc = 0.f;
  if (k < n_bias) {
    const int layer = (int)(k >> 9), c = (int)(k & 511);
    const float* p = a.bias_partials + (size_t)layer * a.bias_layer_stride + c;
    const int cnt = a.bias_count[layer];
    for (int b = lane; b < cnt; b += 64) acc += p[(size_t)b * 512];
    dst = (int64_t)layer * 262656 + 262144 + c;
  } else if (k < n_bias + n_fc3) {
    const int64_t kk = k - n_bias;
    for (int b = lane; b < a.n_loss_blocks; b += 64) acc += a.fc3_partials[(size_t)b * a.fc3_stride + kk];
    dst = a.n_wide + kk;
  } else {
    const int64_t kk = k - n_bias - n_fc3;
    if (kk < 3) {
      // every wave of the fused optimiser sums the loss for itself (NaN check) before it may store: the first 320 partial rows in ONE
      // memory round trip (a loop of dependent load -> add rounds cost the optimiser 1 us per 64 rows); same additions, same order
      float v[5];
#pragma unroll
      for (int u = 0; u < 5; ++u) {
        const int b = lane + 64 * u;
        const float x = a.stat_partials[(size_t)min(b, max(a.n_loss_blocks - 1, 0)) * 4 + kk];
        v[u] = b < a.n_loss_blocks ? x : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 5; ++u)
        if (lane + 64 * u < a.n_loss_blocks) acc += v[u];
      for (int b = lane + 320; b < a.n_loss_blocks; b += 64) acc += a.stat_partials[(size_t)b * 4 + kk];
    }
    // slot 3: this rank's rowseq fault word. It rides in the all-reduced bucket, so that a fault on ONE rank makes EVERY rank skip
    // the optimiser step (adamw_kernel) and the replicas stay identical
    else if (a.fault) {
      const uint32_t amax_bits = absmax_all(a.st, lane);
      if (lane == 0) acc = (*a.fault ? 1.f : 0.f) + (f16_overflow(amax_bits) ? 1024.f : 0.f);   // (+ fp16 overflow)
    }
    dst = a.n_params + kk;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
  return k < n_bias + n_fc3 ? acc * a.st->inv_grad_scale : acc;   // (fp16: gradients arrive scaled; 1 for bf16, an exact product)
}

// (grad_reduce_body follows SmallCols below: its tail is reduced with it)

// ---------------------------------------------------------------------------------------------------
// adamw: torch.optim.AdamW single-tensor semantics on the flat fp32 masters, fused with the bf16 recast of
// W and W^T. One workgroup per 64 x 64 weight tile (transposed copy staged through LDS); the biases and
// fc3 are handled by the trailing workgroups.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float adamw_one(float p, float g, float& m, float& v, const AdamScalars& s) {
  // no fma contraction here: the function is inlined at several sites (tile path, small-parameter path, fused path) and
  // every site must round identically -- acez_train_step is bitwise equal to backward + update
#pragma clang fp contract(off)
  p = p * s.decay;                       // p.mul_(1 - lr * wd)
  m = m + (g - m) * s.one_minus_beta1;   // exp_avg.lerp_(grad, 1 - beta1)
  v = v * s.beta2 + s.one_minus_beta2 * g * g;
  const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
  return p - s.step_size * (m / denom);
}

// The small parameters of the fused step (biases of the wide layers, fc3) and the four statistics: 64 consecutive outputs per
// workgroup, FOUR lanes (a DPP quad) per output. An output is a column sum over partial rows (one per row tile of the GEMM chain, or per
// workgroup of the loss kernel): a load instruction of a wavefront reads 16 adjacent columns of 4 rows -- four full 64-byte lines --
// where tail_output (a wavefront per output, lanes striding the ROWS; round 3's tail_output8: eight outputs) touches 64 different lines with every instruction:
// 193 workgroups of those were the long pole of the optimiser launch (18 us by themselves at batch 5120, against 9.5 us for gather +
// schedule; round 4). The summation ORDER is tail_output's, so the bits are: partial j = rows j, j + 64, ... added in that order, then
// the xor butterfly 32, 16, ..., 1, which pairs partial j with j ^ off at every level -- a fixed binary tree (addition commutes). Lane q
// of the quad holds the partials j = 4 i + q: the levels 32 .. 4 pair i with i ^ 8, 4, 2, 1 inside the lane's registers, the levels 2
// and 1 are two quad permutes.
// LPO lanes per output (4, or 8: half the registers per lane -- wgrad_opt_kernel's multiplier waves request the rows from inside their
// K loop and keep them in registers next to the accumulators): lane q holds the partials j = LPO i + q; the butterfly levels that pair
// i with i ^ (32 / LPO), ... , 1 run in the lane's registers, the last log2(LPO) levels across the lanes of the output.
// issue() requests everything (p, m, v of the parameter and the first 320 partial rows: ONE memory round trip -- as a loop of
// load-then-add rounds the five rounds of the fc3 columns were five dependent round trips, 7 us); finish() reduces, applies the
// optimiser and stores. `late_skip()` (wgrad_opt_kernel: adamw_body's guards) is evaluated inside finish() before anything is stored.
// where the optimiser of the small parameters lives (null params: reduce only -- grad_reduce_kernel's tail)
struct SmallOpt {
  float *params, *m, *v;
  uint16_t* W3b;
  const int64_t* b_off;
  int64_t fc3_off;
  int no, f16;
};
__device__ __forceinline__ SmallOpt small_opt(const AdamArgs& a) { return SmallOpt{a.params, a.m, a.v, a.W3b, a.b_off, a.fc3_off, a.no, a.f16}; }
template <int LPO>
struct SmallCols {
  static_assert(LPO == 4 || LPO == 8, "lanes per output");
  static constexpr int NI = 64 / LPO, TD = 5, PER_BLOCK = 256 / LPO;   // partials per lane; 64-row rounds requested at once; outputs per 256 threads
  float x[TD][NI];
  float p, m, v;
  struct Col {
    const float* base;
    int cnt;
    int64_t stride, dst, ome, k;
  };
  static __device__ __forceinline__ Col decode(const GradReduceArgs& r, const SmallOpt& o, const int b) {
    const int64_t n_bias = (int64_t)r.n_layers * 512, n_fc3 = r.n_params - r.n_wide, n_out = n_bias + n_fc3 + 4;
    Col c;
    c.k = (int64_t)b * PER_BLOCK + ((int)threadIdx.x / LPO);
    c.base = r.stat_partials; c.cnt = 0; c.stride = 0; c.dst = -1; c.ome = -1;
    if (c.k < n_bias) {
      // (the outputs of a wavefront never straddle a layer -- 512 is a multiple of the outputs per wavefront --, so the layer is a scalar:
      // bias_count[layer] / b_off[layer] become scalar loads of the kernel arguments instead of a per-lane load the addresses below wait for)
      const int layer = __builtin_amdgcn_readfirstlane((int)(c.k >> 9)), col = (int)(c.k & 511);
      c.base = r.bias_partials + (size_t)layer * r.bias_layer_stride + col; c.cnt = r.bias_count[layer]; c.stride = 512;
      c.dst = (int64_t)layer * 262656 + 262144 + col;
      if (o.params) c.ome = o.b_off[layer] + col;
    } else if (c.k < n_bias + n_fc3) {
      c.base = r.fc3_partials + (c.k - n_bias); c.cnt = r.n_loss_blocks; c.stride = r.fc3_stride;
      c.dst = r.n_wide + (c.k - n_bias);
      if (o.params) c.ome = o.fc3_off + (c.k - n_bias);
    } else if (c.k < n_out) {
      const int64_t kk = c.k - n_bias - n_fc3;
      if (kk < 3) { c.base = r.stat_partials + kk; c.cnt = r.n_loss_blocks; c.stride = 4; }
      c.dst = r.n_params + kk;
    }
    return c;
  }
  __device__ __forceinline__ void issue(const GradReduceArgs& r, const SmallOpt& o, const int b) {
    const int q = (int)threadIdx.x & (LPO - 1);
    const Col c = decode(r, o, b);
    p = 0.f; m = 0.f; v = 0.f;
    if (q == 0 && c.ome >= 0) { p = o.params[c.ome]; m = o.m[c.ome]; v = o.v[c.ome]; }
    const int last = max(c.cnt - 1, 0);
#pragma unroll
    for (int u = 0; u < TD; ++u) {
      if (__any(64 * u < c.cnt)) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int row = 64 * u + LPO * i + q;
          const float y = c.base[(size_t)min(row, last) * c.stride];   // unconditional load, masked afterwards
          x[u][i] = row < c.cnt ? y : 0.f;
        }
      } else {
#pragma unroll
        for (int i = 0; i < NI; ++i) x[u][i] = 0.f;
      }
    }
  }
  template <class G>
  __device__ __forceinline__ void finish(const GradReduceArgs& r, const SmallOpt& o, const int b, const AdamScalars& s, G&& late_skip) {
    const int lane = (int)threadIdx.x & 63, q = (int)threadIdx.x & (LPO - 1);
    const int64_t n_bias = (int64_t)r.n_layers * 512, n_fc3 = r.n_params - r.n_wide, n_out = n_bias + n_fc3 + 4;
    const Col c = decode(r, o, b);
    const bool skip = late_skip();
    float acc[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i] = 0.f;
#pragma unroll
    for (int u = 0; u < TD; ++u)
#pragma unroll
      for (int i = 0; i < NI; ++i) acc[i] += x[u][i];   // (+0.f where tail_output adds nothing: acc is never -0, so the bits are the same)
    const int last = max(c.cnt - 1, 0);
    for (int u = TD; __any(64 * u < c.cnt); ++u) {
      float y[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int row = 64 * u + LPO * i + q;
        const float z = c.base[(size_t)min(row, last) * c.stride];
        y[i] = row < c.cnt ? z : 0.f;
      }
#pragma unroll
      for (int i = 0; i < NI; ++i) acc[i] += y[i];
    }
#pragma unroll
    for (int off = NI / 2; off >= 1; off >>= 1)
#pragma unroll
      for (int i = 0; i < off; ++i) acc[i] = acc[i] + acc[i + off];
    float g = acc[0];
    if (LPO == 8) g = g + __shfl_xor(g, 4);   // butterfly level 4
    g = ACEZ_DPP_ADD(g, 0x4E, 0xF);           // quad_perm [2,3,0,1]: butterfly level 2
    g = ACEZ_DPP_ADD(g, 0xB1, 0xF);           // quad_perm [1,0,3,2]: butterfly level 1
    if (b == (int)((n_out - 1) / PER_BLOCK) && r.fault) {   // statistics slot 3: the fault word + the fp16 overflow flag (see tail_output)
      const uint32_t amax_bits = absmax_all(r.st, lane);
      if (c.k == n_out - 1) g = (*r.fault ? 1.f : 0.f) + (f16_overflow(amax_bits) ? 1024.f : 0.f);
    }
    if (c.k < n_bias + n_fc3) g *= r.st->inv_grad_scale;   // (fp16: gradients arrive scaled; 1 for bf16, an exact product)
    if (q != 0 || c.dst < 0 || skip) return;
    r.grad[c.dst] = g;
    if (c.ome >= 0) {
      float pp = p, mm = m, vv = v;
      pp = adamw_one(pp, g, mm, vv, s);
      o.params[c.ome] = pp; o.m[c.ome] = mm; o.v[c.ome] = vv;
      const int64_t kf = c.k - n_bias;
      if (kf >= 0 && kf < (int64_t)o.no * 512) o.W3b[kf] = o.f16 ? EltF16::from_f(pp) : f2bf(pp);
    }
  }
};
__device__ __forceinline__ void adamw_small_columns(const AdamArgs& a, const int b, const AdamScalars& s) {
  SmallCols<4> sm;
  const SmallOpt o = small_opt(a);
  sm.issue(a.tail, o, b);
  sm.finish(a.tail, o, b, s, [] { return false; });
}

// Grid: the tail workgroups FIRST (GR_TAIL_LANES lanes per output: biases, fc3, statistics), then the wide part (split flow only). The tail is the
// launch's long pole -- every lane sums up to 80 partials behind two load levels -- and, dispatched behind the 2052 wide workgroups, it
// started when those were done; every load of a workgroup is requested before the schedule's `active` word is looked at (three dependent
// round trips per workgroup of a launch that is one wave of workgroups long). Round 6: 18.4 -> see profiles/r06_dp_host_probe.log.
__device__ __forceinline__ void grad_reduce_body(const GradReduceArgs& a, const int b) {
  const int tail_blocks = grad_reduce_tail_blocks(a.n_layers, a.n_params - a.n_wide);
  if (b >= tail_blocks) {  // weights: 16-byte loads, slabs summed in slab order
    const int64_t i4 = ((int64_t)(b - tail_blocks) * 256 + threadIdx.x) * 4;
    if (a.skip_wide || i4 >= a.n_wide) return;
    if ((i4 % 262656) >= 262144) return;  // bias slots are produced by the tail path
    float4 acc = *reinterpret_cast<const float4*>(a.slabs + i4);
    float4 v1 = acc;
    if (a.nslabs > 1) v1 = *reinterpret_cast<const float4*>(a.slabs + (size_t)a.slab_stride + i4);
    const int active = a.st ? a.st->active : 1;
    const float inv = a.st->inv_grad_scale;
    if (!active) return;   // (a rowseq fault of this step: the tail's first workgroup raises statistics slot 3)
    for (int s = 1; s < a.nslabs; ++s) {
      const float4 v = s == 1 ? v1 : *reinterpret_cast<const float4*>(a.slabs + (size_t)s * a.slab_stride + i4);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
    *reinterpret_cast<float4*>(a.grad + i4) = acc;
    return;
  }
  // the tail: 64 outputs per workgroup, four lanes each, coalesced partial-row reads (SmallCols: tail_output's summation order, the same bits;
  // a wavefront per output -- 1538 workgroups whose lanes stride the partial ROWS -- touched 64 cache lines with every load)
  SmallCols<GR_TAIL_LANES> sm;
  const SmallOpt none{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
  sm.issue(a, none, b);
  if (a.st && !a.st->active) {
    // switched off by a rowseq fault in THIS step (not by the end of the schedule): the bucket keeps whatever it held, but statistics
    // slot 3 must still tell the other ranks, which then all skip the optimiser step
    if (a.fault && *a.fault && b == 0 && threadIdx.x == 0) a.grad[a.n_params + 3] = 1.f;
    return;
  }
  sm.finish(a, none, b, AdamScalars{}, [] { return false; });
}

// One workgroup's share of the optimiser step (b = workgroup index inside the optimiser's part of a launch; tileT: 64 x 66 bf16 LDS).
// The body of adamw_kernel and of adamw_pose_kernel (pose_fused.hip), where the pose network's backward runs beside it.
__device__ __forceinline__ void adamw_body(const AdamArgs& a, const int b, uint16_t (*tileT)[66]) {
  const TrainState* st = a.st;
  const int t = threadIdx.x;
  const int nsmall = adamw_small_blocks(a.n_layers, a.n_fc3, a.slabs != nullptr);
  const bool tile = b >= nsmall;
  // ---- tile blocks: every load of the 64 x 64 tile is issued FIRST (before the loss reduction below, which is a memory round trip
  // of its own, and before any store: written as one load / compute / store loop per row group, the loads of row group i + 1 could
  // not be moved above the stores of row group i -- same arrays, no alias information -- and a workgroup made four dependent round
  // trips instead of one)
  const int tb = b - nsmall, layer = tile ? a.layer_lo + tb / 64 : 0, tl = tb % 64;   // (tile blocks cover layers layer_lo .. layer_hi - 1)
  const int r0 = (tl >> 3) * 64, c0 = (tl & 7) * 64, cc = (t & 15) * 4;
  const int64_t woff = a.w_off[layer];
  float4 p4[4], g4[4], m4[4], v4[4], q1[4];
  if (tile) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = (t >> 4) + 16 * i;
      const int64_t o = woff + (int64_t)(r0 + rr) * 512 + c0 + cc;
      p4[i] = *reinterpret_cast<const float4*>(a.params + o);
      m4[i] = *reinterpret_cast<const float4*>(a.m + o);
      v4[i] = *reinterpret_cast<const float4*>(a.v + o);
      g4[i] = *reinterpret_cast<const float4*>((a.slabs ? a.slabs : a.grad) + o);
      if (a.slabs && a.nslabs > 1) q1[i] = *reinterpret_cast<const float4*>(a.slabs + (size_t)a.slab_stride + o);   // the second split-K slab, in the same round trip
    }
  }
  // Everything the guards below need is requested BEHIND the tile loads and before any of it is looked at: the schedule's `active` flag,
  // the chain fault word, the optimiser scalars (scalar loads) and the loss partials of the NaN check (vector loads) -- one memory round
  // trip for the whole prologue. (Round 3 read `active` first, then the tile, then the fault word, then the partials: three dependent
  // round trips in front of the first store of every workgroup of a launch that lives for a single wave of tiles.)
  const int active = st->active;
  const AdamScalars s = st->adam;
  const float inv_scale = st->inv_grad_scale;
  float lossv;
  int fault_now = 0;
  if (a.slabs) {   // fused step: the statistics are still partials; every wave sums the loss for itself
    fault_now = *a.fault;   // a hand-off poll of rowseq_kernel expired in this step: its gradients are garbage, nothing is updated
    int64_t d;
    lossv = tail_output(a.tail, (int64_t)a.n_layers * 512 + a.n_fc3, threadIdx.x & 63, d);
    if (!active || fault_now) return;
  } else {
    if (!active) return;
    lossv = a.grad[a.n_params];
    if (fmodf(a.grad[a.n_params + 3], 1024.f) != 0.f) {   // some rank's fault word, summed by the all-reduce: every rank skips the step and
      if (b == 0 && threadIdx.x == 0) {               // falls back at its next state read
        *a.fault = 1;
        const_cast<TrainState*>(st)->active = 0;
      }
      return;
    }
  }
  if (lossv != lossv) return;  // NaN loss: the reference aborts before the optimiser step (ace_trainer.py:615-617)
  // fp16: an infinity was stored somewhere in the gradient chain of this step -> no update (GradScaler.step, ace_schedule.py:112); the
  // schedule wave lowers the scale. In the split flow the flag arrives all-reduced in statistics slot 3 (+1024 per overflowing rank).
  if (a.f16 && (a.slabs ? f16_overflow(absmax_all(st, threadIdx.x & 63)) : a.grad[a.n_params + 3] >= 1024.f)) return;
  if (tile) {
    if (a.slabs) {   // same additions, in the same order, as grad_reduce_kernel's wide part
      for (int sl = 1; sl < a.nslabs; ++sl) {
        float4 q4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rr = (t >> 4) + 16 * i;
          if (sl == 1) q4[i] = q1[i];
          else q4[i] = *reinterpret_cast<const float4*>(a.slabs + (size_t)sl * a.slab_stride + woff + (int64_t)(r0 + rr) * 512 + c0 + cc);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { g4[i].x += q4[i].x; g4[i].y += q4[i].y; g4[i].z += q4[i].z; g4[i].w += q4[i].w; }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) { g4[i].x *= inv_scale; g4[i].y *= inv_scale; g4[i].z *= inv_scale; g4[i].w *= inv_scale; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = (t >> 4) + 16 * i;
      const int64_t o = woff + (int64_t)(r0 + rr) * 512 + c0 + cc;
      float4 p = p4[i], m = m4[i], v = v4[i];
      const float4 g = g4[i];
      p.x = adamw_one(p.x, g.x, m.x, v.x, s);
      p.y = adamw_one(p.y, g.y, m.y, v.y, s);
      p.z = adamw_one(p.z, g.z, m.z, v.z, s);
      p.w = adamw_one(p.w, g.w, m.w, v.w, s);
      *reinterpret_cast<float4*>(a.params + o) = p;
      *reinterpret_cast<float4*>(a.m + o) = m;
      *reinterpret_cast<float4*>(a.v + o) = v;
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
      const int rr = (t >> 4) + 16 * i;  // row of W^T tile = column of W
      uint2 pk;
      pk.x = (uint32_t)tileT[rr][cc + 0] | ((uint32_t)tileT[rr][cc + 1] << 16);
      pk.y = (uint32_t)tileT[rr][cc + 2] | ((uint32_t)tileT[rr][cc + 3] << 16);
      *reinterpret_cast<uint2*>(a.WbT + (size_t)layer * 262144 + (size_t)(c0 + rr) * 512 + r0 + cc) = pk;
    }
  } else {
    // small parameters: biases of the wide layers, fc3 weight + bias
    const int64_t n_bias = (int64_t)a.n_layers * 512;
    if (a.slabs) {   // fused step: the partials are reduced here as well (grad_reduce_kernel's tail, output by output, the same bits)
      adamw_small_columns(a, b, s);
      return;
    }
    const int64_t k = (int64_t)b * 256 + t;
    int64_t o = -1;
    if (k < n_bias) o = a.b_off[k >> 9] + (k & 511);
    else if (k < n_bias + a.n_fc3) o = a.fc3_off + (k - n_bias);
    if (o >= 0) {
      float p = a.params[o], m = a.m[o], v = a.v[o];
      p = adamw_one(p, a.grad[o], m, v, s);
      a.params[o] = p; a.m[o] = m; a.v[o] = v;
      if (k >= n_bias && (k - n_bias) < (int64_t)a.no * 512) a.W3b[k - n_bias] = a.f16 ? EltF16::from_f(p) : f2bf(p);
    }
  }
}

}  // namespace acez
