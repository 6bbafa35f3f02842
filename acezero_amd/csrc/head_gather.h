// head_gather.h -- the batch gather's row loop and the fp16 gradient-scale stripes (absmax_*): device bodies shared by the chain unit
// (head_kernels.hip), the optimiser unit (head_optim.hip) and the pose launches that carry a gather (pose_fused.hip).
#pragma once
#include "head_kernels.h"

namespace acez {

// ---------------------------------------------------------------------------------------------------
// gather: out[r][:] = features[idx[r]][:]   (one wave copies one 1 KiB row per instruction)
// ---------------------------------------------------------------------------------------------------
// Rows wave, wave + nwaves, ... of a batch, GR at a time: the loads of a level are issued for all GR rows before anything of the next
// level (one row after the other, every row paid its own idx -> row round trips; two at a time -- round 3 -- the optimiser launch's 1720
// gather waves still walked their three rows in two passes of three dependent levels each). With meta.dst the per-row metadata the
// loss kernel needs (GatherMeta) is looked up beside the copy: a third level for the image index, overlapped with the row stores.
template <int GR = 4>
__device__ __forceinline__ void gather_rows(const uint16_t* __restrict__ feat, const int64_t* __restrict__ idx, uint16_t* __restrict__ out, int n,
                                            int wave, int nwaves, int lane, const GatherMeta& meta) {
  // (meta.hold: the trainer's sticky fault word, a wave-uniform load that travels with the first level and is only looked at in front of
  // the stores; while it is set nothing is stored)
  const bool held = meta.hold && *meta.hold;
  for (int r0 = wave; r0 < n; r0 += GR * nwaves) {
    int r[GR];
    bool ok[GR];
    int64_t s[GR];
#pragma unroll
    for (int j = 0; j < GR; ++j) { r[j] = r0 + j * nwaves; ok[j] = r[j] < n; s[j] = idx[ok[j] ? r[j] : r0]; }
    uint4 v[GR];
#pragma unroll
    for (int j = 0; j < GR; ++j) v[j] = *reinterpret_cast<const uint4*>(feat + s[j] * 512 + lane * 8);
    int view[GR];
    float2 tp[GR];
    if (meta.dst) {
#pragma unroll
      for (int j = 0; j < GR; ++j) { view[j] = meta.view_idx[s[j]]; tp[j] = *reinterpret_cast<const float2*>(meta.target_px + s[j] * 2); }
    }
#pragma unroll
    for (int j = 0; j < GR; ++j)
      if (ok[j] && !held) *reinterpret_cast<uint4*>(out + (size_t)r[j] * 512 + lane * 8) = v[j];
    if (meta.dst) {
      int img[GR];
#pragma unroll
      for (int j = 0; j < GR; ++j) img[j] = meta.view_image[view[j]];
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < GR; ++j)
          if (ok[j] && !held) meta.dst[r[j]] = make_int4(view[j], img[j], __float_as_int(tp[j].x), __float_as_int(tp[j].y));
      }
    }
  }
}

// fp16 gradient-scale control: every kernel that stores propagated gradients folds the largest magnitude it produced (before the
// conversion, in scaled units) into the trainer's 64 striped words (TrainState::dz_absmax_slots) -- a wavefront maximum, then an atomic
// max on the bit pattern (non-negative floats order like unsigned integers; anything above 65504.f is the overflow signal, f16_overflow) of the word of
// this workgroup's stripe. Read (absmax_all) and reset by sched_post_wave.
// The magnitudes are taken BEFORE the conversion, so the overflow test is "larger than fp16's largest finite value", not "is inf": a
// propagated value of 7e4 is a finite float that the conversion stores as inf (round 6: a 25 000-iteration fp16 refit went through
// exactly that window once the scale had climbed to 2^16 -- the update was not skipped and NaN reached the fp32 masters).
__device__ __forceinline__ bool f16_overflow(uint32_t amax_bits) { return amax_bits > 0x477fe000u; }   // 65504.f; inf and NaN patterns are above it
__device__ __forceinline__ void absmax_publish(uint32_t* slots, float amax) {
  amax = wave_max63_nonneg(amax);   // (DPP: no LDS round trips; the maximum is in lane 63)
  if ((threadIdx.x & 63) == 63 && amax > 0.f) atomicMax(slots + (blockIdx.x & 63) * 32, __float_as_uint(amax));
}
// The maximum over 64 stripe words already in registers (one per lane, all 64 lanes call it, every lane returns the result). The bit
// patterns are non-negative floats (or +inf), which order like the unsigned integers they are: a DPP float maximum + one v_readlane, no LDS
// round trips (absmax_all's six ds_bpermute rounds sat between the K loop and the epilogue of every wave of wgrad_opt_kernel in fp16 mode).
__device__ __forceinline__ uint32_t absmax_reduce(uint32_t m) {
  const float f = wave_max63_nonneg(__uint_as_float(m));
  return (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(f), 63);
}
// the maximum over the 64 stripes; all 64 lanes of the wavefront must call it, every lane returns the result
__device__ __forceinline__ uint32_t absmax_all(const TrainState* st, int lane) {
  uint32_t m = __builtin_nontemporal_load(&st->dz_absmax_slots[lane * 32]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
  return m;
}

}  // namespace acez
