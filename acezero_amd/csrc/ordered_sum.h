// ordered_sum.h -- the one fixed order in which the geometry tools add the terms their bit-for-bit tests pin (tests/ordered_sums.py
// restates it): per wavefront the xor butterfly 32, 16, .. 1 (wave_sum); per workgroup the wavefronts ascending (block_sum_terms);
// across workgroups thread t adds rows t, t + THREADS, .. ascending from 0.0 and the threads' sums fold as a workgroup's (sum_rows).
// ICP (geometry_api.hip), tracking (fusion_api.hip), simplify_api.hip's quadrics, buffer_api.hip's warp mean and ransac_rgbd.h's
// block_sum (its own layout: every thread receives every sum) are built on these. Also the one splitmix64 finaliser (mix64).
//
// Deliberately NOT built on them, because their order is another one and that order is what their tests pin: ransac_api.hip's
// wave_tree and wave_tree28 (DPP half and row swaps), align_api.hip's block_sum and block_max_u64 (an LDS binary tree over 256
// slots), cloud_api.hip's block_scan and block_count (integers, __shfl_down), the integer wave_min of geometry_api.hip and of
// mvs_api.hip (DPP, on the SGM path), gemm_common.h's wave_sum63 and the two-level sum of pose_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acez {

// every counter-based stream adds its own constants around this
__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// Every lane ends with the wavefront's sum, the same bits in all of them: at each step the lanes l and l ^ s form v_l + v_(l ^ s) and
// v_(l ^ s) + v_l, and IEEE addition commutes.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
  return v;
}
// N sums, each as above, step by step: the N exchanges of a step are in flight together, where N calls in turn wait for each other
template <class T, int N>
__device__ __forceinline__ void wave_sum(T (&v)[N]) {
  for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v[i] + __shfl_xor(v[i], s, 64);
}

// the TERMS values of every lane of a workgroup of WAVES wavefronts -> their sums. Threads 0 .. TERMS - 1 return the sum of their own
// term, the others 0. One barrier, reached by every thread.
template <int TERMS, int WAVES>
__device__ __forceinline__ double block_sum_terms(const double (&v)[TERMS], double (*s_sum)[TERMS]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < TERMS; ++i) {
    const double w = wave_sum(v[i]);
    if ((t & 63) == 0) s_sum[t >> 6][i] = w;
  }
  __syncthreads();
  double r = 0.0;
  if (t < TERMS) {
    r = s_sum[0][t];
    for (int w = 1; w < WAVES; ++w) r = r + s_sum[w][t];
  }
  return r;
}

// n_rows rows of TERMS sums -> s_total[TERMS], by one workgroup of THREADS threads. After it returns any thread may read s_total.
template <int TERMS, int THREADS>
__device__ __forceinline__ void sum_rows(const double* rows, int64_t n_rows, double (*s_sum)[TERMS], double* s_total) {
  const int t = threadIdx.x;
  double v[TERMS];
#pragma unroll
  for (int i = 0; i < TERMS; ++i) v[i] = 0.0;
  for (int64_t r = t; r < n_rows; r += THREADS)
#pragma unroll
    for (int i = 0; i < TERMS; ++i) v[i] = v[i] + rows[r * TERMS + i];
  const double total = block_sum_terms<TERMS, THREADS / 64>(v, s_sum);
  if (t < TERMS) s_total[t] = total;
  __syncthreads();
}

}  // namespace acez
