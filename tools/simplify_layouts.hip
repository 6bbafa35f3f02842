// simplify_layouts.hip -- MEASUREMENT ONLY (tools/simplify_timing.py builds it into tools/libacez_simplify_layouts.so): the two layouts
// considered for the per-cluster quadric sums of include/acez.h section Q, step 5, side by side on the same tables, so that the choice
// the product made (acezero_amd/csrc/simplify_api.hip: one wavefront per cluster) rests on a number that can be taken again. Both write
// the nine sums of every cluster; they differ in the order of the additions, hence in the last bits. Not part of libacez.so.
//   layout 0  one lane per cluster walks the cluster's corners serially
//   layout 1  one wavefront per cluster: lane l takes the corners l, l + 64, .. of the segment, then an xor butterfly 32, 16, .. 1
//             (the product's order; the product's wavefronts stride over the clusters, these take one each)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../acezero_amd/csrc/simplify_solve.h"

namespace {

using namespace acez;

constexpr int THREADS = 256, WAVE = 64;

struct Tables {
  const float* vertices;
  int m;
  const int32_t* faces;
  int64_t k;
  const int64_t* sorted_keys;
  const int64_t* segments;
  const int64_t* corner_order;
  const int64_t* corner_segments;
  float origin[3];
  float cell;
  int64_t clusters;            // the launch covers the clusters 0 .. clusters - 1 (at most m)
};

__device__ inline bool centre_of(const Tables& t, int64_t c, double* centre) {
  const int64_t lo = t.segments[c], hi = t.segments[c + 1];
  if (lo < 0 || hi > t.m || hi <= lo) return false;
  const int64_t key = t.sorted_keys[lo], mask = ((int64_t)1 << 21) - 1;
  const double index[3] = {(double)(key & mask), (double)((key >> 21) & mask), (double)((key >> 42) & mask)};
  for (int j = 0; j < 3; ++j) centre[j] = (double)t.origin[j] + (index[j] + 0.5) * (double)t.cell;
  return true;
}

__device__ inline void add_corner_at(const Tables& t, int64_t i, const double* centre, double* q) {
  const int64_t corner = t.corner_order[i];
  if (corner < 0 || corner >= 3 * t.k) return;
  const int64_t f = corner / 3;
  const int ia = t.faces[3 * f], ib = t.faces[3 * f + 1], ic = t.faces[3 * f + 2];
  if (ia < 0 || ia >= t.m || ib < 0 || ib >= t.m || ic < 0 || ic >= t.m) return;
  double pa[3], pb[3], pc[3];
  for (int j = 0; j < 3; ++j) {
    pa[j] = (double)t.vertices[3 * (int64_t)ia + j] - centre[j];
    pb[j] = (double)t.vertices[3 * (int64_t)ib + j] - centre[j];
    pc[j] = (double)t.vertices[3 * (int64_t)ic + j] - centre[j];
  }
  simplify_add_corner(pa, pb, pc, q);
}

__global__ void __launch_bounds__(THREADS) lane_per_cluster(Tables t, double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (c >= t.clusters) return;
  double centre[3], q[SIMPLIFY_TERMS];
  if (!centre_of(t, c, centre)) return;
  for (int j = 0; j < SIMPLIFY_TERMS; ++j) q[j] = 0.0;
  int64_t lo = t.corner_segments[c], hi = t.corner_segments[c + 1];
  if (lo < 0 || hi > 3 * t.k) lo = hi = 0;
  for (int64_t i = lo; i < hi; ++i) add_corner_at(t, i, centre, q);
  for (int j = 0; j < SIMPLIFY_TERMS; ++j) out[SIMPLIFY_TERMS * c + j] = q[j];
}

__global__ void __launch_bounds__(THREADS) wave_per_cluster(Tables t, double* __restrict__ out) {
  const int lane = threadIdx.x % WAVE;
  const int64_t c = (int64_t)blockIdx.x * (THREADS / WAVE) + threadIdx.x / WAVE;           // the same for the whole wavefront
  if (c >= t.clusters) return;
  double centre[3], q[SIMPLIFY_TERMS];
  if (!centre_of(t, c, centre)) return;
  for (int j = 0; j < SIMPLIFY_TERMS; ++j) q[j] = 0.0;
  int64_t lo = t.corner_segments[c], hi = t.corner_segments[c + 1];
  if (lo < 0 || hi > 3 * t.k) lo = hi = 0;
  for (int64_t i = lo + lane; i < hi; i += WAVE) add_corner_at(t, i, centre, q);
  for (int step = WAVE / 2; step >= 1; step /= 2)
    for (int j = 0; j < SIMPLIFY_TERMS; ++j) q[j] = q[j] + __shfl_xor(q[j], step, WAVE);
  if (lane == 0)
    for (int j = 0; j < SIMPLIFY_TERMS; ++j) out[SIMPLIFY_TERMS * c + j] = q[j];
}

}  // namespace

// d_out double [m][9], written for the clusters only. 0 on success, 1 for an argument that cannot be right, 2 for a launch error.
extern "C" int simplify_layout_accumulate(int layout, int64_t clusters, const float* d_vertices, int64_t m, const int32_t* d_faces, int64_t k,
                                          const int64_t* d_sorted_keys, const int64_t* d_segments, const int64_t* d_corner_order,
                                          const int64_t* d_corner_segments, float origin_x, float origin_y, float origin_z, float cell,
                                          double* d_out, void* stream) {
  if (m <= 0 || k <= 0 || m >= ((int64_t)1 << 31) || k >= ((int64_t)1 << 31) || (layout != 0 && layout != 1) || clusters <= 0 || clusters > m) return 1;
  if (!d_vertices || !d_faces || !d_sorted_keys || !d_segments || !d_corner_order || !d_corner_segments || !d_out) return 1;
  const Tables t = {d_vertices, (int)m, d_faces, k, d_sorted_keys, d_segments, d_corner_order, d_corner_segments, {origin_x, origin_y, origin_z}, cell, clusters};
  const int per_block = layout == 0 ? THREADS : THREADS / WAVE;
  const unsigned blocks = (unsigned)((clusters + per_block - 1) / per_block);
  if (layout == 0) hipLaunchKernelGGL(lane_per_cluster, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, t, d_out);
  else hipLaunchKernelGGL(wave_per_cluster, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, t, d_out);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
