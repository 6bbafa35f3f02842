// simplify_api.hip -- a mesh with fewer faces: quadric vertex clustering (include/acez.h section Q: acez_simplify_keys,
// acez_simplify_clusters, acez_simplify_faces, acez_simplify_quadrics, acez_simplify_place, acez_simplify_unique). simplify_mesh.py,
// fuse_depth.py --simplify_cell.
//
// The header's section Q is the definition; tests/simplify_restated.py restates it in numpy. The stable sorts, the prefix sums and the
// segment searches between the launches are the caller's (acezero_amd/simplify.py, torch on the device); the compaction at the end is
// section P's acez_mesh_compact.
//
// keys      one lane per vertex: the 3 x 21 bit key of its cell in fp32 (one rounding per operation), or NO_CELL.
// clusters  one lane per sorted position: the cluster of the vertex that stands there, scattered back to vertex order.
// faces     one lane per face: its class, the clusters of its corners (the keys the corner sort takes) and, where the three clusters
//           differ, the triple rotated so that its smallest id comes first.
// quadrics  ONE WAVEFRONT PER CLUSTER adds the plane quadrics of the cluster's corners in fp64: lane l takes the corners l, l + 64, ..
//           of the cluster's segment (ascending 3 face + corner) serially, then a fixed xor butterfly. That is the summation order of
//           the definition. Measured against one lane per cluster on fused rooms (tools/simplify_timing.py): a
//           cluster has 50 to 70 corners, up to some 200, each three gathered vertices, and a lane that walks them alone waits for every
//           gather in turn, while the wavefront has them all in flight at once. The gathers are neighbours in cluster order: L2.
// place     one lane per cluster walks the cluster's vertices (ascending vertex id) for the mean and the colour, serially, in fp64,
//           and solves the cluster's quadric (simplify_solve.h).
// unique    one lane per position of the faces sorted by their triples: a face is kept iff it is the first of its run.
// Nothing waits on anything: no atomics, no communication but the butterfly's register exchange inside a wavefront, every loop bounded
// by a segment length, by m or by svd3's sweep cap; every store has one writer, except the byte stores of 1 into cluster_used. Every index formed from device data (an order, a
// segment bound, a face's vertices, a cluster) is range-checked before it is used as an address: wrong tables give wrong numbers,
// never an access out of bounds.
#include <math.h>
#include <stdint.h>

#include "acez_common.h"
#include "launch1d.h"
#include "ordered_sum.h"
#include "simplify_solve.h"

namespace {

using namespace acez;

constexpr int SQ_THREADS = 256, SQ_WAVE = 64;
constexpr int64_t SQ_QUADRIC_BLOCKS = 4096;      // of four wavefronts: enough to fill 256 CUs several times over, whatever m is
constexpr int SQ_AXIS_BITS = 21;
constexpr int64_t SQ_AXIS_CELLS = (int64_t)1 << SQ_AXIS_BITS;
constexpr int64_t SQ_NO_CELL = INT64_MAX;
enum : uint8_t { SQ_INVALID = 0, SQ_DEGENERATE = 1, SQ_COLLAPSED = 2, SQ_CANDIDATE = 3 };

// floor((p - origin) / cell) in fp32; -1 if it is no index of the grid (p not finite, or the host's check was given other bounds)
__host__ __device__ inline int64_t axis_cell(float p, float origin, float cell) {
  const float f = floorf((p - origin) / cell);
  return f >= 0.0f && f < (float)(SQ_AXIS_CELLS - 1) ? (int64_t)f : -1;       // an axis has at most 2^21 - 1 cells
}

__global__ void __launch_bounds__(SQ_THREADS) keys_kernel(const float* __restrict__ vertices, int m, float ox, float oy, float oz, float cell,
                                                          int64_t* __restrict__ keys) {
  const int64_t v = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x;
  if (v >= m) return;
  const float x = vertices[3 * v], y = vertices[3 * v + 1], z = vertices[3 * v + 2];
  int64_t key = SQ_NO_CELL;
  if (isfinite(x) && isfinite(y) && isfinite(z)) {
    const int64_t i = axis_cell(x, ox, cell), j = axis_cell(y, oy, cell), l = axis_cell(z, oz, cell);
    if (i >= 0 && j >= 0 && l >= 0) key = i | (j << SQ_AXIS_BITS) | (l << (2 * SQ_AXIS_BITS));
  }
  keys[v] = key;
}

__global__ void __launch_bounds__(SQ_THREADS) clusters_kernel(const int64_t* __restrict__ order, const int32_t* __restrict__ cluster_sorted, int m,
                                                              int32_t* __restrict__ vertex_cluster) {
  const int64_t i = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x;
  if (i >= m) return;
  const int64_t v = order[i];
  if (v < 0 || v >= m) return;
  const int c = cluster_sorted[i];
  vertex_cluster[v] = c >= 0 && c < m ? c : -1;
}

__global__ void __launch_bounds__(SQ_THREADS) faces_kernel(const int32_t* __restrict__ faces, int64_t k, const int32_t* __restrict__ vertex_cluster,
                                                           int m, uint8_t* __restrict__ face_class, int32_t* __restrict__ triples,
                                                           int32_t* __restrict__ corner_keys) {
  const int64_t t = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x;
  if (t >= k) return;
  const int a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
  uint8_t cls = SQ_INVALID;
  int ca = m, cb = m, cc = m;                              // the corner keys of a face that does not count sort behind every cluster
  int r0 = m, r1 = m, r2 = m;
  if (a >= 0 && a < m && b >= 0 && b < m && c >= 0 && c < m) {
    if (a == b || b == c || a == c) {
      cls = SQ_DEGENERATE;
    } else {
      const int xa = vertex_cluster[a], xb = vertex_cluster[b], xc = vertex_cluster[c];
      if (xa >= 0 && xa < m && xb >= 0 && xb < m && xc >= 0 && xc < m) {       // else a vertex without a cell: invalid
        ca = xa; cb = xb; cc = xc;
        if (xa == xb || xb == xc || xa == xc) {
          cls = SQ_COLLAPSED;
        } else {
          cls = SQ_CANDIDATE;
          if (xa < xb && xa < xc) { r0 = xa; r1 = xb; r2 = xc; }
          else if (xb < xc) { r0 = xb; r1 = xc; r2 = xa; }
          else { r0 = xc; r1 = xa; r2 = xb; }
        }
      }
    }
  }
  face_class[t] = cls;
  triples[3 * t] = r0; triples[3 * t + 1] = r1; triples[3 * t + 2] = r2;
  corner_keys[3 * t] = ca; corner_keys[3 * t + 1] = cb; corner_keys[3 * t + 2] = cc;
}

// The cell centre of the cluster whose vertices stand at the sorted positions lo .. of the keys.
__device__ __forceinline__ void cell_centre(const int64_t* __restrict__ sorted_keys, int64_t lo, float ox, float oy, float oz, float cell, double* centre) {
  const int64_t key = sorted_keys[lo];
  const int64_t mask = SQ_AXIS_CELLS - 1;
  const double index[3] = {(double)(key & mask), (double)((key >> SQ_AXIS_BITS) & mask), (double)((key >> (2 * SQ_AXIS_BITS)) & mask)};
  centre[0] = (double)ox + (index[0] + 0.5) * (double)cell;
  centre[1] = (double)oy + (index[1] + 0.5) * (double)cell;
  centre[2] = (double)oz + (index[2] + 0.5) * (double)cell;
}

// One wavefront per cluster, the wavefronts striding over the clusters. Lane l adds the corners l, l + 64, .. of the cluster's segment
// corner_seg[c] .. corner_seg[c + 1] - 1 to its nine sums, serially; then wave_sum (ordered_sum.h) and lane 0 stores. The clusters
// are 0 .. K - 1 without a gap, so the first empty vertex segment ends a wavefront's walk: the loop is bounded by m / (the number of
// wavefronts).
__global__ void __launch_bounds__(SQ_THREADS) quadrics_kernel(const float* __restrict__ vertices, int m, const int32_t* __restrict__ faces, int64_t k,
                                                              const int64_t* __restrict__ sorted_keys, const int64_t* __restrict__ seg,
                                                              const int64_t* __restrict__ corner_order, const int64_t* __restrict__ corner_seg,
                                                              float ox, float oy, float oz, float cell, double* __restrict__ out_quadrics) {
  const int lane = threadIdx.x % SQ_WAVE;
  const int64_t waves = (int64_t)gridDim.x * (SQ_THREADS / SQ_WAVE);
  for (int64_t c = (int64_t)blockIdx.x * (SQ_THREADS / SQ_WAVE) + threadIdx.x / SQ_WAVE; c < m; c += waves) {      // c is the wavefront's
    const int64_t lo = seg[c], hi = seg[c + 1];
    if (lo < 0 || hi > m || hi <= lo) break;
    double centre[3], q[SIMPLIFY_TERMS];
    cell_centre(sorted_keys, lo, ox, oy, oz, cell, centre);
    for (int j = 0; j < SIMPLIFY_TERMS; ++j) q[j] = 0.0;
    int64_t clo = corner_seg[c], chi = corner_seg[c + 1];
    if (clo < 0 || chi > 3 * k) clo = chi = 0;
    for (int64_t i = clo + lane; i < chi; i += SQ_WAVE) {
      const int64_t corner = corner_order[i];
      if (corner < 0 || corner >= 3 * k) continue;
      const int64_t t = corner / 3;
      const int ia = faces[3 * t], ib = faces[3 * t + 1], ic = faces[3 * t + 2];
      if (ia < 0 || ia >= m || ib < 0 || ib >= m || ic < 0 || ic >= m) continue;
      double pa[3], pb[3], pc[3];
      for (int j = 0; j < 3; ++j) {
        pa[j] = (double)vertices[3 * (int64_t)ia + j] - centre[j];
        pb[j] = (double)vertices[3 * (int64_t)ib + j] - centre[j];
        pc[j] = (double)vertices[3 * (int64_t)ic + j] - centre[j];
      }
      simplify_add_corner(pa, pb, pc, q);
    }
    wave_sum(q);
    if (lane == 0)
      for (int j = 0; j < SIMPLIFY_TERMS; ++j) out_quadrics[SIMPLIFY_TERMS * c + j] = q[j];
  }
}

// lane c is cluster c: positions seg[c] .. seg[c + 1] - 1 of the sorted vertices. A lane past the last cluster finds an empty segment
// and writes nothing. quadrics: the nine sums of every cluster (quadrics_kernel), or null for the mean placement.
__global__ void __launch_bounds__(SQ_THREADS) place_kernel(const float* __restrict__ vertices, const uint8_t* __restrict__ colours, int m,
                                                           const int64_t* __restrict__ sorted_keys, const int64_t* __restrict__ order,
                                                           const int64_t* __restrict__ seg, const double* __restrict__ quadrics, float ox, float oy,
                                                           float oz, float cell, float* __restrict__ out_vertices,
                                                           uint8_t* __restrict__ out_colours, uint8_t* __restrict__ out_fallback) {
  const int64_t c = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x;
  if (c >= m) return;
  const int64_t lo = seg[c], hi = seg[c + 1];
  if (lo < 0 || hi > m || hi <= lo) return;
  double sum[3] = {0.0, 0.0, 0.0};
  int64_t rgb[3] = {0, 0, 0};
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t v = order[i];
    if (v < 0 || v >= m) continue;
    for (int j = 0; j < 3; ++j) sum[j] = sum[j] + (double)vertices[3 * v + j];
    if (colours)
      for (int j = 0; j < 3; ++j) rgb[j] += colours[3 * v + j];
  }
  const int64_t count = hi - lo;
  const double mean[3] = {sum[0] / (double)count, sum[1] / (double)count, sum[2] / (double)count};
  if (out_colours)
    for (int j = 0; j < 3; ++j) out_colours[3 * c + j] = (uint8_t)((2 * rgb[j] + count) / (2 * count));
  bool solved = false;
  double x[3];
  if (quadrics) {
    double centre[3], q[SIMPLIFY_TERMS];
    cell_centre(sorted_keys, lo, ox, oy, oz, cell, centre);
    for (int j = 0; j < SIMPLIFY_TERMS; ++j) q[j] = quadrics[SIMPLIFY_TERMS * c + j];
    const double rel[3] = {mean[0] - centre[0], mean[1] - centre[1], mean[2] - centre[2]};
    solved = simplify_solve(q, rel, (double)cell, x);
    for (int j = 0; j < 3; ++j) x[j] = centre[j] + x[j];
  }
  for (int j = 0; j < 3; ++j) out_vertices[3 * c + j] = (float)(solved ? x[j] : mean[j]);
  out_fallback[c] = quadrics && !solved ? 1 : 0;
}

// position i of the faces sorted by (first, second, third) of their triples, equal triples in input order
__global__ void __launch_bounds__(SQ_THREADS) unique_kernel(const int32_t* __restrict__ triples, const uint8_t* __restrict__ face_class,
                                                            const int64_t* __restrict__ perm, int64_t k, int m, uint8_t* __restrict__ face_keep,
                                                            uint8_t* cluster_used) {
  const int64_t i = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x;
  if (i >= k) return;
  const int64_t t = perm[i];
  if (t < 0 || t >= k) return;
  if (face_class[t] != SQ_CANDIDATE) return;                                 // face_keep was cleared
  const int r0 = triples[3 * t], r1 = triples[3 * t + 1], r2 = triples[3 * t + 2];
  if (i > 0) {
    const int64_t p = perm[i - 1];
    if (p >= 0 && p < k && face_class[p] == SQ_CANDIDATE && triples[3 * p] == r0 && triples[3 * p + 1] == r1 && triples[3 * p + 2] == r2) return;
  }
  if (r0 < 0 || r0 >= m || r1 < 0 || r1 >= m || r2 < 0 || r2 >= m) return;
  face_keep[t] = 1;
  cluster_used[r0] = 1;
  cluster_used[r1] = 1;
  cluster_used[r2] = 1;
}

// the grid of step 1: finite bounds, a positive finite cell, and fewer than 2^21 cells on every axis
inline bool grid_ok(const float* o, const float* h, float cell) {
  if (!(isfinite(cell) && cell > 0.0f)) return false;
  for (int j = 0; j < 3; ++j) {
    if (!(isfinite(o[j]) && isfinite(h[j]) && h[j] >= o[j])) return false;
    if (axis_cell(h[j], o[j], cell) < 0) return false;
  }
  return true;
}

}  // namespace

extern "C" int acez_simplify_keys(const float* d_vertices, int64_t m, float origin_x, float origin_y, float origin_z, float max_x, float max_y,
                                  float max_z, float cell, int64_t* d_keys, void* stream) {
  ACEZ_REQUIRE_COUNTS(m);
  const float o[3] = {origin_x, origin_y, origin_z}, h[3] = {max_x, max_y, max_z};
  ACEZ_REQUIRE(grid_ok(o, h, cell), "the cell must be positive and finite, the bounds finite and ordered, and an axis have fewer than 2^21 cells");
  ACEZ_REQUIRE(m == 0 || (d_vertices && d_keys), "null pointer");
  if (int rc = acez::require_device("meshes are simplified on a gfx950 GPU")) return rc;
  if (m == 0) return ACEZ_OK;
  hipLaunchKernelGGL(keys_kernel, dim3(blocks_for(m, SQ_THREADS)), dim3(SQ_THREADS), 0, (hipStream_t)stream, d_vertices, (int)m, origin_x, origin_y, origin_z,
                     cell, d_keys);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_simplify_clusters(const int64_t* d_order, const int32_t* d_cluster_sorted, int64_t m, int32_t* d_vertex_cluster, void* stream) {
  ACEZ_REQUIRE_COUNTS(m);
  ACEZ_REQUIRE(m == 0 || (d_order && d_cluster_sorted && d_vertex_cluster), "null pointer");
  if (int rc = acez::require_device("meshes are simplified on a gfx950 GPU")) return rc;
  if (m == 0) return ACEZ_OK;
  hipStream_t s = (hipStream_t)stream;
  ACEZ_HIP_CHECK(hipMemsetAsync(d_vertex_cluster, 0xff, sizeof(int32_t) * (size_t)m, s));      // -1: no cluster
  hipLaunchKernelGGL(clusters_kernel, dim3(blocks_for(m, SQ_THREADS)), dim3(SQ_THREADS), 0, s, d_order, d_cluster_sorted, (int)m, d_vertex_cluster);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_simplify_faces(const int32_t* d_faces, int64_t k, const int32_t* d_vertex_cluster, int64_t m, uint8_t* d_face_class,
                                   int32_t* d_triples, int32_t* d_corner_keys, void* stream) {
  ACEZ_REQUIRE_COUNTS(m, k);
  ACEZ_REQUIRE((m == 0 || d_vertex_cluster) && (k == 0 || (d_faces && d_face_class && d_triples && d_corner_keys)), "null pointer");
  if (int rc = acez::require_device("meshes are simplified on a gfx950 GPU")) return rc;
  if (k == 0) return ACEZ_OK;
  hipLaunchKernelGGL(faces_kernel, dim3(blocks_for(k, SQ_THREADS)), dim3(SQ_THREADS), 0, (hipStream_t)stream, d_faces, k, d_vertex_cluster, (int)m, d_face_class,
                     d_triples, d_corner_keys);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_simplify_quadrics(const float* d_vertices, int64_t m, const int32_t* d_faces, int64_t k, const int64_t* d_sorted_keys,
                                      const int64_t* d_segments, const int64_t* d_corner_order, const int64_t* d_corner_segments, float origin_x,
                                      float origin_y, float origin_z, float cell, double* d_out_quadrics, void* stream) {
  ACEZ_REQUIRE_COUNTS(m, k);
  ACEZ_REQUIRE(isfinite(cell) && cell > 0.0f && isfinite(origin_x) && isfinite(origin_y) && isfinite(origin_z),
               "the cell must be positive and finite, the origin finite");
  ACEZ_REQUIRE(m == 0 || (d_vertices && d_sorted_keys && d_segments && d_corner_segments && d_out_quadrics), "null pointer");
  ACEZ_REQUIRE(m == 0 || k == 0 || (d_faces && d_corner_order), "null pointer");
  if (int rc = acez::require_device("meshes are simplified on a gfx950 GPU")) return rc;
  if (m == 0) return ACEZ_OK;
  const int64_t blocks = (m + SQ_THREADS / SQ_WAVE - 1) / (SQ_THREADS / SQ_WAVE);
  hipLaunchKernelGGL(quadrics_kernel, dim3((unsigned)(blocks < SQ_QUADRIC_BLOCKS ? blocks : SQ_QUADRIC_BLOCKS)), dim3(SQ_THREADS), 0, (hipStream_t)stream,
                     d_vertices, (int)m, d_faces, k, d_sorted_keys, d_segments, d_corner_order, d_corner_segments, origin_x, origin_y, origin_z, cell,
                     d_out_quadrics);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_simplify_place(const float* d_vertices, const uint8_t* d_colours, int64_t m, const int64_t* d_sorted_keys,
                                   const int64_t* d_order, const int64_t* d_segments, const double* d_quadrics, float origin_x, float origin_y,
                                   float origin_z, float cell, float* d_out_vertices, uint8_t* d_out_colours, uint8_t* d_out_fallback,
                                   void* stream) {
  ACEZ_REQUIRE_COUNTS(m);
  ACEZ_REQUIRE(isfinite(cell) && cell > 0.0f && isfinite(origin_x) && isfinite(origin_y) && isfinite(origin_z),
               "the cell must be positive and finite, the origin finite");
  ACEZ_REQUIRE((d_colours == nullptr) == (d_out_colours == nullptr), "vertex colours and output colours go together");
  ACEZ_REQUIRE(m == 0 || (d_vertices && d_sorted_keys && d_order && d_segments && d_out_vertices && d_out_fallback), "null pointer");
  if (int rc = acez::require_device("meshes are simplified on a gfx950 GPU")) return rc;
  if (m == 0) return ACEZ_OK;
  hipLaunchKernelGGL(place_kernel, dim3(blocks_for(m, SQ_THREADS)), dim3(SQ_THREADS), 0, (hipStream_t)stream, d_vertices, d_colours, (int)m, d_sorted_keys, d_order,
                     d_segments, d_quadrics, origin_x, origin_y, origin_z, cell, d_out_vertices, d_out_colours, d_out_fallback);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_simplify_unique(const int32_t* d_triples, const uint8_t* d_face_class, const int64_t* d_perm, int64_t k, int64_t m,
                                    uint8_t* d_face_keep, uint8_t* d_cluster_used, void* stream) {
  ACEZ_REQUIRE_COUNTS(m, k);
  ACEZ_REQUIRE((m == 0 || d_cluster_used) && (k == 0 || (d_triples && d_face_class && d_perm && d_face_keep)), "null pointer");
  if (int rc = acez::require_device("meshes are simplified on a gfx950 GPU")) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (m > 0) ACEZ_HIP_CHECK(hipMemsetAsync(d_cluster_used, 0, (size_t)m, s));
  if (k == 0) return ACEZ_OK;
  ACEZ_HIP_CHECK(hipMemsetAsync(d_face_keep, 0, (size_t)k, s));
  if (m == 0) return ACEZ_OK;
  hipLaunchKernelGGL(unique_kernel, dim3(blocks_for(k, SQ_THREADS)), dim3(SQ_THREADS), 0, s, d_triples, d_face_class, d_perm, k, (int)m, d_face_keep, d_cluster_used);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
