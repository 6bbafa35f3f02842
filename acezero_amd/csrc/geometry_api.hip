// geometry_api.hip -- nearest-neighbour distances between two point clouds on a uniform grid, and the voxel downsample
// (include/acez.h section N: acez_geom_cells, acez_geom_nearest, acez_geom_voxel_means), and the ICP loop built on the search
// (acez_geom_icp_accumulate, acez_geom_icp_update). eval_geometry.py.
//
// The header's section N is the definition: every float operation below is written in its order, the unit is built with
// -ffp-contract=off, and tests/geometry_restated.py restates it in numpy float32 for the bit-for-bit comparison.
//
// cells        one thread per point: its linear cell, or -1.
// nearest      one lane per query, GN_THREADS queries per workgroup. The caller passes the queries ordered by their own cell, so a
//              workgroup's queries usually lie in one or two cells. The workgroup takes the box of its queries' cells (wave
//              reductions through LDS, no atomics). COMPACT box (at most GE_MAX_ROWS rows of cells around it, at most GE_MAX_ISPAN
//              cells along x): the rows' ranges of the sorted reference array -- x is the fastest axis, so the cells i0 .. i1 of
//              a row are ONE contiguous range -- are staged into LDS in chunks of GE_CHUNK points and every lane scans every
//              staged point (a lane then also sees points outside its own 27 cells: harmless, the result is a minimum over all
//              references within R). Otherwise (queries scattered over many sparse cells) every lane walks the nine ranges of its
//              own 3 x 3 x 3 cells through L2. Both forms give the same bits.
// voxel_means  one lane per segment, a sequential sum in array order.
// icp          ACCUMULATE is the nearest kernel with the query computed from the source point and the device-resident transform, and
//              with the 18 fp64 moments of the lane's correspondence reduced per workgroup in ordered_sum.h's order (one search_nearest
//              for both kernels); UPDATE is one workgroup that sums the workgroups' rows and runs the solve of icp_solve.h. Both return
//              at once when the state says the loop has stopped (device_loop.h): a whole stage is enqueued without a host round trip.
// No atomics, no communication between workgroups, plain loads and stores. Every range read from the cell table is clamped to
// [0, m], so every loop is bounded by m and a malformed table cannot cause a read out of bounds.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "acez_common.h"
#include "icp_solve.h"
#include "launch1d.h"
#include "ordered_sum.h"

namespace {

using namespace acez;

constexpr int GE_THREADS = 256;     // cells, voxel means
constexpr int GN_THREADS = 256;     // nearest: queries per workgroup
constexpr int GN_WAVES = GN_THREADS / 64;
constexpr int GE_CHUNK = 1024;      // staged points per pass: 16 KiB of LDS
constexpr int GE_MAX_ROWS = 12;     // (jspan + 2) * (kspan + 2) with the queries in one row of cells, or in two adjacent rows
constexpr int GE_MAX_ISPAN = 4;     // the staged x-range is at most 6 cells where a lane's own is 3
constexpr int GE_MAX_DIM = 1024;
constexpr int64_t GE_MAX_CELLS = (int64_t)1 << 24;

struct Grid {
  float ox, oy, oz, c;
  int nx, ny, nz;
};

// floor((x - o) / c) clamped to -1 .. n; -1 for NaN
__device__ inline int axis_cell(float x, float o, float c, int n) {
  const float f = floorf((x - o) / c);
  return f >= 0.0f ? (f < (float)n ? (int)f : n) : -1;
}

__device__ inline int clamp_m(int v, int m) { return v < 0 ? 0 : (v > m ? m : v); }

__global__ void __launch_bounds__(GE_THREADS) geom_cells_kernel(const float* __restrict__ pts, int64_t n, Grid g, int32_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * GE_THREADS + threadIdx.x;
  if (p >= n) return;
  const float x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
  const int i = axis_cell(x, g.ox, g.c, g.nx), j = axis_cell(y, g.oy, g.c, g.ny), k = axis_cell(z, g.oz, g.c, g.nz);
  const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && i >= 0 && i < g.nx && j >= 0 && j < g.ny && k >= 0 && k < g.nz;
  out[p] = ok ? (k * g.ny + j) * g.nx + i : -1;
}

// The search of NEAREST for one lane's query (qx, qy, qz); `live` says whether the lane has one. Called by all GN_THREADS lanes of a
// workgroup (it holds barriers). The winner's position in the sorted reference array comes along for the caller that wants its
// coordinates (ICP); the nearest kernel leaves it unused.
struct Best {
  float d2;
  int idx;
  int pos;
};

__device__ __forceinline__ void consider(float qx, float qy, float qz, float px, float py, float pz, int idx, int pos, float r2, Best& b) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  if (d2 <= r2 && (d2 < b.d2 || (d2 == b.d2 && idx < b.idx))) {
    b.d2 = d2;
    b.idx = idx;
    b.pos = pos;
  }
}

__device__ inline int wave_min(int v) {
  for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
  return v;
}

__device__ __forceinline__ Best search_nearest(const float* __restrict__ ref, const int32_t* __restrict__ ref_index,
                                               const int32_t* __restrict__ cell_start, int m, const Grid& g, float qx, float qy, float qz,
                                               bool live, float r2, int plain) {
  __shared__ float4 s_pts[GE_CHUNK];
  __shared__ int s_red[GN_WAVES][6];
  __shared__ int s_lo[GE_MAX_ROWS], s_hi[GE_MAX_ROWS];
  const int t = threadIdx.x;
  const int ci = axis_cell(qx, g.ox, g.c, g.nx), cj = axis_cell(qy, g.oy, g.c, g.ny), ck = axis_cell(qz, g.oz, g.c, g.nz);
  Best best{INFINITY, INT_MAX, 0};

  // the box of the workgroup's live query cells: min and max per axis (max as the min of the negation)
  {
    const int v[6] = {live ? ci : INT_MAX, live ? cj : INT_MAX, live ? ck : INT_MAX, live ? -ci : INT_MAX, live ? -cj : INT_MAX, live ? -ck : INT_MAX};
    for (int a = 0; a < 6; ++a) {
      const int r = wave_min(v[a]);
      if ((t & 63) == 0) s_red[t >> 6][a] = r;
    }
  }
  __syncthreads();
  int box[6];
  for (int a = 0; a < 6; ++a) {
    int r = s_red[0][a];
    for (int w = 1; w < GN_WAVES; ++w) r = min(r, s_red[w][a]);
    box[a] = r;
  }
  const bool any = box[0] != INT_MAX;                             // a live query in this workgroup (uniform)
  const int imin = box[0], jmin = box[1], kmin = box[2], imax = -box[3], jmax = -box[4], kmax = -box[5];
  const int jrows = any ? jmax - jmin + 3 : 0, krows = any ? kmax - kmin + 3 : 0;     // at most 1024 + 4 each
  const bool compact = any && !plain && jrows * krows <= GE_MAX_ROWS && imax - imin + 1 <= GE_MAX_ISPAN;   // uniform

  if (compact) {
    const int rows = jrows * krows;
    if (t < rows) {
      const int j = jmin - 1 + t % jrows, k = kmin - 1 + t / jrows;
      const int i0 = max(imin - 1, 0), i1 = min(imax + 1, g.nx - 1);
      int lo = 0, hi = 0;
      if (j >= 0 && j < g.ny && k >= 0 && k < g.nz && i0 <= i1) {
        const int base = (k * g.ny + j) * g.nx;
        lo = clamp_m(cell_start[base + i0], m);
        hi = clamp_m(cell_start[base + i1 + 1], m);
        if (hi < lo) hi = lo;
      }
      s_lo[t] = lo;
      s_hi[t] = hi;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const int lo = s_lo[r], hi = s_hi[r];
      for (int at = lo; at < hi; at += GE_CHUNK) {
        const int cnt = min(GE_CHUNK, hi - at);
        __syncthreads();                                          // the previous chunk has been scanned
        for (int e = t; e < cnt; e += GN_THREADS) {
          const int64_t p = (int64_t)at + e;
          s_pts[e] = make_float4(ref[3 * p], ref[3 * p + 1], ref[3 * p + 2], __int_as_float(ref_index[p]));
        }
        __syncthreads();
        if (live)
#pragma unroll 4
          for (int e = 0; e < cnt; ++e) {
            const float4 pt = s_pts[e];
            consider(qx, qy, qz, pt.x, pt.y, pt.z, __float_as_int(pt.w), at + e, r2, best);
          }
      }
    }
  } else if (live) {
    const int i0 = max(ci - 1, 0), i1 = min(ci + 1, g.nx - 1);
    for (int dk = -1; dk <= 1; ++dk)
      for (int dj = -1; dj <= 1; ++dj) {
        const int j = cj + dj, k = ck + dk;
        if (j < 0 || j >= g.ny || k < 0 || k >= g.nz || i0 > i1) continue;
        const int base = (k * g.ny + j) * g.nx;
        const int lo = clamp_m(cell_start[base + i0], m), hi = clamp_m(cell_start[base + i1 + 1], m);
#pragma unroll 4
        for (int64_t p = lo; p < hi; ++p) consider(qx, qy, qz, ref[3 * p], ref[3 * p + 1], ref[3 * p + 2], ref_index[p], (int)p, r2, best);
      }
  }
  return best;
}

__global__ void __launch_bounds__(GN_THREADS) geom_nearest_kernel(const float* __restrict__ ref, const int32_t* __restrict__ ref_index,
                                                                   const int32_t* __restrict__ cell_start, int m, Grid g,
                                                                   const float* __restrict__ query, int64_t n, float r2,
                                                                   float* __restrict__ out_d2, int32_t* __restrict__ out_index, int plain) {
  const int64_t q = (int64_t)blockIdx.x * GN_THREADS + threadIdx.x;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  bool live = false;
  if (q < n) {
    qx = query[3 * q], qy = query[3 * q + 1], qz = query[3 * q + 2];
    live = isfinite(qx) && isfinite(qy) && isfinite(qz);
  }
  const Best best = search_nearest(ref, ref_index, cell_start, m, g, qx, qy, qz, live, r2, plain);
  if (q < n) {
    out_d2[q] = best.d2;
    out_index[q] = best.idx == INT_MAX ? -1 : best.idx;
  }
}

// ACCUMULATE: one lane per source point. x' = T x in fp64 rounded once, the search of NEAREST on x', the 18 terms of the lane's
// correspondence (zeros without one), one row of sums per workgroup.
__global__ void __launch_bounds__(GN_THREADS) geom_icp_accumulate_kernel(const float* __restrict__ ref, const int32_t* __restrict__ ref_index,
                                                                          const int32_t* __restrict__ cell_start, int m, Grid g,
                                                                          const float* __restrict__ src, int64_t n, float r2, float px, float py,
                                                                          float pz, const double* state, double* __restrict__ partials, int plain) {
  __shared__ double s_sum[GN_WAVES][ICP_TERMS];
  if (state[LOOP_STATUS] != LOOP_RUNNING) return;                 // the loop has stopped (uniform over the grid)
  const int t = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * GN_THREADS + t;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  bool live = false;
  if (q < n) {
    const double x = src[3 * q], y = src[3 * q + 1], z = src[3 * q + 2];
    qx = (float)(((state[0] * x + state[1] * y) + state[2] * z) + state[3]);
    qy = (float)(((state[4] * x + state[5] * y) + state[6] * z) + state[7]);
    qz = (float)(((state[8] * x + state[9] * y) + state[10] * z) + state[11]);
    live = isfinite(qx) && isfinite(qy) && isfinite(qz);
  }
  const Best best = search_nearest(ref, ref_index, cell_start, m, g, qx, qy, qz, live, r2, plain);
  double v[ICP_TERMS];
  for (int i = 0; i < ICP_TERMS; ++i) v[i] = 0.0;
  if (live && best.idx != INT_MAX) {                              // then 0 <= best.pos < m
    const int64_t p = best.pos;
    const double a[3] = {(double)qx - (double)px, (double)qy - (double)py, (double)qz - (double)pz};
    const double b[3] = {(double)ref[3 * p] - (double)px, (double)ref[3 * p + 1] - (double)py, (double)ref[3 * p + 2] - (double)pz};
    v[0] = 1.0;
    for (int c = 0; c < 3; ++c) {
      v[1 + c] = a[c];
      v[4 + c] = b[c];
      for (int r = 0; r < 3; ++r) v[7 + 3 * r + c] = b[r] * a[c];
    }
    v[16] = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    v[17] = (double)best.d2;
  }
  const double total = block_sum_terms<ICP_TERMS, GN_WAVES>(v, s_sum);
  if (t < ICP_TERMS) partials[(int64_t)blockIdx.x * ICP_TERMS + t] = total;
}

// UPDATE: one workgroup sums the partial rows (sum_rows of ordered_sum.h), thread 0 runs icp_update (icp_solve.h) on the totals.
__global__ void __launch_bounds__(GN_THREADS) geom_icp_update_kernel(const double* __restrict__ partials, int64_t rows, int64_t n, float px,
                                                                      float py, float pz, int with_scale, double rel_fitness, double rel_rmse,
                                                                      int max_iterations, double* state, double* history) {
  __shared__ double s_sum[GN_WAVES][ICP_TERMS];
  __shared__ double s_total[ICP_TERMS];
  if (!loop_live(state, max_iterations)) return;                  // uniform
  sum_rows<ICP_TERMS, GN_THREADS>(partials, rows, s_sum, s_total);
  if (threadIdx.x == 0) {
    const double pivot[3] = {(double)px, (double)py, (double)pz};
    icp_update(state, s_total, n, pivot, with_scale, rel_fitness, rel_rmse, history);
  }
}

__global__ void __launch_bounds__(GE_THREADS) geom_voxel_means_kernel(const float* __restrict__ pts, int64_t n, const int32_t* __restrict__ seg_start,
                                                                       int64_t s, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * GE_THREADS + threadIdx.x;
  if (v >= s) return;
  int64_t lo = seg_start[v], hi = seg_start[v + 1];
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < lo ? lo : (hi > n ? n : hi);
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (int64_t p = lo; p < hi; ++p) {
    sx = sx + pts[3 * p];
    sy = sy + pts[3 * p + 1];
    sz = sz + pts[3 * p + 2];
  }
  const float cnt = (float)(hi - lo);
  out[3 * v] = sx / cnt;
  out[3 * v + 1] = sy / cnt;
  out[3 * v + 2] = sz / cnt;
}

}  // namespace

#define GE_REQUIRE_GRID()                                                                                                          \
  ACEZ_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= GE_MAX_DIM && ny <= GE_MAX_DIM && nz <= GE_MAX_DIM,                          \
               "grid dimensions must be in 1 .. 1024");                                                                            \
  ACEZ_REQUIRE((int64_t)nx * ny * nz <= GE_MAX_CELLS, "grid too large (more than 2^24 cells)");                                    \
  ACEZ_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz), "non-finite grid origin");                                            \
  ACEZ_REQUIRE(isfinite(cell) && cell > 0.0f, "the cell edge must be positive and finite")

extern "C" int acez_geom_cells(const float* d_points, int64_t n, float ox, float oy, float oz, float cell, int nx, int ny, int nz,
                               int32_t* d_out_cells, void* stream) {
  ACEZ_REQUIRE_POINT_COUNTS(n);
  ACEZ_REQUIRE(n == 0 || (d_points && d_out_cells), "null pointer");
  GE_REQUIRE_GRID();
  if (int rc = acez::require_device("the point grid runs on a gfx950 GPU")) return rc;
  if (n == 0) return ACEZ_OK;
  const Grid g{ox, oy, oz, cell, nx, ny, nz};
  hipLaunchKernelGGL(geom_cells_kernel, dim3(blocks_for(n, GE_THREADS)), dim3(GE_THREADS), 0, (hipStream_t)stream, d_points, n, g, d_out_cells);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_geom_nearest(const float* d_ref, const int32_t* d_ref_index, const int32_t* d_cell_start, int64_t m, float ox, float oy,
                                 float oz, float cell, int nx, int ny, int nz, const float* d_query, int64_t n, float radius,
                                 float* d_out_d2, int32_t* d_out_index, void* stream) {
  ACEZ_REQUIRE_POINT_COUNTS(m, n);
  ACEZ_REQUIRE(d_cell_start && (m == 0 || (d_ref && d_ref_index)) && (n == 0 || (d_query && d_out_d2 && d_out_index)), "null pointer");
  GE_REQUIRE_GRID();
  ACEZ_REQUIRE(isfinite(radius) && radius > 0.0f, "the radius must be positive and finite");
  // with this margin a reference within the radius is never two cells away (section N)
  ACEZ_REQUIRE(!(cell < radius * 1.0009765625f), "the cell edge must be at least radius * (1 + 2^-10)");
  if (int rc = acez::require_device("the nearest-neighbour search runs on a gfx950 GPU")) return rc;
  if (n == 0) return ACEZ_OK;
  const Grid g{ox, oy, oz, cell, nx, ny, nz};
  const int plain = ACEZ_DIAG_ENV("ACEZ_GEOM_PLAIN") != nullptr;    // diagnostics build: every workgroup takes the per-lane form
  hipLaunchKernelGGL(geom_nearest_kernel, dim3(blocks_for(n, GN_THREADS)), dim3(GN_THREADS), 0, (hipStream_t)stream, d_ref, d_ref_index, d_cell_start,
                     (int)m, g, d_query, n, radius * radius, d_out_d2, d_out_index, plain);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_geom_voxel_means(const float* d_points, int64_t n, const int32_t* d_segment_start, int64_t segments, float* d_out_means,
                                     void* stream) {
  ACEZ_REQUIRE_COUNTS(n, segments);
  ACEZ_REQUIRE(d_segment_start && (n == 0 || d_points) && (segments == 0 || d_out_means), "null pointer");
  if (int rc = acez::require_device("the voxel downsample runs on a gfx950 GPU")) return rc;
  if (segments == 0) return ACEZ_OK;
  hipLaunchKernelGGL(geom_voxel_means_kernel, dim3(blocks_for(segments, GE_THREADS)), dim3(GE_THREADS), 0, (hipStream_t)stream, d_points, n,
                     d_segment_start, segments, d_out_means);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_geom_icp_accumulate(const float* d_ref, const int32_t* d_ref_index, const int32_t* d_cell_start, int64_t m, float ox,
                                        float oy, float oz, float cell, int nx, int ny, int nz, const float* d_src, int64_t n, float radius,
                                        float px, float py, float pz, const double* d_state, double* d_partials, void* stream) {
  ACEZ_REQUIRE(m >= 0 && m <= ACEZ_MAX_COUNT && n >= 1 && n <= ACEZ_MAX_COUNT, "point count out of range (references 0 .. 2^31 - 1, sources 1 .. 2^31 - 1)");
  ACEZ_REQUIRE(d_cell_start && (m == 0 || (d_ref && d_ref_index)) && d_src && d_state && d_partials, "null pointer");
  GE_REQUIRE_GRID();
  ACEZ_REQUIRE(isfinite(radius) && radius > 0.0f, "the radius must be positive and finite");
  ACEZ_REQUIRE(!(cell < radius * 1.0009765625f), "the cell edge must be at least radius * (1 + 2^-10)");
  ACEZ_REQUIRE(isfinite(px) && isfinite(py) && isfinite(pz), "non-finite pivot");
  if (int rc = acez::require_device("the ICP correspondence search runs on a gfx950 GPU")) return rc;
  const Grid g{ox, oy, oz, cell, nx, ny, nz};
  const int plain = ACEZ_DIAG_ENV("ACEZ_GEOM_PLAIN") != nullptr;    // diagnostics build: every workgroup takes the per-lane form
  hipLaunchKernelGGL(geom_icp_accumulate_kernel, dim3(blocks_for(n, GN_THREADS)), dim3(GN_THREADS), 0, (hipStream_t)stream,
                     d_ref, d_ref_index, d_cell_start, (int)m, g, d_src, n, radius * radius, px, py, pz, d_state, d_partials, plain);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_geom_icp_update(const double* d_partials, int64_t n, float px, float py, float pz, int with_scale, double rel_fitness,
                                    double rel_rmse, int max_iterations, double* d_state, double* d_history, void* stream) {
  ACEZ_REQUIRE(n >= 1 && n <= ACEZ_MAX_COUNT, "point count out of range (sources 1 .. 2^31 - 1)");
  ACEZ_REQUIRE(d_partials && d_state && d_history, "null pointer");
  ACEZ_REQUIRE(isfinite(px) && isfinite(py) && isfinite(pz), "non-finite pivot");
  ACEZ_REQUIRE(max_iterations >= 1, "max_iterations must be at least 1");
  ACEZ_REQUIRE(isfinite(rel_fitness) && rel_fitness >= 0.0 && isfinite(rel_rmse) && rel_rmse >= 0.0,
               "the tolerances must be finite and not negative");
  if (int rc = acez::require_device("the ICP update runs on a gfx950 GPU")) return rc;
  hipLaunchKernelGGL(geom_icp_update_kernel, dim3(1), dim3(GN_THREADS), 0, (hipStream_t)stream, d_partials, (n + GN_THREADS - 1) / GN_THREADS, n,
                     px, py, pz, with_scale != 0, rel_fitness, rel_rmse, max_iterations, d_state, d_history);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
