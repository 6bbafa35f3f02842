// geometry_api.hip -- nearest-neighbour distances between two point clouds on a uniform grid, and the voxel downsample
// (include/acez.h section N: acez_geom_cells, acez_geom_nearest, acez_geom_voxel_means). eval_geometry.py.
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
// No atomics, no communication between workgroups, plain loads and stores. Every range read from the cell table is clamped to
// [0, m], so every loop is bounded by m and a malformed table cannot cause a read out of bounds.
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "acez_common.h"

namespace {

constexpr int GE_THREADS = 256;     // cells, voxel means
constexpr int GN_THREADS = 256;     // nearest: queries per workgroup
constexpr int GN_WAVES = GN_THREADS / 64;
constexpr int GE_CHUNK = 1024;      // staged points per pass: 16 KiB of LDS
constexpr int GE_MAX_ROWS = 12;     // (jspan + 2) * (kspan + 2) with the queries in one row of cells, or in two adjacent rows
constexpr int GE_MAX_ISPAN = 4;     // the staged x-range is at most 6 cells where a lane's own is 3
constexpr int GE_MAX_DIM = 1024;
constexpr int64_t GE_MAX_CELLS = (int64_t)1 << 24;
constexpr int64_t GE_MAX_COUNT = ((int64_t)1 << 31) - 1;

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

struct Best {
  float d2;
  int idx;
};

__device__ inline void consider(float qx, float qy, float qz, float px, float py, float pz, int idx, float r2, Best& b) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  if (d2 <= r2 && (d2 < b.d2 || (d2 == b.d2 && idx < b.idx))) {
    b.d2 = d2;
    b.idx = idx;
  }
}

__device__ inline int wave_min(int v) {
  for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
  return v;
}

__global__ void __launch_bounds__(GN_THREADS) geom_nearest_kernel(const float* __restrict__ ref, const int32_t* __restrict__ ref_index,
                                                                   const int32_t* __restrict__ cell_start, int m, Grid g,
                                                                   const float* __restrict__ query, int64_t n, float r2,
                                                                   float* __restrict__ out_d2, int32_t* __restrict__ out_index, int plain) {
  __shared__ float4 s_pts[GE_CHUNK];
  __shared__ int s_red[GN_WAVES][6];
  __shared__ int s_lo[GE_MAX_ROWS], s_hi[GE_MAX_ROWS];
  const int t = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * GN_THREADS + t;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  bool live = false;
  if (q < n) {
    qx = query[3 * q], qy = query[3 * q + 1], qz = query[3 * q + 2];
    live = isfinite(qx) && isfinite(qy) && isfinite(qz);
  }
  const int ci = axis_cell(qx, g.ox, g.c, g.nx), cj = axis_cell(qy, g.oy, g.c, g.ny), ck = axis_cell(qz, g.oz, g.c, g.nz);
  Best best{INFINITY, INT_MAX};

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
            consider(qx, qy, qz, pt.x, pt.y, pt.z, __float_as_int(pt.w), r2, best);
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
        for (int64_t p = lo; p < hi; ++p) consider(qx, qy, qz, ref[3 * p], ref[3 * p + 1], ref[3 * p + 2], ref_index[p], r2, best);
      }
  }
  if (q < n) {
    out_d2[q] = best.d2;
    out_index[q] = best.idx == INT_MAX ? -1 : best.idx;
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

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + GE_THREADS - 1) / GE_THREADS); }

}  // namespace

#define GE_REQUIRE_GRID()                                                                                                          \
  ACEZ_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= GE_MAX_DIM && ny <= GE_MAX_DIM && nz <= GE_MAX_DIM,                          \
               "grid dimensions must be in 1 .. 1024");                                                                            \
  ACEZ_REQUIRE((int64_t)nx * ny * nz <= GE_MAX_CELLS, "grid too large (more than 2^24 cells)");                                    \
  ACEZ_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz), "non-finite grid origin");                                            \
  ACEZ_REQUIRE(isfinite(cell) && cell > 0.0f, "the cell edge must be positive and finite")

extern "C" int acez_geom_cells(const float* d_points, int64_t n, float ox, float oy, float oz, float cell, int nx, int ny, int nz,
                               int32_t* d_out_cells, void* stream) {
  ACEZ_REQUIRE(n >= 0 && n <= GE_MAX_COUNT, "point count out of range (0 .. 2^31 - 1)");
  ACEZ_REQUIRE(n == 0 || (d_points && d_out_cells), "null pointer");
  GE_REQUIRE_GRID();
  if (int rc = acez::require_device("the point grid runs on a gfx950 GPU")) return rc;
  if (n == 0) return ACEZ_OK;
  const Grid g{ox, oy, oz, cell, nx, ny, nz};
  hipLaunchKernelGGL(geom_cells_kernel, dim3(blocks_for(n)), dim3(GE_THREADS), 0, (hipStream_t)stream, d_points, n, g, d_out_cells);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_geom_nearest(const float* d_ref, const int32_t* d_ref_index, const int32_t* d_cell_start, int64_t m, float ox, float oy,
                                 float oz, float cell, int nx, int ny, int nz, const float* d_query, int64_t n, float radius,
                                 float* d_out_d2, int32_t* d_out_index, void* stream) {
  ACEZ_REQUIRE(m >= 0 && m <= GE_MAX_COUNT && n >= 0 && n <= GE_MAX_COUNT, "point count out of range (0 .. 2^31 - 1)");
  ACEZ_REQUIRE(d_cell_start && (m == 0 || (d_ref && d_ref_index)) && (n == 0 || (d_query && d_out_d2 && d_out_index)), "null pointer");
  GE_REQUIRE_GRID();
  ACEZ_REQUIRE(isfinite(radius) && radius > 0.0f, "the radius must be positive and finite");
  // with this margin a reference within the radius is never two cells away (section N)
  ACEZ_REQUIRE(!(cell < radius * 1.0009765625f), "the cell edge must be at least radius * (1 + 2^-10)");
  if (int rc = acez::require_device("the nearest-neighbour search runs on a gfx950 GPU")) return rc;
  if (n == 0) return ACEZ_OK;
  const Grid g{ox, oy, oz, cell, nx, ny, nz};
  const int plain = ACEZ_DIAG_ENV("ACEZ_GEOM_PLAIN") != nullptr;    // diagnostics build: every workgroup takes the per-lane form
  hipLaunchKernelGGL(geom_nearest_kernel, dim3((unsigned)((n + GN_THREADS - 1) / GN_THREADS)), dim3(GN_THREADS), 0, (hipStream_t)stream, d_ref, d_ref_index, d_cell_start,
                     (int)m, g, d_query, n, radius * radius, d_out_d2, d_out_index, plain);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_geom_voxel_means(const float* d_points, int64_t n, const int32_t* d_segment_start, int64_t segments, float* d_out_means,
                                     void* stream) {
  ACEZ_REQUIRE(n >= 0 && n <= GE_MAX_COUNT && segments >= 0 && segments <= GE_MAX_COUNT, "count out of range (0 .. 2^31 - 1)");
  ACEZ_REQUIRE(d_segment_start && (n == 0 || d_points) && (segments == 0 || d_out_means), "null pointer");
  if (int rc = acez::require_device("the voxel downsample runs on a gfx950 GPU")) return rc;
  if (segments == 0) return ACEZ_OK;
  hipLaunchKernelGGL(geom_voxel_means_kernel, dim3(blocks_for(segments)), dim3(GE_THREADS), 0, (hipStream_t)stream, d_points, n,
                     d_segment_start, segments, d_out_means);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
