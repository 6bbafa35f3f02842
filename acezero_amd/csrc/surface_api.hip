// surface_api.hip -- a mesh scored by its surface, not by its vertices: area-proportional samples of the faces, and the polygon crop of
// the Tanks and Temples crop files (include/acez.h section O: acez_geom_face_counts, acez_geom_sample_faces, acez_geom_crop_polygon).
// eval_geometry.py --sample_spacing / --crop_file.
//
// The header's section O is the definition: every operation below is written in its order, the unit is built with -ffp-contract=off,
// and tests/surface_restated.py restates it in numpy (fp64 and uint64) for the bit-for-bit comparison.
//
// counts   one lane per face: the fp64 area, and the face's own number of samples from its own random draw.
// sample   one lane per sample. The lane finds its face in the exclusive offsets by a binary search of its own: ceil(log2 k) steps, the
//          same number in every lane, no branch that depends on the data. Neighbouring lanes hold neighbouring samples, so all but the
//          last few steps read the same address in the whole wavefront (one request, served from L2), and the steps that differ touch
//          one or two cache lines. The alternative, one search per wavefront and a walk along the offsets from there, has a trip count
//          that depends on the data (a run of faces without samples is walked by every lane behind it) and serialises the wavefront
//          where the binary search does not; DESIGN.md section 4n.
// crop     one lane per point, the polygon staged in LDS as doubles; every lane walks all edges, so each LDS read is a broadcast.
// No atomics, no communication between workgroups, plain loads and stores. Every index read from device memory (a face's vertices, a
// lane's face) is clamped to its array before it is used as an address: wrong tables give wrong numbers, never an access out of bounds.
#include <math.h>
#include <stdint.h>

#include "acez_common.h"
#include "launch1d.h"
#include "ransac_math.h"

namespace {

using namespace acez;
using rsm::mix64;

constexpr int SF_THREADS = 256;
constexpr int SF_MAX_POLYGON = 1024;
constexpr uint64_t SF_STRIDE = 0xD1B54A32D192ED03ULL;
constexpr double SF_2_53 = 1.0 / 9007199254740992.0;   // 2^-53
constexpr double SF_2_24 = 1.0 / 16777216.0;            // 2^-24

__device__ __forceinline__ uint64_t face_key(uint64_t seed_mixed, int64_t t) { return mix64(seed_mixed ^ (uint64_t)t); }

__device__ __forceinline__ int clamp_index(int v, int m) { return v < 0 ? 0 : (v > m - 1 ? m - 1 : v); }

__global__ void __launch_bounds__(SF_THREADS) face_counts_kernel(const float* __restrict__ vertices, int m, const int32_t* __restrict__ faces,
                                                                 int64_t k, double density, uint64_t seed_mixed,
                                                                 int32_t* __restrict__ counts, double* __restrict__ areas) {
  const int64_t t = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x;
  if (t >= k) return;
  const int ia = faces[3 * t], ib = faces[3 * t + 1], ic = faces[3 * t + 2];
  double area = -1.0;
  int count = 0;
  if (ia >= 0 && ia < m && ib >= 0 && ib < m && ic >= 0 && ic < m) {
    const double ax = vertices[3 * (int64_t)ia], ay = vertices[3 * (int64_t)ia + 1], az = vertices[3 * (int64_t)ia + 2];
    const double e1x = (double)vertices[3 * (int64_t)ib] - ax, e1y = (double)vertices[3 * (int64_t)ib + 1] - ay,
                 e1z = (double)vertices[3 * (int64_t)ib + 2] - az;
    const double e2x = (double)vertices[3 * (int64_t)ic] - ax, e2y = (double)vertices[3 * (int64_t)ic + 1] - ay,
                 e2z = (double)vertices[3 * (int64_t)ic + 2] - az;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double s = (nx * nx + ny * ny) + nz * nz;
    const double a = 0.5 * sqrt(s);
    if (isfinite(a)) {
      area = a;
      const double x = a * density, f = floor(x);
      const double u0 = (double)(face_key(seed_mixed, t) >> 11) * SF_2_53;
      count = (f < 1073741824.0 ? (int)f : 1 << 30) + (u0 < x - f ? 1 : 0);
    }
  }
  counts[t] = count;
  areas[t] = area;
}

__global__ void __launch_bounds__(SF_THREADS) sample_faces_kernel(const float* __restrict__ vertices, int m, const int32_t* __restrict__ faces,
                                                                  int k, const int64_t* __restrict__ offsets, int64_t n, uint64_t seed_mixed,
                                                                  const uint8_t* __restrict__ colours, float* __restrict__ points,
                                                                  int32_t* __restrict__ face_index, uint8_t* __restrict__ out_colours) {
  const int64_t j = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x;
  if (j >= n) return;
  // the last t in 0 .. k - 1 with offsets[t] <= j: offsets[lo] <= j < offsets[hi] with offsets[k] taken as +inf; mid is in 1 .. k - 1
  int lo = 0, hi = k;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    const bool le = offsets[mid] <= j;
    lo = le ? mid : lo;
    hi = le ? hi : mid;
  }
  const int t = lo;
  const uint64_t i = (uint64_t)j - (uint64_t)offsets[t];
  const uint64_t r = mix64(face_key(seed_mixed, t) + (i + 1) * SF_STRIDE);
  double u = (double)(r >> 40) * SF_2_24, v = (double)((r >> 16) & 0xFFFFFF) * SF_2_24;
  if (u + v > 1.0) {
    u = 1.0 - u;
    v = 1.0 - v;
  }
  const int64_t ia = clamp_index(faces[3 * (int64_t)t], m), ib = clamp_index(faces[3 * (int64_t)t + 1], m),
                ic = clamp_index(faces[3 * (int64_t)t + 2], m);
  for (int c = 0; c < 3; ++c) {
    const double a = vertices[3 * ia + c];
    const double e1 = (double)vertices[3 * ib + c] - a, e2 = (double)vertices[3 * ic + c] - a;
    points[3 * j + c] = (float)((a + u * e1) + v * e2);
  }
  face_index[j] = t;
  if (colours) {
    const double w = (1.0 - u) - v;
    for (int c = 0; c < 3; ++c) {
      const double q = floor((((w * (double)colours[3 * ia + c] + u * (double)colours[3 * ib + c]) + v * (double)colours[3 * ic + c])) + 0.5);
      out_colours[3 * j + c] = (uint8_t)(q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q));
    }
  }
}

// axis 0 (X): (u, v, w) = (y, z, x); 1 (Y): (x, z, y); 2 (Z): (x, y, z)
__global__ void __launch_bounds__(SF_THREADS) crop_polygon_kernel(const float* __restrict__ pts, int64_t n, const float* __restrict__ polygon,
                                                                  int corners, int axis, float axis_min, float axis_max,
                                                                  uint8_t* __restrict__ keep) {
  __shared__ double s_u[SF_MAX_POLYGON], s_v[SF_MAX_POLYGON];
  for (int e = threadIdx.x; e < corners; e += SF_THREADS) {
    s_u[e] = polygon[2 * e];
    s_v[e] = polygon[2 * e + 1];
  }
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x;
  if (p >= n) return;
  const float x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
  const float uf = axis == 0 ? y : x, vf = axis == 2 ? y : z, w = axis == 0 ? x : (axis == 1 ? y : z);
  const double u = uf, v = vf;
  int crossings = 0;
  double ui = s_u[corners - 1], vi = s_v[corners - 1];            // edge corners - 1 -> 0 first: the parity does not depend on the order
  for (int e = 0; e < corners; ++e) {
    const double uj = s_u[e], vj = s_v[e];
    if ((vi > v) != (vj > v)) {
      const double lhs = (u - ui) * (vj - vi), rhs = (v - vi) * (uj - ui);
      crossings += (vj > vi ? lhs < rhs : lhs > rhs) ? 1 : 0;
    }
    ui = uj;
    vi = vj;
  }
  const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && axis_min <= w && w <= axis_max && (crossings & 1);
  keep[p] = ok ? 1 : 0;
}

}  // namespace

extern "C" int acez_geom_face_counts(const float* d_vertices, int64_t m, const int32_t* d_faces, int64_t k, double density, uint64_t seed,
                                     int32_t* d_out_counts, double* d_out_areas, void* stream) {
  ACEZ_REQUIRE_COUNTS(m, k);
  ACEZ_REQUIRE((m == 0 || d_vertices) && (k == 0 || (d_faces && d_out_counts && d_out_areas)), "null pointer");
  ACEZ_REQUIRE(isfinite(density) && density > 0.0, "the density must be positive and finite");
  if (int rc = acez::require_device("the mesh sampler runs on a gfx950 GPU")) return rc;
  if (k == 0) return ACEZ_OK;
  hipLaunchKernelGGL(face_counts_kernel, dim3(blocks_for(k, SF_THREADS)), dim3(SF_THREADS), 0, (hipStream_t)stream, d_vertices, (int)m, d_faces, k, density,
                     mix64(seed), d_out_counts, d_out_areas);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_geom_sample_faces(const float* d_vertices, int64_t m, const int32_t* d_faces, int64_t k, const int64_t* d_offsets, int64_t n,
                                      uint64_t seed, const uint8_t* d_colours, float* d_out_points, int32_t* d_out_face,
                                      uint8_t* d_out_colours, void* stream) {
  ACEZ_REQUIRE_COUNTS(m, k, n);
  ACEZ_REQUIRE(n == 0 || (m >= 1 && k >= 1), "samples of a mesh without vertices or without faces");
  ACEZ_REQUIRE(n == 0 || (d_vertices && d_faces && d_offsets && d_out_points && d_out_face), "null pointer");
  ACEZ_REQUIRE((d_colours == nullptr) == (d_out_colours == nullptr), "vertex colours and sample colours go together");
  if (int rc = acez::require_device("the mesh sampler runs on a gfx950 GPU")) return rc;
  if (n == 0) return ACEZ_OK;
  hipLaunchKernelGGL(sample_faces_kernel, dim3(blocks_for(n, SF_THREADS)), dim3(SF_THREADS), 0, (hipStream_t)stream, d_vertices, (int)m, d_faces, (int)k,
                     d_offsets, n, mix64(seed), d_colours, d_out_points, d_out_face, d_out_colours);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_geom_crop_polygon(const float* d_points, int64_t n, const float* d_polygon, int corners, int axis, float axis_min,
                                      float axis_max, uint8_t* d_out_keep, void* stream) {
  ACEZ_REQUIRE_POINT_COUNTS(n);
  ACEZ_REQUIRE(corners >= 3 && corners <= SF_MAX_POLYGON, "the polygon must have 3 .. 1024 corners");
  ACEZ_REQUIRE(d_polygon && (n == 0 || (d_points && d_out_keep)), "null pointer");
  ACEZ_REQUIRE(axis >= 0 && axis <= 2, "the orthogonal axis must be 0, 1 or 2");
  ACEZ_REQUIRE(isfinite(axis_min) && isfinite(axis_max) && axis_min <= axis_max, "the axis bounds must be finite, the lower not above the upper");
  if (int rc = acez::require_device("the polygon crop runs on a gfx950 GPU")) return rc;
  if (n == 0) return ACEZ_OK;
  hipLaunchKernelGGL(crop_polygon_kernel, dim3(blocks_for(n, SF_THREADS)), dim3(SF_THREADS), 0, (hipStream_t)stream, d_points, n, d_polygon, corners, axis,
                     axis_min, axis_max, d_out_keep);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
