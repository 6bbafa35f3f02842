// fusion_api.hip -- TSDF fusion of depth maps and surface-net mesh extraction (include/acez.h section K: acez_tsdf_integrate,
// acez_tsdf_cells, acez_tsdf_faces). fuse_depth.py.
//
// The header's section K is the definition: every float operation below is written in its order, the unit is built with
// -ffp-contract=off, and tests/tsdf_restated.py restates it in numpy float32 for the bit-for-bit comparison.
//
// integrate  one 256-thread workgroup per brick of 32 x 4 x 2 voxels (x fastest: a wave is two rows of 32 voxels, two 128-byte
//            segments per volume load or store; one voxel per thread, so the accesses are 4 bytes per lane -- 16 bytes per lane would
//            need four voxels per thread). The voxel is read once, stays in registers over the call's frames and is written once, and
//            only if a frame touched it. The frame index is uniform, so a row is read through scalar loads. The frustum test runs
//            once per (brick, frame), thread f on frame f, before the walk; its verdicts sit in LDS and the skip is wave-uniform.
// cells      one thread per voxel index; flags the active cells, or (second mode) writes their vertices at their ranks.
// faces      one thread per (axis, voxel index); flags the quads, or (second mode) writes their triangles at their ranks.
// No atomics, no communication between workgroups, plain loads and stores.
#include <math.h>
#include <stdint.h>

#include "acez_common.h"

namespace {

constexpr int FU_THREADS = 256;
constexpr int FU_BX = 32, FU_BY = 4, FU_BZ = 2;   // the brick; FU_BX * FU_BY * FU_BZ == FU_THREADS
constexpr int FU_MAX_SIDE = 32768;
constexpr double FU_SLACK = 1e-5;                  // of the magnitudes entering a plane's value; rounding of steps 1-4 is below 5e-7 of them

struct Volume {
  int nx, ny, nz;
  float ox, oy, oz, v;
};

// true: no voxel of the box [lo, hi] (voxel centres, world) can pass steps 3 and 5 for this frame. Every plane value is linear in
// the point, so its extremes over the box are at the corners; `slack` covers the difference between the double value and what a
// voxel's thread computes in fp32.
__device__ bool brick_outside(const acez_tsdf_frame& fr, const double lo[3], const double hi[3]) {
  const double ax = fmax(fabs(lo[0]), fabs(hi[0])), ay = fmax(fabs(lo[1]), fabs(hi[1])), az = fmax(fabs(lo[2]), fabs(hi[2]));
  double M[3];
  for (int r = 0; r < 3; ++r)
    M[r] = fabs((double)fr.m[4 * r]) * ax + fabs((double)fr.m[4 * r + 1]) * ay + fabs((double)fr.m[4 * r + 2]) * az + fabs((double)fr.m[4 * r + 3]);
  const double f = fr.focal, w = fr.w, h = fr.h;
  const double sz = FU_SLACK * M[2];
  const double su = FU_SLACK * (f * M[0] + (fabs((double)fr.ppx) + w + 1.0) * M[2]);
  const double sv = FU_SLACK * (f * M[1] + (fabs((double)fr.ppy) + h + 1.0) * M[2]);
  const double bu0 = (double)fr.ppx + 0.5, bu1 = (double)fr.ppx - w + 0.5;
  const double bv0 = (double)fr.ppy + 0.5, bv1 = (double)fr.ppy - h + 0.5;
  bool behind = true, left = true, right = true, above = true, below = true;
  for (int c = 0; c < 8; ++c) {
    const double x = (c & 1) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 4) ? hi[2] : lo[2];
    const double xc = fr.m[0] * x + fr.m[1] * y + fr.m[2] * z + fr.m[3];
    const double yc = fr.m[4] * x + fr.m[5] * y + fr.m[6] * z + fr.m[7];
    const double zc = fr.m[8] * x + fr.m[9] * y + fr.m[10] * z + fr.m[11];
    behind = behind && (zc < -sz);                       // inside needs zc > 0
    left = left && (f * xc + bu0 * zc < -su);            // inside needs u >= -0.5     <=> f xc + (ppx + 0.5) zc >= 0     (zc > 0)
    right = right && (f * xc + bu1 * zc > su);           // inside needs u < w - 0.5   <=> f xc + (ppx - w + 0.5) zc < 0
    above = above && (f * yc + bv0 * zc < -sv);
    below = below && (f * yc + bv1 * zc > sv);
  }
  return behind || left || right || above || below;
}

__global__ void __launch_bounds__(FU_THREADS) integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ colour,
                                                               Volume vol, float tau, const uint16_t* __restrict__ depth,
                                                               const uint8_t* __restrict__ rgb, const acez_tsdf_frame* __restrict__ frames,
                                                               int n_frames, float depth_unit, float max_depth, float max_weight,
                                                               int frustum_skip) {
  __shared__ uint8_t s_skip[ACEZ_TSDF_MAX_FRAMES];
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * FU_BX, j0 = blockIdx.y * FU_BY, k0 = blockIdx.z * FU_BZ;
  if (frustum_skip) {
    if (t < n_frames) {
      const int i1 = min(i0 + FU_BX, vol.nx) - 1, j1 = min(j0 + FU_BY, vol.ny) - 1, k1 = min(k0 + FU_BZ, vol.nz) - 1;
      const double v = vol.v;
      const double lo[3] = {vol.ox + i0 * v, vol.oy + j0 * v, vol.oz + k0 * v};
      const double hi[3] = {vol.ox + i1 * v, vol.oy + j1 * v, vol.oz + k1 * v};
      s_skip[t] = brick_outside(frames[t], lo, hi) ? 1 : 0;
    }
    __syncthreads();
  }
  const int i = i0 + (t & (FU_BX - 1)), j = j0 + ((t >> 5) & (FU_BY - 1)), k = k0 + (t >> 7);
  if (i >= vol.nx || j >= vol.ny || k >= vol.nz) return;   // (after the only barrier)
  const int64_t n_vox = (int64_t)vol.nx * vol.ny * vol.nz;
  const int64_t at = ((int64_t)k * vol.ny + j) * vol.nx + i;
  const float px = vol.ox + (float)i * vol.v;
  const float py = vol.oy + (float)j * vol.v;
  const float pz = vol.oz + (float)k * vol.v;
  float d_t = tsdf[at], d_w = weight[at];
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  const bool with_colour = colour != nullptr && rgb != nullptr;
  if (with_colour) {
    c0 = colour[at];
    c1 = colour[n_vox + at];
    c2 = colour[2 * n_vox + at];
  }
  bool touched = false;
  for (int f = 0; f < n_frames; ++f) {
    if (frustum_skip && s_skip[f]) continue;                // uniform over the workgroup
    const acez_tsdf_frame& fr = frames[f];                   // uniform address: scalar loads
    const float xc = ((fr.m[0] * px + fr.m[1] * py) + fr.m[2] * pz) + fr.m[3];
    const float yc = ((fr.m[4] * px + fr.m[5] * py) + fr.m[6] * pz) + fr.m[7];
    const float zc = ((fr.m[8] * px + fr.m[9] * py) + fr.m[10] * pz) + fr.m[11];
    if (!(zc > 0.0f)) continue;
    const float u = (fr.focal * xc) / zc + fr.ppx;
    const float w_ = (fr.focal * yc) / zc + fr.ppy;
    if (!(u >= -0.5f && u < (float)fr.w - 0.5f && w_ >= -0.5f && w_ < (float)fr.h - 0.5f)) continue;
    const int ix = min((int)floorf(u + 0.5f), fr.w - 1);
    const int iy = min((int)floorf(w_ + 0.5f), fr.h - 1);
    const int64_t pix = fr.offset + (int64_t)iy * fr.w + ix;   // in [offset, offset + h * w): the host checked that range
    const uint16_t raw = depth[pix];
    if (raw == 0) continue;
    const float d = (float)raw * depth_unit;
    if (d > max_depth) continue;
    const float sdf = d - zc;
    if (sdf < -tau) continue;
    const float tt = fminf(1.0f, sdf / tau);
    const float w1 = d_w + 1.0f;
    d_t = (d_t * d_w + tt) / w1;
    if (with_colour) {
      c0 = (c0 * d_w + (float)rgb[3 * pix]) / w1;
      c1 = (c1 * d_w + (float)rgb[3 * pix + 1]) / w1;
      c2 = (c2 * d_w + (float)rgb[3 * pix + 2]) / w1;
    }
    d_w = fminf(w1, max_weight);
    touched = true;
  }
  if (!touched) return;
  tsdf[at] = d_t;
  weight[at] = d_w;
  if (with_colour) {
    colour[at] = c0;
    colour[n_vox + at] = c1;
    colour[2 * n_vox + at] = c2;
  }
}

// corner numbers (dx + 2 dy + 4 dz) of the 12 edges, lower end first; the axis of edge e is e / 4
__device__ const int8_t kEdgeA[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3};
__device__ const int8_t kEdgeB[12] = {1, 3, 5, 7, 2, 3, 6, 7, 4, 5, 6, 7};

__global__ void __launch_bounds__(FU_THREADS) cells_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                           const float* __restrict__ colour, Volume vol, float min_weight,
                                                           uint8_t* __restrict__ active, const int32_t* __restrict__ rank,
                                                           float* __restrict__ out_v, uint8_t* __restrict__ out_c, int64_t n_vertices) {
  const int64_t n_vox = (int64_t)vol.nx * vol.ny * vol.nz;
  const int64_t at = (int64_t)blockIdx.x * FU_THREADS + threadIdx.x;
  if (at >= n_vox) return;
  const int i = (int)(at % vol.nx), j = (int)((at / vol.nx) % vol.ny), k = (int)(at / ((int64_t)vol.nx * vol.ny));
  const bool in_range = i < vol.nx - 1 && j < vol.ny - 1 && k < vol.nz - 1;
  if (!in_range) {
    if (!rank) active[at] = 0;
    return;
  }
  if (rank && !active[at]) return;
  float d[8];
  int64_t idx[8];
  bool known = true;
  int inside = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    idx[c] = at + (c & 1) + (int64_t)((c >> 1) & 1) * vol.nx + (int64_t)(c >> 2) * vol.nx * vol.ny;
    d[c] = tsdf[idx[c]];
    known = known && (weight[idx[c]] >= min_weight);
    inside += d[c] < 0.0f ? 1 : 0;
  }
  const bool is_active = known && inside != 0 && inside != 8;
  if (!rank) {
    active[at] = is_active ? 1 : 0;
    return;
  }
  const int64_t id = (int64_t)rank[at] - 1;
  if (!is_active || id < 0 || id >= n_vertices) return;
  const bool with_colour = colour != nullptr && out_c != nullptr;
  float sum[3] = {0.0f, 0.0f, 0.0f}, csum[3] = {0.0f, 0.0f, 0.0f};
  int count = 0;
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    const int a = kEdgeA[e], b = kEdgeB[e];
    const float da = d[a], db = d[b];
    if ((da < 0.0f) == (db < 0.0f)) continue;
    const float s = da / (da - db);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const float pa = (float)((a >> ax) & 1), pb = (float)((b >> ax) & 1);
      sum[ax] = sum[ax] + (pa + s * (pb - pa));
    }
    if (with_colour) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float ca = colour[ch * n_vox + idx[a]], cb = colour[ch * n_vox + idx[b]];
        csum[ch] = csum[ch] + (ca + s * (cb - ca));
      }
    }
    ++count;
  }
  const float n = (float)count;                             // >= 1: an active cell has a crossing
  out_v[3 * id] = vol.ox + ((float)i + sum[0] / n) * vol.v;
  out_v[3 * id + 1] = vol.oy + ((float)j + sum[1] / n) * vol.v;
  out_v[3 * id + 2] = vol.oz + ((float)k + sum[2] / n) * vol.v;
  if (with_colour) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out_c[3 * id + ch] = (uint8_t)fminf(fmaxf(floorf(csum[ch] / n + 0.5f), 0.0f), 255.0f);
  }
}

__global__ void __launch_bounds__(FU_THREADS) faces_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, Volume vol,
                                                           float min_weight, const uint8_t* __restrict__ active, uint8_t* __restrict__ flags,
                                                           const int32_t* __restrict__ vrank, const int32_t* __restrict__ erank,
                                                           int32_t* __restrict__ out_f, int64_t n_faces) {
  const int64_t n_vox = (int64_t)vol.nx * vol.ny * vol.nz;
  const int64_t e = (int64_t)blockIdx.x * FU_THREADS + threadIdx.x;
  if (e >= 3 * n_vox) return;
  const int axis = (int)(e / n_vox);
  const int64_t at = e - axis * n_vox;
  if (erank && !flags[e]) return;
  const int p[3] = {(int)(at % vol.nx), (int)((at / vol.nx) % vol.ny), (int)(at / ((int64_t)vol.nx * vol.ny))};
  const int dims[3] = {vol.nx, vol.ny, vol.nz};
  const int64_t stride[3] = {1, vol.nx, (int64_t)vol.nx * vol.ny};
  const int b = (axis + 1) % 3, c = (axis + 2) % 3;
  // the four cells p - e_b - e_c, p - e_c, p, p - e_b exist iff p_a <= n_a - 2 and 1 <= p_b <= n_b - 2 (p_c alike)
  bool quad = p[axis] < dims[axis] - 1 && p[b] >= 1 && p[b] < dims[b] - 1 && p[c] >= 1 && p[c] < dims[c] - 1;
  int64_t cell[4] = {0, 0, 0, 0};
  bool lower_inside = false;
  if (quad) {
    const int64_t hi = at + stride[axis];
    const float da = tsdf[at], db = tsdf[hi];
    lower_inside = da < 0.0f;
    cell[0] = at - stride[b] - stride[c];
    cell[1] = at - stride[c];
    cell[2] = at;
    cell[3] = at - stride[b];
    quad = weight[at] >= min_weight && weight[hi] >= min_weight && lower_inside != (db < 0.0f) && active[cell[0]] && active[cell[1]] &&
           active[cell[2]] && active[cell[3]];
  }
  if (!erank) {
    flags[e] = quad ? 1 : 0;
    return;
  }
  const int64_t row = 2 * ((int64_t)erank[e] - 1);
  if (!quad || row < 0 || row + 2 > n_faces) return;
  const int32_t v0 = vrank[cell[0]] - 1, v1 = vrank[cell[1]] - 1, v2 = vrank[cell[2]] - 1, v3 = vrank[cell[3]] - 1;
  int32_t* o = out_f + 3 * row;
  o[0] = v0;
  o[1] = lower_inside ? v1 : v2;
  o[2] = lower_inside ? v2 : v1;
  o[3] = v0;
  o[4] = lower_inside ? v2 : v3;
  o[5] = lower_inside ? v3 : v2;
}

bool finite_all(const float* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!isfinite(p[i])) return false;
  return true;
}

}  // namespace

#define FU_REQUIRE_DIMS(limit)                                                                                        \
  ACEZ_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "volume dimensions must be at least 1");                                \
  ACEZ_REQUIRE((int64_t)nx * ny <= (limit) && (int64_t)nx * ny * nz <= (limit), "volume too large for 32-bit voxel indices")

extern "C" int acez_tsdf_integrate(float* d_tsdf, float* d_weight, float* d_colour, int nx, int ny, int nz, float ox, float oy, float oz,
                                   float voxel_size, float truncation, const uint16_t* d_depth, const uint8_t* d_rgb, int64_t n_pixels,
                                   const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames, float depth_unit,
                                   float max_depth, float max_weight, int frustum_skip, void* stream) {
  ACEZ_REQUIRE(d_tsdf && d_weight && d_depth && h_frames && d_frames, "null pointer");
  ACEZ_REQUIRE(!d_rgb || d_colour, "colour images without a colour volume");
  FU_REQUIRE_DIMS(((int64_t)1 << 31) - 1);
  const float scal[8] = {ox, oy, oz, voxel_size, truncation, depth_unit, max_depth, max_weight};
  ACEZ_REQUIRE(finite_all(scal, 8), "non-finite origin, voxel size, truncation, depth unit, depth limit or weight cap");
  ACEZ_REQUIRE(voxel_size > 0.0f && truncation > 0.0f, "voxel size and truncation must be positive");
  ACEZ_REQUIRE(depth_unit > 0.0f && max_depth > 0.0f && max_weight > 0.0f, "depth unit, depth limit and weight cap must be positive");
  ACEZ_REQUIRE(n_frames >= 0 && n_frames <= ACEZ_TSDF_MAX_FRAMES, "frame count out of range (0 .. 256 per call)");
  ACEZ_REQUIRE(n_pixels >= 0, "negative depth buffer length");
  for (int f = 0; f < n_frames; ++f) {
    const acez_tsdf_frame& fr = h_frames[f];
    ACEZ_REQUIRE(fr.h >= 1 && fr.w >= 1 && fr.h <= FU_MAX_SIDE && fr.w <= FU_MAX_SIDE, "frame size out of range (1 .. 32768 px per side)");
    ACEZ_REQUIRE(finite_all(fr.m, 12) && isfinite(fr.focal) && isfinite(fr.ppx) && isfinite(fr.ppy), "non-finite pose or intrinsics in the frame table");
    ACEZ_REQUIRE(fr.focal > 0.0f, "focal length must be positive");
    ACEZ_REQUIRE(fr.offset >= 0 && fr.offset <= n_pixels && (int64_t)fr.h * fr.w <= n_pixels - fr.offset, "frame past the end of the depth buffer");
  }
  ACEZ_REQUIRE((ny + FU_BY - 1) / FU_BY <= 65535 && (nz + FU_BZ - 1) / FU_BZ <= 65535, "volume too large (more than 65535 bricks along y or z)");
  if (int rc = acez::require_device("TSDF integration runs on a gfx950 GPU")) return rc;
  if (n_frames == 0) return ACEZ_OK;
  hipStream_t s = (hipStream_t)stream;
  ACEZ_HIP_CHECK(hipMemcpyAsync(d_frames, h_frames, sizeof(acez_tsdf_frame) * (size_t)n_frames, hipMemcpyHostToDevice, s));
  ACEZ_HIP_CHECK(hipStreamSynchronize(s));   // h_frames is the caller's again
  const dim3 grid((nx + FU_BX - 1) / FU_BX, (ny + FU_BY - 1) / FU_BY, (nz + FU_BZ - 1) / FU_BZ);
  const Volume vol{nx, ny, nz, ox, oy, oz, voxel_size};
  hipLaunchKernelGGL(integrate_kernel, grid, dim3(FU_THREADS), 0, s, d_tsdf, d_weight, d_colour, vol, truncation, d_depth, d_rgb,
                     (const acez_tsdf_frame*)d_frames, n_frames, depth_unit, max_depth, max_weight, frustum_skip);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_tsdf_cells(const float* d_tsdf, const float* d_weight, const float* d_colour, int nx, int ny, int nz, float ox, float oy,
                               float oz, float voxel_size, float min_weight, uint8_t* d_active, const int32_t* d_vertex_rank,
                               float* d_out_vertices, uint8_t* d_out_colours, int64_t n_vertices, void* stream) {
  ACEZ_REQUIRE(d_tsdf && d_weight && d_active, "null pointer");
  FU_REQUIRE_DIMS((((int64_t)1 << 31) - 1) / 3);
  ACEZ_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(voxel_size) && voxel_size > 0.0f, "voxel size must be positive, the origin finite");
  ACEZ_REQUIRE(n_vertices >= 0, "negative vertex count");
  ACEZ_REQUIRE(!d_vertex_rank || n_vertices == 0 || d_out_vertices, "vertex ranks without a vertex buffer");
  if (int rc = acez::require_device("mesh extraction runs on a gfx950 GPU")) return rc;
  if (d_vertex_rank && n_vertices == 0) return ACEZ_OK;
  const int64_t n_vox = (int64_t)nx * ny * nz;
  const Volume vol{nx, ny, nz, ox, oy, oz, voxel_size};
  hipLaunchKernelGGL(cells_kernel, dim3((unsigned)((n_vox + FU_THREADS - 1) / FU_THREADS)), dim3(FU_THREADS), 0, (hipStream_t)stream, d_tsdf,
                     d_weight, d_colour, vol, min_weight, d_active, d_vertex_rank, d_out_vertices, d_out_colours, n_vertices);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_tsdf_faces(const float* d_tsdf, const float* d_weight, int nx, int ny, int nz, float min_weight, const uint8_t* d_active,
                               uint8_t* d_edge_flags, const int32_t* d_vertex_rank, const int32_t* d_edge_rank, int32_t* d_out_faces,
                               int64_t n_faces, void* stream) {
  ACEZ_REQUIRE(d_tsdf && d_weight && d_active && d_edge_flags, "null pointer");
  FU_REQUIRE_DIMS((((int64_t)1 << 31) - 1) / 3);
  ACEZ_REQUIRE(n_faces >= 0, "negative face count");
  ACEZ_REQUIRE(!d_edge_rank || n_faces == 0 || (d_vertex_rank && d_out_faces), "edge ranks without vertex ranks or a face buffer");
  if (int rc = acez::require_device("mesh extraction runs on a gfx950 GPU")) return rc;
  if (d_edge_rank && n_faces == 0) return ACEZ_OK;
  const int64_t n_edges = 3 * (int64_t)nx * ny * nz;
  const Volume vol{nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f};
  hipLaunchKernelGGL(faces_kernel, dim3((unsigned)((n_edges + FU_THREADS - 1) / FU_THREADS)), dim3(FU_THREADS), 0, (hipStream_t)stream, d_tsdf,
                     d_weight, vol, min_weight, d_active, d_edge_flags, d_vertex_rank, d_edge_rank, d_out_faces, n_faces);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
