// fusion_api.hip -- TSDF fusion of depth maps, surface-net mesh extraction and frame-to-model tracking (include/acez.h sections K, K2,
// K3: acez_tsdf_integrate, acez_tsdf_cells, acez_tsdf_faces, ...). fuse_depth.py.
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
//
// Section K2 (acez_tsdf_mark, acez_tsdf_integrate_blocks, acez_tsdf_cells_blocks, acez_tsdf_faces_blocks) is the same function on a
// block-sparse volume: 8 x 8 x 8 blocks, stored only where depth puts a surface, found through a table.
// mark             one thread per depth pixel; thread 0 of a workgroup (one frame) inverts the pose in double into LDS; plain byte
//                  stores of 1, every thread that hits a block stores the same value.
// integrate_blocks one 512-thread workgroup per allocated block, thread t = voxel t (x fastest): a wave is one z slice of the block,
//                  256 contiguous bytes per volume load or store. The per-voxel walk is fuse_frames(), the dense kernel's.
// cells_blocks,    one 512-thread workgroup per allocated block; the block and its one-voxel halo (a 10^3 tile of storage offsets,
// faces_blocks     tsdf, weight and, for the faces, the active flags) go to LDS through the table, 13 KB.
//
// Section K3 (acez_tsdf_track_accumulate, acez_tsdf_track_accumulate_blocks, acez_tsdf_track_update) refines poses against the volume:
// accumulate  grid (tiles of the call's largest frame, frames), one lane per depth pixel of a 256-pixel row segment: the pixel's world
//             point under the frame's device-resident pose (fp64), the trilinear tsdf and its gradient from eight (tsdf, weight)
//             pairs, the 29 Gauss-Newton terms, reduced in the order of ordered_sum.h to one row per tile. The dense and the block
//             kernel are one template over the function that finds a voxel's element.
// update      one 256-thread workgroup per frame: the rows' sums in that order, then track_solve.h on thread 0.
//
// The dense and the block kernels differ in where a voxel lies, not in what happens to it. The steps they share are device functions:
// frustum_verdicts (the per-frame skip of a workgroup's box, with the barrier), update_voxel (load, fuse_frames over the call's frames,
// store if touched), write_vertex and write_quad. The host's checks of the frame arguments are check_frame_call, the rows' own checks
// and the table's upload are frame_table.h's, which mvs_api.hip shares.
#include <math.h>
#include <stdint.h>

#include "acez_common.h"
#include "frame_table.h"
#include "ordered_sum.h"
#include "track_solve.h"

namespace {

constexpr int FU_THREADS = 256;
constexpr int FU_BX = 32, FU_BY = 4, FU_BZ = 2;   // the brick; FU_BX * FU_BY * FU_BZ == FU_THREADS
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

// Section K's steps 2-9 for one voxel at (px, py, pz) over the call's frames in table order: the one per-voxel update, used by the dense
// kernel and by the block kernel. `skip` (LDS, one verdict per frame, read if use_skip) is uniform over the workgroup. true: a frame touched it.
__device__ __forceinline__ bool fuse_frames(float px, float py, float pz, float& d_t, float& d_w, float& c0, float& c1, float& c2,
                                            bool with_colour, float tau, const uint16_t* __restrict__ depth, const uint8_t* __restrict__ rgb,
                                            const acez_tsdf_frame* __restrict__ frames, int n_frames, float depth_unit, float max_depth,
                                            float max_weight, bool use_skip, const uint8_t* skip) {
  bool touched = false;
  for (int f = 0; f < n_frames; ++f) {
    if (use_skip && skip[f]) continue;                       // uniform over the workgroup
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
  return touched;
}

// The frustum test of a workgroup's box of voxels, (i0, j0, k0) of extent (ex, ey, ez) clipped to the grid: thread f tests frame f,
// the verdicts go to s_skip. Ends with the workgroup's only barrier; without the skip there is none.
__device__ __forceinline__ void frustum_verdicts(const Volume& vol, int i0, int j0, int k0, int ex, int ey, int ez,
                                                 const acez_tsdf_frame* __restrict__ frames, int n_frames, int frustum_skip, uint8_t* s_skip) {
  if (!frustum_skip) return;
  const int t = threadIdx.x;
  if (t < n_frames) {
    const int i1 = min(i0 + ex, vol.nx) - 1, j1 = min(j0 + ey, vol.ny) - 1, k1 = min(k0 + ez, vol.nz) - 1;
    const double v = vol.v;
    const double lo[3] = {vol.ox + i0 * v, vol.oy + j0 * v, vol.oz + k0 * v};
    const double hi[3] = {vol.ox + i1 * v, vol.oy + j1 * v, vol.oz + k1 * v};
    s_skip[t] = brick_outside(frames[t], lo, hi) ? 1 : 0;
  }
  __syncthreads();
}

// The voxel (i, j, k), stored at element `at` of planes of `plane` elements: read once, fuse_frames() over the call's frames in
// registers, written once and only if a frame touched it.
__device__ __forceinline__ void update_voxel(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ colour, int64_t at,
                                             int64_t plane, const Volume& vol, int i, int j, int k, float tau,
                                             const uint16_t* __restrict__ depth, const uint8_t* __restrict__ rgb,
                                             const acez_tsdf_frame* __restrict__ frames, int n_frames, float depth_unit, float max_depth,
                                             float max_weight, int frustum_skip, const uint8_t* s_skip) {
  const float px = vol.ox + (float)i * vol.v;
  const float py = vol.oy + (float)j * vol.v;
  const float pz = vol.oz + (float)k * vol.v;
  float d_t = tsdf[at], d_w = weight[at];
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  const bool with_colour = colour != nullptr && rgb != nullptr;
  if (with_colour) {
    c0 = colour[at];
    c1 = colour[plane + at];
    c2 = colour[2 * plane + at];
  }
  const bool touched = fuse_frames(px, py, pz, d_t, d_w, c0, c1, c2, with_colour, tau, depth, rgb, frames, n_frames, depth_unit, max_depth,
                                   max_weight, frustum_skip != 0, s_skip);
  if (!touched) return;
  tsdf[at] = d_t;
  weight[at] = d_w;
  if (with_colour) {
    colour[at] = c0;
    colour[plane + at] = c1;
    colour[2 * plane + at] = c2;
  }
}

__global__ void __launch_bounds__(FU_THREADS) integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ colour,
                                                               Volume vol, float tau, const uint16_t* __restrict__ depth,
                                                               const uint8_t* __restrict__ rgb, const acez_tsdf_frame* __restrict__ frames,
                                                               int n_frames, float depth_unit, float max_depth, float max_weight,
                                                               int frustum_skip) {
  __shared__ uint8_t s_skip[ACEZ_TSDF_MAX_FRAMES];
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * FU_BX, j0 = blockIdx.y * FU_BY, k0 = blockIdx.z * FU_BZ;
  frustum_verdicts(vol, i0, j0, k0, FU_BX, FU_BY, FU_BZ, frames, n_frames, frustum_skip, s_skip);
  const int i = i0 + (t & (FU_BX - 1)), j = j0 + ((t >> 5) & (FU_BY - 1)), k = k0 + (t >> 7);
  if (i >= vol.nx || j >= vol.ny || k >= vol.nz) return;   // (after the only barrier)
  update_voxel(tsdf, weight, colour, ((int64_t)k * vol.ny + j) * vol.nx + i, (int64_t)vol.nx * vol.ny * vol.nz, vol, i, j, k, tau, depth, rgb,
               frames, n_frames, depth_unit, max_depth, max_weight, frustum_skip, s_skip);
}

// corner numbers (dx + 2 dy + 4 dz) of the 12 edges, lower end first; the axis of edge e is e / 4
__device__ const int8_t kEdgeA[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3};
__device__ const int8_t kEdgeB[12] = {1, 3, 5, 7, 2, 3, 6, 7, 4, 5, 6, 7};

// Section K's vertex of the active cell (i, j, k) with corner values d[8], written to row `id`: the one definition, used by the dense
// and by the block kernel. idx[c] is corner c's element in a colour plane, `plane` the length of one plane.
__device__ __forceinline__ void write_vertex(const float d[8], const int64_t idx[8], const float* __restrict__ colour, int64_t plane,
                                             const Volume& vol, int i, int j, int k, int64_t id, float* __restrict__ out_v,
                                             uint8_t* __restrict__ out_c) {
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
        const float ca = colour[ch * plane + idx[a]], cb = colour[ch * plane + idx[b]];
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
  write_vertex(d, idx, colour, n_vox, vol, i, j, k, id, out_v, out_c);
}

// The two triangles of a quad, rows `row` and `row + 1` of the faces, from its four cells' vertex ids in the order section K walks them;
// the winding turns with the side the surface is seen from.
__device__ __forceinline__ void write_quad(int32_t* __restrict__ out_f, int64_t row, int32_t v0, int32_t v1, int32_t v2, int32_t v3,
                                           bool lower_inside) {
  int32_t* o = out_f + 3 * row;
  o[0] = v0;
  o[1] = lower_inside ? v1 : v2;
  o[2] = lower_inside ? v2 : v1;
  o[3] = v0;
  o[4] = lower_inside ? v2 : v3;
  o[5] = lower_inside ? v3 : v2;
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
  write_quad(out_f, row, vrank[cell[0]] - 1, vrank[cell[1]] - 1, vrank[cell[2]] - 1, vrank[cell[3]] - 1, lower_inside);
}

// ---------------------------------------------------------------------------------------------- section K2: the block-sparse volume
constexpr int SB = 8, SB_VOX = SB * SB * SB;      // a block; SB_VOX threads per workgroup, thread t = voxel t of the block, x fastest
constexpr int SB_TILE = SB + 2, SB_TILE_N = SB_TILE * SB_TILE * SB_TILE;   // the block and its one-voxel halo, local coordinates -1 .. 8
constexpr int MK_THREADS = 256;

struct Blocks {
  int bx, by, bz;        // the block grid, ceil(n / 8) per axis
  int n_blocks;          // allocated blocks = slots
};

// Per frame, in double, in this order (tests/tsdf_sparse_restated.py restates it): the inverse of the pose's 3 x 3 part by cofactors,
// and the world slack per axis. Thread 0 of a workgroup writes them to LDS.
struct MarkFrame {
  double inv[9];         // world = inv * (camera - t)
  double t[3];
  double slack[3];       // world, per axis: sum_r |inv[a][r]| * FU_SLACK * M_r
  double su, sv;         // pixels
};

__device__ void mark_frame(const acez_tsdf_frame& fr, const Volume& vol, MarkFrame& o) {
  const double r00 = fr.m[0], r01 = fr.m[1], r02 = fr.m[2], r10 = fr.m[4], r11 = fr.m[5], r12 = fr.m[6], r20 = fr.m[8], r21 = fr.m[9], r22 = fr.m[10];
  const double c00 = r11 * r22 - r12 * r21, c01 = r02 * r21 - r01 * r22, c02 = r01 * r12 - r02 * r11;
  const double c10 = r12 * r20 - r10 * r22, c11 = r00 * r22 - r02 * r20, c12 = r02 * r10 - r00 * r12;
  const double c20 = r10 * r21 - r11 * r20, c21 = r01 * r20 - r00 * r21, c22 = r00 * r11 - r01 * r10;
  const double det = (r00 * c00 + r01 * c10) + r02 * c20;
  const double c[9] = {c00, c01, c02, c10, c11, c12, c20, c21, c22};
  for (int e = 0; e < 9; ++e) o.inv[e] = c[e] / det;
  o.t[0] = fr.m[3];
  o.t[1] = fr.m[7];
  o.t[2] = fr.m[11];
  const double v = vol.v;
  const double o3[3] = {vol.ox, vol.oy, vol.oz};
  const int n3[3] = {vol.nx, vol.ny, vol.nz};
  double A[3], e3[3];
  for (int a = 0; a < 3; ++a) A[a] = fmax(fabs(o3[a]), fabs(o3[a] + (double)(n3[a] - 1) * v));
  for (int r = 0; r < 3; ++r) {
    const double M = ((fabs((double)fr.m[4 * r]) * A[0] + fabs((double)fr.m[4 * r + 1]) * A[1]) + fabs((double)fr.m[4 * r + 2]) * A[2]) + fabs((double)fr.m[4 * r + 3]);
    e3[r] = FU_SLACK * M;
  }
  for (int a = 0; a < 3; ++a) o.slack[a] = (fabs(o.inv[3 * a]) * e3[0] + fabs(o.inv[3 * a + 1]) * e3[1]) + fabs(o.inv[3 * a + 2]) * e3[2];
  o.su = FU_SLACK * ((fabs((double)fr.ppx) + (double)fr.w) + 1.0);
  o.sv = FU_SLACK * ((fabs((double)fr.ppy) + (double)fr.h) + 1.0);
}

// grid (ceil(largest h * w / 256), n_frames): workgroup (x, f) takes 256 pixels of frame f
__global__ void __launch_bounds__(MK_THREADS) mark_kernel(uint8_t* __restrict__ flags, Volume vol, Blocks bl, float tau,
                                                          const uint16_t* __restrict__ depth, const acez_tsdf_frame* __restrict__ frames,
                                                          float depth_unit, float max_depth) {
  __shared__ MarkFrame s_mf;
  const acez_tsdf_frame& fr = frames[blockIdx.y];             // uniform address: scalar loads
  if (threadIdx.x == 0) mark_frame(fr, vol, s_mf);
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * MK_THREADS + threadIdx.x;
  if (p >= (int64_t)fr.h * fr.w) return;                      // (after the only barrier)
  const uint16_t raw = depth[fr.offset + p];                  // in [offset, offset + h * w): the host checked that range
  if (raw == 0) return;
  const float d = (float)raw * depth_unit;
  if (d > max_depth) return;
  const int ix = (int)(p % fr.w), iy = (int)(p / fr.w);
  const double dd = d, f = fr.focal;
  const double sd = FU_SLACK * (dd + (double)tau);
  const double zs[2] = {fmax(dd - sd, 0.0), (dd + (double)tau) + sd};
  const double us[2] = {((double)ix - 0.5) - s_mf.su, ((double)ix + 0.5) + s_mf.su};
  const double ws[2] = {((double)iy - 0.5) - s_mf.sv, ((double)iy + 0.5) + s_mf.sv};
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int c = 0; c < 8; ++c) {
    const double z = zs[c >> 2];
    const double x = ((us[c & 1] - (double)fr.ppx) / f) * z, y = ((ws[(c >> 1) & 1] - (double)fr.ppy) / f) * z;
    const double qx = x - s_mf.t[0], qy = y - s_mf.t[1], qz = z - s_mf.t[2];
    for (int a = 0; a < 3; ++a) {
      const double wa = (s_mf.inv[3 * a] * qx + s_mf.inv[3 * a + 1] * qy) + s_mf.inv[3 * a + 2] * qz;
      lo[a] = fmin(lo[a], wa);
      hi[a] = fmax(hi[a], wa);
    }
  }
  const double v = vol.v;
  const double o3[3] = {vol.ox, vol.oy, vol.oz};
  const int n3[3] = {vol.nx, vol.ny, vol.nz};
  int b0[3], b1[3];
  for (int a = 0; a < 3; ++a) {
    const double first = fmax(floor(((lo[a] - s_mf.slack[a]) - o3[a]) / v) - 1.0, 0.0);
    const double last = fmin(ceil(((hi[a] + s_mf.slack[a]) - o3[a]) / v) + 1.0, (double)(n3[a] - 1));
    if (!(first <= last)) return;                             // the box misses the grid (or is not a number)
    b0[a] = (int)first >> 3;
    b1[a] = (int)last >> 3;
  }
  for (int bk = b0[2]; bk <= b1[2]; ++bk)
    for (int bj = b0[1]; bj <= b1[1]; ++bj)
      for (int bi = b0[0]; bi <= b1[0]; ++bi) flags[((int64_t)bk * bl.by + bj) * bl.bx + bi] = 1;
}

__global__ void __launch_bounds__(SB_VOX) integrate_blocks_kernel(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ colour,
                                                                  const int32_t* __restrict__ slot_blocks, Volume vol, Blocks bl, float tau,
                                                                  const uint16_t* __restrict__ depth, const uint8_t* __restrict__ rgb,
                                                                  const acez_tsdf_frame* __restrict__ frames, int n_frames, float depth_unit,
                                                                  float max_depth, float max_weight, int frustum_skip) {
  __shared__ uint8_t s_skip[ACEZ_TSDF_MAX_FRAMES];
  const int t = threadIdx.x;
  const int64_t b = slot_blocks[blockIdx.x];                  // uniform
  if (b < 0 || b >= (int64_t)bl.bx * bl.by * bl.bz) return;   // not a block of this grid: nothing is read or written (uniform)
  const int i0 = (int)(b % bl.bx) * SB, j0 = (int)((b / bl.bx) % bl.by) * SB, k0 = (int)(b / ((int64_t)bl.bx * bl.by)) * SB;
  frustum_verdicts(vol, i0, j0, k0, SB, SB, SB, frames, n_frames, frustum_skip, s_skip);
  const int i = i0 + (t & 7), j = j0 + ((t >> 3) & 7), k = k0 + (t >> 6);
  if (i >= vol.nx || j >= vol.ny || k >= vol.nz) return;   // (after the only barrier) a partial block's voxels beyond the grid
  update_voxel(tsdf, weight, colour, (int64_t)blockIdx.x * SB_VOX + t, (int64_t)bl.n_blocks * SB_VOX, vol, i, j, k, tau, depth, rgb, frames,
               n_frames, depth_unit, max_depth, max_weight, frustum_skip, s_skip);
}

__device__ __forceinline__ int tile_at(int li, int lj, int lk) { return ((lk + 1) * SB_TILE + (lj + 1)) * SB_TILE + (li + 1); }

// The storage element (slot * 512 + voxel) of every voxel of the 10^3 tile around the block at (i0, j0, k0), -1 for a voxel outside
// the grid, in a block without a slot or with a table entry that is no slot (>= n_blocks). Ends with a barrier.
__device__ void load_tile_offsets(const int32_t* __restrict__ table, const Volume& vol, const Blocks& bl, int i0, int j0, int k0,
                                  int32_t* s_off) {
  for (int e = threadIdx.x; e < SB_TILE_N; e += SB_VOX) {
    const int gi = i0 + e % SB_TILE - 1, gj = j0 + (e / SB_TILE) % SB_TILE - 1, gk = k0 + e / (SB_TILE * SB_TILE) - 1;
    int32_t off = -1;
    if (gi >= 0 && gj >= 0 && gk >= 0 && gi < vol.nx && gj < vol.ny && gk < vol.nz) {
      const int32_t slot = table[((int64_t)(gk >> 3) * bl.by + (gj >> 3)) * bl.bx + (gi >> 3)];
      if (slot >= 0 && slot < bl.n_blocks) off = slot * SB_VOX + ((gk & 7) * SB + (gj & 7)) * SB + (gi & 7);
    }
    s_off[e] = off;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(SB_VOX) cells_blocks_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                              const float* __restrict__ colour, const int32_t* __restrict__ table,
                                                              const int32_t* __restrict__ slot_blocks, Volume vol, Blocks bl, float min_weight,
                                                              uint8_t* __restrict__ active, const int32_t* __restrict__ rank,
                                                              float* __restrict__ out_v, uint8_t* __restrict__ out_c, int64_t n_vertices) {
  __shared__ int32_t s_off[SB_TILE_N];
  __shared__ float s_t[SB_TILE_N], s_w[SB_TILE_N];
  const int t = threadIdx.x;
  const int64_t at = (int64_t)blockIdx.x * SB_VOX + t;
  const int64_t b = slot_blocks[blockIdx.x];                  // uniform
  if (b < 0 || b >= (int64_t)bl.bx * bl.by * bl.bz) {          // not a block of this grid (uniform)
    if (!rank) active[at] = 0;
    return;
  }
  const int i0 = (int)(b % bl.bx) * SB, j0 = (int)((b / bl.bx) % bl.by) * SB, k0 = (int)(b / ((int64_t)bl.bx * bl.by)) * SB;
  load_tile_offsets(table, vol, bl, i0, j0, k0, s_off);
  for (int e = t; e < SB_TILE_N; e += SB_VOX) {
    const int32_t off = s_off[e];
    s_t[e] = off >= 0 ? tsdf[off] : 1.0f;
    s_w[e] = off >= 0 ? weight[off] : 0.0f;                    // unknown: min_weight > 0
  }
  __syncthreads();
  const int li = t & 7, lj = (t >> 3) & 7, lk = t >> 6;
  if (rank && !active[at]) return;
  float d[8];
  int64_t idx[8];
  bool known = true;
  int inside = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int e = tile_at(li + (c & 1), lj + ((c >> 1) & 1), lk + (c >> 2));
    idx[c] = s_off[e];
    d[c] = s_t[e];
    known = known && (s_w[e] >= min_weight);
    inside += d[c] < 0.0f ? 1 : 0;
  }
  const bool is_active = known && inside != 0 && inside != 8;
  if (!rank) {
    active[at] = is_active ? 1 : 0;
    return;
  }
  const int64_t id = (int64_t)rank[at] - 1;
  if (!is_active || id < 0 || id >= n_vertices) return;
  write_vertex(d, idx, colour, (int64_t)bl.n_blocks * SB_VOX, vol, i0 + li, j0 + lj, k0 + lk, id, out_v, out_c);
}

__global__ void __launch_bounds__(SB_VOX) faces_blocks_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                              const int32_t* __restrict__ table, const int32_t* __restrict__ slot_blocks,
                                                              Volume vol, Blocks bl, float min_weight, const uint8_t* __restrict__ active,
                                                              uint8_t* __restrict__ flags, const int32_t* __restrict__ vrank,
                                                              const int32_t* __restrict__ erank, int32_t* __restrict__ out_f, int64_t n_faces) {
  __shared__ int32_t s_off[SB_TILE_N];
  __shared__ float s_t[SB_TILE_N], s_w[SB_TILE_N];
  __shared__ uint8_t s_a[SB_TILE_N];
  const int t = threadIdx.x;
  const int64_t plane = (int64_t)bl.n_blocks * SB_VOX;
  const int64_t at = (int64_t)blockIdx.x * SB_VOX + t;
  const int64_t b = slot_blocks[blockIdx.x];                  // uniform
  if (b < 0 || b >= (int64_t)bl.bx * bl.by * bl.bz) {          // not a block of this grid (uniform)
    if (!erank)
      for (int axis = 0; axis < 3; ++axis) flags[axis * plane + at] = 0;
    return;
  }
  const int i0 = (int)(b % bl.bx) * SB, j0 = (int)((b / bl.bx) % bl.by) * SB, k0 = (int)(b / ((int64_t)bl.bx * bl.by)) * SB;
  load_tile_offsets(table, vol, bl, i0, j0, k0, s_off);
  for (int e = t; e < SB_TILE_N; e += SB_VOX) {
    const int32_t off = s_off[e];
    s_t[e] = off >= 0 ? tsdf[off] : 1.0f;
    s_w[e] = off >= 0 ? weight[off] : 0.0f;
    s_a[e] = off >= 0 ? active[off] : 0;                       // a cell outside the grid or in a block without a slot is not active
  }
  __syncthreads();
  const int l[3] = {t & 7, (t >> 3) & 7, t >> 6};
  const int step[3] = {1, SB_TILE, SB_TILE * SB_TILE};
  const int here = tile_at(l[0], l[1], l[2]);
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    const int64_t e = axis * plane + at;
    if (erank && !flags[e]) continue;
    const int bb = (axis + 1) % 3, cc = (axis + 2) % 3;
    const int hi = here + step[axis];
    const int cell[4] = {here - step[bb] - step[cc], here - step[cc], here, here - step[bb]};
    const bool lower_inside = s_t[here] < 0.0f;
    const bool quad = s_w[here] >= min_weight && s_w[hi] >= min_weight && lower_inside != (s_t[hi] < 0.0f) && s_a[cell[0]] && s_a[cell[1]] &&
                      s_a[cell[2]] && s_a[cell[3]];
    if (!erank) {
      flags[e] = quad ? 1 : 0;
      continue;
    }
    const int64_t row = 2 * ((int64_t)erank[e] - 1);
    if (!quad || row < 0 || row + 2 > n_faces) continue;
    write_quad(out_f, row, vrank[s_off[cell[0]]] - 1, vrank[s_off[cell[1]]] - 1, vrank[s_off[cell[2]]] - 1, vrank[s_off[cell[3]]] - 1, lower_inside);
  }
}

// ---------------------------------------------------------------------------------------------- section K3: tracking frames against the volume
constexpr int TK_THREADS = 256, TK_WAVES = TK_THREADS / 64;
using acez::TRACK_TERMS;
using acez::TRACK_STATE;

// where a voxel lies: its element in d_tsdf / d_weight, or -1 for a voxel that has no storage (sparse: a block without a slot).
// The caller has checked 0 <= i < nx (and alike), so every index formed here is inside the volume or the block table.
struct DenseAt {
  __device__ __forceinline__ int64_t operator()(const Volume& vol, int i, int j, int k) const { return ((int64_t)k * vol.ny + j) * vol.nx + i; }
};
struct BlocksAt {
  const int32_t* __restrict__ table;
  Blocks bl;
  __device__ __forceinline__ int64_t operator()(const Volume&, int i, int j, int k) const {
    const int32_t slot = table[((int64_t)(k >> 3) * bl.by + (j >> 3)) * bl.bx + (i >> 3)];
    if (slot < 0 || slot >= bl.n_blocks) return -1;
    return (int64_t)slot * SB_VOX + ((k & 7) * SB + (j & 7)) * SB + (i & 7);
  }
};

// ACCUMULATE: workgroup (x, f) takes the pixels 256 x .. 256 x + 255 of frame f, one lane per pixel, and writes one row of sums.
template <class At>
__global__ void __launch_bounds__(TK_THREADS) track_accumulate_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, At at,
                                                                       Volume vol, float tau, const uint16_t* __restrict__ depth,
                                                                       const acez_tsdf_frame* __restrict__ frames, float depth_unit,
                                                                       float max_depth, float min_weight, const double* __restrict__ state,
                                                                       double* __restrict__ partials) {
  __shared__ double s_sum[TK_WAVES][TRACK_TERMS];
  const int f = blockIdx.y;
  const double* st = state + (int64_t)f * TRACK_STATE;          // uniform addresses: scalar loads
  if (st[acez::LOOP_STATUS] != acez::LOOP_RUNNING) return;      // this frame's loop has stopped (uniform over the workgroup)
  const acez_tsdf_frame& fr = frames[f];
  const int64_t n_pix = (int64_t)fr.h * fr.w;
  if ((int64_t)blockIdx.x * TK_THREADS >= n_pix) return;        // a tile past this frame's own count (uniform)
  const int t = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * TK_THREADS + t;
  double v[TRACK_TERMS];
#pragma unroll
  for (int i = 0; i < TRACK_TERMS; ++i) v[i] = 0.0;
  const uint16_t raw = p < n_pix ? depth[fr.offset + p] : (uint16_t)0;   // in [offset, offset + h * w): the host checked that range
  const float d32 = (float)raw * depth_unit;
  if (raw != 0 && !(d32 > max_depth)) {
    const int ix = (int)(p % fr.w), iy = (int)(p / fr.w);
    const double z = d32;
    const double x = (((double)ix - (double)fr.ppx) * z) / (double)fr.focal;
    const double y = (((double)iy - (double)fr.ppy) * z) / (double)fr.focal;
    const double tr[3] = {st[3], st[7], st[11]};
    double pw[3], g[3], fl[3];
    bool ok = true;
    const double o3[3] = {vol.ox, vol.oy, vol.oz};
    const int n3[3] = {vol.nx, vol.ny, vol.nz};
    const double vs = vol.v;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      pw[a] = ((st[4 * a] * x + st[4 * a + 1] * y) + st[4 * a + 2] * z) + tr[a];
      g[a] = (pw[a] - o3[a]) / vs;
      fl[a] = floor(g[a]);
      ok = ok && isfinite(g[a]) && fl[a] >= 0.0 && fl[a] <= (double)(n3[a] - 2);
    }
    if (ok) {
      const int i0 = (int)fl[0], j0 = (int)fl[1], k0 = (int)fl[2];    // 0 <= i0 <= nx - 2 (and alike): all eight corners are voxels
      double c[8];
      bool known = true, cut = false;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t el = at(vol, i0 + (e & 1), j0 + ((e >> 1) & 1), k0 + (e >> 2));
        const float w = el >= 0 ? weight[el] : 0.0f;
        const float tv = el >= 0 ? tsdf[el] : 1.0f;
        known = known && (w >= min_weight);
        cut = cut || !(tv >= 1.0f);
        c[e] = tv;
      }
      if (known && cut) {
        const double fx = g[0] - fl[0], fy = g[1] - fl[1], fz = g[2] - fl[2];
        // along x: the four edges (dy, dz) = (0,0), (1,0), (0,1), (1,1); their differences are the x-derivative's corners
        const double dx00 = c[1] - c[0], dx10 = c[3] - c[2], dx01 = c[5] - c[4], dx11 = c[7] - c[6];
        const double c00 = c[0] + fx * dx00, c10 = c[2] + fx * dx10, c01 = c[4] + fx * dx01, c11 = c[6] + fx * dx11;
        const double dy0 = c10 - c00, dy1 = c11 - c01;
        const double c0 = c00 + fy * dy0, c1 = c01 + fy * dy1;
        const double dz = c1 - c0;
        const double value = c0 + fz * dz;
        const double gx0 = dx00 + fy * (dx10 - dx00), gx1 = dx01 + fy * (dx11 - dx01);
        const double gx = gx0 + fz * (gx1 - gx0);
        const double gy = dy0 + fz * (dy1 - dy0);
        const double td = tau, scale = td / vs;
        const double r = td * value;
        const double n[3] = {scale * gx, scale * gy, scale * dz};
        const double a[3] = {pw[0] - tr[0], pw[1] - tr[1], pw[2] - tr[2]};
        const double J[6] = {n[0], n[1], n[2], a[1] * n[2] - a[2] * n[1], a[2] * n[0] - a[0] * n[2], a[0] * n[1] - a[1] * n[0]};
        v[0] = 1.0;
        int o = acez::TRACK_H;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = i; j < 6; ++j) v[o++] = J[i] * J[j];
#pragma unroll
        for (int i = 0; i < 6; ++i) v[acez::TRACK_B + i] = J[i] * r;
        v[acez::TRACK_R2] = r * r;
      }
    }
  }
  const double total = acez::block_sum_terms<TRACK_TERMS, TK_WAVES>(v, s_sum);
  if (t < TRACK_TERMS) partials[((int64_t)f * gridDim.x + blockIdx.x) * TRACK_TERMS + t] = total;
}

// UPDATE: one workgroup per frame sums the frame's partial rows (sum_rows of ordered_sum.h), thread 0 runs track_update (track_solve.h)
// on the totals.
__global__ void __launch_bounds__(TK_THREADS) track_update_kernel(const double* __restrict__ partials, int tiles,
                                                                   const acez_tsdf_frame* __restrict__ frames, double rel_rms, double damping,
                                                                   double min_count, int max_iterations, double* state, double* history) {
  __shared__ double s_sum[TK_WAVES][TRACK_TERMS];
  __shared__ double s_total[TRACK_TERMS];
  const int f = blockIdx.x;
  double* st = state + (int64_t)f * TRACK_STATE;
  if (!acez::loop_live(st, max_iterations)) return;                        // uniform
  const acez_tsdf_frame& fr = frames[f];
  int64_t rows = ((int64_t)fr.h * fr.w + TK_THREADS - 1) / TK_THREADS;     // the table is device data: bound what is formed from it
  rows = rows < 0 ? 0 : (rows > tiles ? tiles : rows);
  acez::sum_rows<TRACK_TERMS, TK_THREADS>(partials + (int64_t)f * tiles * TRACK_TERMS, rows, s_sum, s_total);
  if (threadIdx.x == 0) acez::track_update(st, s_total, rel_rms, damping, min_count, history + (int64_t)f * max_iterations * acez::TRACK_RECORD);
}

}  // namespace

#define FU_REQUIRE_DIMS(limit)                                                                                        \
  ACEZ_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "volume dimensions must be at least 1");                                \
  ACEZ_REQUIRE((int64_t)nx * ny <= (limit) && (int64_t)nx * ny * nz <= (limit), "volume too large for 32-bit voxel indices")

// what the three frame-taking entry points share: the fusion scalars (max_weight: null where the entry point has no weight cap), the
// frame count and the table's rows, which bound every index a kernel forms from them
static int check_frame_call(float truncation, float depth_unit, float max_depth, const float* max_weight, int64_t n_pixels,
                            const acez_tsdf_frame* h_frames, int n_frames) {
  const float scal[3] = {truncation, depth_unit, max_depth};
  ACEZ_REQUIRE(acez::finite_all(scal, 3), "non-finite truncation, depth unit or depth limit");
  ACEZ_REQUIRE(truncation > 0.0f, "truncation must be positive");
  ACEZ_REQUIRE(depth_unit > 0.0f && max_depth > 0.0f, "depth unit and depth limit must be positive");
  ACEZ_REQUIRE(!max_weight || (isfinite(*max_weight) && *max_weight > 0.0f), "weight cap must be positive and finite");
  ACEZ_REQUIRE(n_frames >= 0 && n_frames <= ACEZ_TSDF_MAX_FRAMES, "frame count out of range (0 .. 256 per call)");
  ACEZ_REQUIRE(n_pixels >= 0, "negative depth buffer length");
  for (int f = 0; f < n_frames; ++f)
    if (int rc = acez::check_frame(h_frames[f], n_pixels)) return rc;
  return ACEZ_OK;
}

extern "C" int acez_tsdf_integrate(float* d_tsdf, float* d_weight, float* d_colour, int nx, int ny, int nz, float ox, float oy, float oz,
                                   float voxel_size, float truncation, const uint16_t* d_depth, const uint8_t* d_rgb, int64_t n_pixels,
                                   const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames, float depth_unit,
                                   float max_depth, float max_weight, int frustum_skip, void* stream) {
  ACEZ_REQUIRE(d_tsdf && d_weight && d_depth && h_frames && d_frames, "null pointer");
  ACEZ_REQUIRE(!d_rgb || d_colour, "colour images without a colour volume");
  FU_REQUIRE_DIMS(((int64_t)1 << 31) - 1);
  ACEZ_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(voxel_size) && voxel_size > 0.0f, "voxel size must be positive, the origin finite");
  if (int rc = check_frame_call(truncation, depth_unit, max_depth, &max_weight, n_pixels, h_frames, n_frames)) return rc;
  ACEZ_REQUIRE((ny + FU_BY - 1) / FU_BY <= 65535 && (nz + FU_BZ - 1) / FU_BZ <= 65535, "volume too large (more than 65535 bricks along y or z)");
  if (int rc = acez::require_device("TSDF integration runs on a gfx950 GPU")) return rc;
  if (n_frames == 0) return ACEZ_OK;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = acez::upload_frames(d_frames, h_frames, n_frames, s)) return rc;
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

// ---------------------------------------------------------------------------------------------- section K2: the block-sparse volume
// the virtual grid and its block grid; fills `bl`
static int check_block_grid(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, int n_blocks, Blocks* bl) {
  ACEZ_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, "volume dimensions must be at least 1");
  ACEZ_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(voxel_size) && voxel_size > 0.0f, "voxel size must be positive, the origin finite");
  const int64_t bx = ((int64_t)nx + SB - 1) / SB, by = ((int64_t)ny + SB - 1) / SB, bz = ((int64_t)nz + SB - 1) / SB;
  ACEZ_REQUIRE(bx * by < ((int64_t)1 << 31) && bx * by * bz < ((int64_t)1 << 31), "block grid too large (2^31 blocks or more)");
  ACEZ_REQUIRE(n_blocks >= 0, "negative block count");
  ACEZ_REQUIRE(n_blocks <= bx * by * bz, "more blocks than the block grid has");
  *bl = Blocks{(int)bx, (int)by, (int)bz, n_blocks};
  return ACEZ_OK;
}

extern "C" int acez_tsdf_mark(uint8_t* d_block_flags, int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, float truncation,
                              const uint16_t* d_depth, int64_t n_pixels, const acez_tsdf_frame* h_frames, int n_frames,
                              acez_tsdf_frame* d_frames, float depth_unit, float max_depth, void* stream) {
  ACEZ_REQUIRE(d_block_flags && d_depth && h_frames && d_frames, "null pointer");
  Blocks bl;
  if (int rc = check_block_grid(nx, ny, nz, ox, oy, oz, voxel_size, 0, &bl)) return rc;
  if (int rc = check_frame_call(truncation, depth_unit, max_depth, nullptr, n_pixels, h_frames, n_frames)) return rc;
  int64_t most = 0;
  for (int f = 0; f < n_frames; ++f) {
    const float* m = h_frames[f].m;
    const double det = ((double)m[0] * ((double)m[5] * m[10] - (double)m[6] * m[9]) + (double)m[1] * ((double)m[6] * m[8] - (double)m[4] * m[10])) +
                       (double)m[2] * ((double)m[4] * m[9] - (double)m[5] * m[8]);
    ACEZ_REQUIRE(isfinite(det) && fabs(det) >= 1e-6, "singular pose in the frame table");
    most = most > (int64_t)h_frames[f].h * h_frames[f].w ? most : (int64_t)h_frames[f].h * h_frames[f].w;
  }
  if (int rc = acez::require_device("marking TSDF blocks runs on a gfx950 GPU")) return rc;
  if (n_frames == 0) return ACEZ_OK;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = acez::upload_frames(d_frames, h_frames, n_frames, s)) return rc;
  const Volume vol{nx, ny, nz, ox, oy, oz, voxel_size};
  hipLaunchKernelGGL(mark_kernel, dim3((unsigned)((most + MK_THREADS - 1) / MK_THREADS), (unsigned)n_frames), dim3(MK_THREADS), 0, s, d_block_flags,
                     vol, bl, truncation, d_depth, (const acez_tsdf_frame*)d_frames, depth_unit, max_depth);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_tsdf_integrate_blocks(float* d_tsdf, float* d_weight, float* d_colour, const int32_t* d_slot_blocks, int n_blocks, int nx,
                                          int ny, int nz, float ox, float oy, float oz, float voxel_size, float truncation,
                                          const uint16_t* d_depth, const uint8_t* d_rgb, int64_t n_pixels, const acez_tsdf_frame* h_frames,
                                          int n_frames, acez_tsdf_frame* d_frames, float depth_unit, float max_depth, float max_weight,
                                          int frustum_skip, void* stream) {
  ACEZ_REQUIRE(d_tsdf && d_weight && d_slot_blocks && d_depth && h_frames && d_frames, "null pointer");
  ACEZ_REQUIRE(!d_rgb || d_colour, "colour images without a colour volume");
  Blocks bl;
  if (int rc = check_block_grid(nx, ny, nz, ox, oy, oz, voxel_size, n_blocks, &bl)) return rc;
  if (int rc = check_frame_call(truncation, depth_unit, max_depth, &max_weight, n_pixels, h_frames, n_frames)) return rc;
  if (int rc = acez::require_device("TSDF integration runs on a gfx950 GPU")) return rc;
  if (n_frames == 0 || n_blocks == 0) return ACEZ_OK;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = acez::upload_frames(d_frames, h_frames, n_frames, s)) return rc;
  const Volume vol{nx, ny, nz, ox, oy, oz, voxel_size};
  hipLaunchKernelGGL(integrate_blocks_kernel, dim3((unsigned)n_blocks), dim3(SB_VOX), 0, s, d_tsdf, d_weight, d_colour, d_slot_blocks, vol, bl,
                     truncation, d_depth, d_rgb, (const acez_tsdf_frame*)d_frames, n_frames, depth_unit, max_depth, max_weight, frustum_skip);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

// the extraction's outputs are indexed in 32 bits: [3][n_blocks][512] edge flags and their int32 prefix sum
#define FU_REQUIRE_BLOCK_COUNT() \
  ACEZ_REQUIRE((int64_t)n_blocks * SB_VOX <= (((int64_t)1 << 31) - 1) / 3, "too many blocks for 32-bit voxel indices")

extern "C" int acez_tsdf_cells_blocks(const float* d_tsdf, const float* d_weight, const float* d_colour, const int32_t* d_block_table,
                                      const int32_t* d_slot_blocks, int n_blocks, int nx, int ny, int nz, float ox, float oy, float oz,
                                      float voxel_size, float min_weight, uint8_t* d_active, const int32_t* d_vertex_rank,
                                      float* d_out_vertices, uint8_t* d_out_colours, int64_t n_vertices, void* stream) {
  ACEZ_REQUIRE(d_tsdf && d_weight && d_block_table && d_slot_blocks && d_active, "null pointer");
  Blocks bl;
  if (int rc = check_block_grid(nx, ny, nz, ox, oy, oz, voxel_size, n_blocks, &bl)) return rc;
  FU_REQUIRE_BLOCK_COUNT();
  ACEZ_REQUIRE(min_weight > 0.0f, "min_weight must be positive (a voxel without a block has weight 0)");
  ACEZ_REQUIRE(n_vertices >= 0, "negative vertex count");
  ACEZ_REQUIRE(!d_vertex_rank || n_vertices == 0 || d_out_vertices, "vertex ranks without a vertex buffer");
  if (int rc = acez::require_device("mesh extraction runs on a gfx950 GPU")) return rc;
  if (n_blocks == 0 || (d_vertex_rank && n_vertices == 0)) return ACEZ_OK;
  const Volume vol{nx, ny, nz, ox, oy, oz, voxel_size};
  hipLaunchKernelGGL(cells_blocks_kernel, dim3((unsigned)n_blocks), dim3(SB_VOX), 0, (hipStream_t)stream, d_tsdf, d_weight, d_colour,
                     d_block_table, d_slot_blocks, vol, bl, min_weight, d_active, d_vertex_rank, d_out_vertices, d_out_colours, n_vertices);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_tsdf_faces_blocks(const float* d_tsdf, const float* d_weight, const int32_t* d_block_table, const int32_t* d_slot_blocks,
                                      int n_blocks, int nx, int ny, int nz, float min_weight, const uint8_t* d_active, uint8_t* d_edge_flags,
                                      const int32_t* d_vertex_rank, const int32_t* d_edge_rank, int32_t* d_out_faces, int64_t n_faces,
                                      void* stream) {
  ACEZ_REQUIRE(d_tsdf && d_weight && d_block_table && d_slot_blocks && d_active && d_edge_flags, "null pointer");
  Blocks bl;
  if (int rc = check_block_grid(nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f, n_blocks, &bl)) return rc;
  FU_REQUIRE_BLOCK_COUNT();
  ACEZ_REQUIRE(min_weight > 0.0f, "min_weight must be positive (a voxel without a block has weight 0)");
  ACEZ_REQUIRE(n_faces >= 0, "negative face count");
  ACEZ_REQUIRE(!d_edge_rank || n_faces == 0 || (d_vertex_rank && d_out_faces), "edge ranks without vertex ranks or a face buffer");
  if (int rc = acez::require_device("mesh extraction runs on a gfx950 GPU")) return rc;
  if (n_blocks == 0 || (d_edge_rank && n_faces == 0)) return ACEZ_OK;
  const Volume vol{nx, ny, nz, 0.0f, 0.0f, 0.0f, 1.0f};
  hipLaunchKernelGGL(faces_blocks_kernel, dim3((unsigned)n_blocks), dim3(SB_VOX), 0, (hipStream_t)stream, d_tsdf, d_weight, d_block_table,
                     d_slot_blocks, vol, bl, min_weight, d_active, d_edge_flags, d_vertex_rank, d_edge_rank, d_out_faces, n_faces);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

// ---------------------------------------------------------------------------------------------- section K3: tracking frames against the volume
// what the two ACCUMULATE entry points share; fills `tiles`, the rows per frame of d_partials = the grid's x extent
static int check_track_call(const uint16_t* d_depth, const acez_tsdf_frame* h_frames, acez_tsdf_frame* d_frames, const double* d_state,
                            const double* d_partials, float ox, float oy, float oz, float voxel_size, float truncation, float depth_unit,
                            float max_depth, float min_weight, int64_t n_pixels, int n_frames, int* tiles) {
  ACEZ_REQUIRE(d_depth && h_frames && d_frames && d_state && d_partials, "null pointer");
  ACEZ_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(voxel_size) && voxel_size > 0.0f, "voxel size must be positive, the origin finite");
  if (int rc = check_frame_call(truncation, depth_unit, max_depth, nullptr, n_pixels, h_frames, n_frames)) return rc;
  ACEZ_REQUIRE(isfinite(min_weight), "min_weight must be finite");
  int64_t most = 0;
  for (int f = 0; f < n_frames; ++f) most = most > (int64_t)h_frames[f].h * h_frames[f].w ? most : (int64_t)h_frames[f].h * h_frames[f].w;
  *tiles = (int)((most + TK_THREADS - 1) / TK_THREADS);       // <= 2^30 / 256
  return ACEZ_OK;
}

template <class At>
static int launch_track_accumulate(const float* d_tsdf, const float* d_weight, At at, const Volume& vol, float truncation,
                                   const uint16_t* d_depth, const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames,
                                   int upload, float depth_unit, float max_depth, float min_weight, const double* d_state,
                                   double* d_partials, int tiles, hipStream_t s) {
  if (n_frames == 0) return ACEZ_OK;
  if (upload)
    if (int rc = acez::upload_frames(d_frames, h_frames, n_frames, s)) return rc;
  hipLaunchKernelGGL(track_accumulate_kernel<At>, dim3((unsigned)tiles, (unsigned)n_frames), dim3(TK_THREADS), 0, s, d_tsdf, d_weight, at, vol,
                     truncation, d_depth, (const acez_tsdf_frame*)d_frames, depth_unit, max_depth, min_weight, d_state, d_partials);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_tsdf_track_accumulate(const float* d_tsdf, const float* d_weight, int nx, int ny, int nz, float ox, float oy, float oz,
                                          float voxel_size, float truncation, const uint16_t* d_depth, int64_t n_pixels,
                                          const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames, int upload,
                                          float depth_unit, float max_depth, float min_weight, const double* d_state, double* d_partials,
                                          void* stream) {
  ACEZ_REQUIRE(d_tsdf && d_weight, "null pointer");
  FU_REQUIRE_DIMS(((int64_t)1 << 31) - 1);
  int tiles = 0;
  if (int rc = check_track_call(d_depth, h_frames, d_frames, d_state, d_partials, ox, oy, oz, voxel_size, truncation, depth_unit, max_depth,
                                min_weight, n_pixels, n_frames, &tiles))
    return rc;
  if (int rc = acez::require_device("tracking against the TSDF volume runs on a gfx950 GPU")) return rc;
  const Volume vol{nx, ny, nz, ox, oy, oz, voxel_size};
  return launch_track_accumulate(d_tsdf, d_weight, DenseAt{}, vol, truncation, d_depth, h_frames, n_frames, d_frames, upload, depth_unit,
                                 max_depth, min_weight, d_state, d_partials, tiles, (hipStream_t)stream);
}

extern "C" int acez_tsdf_track_accumulate_blocks(const float* d_tsdf, const float* d_weight, const int32_t* d_block_table,
                                                 const int32_t* d_slot_blocks, int n_blocks, int nx, int ny, int nz, float ox, float oy,
                                                 float oz, float voxel_size, float truncation, const uint16_t* d_depth, int64_t n_pixels,
                                                 const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames, int upload,
                                                 float depth_unit, float max_depth, float min_weight, const double* d_state,
                                                 double* d_partials, void* stream) {
  ACEZ_REQUIRE(d_block_table && (n_blocks <= 0 || (d_tsdf && d_weight && d_slot_blocks)), "null pointer");
  Blocks bl;
  if (int rc = check_block_grid(nx, ny, nz, ox, oy, oz, voxel_size, n_blocks, &bl)) return rc;
  int tiles = 0;
  if (int rc = check_track_call(d_depth, h_frames, d_frames, d_state, d_partials, ox, oy, oz, voxel_size, truncation, depth_unit, max_depth,
                                min_weight, n_pixels, n_frames, &tiles))
    return rc;
  ACEZ_REQUIRE(min_weight > 0.0f, "min_weight must be positive (a voxel without a block has weight 0)");
  if (int rc = acez::require_device("tracking against the TSDF volume runs on a gfx950 GPU")) return rc;
  const Volume vol{nx, ny, nz, ox, oy, oz, voxel_size};
  return launch_track_accumulate(d_tsdf, d_weight, BlocksAt{d_block_table, bl}, vol, truncation, d_depth, h_frames, n_frames, d_frames, upload,
                                 depth_unit, max_depth, min_weight, d_state, d_partials, tiles, (hipStream_t)stream);
}

extern "C" int acez_tsdf_track_update(const double* d_partials, int tiles, const acez_tsdf_frame* d_frames, int n_frames, double rel_rms,
                                      double damping, int min_count, int max_iterations, double* d_state, double* d_history, void* stream) {
  ACEZ_REQUIRE(d_partials && d_frames && d_state && d_history, "null pointer");
  ACEZ_REQUIRE(n_frames >= 0 && n_frames <= ACEZ_TSDF_MAX_FRAMES, "frame count out of range (0 .. 256 per call)");
  ACEZ_REQUIRE(tiles >= 0, "negative tile count");
  ACEZ_REQUIRE(max_iterations >= 1, "max_iterations must be at least 1");
  ACEZ_REQUIRE(isfinite(rel_rms) && rel_rms >= 0.0 && isfinite(damping) && damping >= 0.0, "the tolerance and the damping must be finite and not negative");
  ACEZ_REQUIRE(min_count >= 6, "min_count must be at least 6 (the unknowns of a pose)");
  if (int rc = acez::require_device("the tracking update runs on a gfx950 GPU")) return rc;
  if (n_frames == 0) return ACEZ_OK;
  hipLaunchKernelGGL(track_update_kernel, dim3((unsigned)n_frames), dim3(TK_THREADS), 0, (hipStream_t)stream, d_partials, tiles, d_frames, rel_rms,
                     damping, (double)min_count, max_iterations, d_state, d_history);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
