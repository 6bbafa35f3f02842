// reproject_api.hip -- reprojection score of held-out views (include/acez.h section J: acez_reproject_score,
// acez_reproject_scratch_size, acez_reproject_cell_means). benchmark_poses.py --method reproject.
//
// M coloured points are seen from T views on a grid of oh x ow cells (one cell = one 8 x 8 px block of the network's input frame,
// the resolution of the scene-coordinate map). One call is four passes on the caller's stream:
//   1. clear       every view's key plane to ~0, its sums and the per-view outputs to 0;
//   2. nearest     grid (point chunk, view): project in fp32, drop z < 0.1 and cells outside the grid, 64-bit atomicMin of
//                  (depth bits << 32 | point index) on the view's cell -- render_api.hip's key: positive floats order like their bit
//                  patterns, equal depths go to the lower index;
//   3. accumulate  same grid, same projection: a point with z <= zmin * (1 + band) of its cell adds R, G, B and 1 to the cell's four
//                  32-bit sums (integer atomicAdd);
//   4. score       per cell with count > 0: colour = (sum + count / 2) / count, squared integer differences to the target over the
//                  three channels into the view's 64-bit sum, the cell into the view's covered count (one atomic of each per block).
// Minima and integer sums do not depend on the order in which the atomics land: a call's outputs are a function of its inputs.
// Every float operation is written out in the order tests/reproject_restated.py restates it in numpy float32; the unit is built with
// -ffp-contract=off and uses only * + comparisons, floor and ONE division per projection (the reciprocal of the depth).
#include <math.h>
#include <stdint.h>
#include "acez_common.h"

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_VIEW_FLOATS = 15;              // 12 world -> camera (3 x 4 rows), focal, cx, cy (cell units)
constexpr float RP_ZMIN = 0.1f;
constexpr int64_t RP_MAX_POINTS = (int64_t)1 << 24;   // 255 * 2^24 < 2^32: a cell's 32-bit colour sums hold every point of the call
constexpr int RP_MAX_SIDE = 4096;
constexpr int RP_POINT_BLOCKS = 4096;           // blocks of a point pass over all views: a few per CU slot, the rest is a grid stride

struct View {
  float m[12];
  float f, cx, cy;
};

__device__ __forceinline__ View load_view(const float* __restrict__ views, int v) {
  View c;
  const float* p = views + (int64_t)v * RP_VIEW_FLOATS;     // uniform per block: scalar loads
  for (int k = 0; k < 12; ++k) c.m[k] = p[k];
  c.f = p[12];
  c.cx = p[13];
  c.cy = p[14];
  return c;
}

// the cell of world point (x, y, z) in view c and its depth; false: behind the 0.1 plane, outside the grid, or not a number
__device__ __forceinline__ bool project(const View& c, float x, float y, float z, int oh, int ow, int& cell, float& depth) {
  const float xc = c.m[0] * x + c.m[1] * y + c.m[2] * z + c.m[3];
  const float yc = c.m[4] * x + c.m[5] * y + c.m[6] * z + c.m[7];
  const float zc = c.m[8] * x + c.m[9] * y + c.m[10] * z + c.m[11];
  if (!(zc >= RP_ZMIN)) return false;
  const float iz = 1.0f / zc;
  const float u = c.cx + (c.f * xc) * iz;
  const float v = c.cy + (c.f * yc) * iz;
  if (!(u >= 0.0f && u < (float)ow && v >= 0.0f && v < (float)oh)) return false;   // (-0.0 is inside: it is cell 0)
  cell = (int)floorf(v) * ow + (int)floorf(u);
  depth = zc;
  return true;
}

__global__ void __launch_bounds__(RP_THREADS) clear_kernel(unsigned long long* __restrict__ keys, uint32_t* __restrict__ sums, int64_t cells,
                                                           long long* __restrict__ sse, int32_t* __restrict__ covered, int n_views) {
  const int64_t stride = (int64_t)gridDim.x * RP_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x; i < cells; i += stride) {
    keys[i] = ~0ull;
    sums[4 * i] = 0u; sums[4 * i + 1] = 0u; sums[4 * i + 2] = 0u; sums[4 * i + 3] = 0u;
    if (i < n_views) {
      sse[i] = 0;
      covered[i] = 0;
    }
  }
  // (n_views <= cells always: every view has at least one cell)
}

__global__ void __launch_bounds__(RP_THREADS) nearest_kernel(const float* __restrict__ xyz, int64_t n, const float* __restrict__ views,
                                                             int oh, int ow, unsigned long long* __restrict__ keys) {
  const int v = blockIdx.y;
  const View c = load_view(views, v);
  unsigned long long* plane = keys + (int64_t)v * oh * ow;
  for (int64_t i = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RP_THREADS) {
    int cell;
    float d;
    if (!project(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], oh, ow, cell, d)) continue;
    atomicMin(plane + cell, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(uint32_t)i);
  }
}

__global__ void __launch_bounds__(RP_THREADS) accumulate_kernel(const float* __restrict__ xyz, const uint8_t* __restrict__ rgb, int64_t n,
                                                                const float* __restrict__ views, int oh, int ow, float one_plus_band,
                                                                const unsigned long long* __restrict__ keys, uint32_t* __restrict__ sums) {
  const int v = blockIdx.y;
  const View c = load_view(views, v);
  const int64_t base = (int64_t)v * oh * ow;
  for (int64_t i = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RP_THREADS) {
    int cell;
    float d;
    if (!project(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], oh, ow, cell, d)) continue;
    const float zmin = __uint_as_float((uint32_t)(keys[base + cell] >> 32));   // (the nearest pass has written this cell: d itself at the least)
    if (!(d <= zmin * one_plus_band)) continue;
    uint32_t* s = sums + 4 * (base + cell);
    atomicAdd(s, (uint32_t)rgb[3 * i]);
    atomicAdd(s + 1, (uint32_t)rgb[3 * i + 1]);
    atomicAdd(s + 2, (uint32_t)rgb[3 * i + 2]);
    atomicAdd(s + 3, 1u);
  }
}

__global__ void __launch_bounds__(RP_THREADS) score_kernel(const uint32_t* __restrict__ sums, const uint8_t* __restrict__ targets, int hw,
                                                           long long* __restrict__ sse, int32_t* __restrict__ covered,
                                                           uint8_t* __restrict__ image, uint8_t* __restrict__ mask) {
  __shared__ unsigned long long s_sse[RP_THREADS];
  __shared__ int s_cov[RP_THREADS];
  const int v = blockIdx.y;
  const int64_t base = (int64_t)v * hw;
  unsigned long long acc = 0;
  int cov = 0;
  for (int p = blockIdx.x * RP_THREADS + threadIdx.x; p < hw; p += gridDim.x * RP_THREADS) {
    const uint32_t* s = sums + 4 * (base + p);
    const uint32_t cnt = s[3];
    uint32_t col[3] = {0u, 0u, 0u};
    if (cnt > 0u) {
      const uint8_t* t = targets + 3 * (base + p);
      for (int k = 0; k < 3; ++k) {
        col[k] = (s[k] + cnt / 2u) / cnt;         // half up; (255 * cnt + cnt / 2 < 2^32 for cnt <= 2^24)
        const int diff = (int)col[k] - (int)t[k];
        acc += (unsigned long long)(diff * diff);
      }
      ++cov;
    }
    if (image) {
      image[3 * (base + p)] = (uint8_t)col[0];
      image[3 * (base + p) + 1] = (uint8_t)col[1];
      image[3 * (base + p) + 2] = (uint8_t)col[2];
    }
    if (mask) mask[base + p] = cnt > 0u ? 1 : 0;
  }
  s_sse[threadIdx.x] = acc;
  s_cov[threadIdx.x] = cov;
  __syncthreads();
  for (int w = RP_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s_sse[threadIdx.x] += s_sse[threadIdx.x + w];
      s_cov[threadIdx.x] += s_cov[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && s_cov[0] > 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(sse + v), s_sse[0]);
    atomicAdd(covered + v, s_cov[0]);
  }
}

// uint8 RGB mean of every 8 x 8 px cell (a cell cut by the frame's edge: of the pixels it has), half up
__global__ void __launch_bounds__(RP_THREADS) cell_means_kernel(const uint8_t* __restrict__ frames, int64_t total, int H, int W, int oh, int ow,
                                                                uint8_t* __restrict__ out) {
  for (int64_t o = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x; o < total; o += (int64_t)gridDim.x * RP_THREADS) {
    const int cx = (int)(o % ow), cy = (int)((o / ow) % oh);
    const int64_t f = o / ((int64_t)oh * ow);
    const int x0 = cx * 8, x1 = min(x0 + 8, W), y0 = cy * 8, y1 = min(y0 + 8, H);
    const uint8_t* img = frames + f * (int64_t)H * W * 3;
    uint32_t s[3] = {0u, 0u, 0u};
    for (int y = y0; y < y1; ++y) {
      const uint8_t* row = img + ((int64_t)y * W + x0) * 3;
      for (int x = 0; x < x1 - x0; ++x) {
        s[0] += row[3 * x];
        s[1] += row[3 * x + 1];
        s[2] += row[3 * x + 2];
      }
    }
    const uint32_t cnt = (uint32_t)((x1 - x0) * (y1 - y0));
    for (int k = 0; k < 3; ++k) out[3 * o + k] = (uint8_t)((s[k] + cnt / 2u) / cnt);
  }
}

int blocks_for(int64_t items, int64_t cap) {
  const int64_t b = (items + RP_THREADS - 1) / RP_THREADS;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

extern "C" int acez_reproject_scratch_size(int n_views, int oh, int ow, int64_t* out_bytes) {
  ACEZ_REQUIRE(out_bytes, "null pointer");
  ACEZ_REQUIRE(n_views >= 1 && n_views <= 65535, "view count out of range (1 .. 65535)");
  ACEZ_REQUIRE(oh >= 1 && ow >= 1 && oh <= RP_MAX_SIDE && ow <= RP_MAX_SIDE, "grid size out of range (1 .. 4096 cells per side)");
  *out_bytes = (int64_t)n_views * oh * ow * (int64_t)(sizeof(unsigned long long) + 4 * sizeof(uint32_t));
  return ACEZ_OK;
}

extern "C" int acez_reproject_score(const float* d_xyz, const uint8_t* d_rgb, int64_t n_points, const float* d_views, int n_views, int oh,
                                    int ow, const uint8_t* d_targets, float depth_band, void* d_scratch, int64_t scratch_bytes,
                                    int64_t* d_out_sse, int32_t* d_out_covered, uint8_t* d_out_image, uint8_t* d_out_mask, void* stream) {
  ACEZ_REQUIRE(d_views && d_targets && d_scratch && d_out_sse && d_out_covered, "null pointer");
  ACEZ_REQUIRE(n_points >= 0 && n_points <= RP_MAX_POINTS, "point count out of range (0 .. 2^24)");
  ACEZ_REQUIRE(n_points == 0 || (d_xyz && d_rgb), "points without coordinates or colours");
  ACEZ_REQUIRE(depth_band >= 0.0f && depth_band <= 1.0f, "depth band out of range (0 .. 1)");
  int64_t need = 0;
  if (int rc = acez_reproject_scratch_size(n_views, oh, ow, &need)) return rc;
  ACEZ_REQUIRE(scratch_bytes >= need, "scratch too small (see acez_reproject_scratch_size)");
  ACEZ_REQUIRE(((uintptr_t)d_scratch & 7) == 0, "scratch must be 8-byte aligned");
  if (int rc = acez::require_device("the reprojection score runs on a gfx950 GPU")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int hw = oh * ow;
  const int64_t cells = (int64_t)n_views * hw;
  unsigned long long* keys = (unsigned long long*)d_scratch;
  uint32_t* sums = (uint32_t*)(keys + cells);
  const float one_plus_band = (float)(1.0 + (double)depth_band);        // rounded once; the kernel's product once more
  hipLaunchKernelGGL(clear_kernel, dim3(blocks_for(cells, 2048)), dim3(RP_THREADS), 0, s, keys, sums, cells, (long long*)d_out_sse,
                     d_out_covered, n_views);
  ACEZ_HIP_CHECK(hipGetLastError());
  if (n_points > 0) {
    const int per_view = RP_POINT_BLOCKS / n_views;
    const dim3 grid(blocks_for(n_points, per_view < 1 ? 1 : per_view), n_views);
    hipLaunchKernelGGL(nearest_kernel, grid, dim3(RP_THREADS), 0, s, d_xyz, n_points, d_views, oh, ow, keys);
    ACEZ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(accumulate_kernel, grid, dim3(RP_THREADS), 0, s, d_xyz, d_rgb, n_points, d_views, oh, ow, one_plus_band,
                       (const unsigned long long*)keys, sums);
    ACEZ_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(score_kernel, dim3(blocks_for(hw, 64), n_views), dim3(RP_THREADS), 0, s, (const uint32_t*)sums, d_targets, hw,
                     (long long*)d_out_sse, d_out_covered, d_out_image, d_out_mask);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_reproject_cell_means(const uint8_t* d_frames, int n_frames, int H, int W, uint8_t* d_out, void* stream) {
  ACEZ_REQUIRE(d_frames && d_out, "null pointer");
  ACEZ_REQUIRE(n_frames >= 1 && n_frames <= 65535, "frame count out of range (1 .. 65535)");
  ACEZ_REQUIRE(H >= 1 && W >= 1 && H <= 8 * RP_MAX_SIDE && W <= 8 * RP_MAX_SIDE, "frame size out of range (1 .. 32768 px per side)");
  if (int rc = acez::require_device("the cell means run on a gfx950 GPU")) return rc;
  const int oh = (H + 7) / 8, ow = (W + 7) / 8;
  const int64_t total = (int64_t)n_frames * oh * ow;
  hipLaunchKernelGGL(cell_means_kernel, dim3(blocks_for(total, 65536)), dim3(RP_THREADS), 0, (hipStream_t)stream, d_frames, total, H, W, oh,
                     ow, d_out);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
