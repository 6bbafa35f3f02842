// mvs_api.hip -- plane-sweep multi-view stereo: dense depth per frame of an RGB reconstruction (include/acez.h section L:
// acez_mvs_prefilter, acez_mvs_relative, acez_mvs_sweep, acez_mvs_check). estimate_depth.py.
//
// The header's section L is the definition: every float operation below is written in its order, the unit is built with
// -ffp-contract=off, and tests/mvs_restated.py restates it in numpy float32 and integers for the bit-for-bit comparison.
//
// prefilter  one thread per pixel, blockIdx.y = the frame (its row is read through scalar loads); integers only.
// sweep      one 256-thread workgroup per 16 x 16 reference pixels. A thread owns up to three pixels of the (16 + 2w)^2 halo tile
//            (their g_r and rays stay in registers over the planes) and, per plane and source, writes their raw costs to LDS; after
//            one barrier every thread sums its own window from LDS. Two LDS tiles alternate, so a step needs one barrier. The
//            relative poses and intrinsics are launch arguments. Eight views of 20 scalars do not fit the scalar register file
//            (unrolled over the slots the kernel spilled 166 of them to vector lanes), so thread 0 copies them once, from constant
//            offsets, into LDS, and a step reads its view from there at one address per wave. A_s is an ascending list of eight
//            registers that every source is inserted into. No cost volume exists in memory, and there is no scratch.
// check      one thread per reference pixel; the sources unrolled over the 8 slots, read at constant offsets (scalar registers).
// The three above: no atomics, no communication between workgroups, plain loads and stores.
//
// Section M (semi-global aggregation of the plane costs: acez_mvs_volume, acez_mvs_aggregate, acez_mvs_select):
// volume     the sweep kernel's second instantiation (template parameter VOLUME): the same plane loop, but C(p, k) and V(p, k) go to
//            memory per plane (uint16, V in bit 15, [y][x][k]) instead of into the best-four registers.
// aggregate  one wavefront walks one scanline of one direction; a 256-thread workgroup holds four of them, the grid all scanlines of
//            all directions of the call. Lane l holds the planes l, l + 64, ...: L_r(q, .) stays in registers from step to step, the
//            k - 1 / k + 1 neighbours come from one wave rotate each (DPP; lane 0 / 63 take the neighbouring register's rotated
//            value), min_j L_r(q, j) from a DPP reduction inside each row of 16 lanes and four lane reads. A step reads the
//            pixel's D costs as one contiguous run, requested AG_AHEAD steps before it is needed, and adds L_r into S with 32-bit
//            integer atomics that return nothing: the directions run side by side, and integer addition makes the sum
//            independent of their order. No LDS.
// select     16 lanes per pixel: a first pass over the D values finds the first minimum (the key X * 1024 + k), a second C2.
#include <math.h>
#include <stdint.h>

#include "acez_common.h"
#include "frame_table.h"

namespace {

constexpr int MV_THREADS = 256;
constexpr int MV_TILE = 16;
constexpr int MV_MAX_RADIUS = 4;
constexpr int MV_MAX_HALO = (MV_TILE + 2 * MV_MAX_RADIUS) * (MV_TILE + 2 * MV_MAX_RADIUS);   // 576
constexpr int MV_PER_THREAD = (MV_MAX_HALO + MV_THREADS - 1) / MV_THREADS;                    // 3
constexpr int MV_IN_VIEW = 0x8000;      // bit 15 of an LDS entry; the raw cost (<= 255) is below it
constexpr int MV_NO_COST = 1 << 28;     // an unused source slot: above any A_s (<= 81 * 255)

struct View {        // a source as the kernels see it: the relative pose reference -> source and the source's own row
  float m[12];
  float focal, ppx, ppy;
  int h, w;
  int64_t offset;
};

struct SweepArgs {
  View src[ACEZ_MVS_MAX_SOURCES];
  float focal, ppx, ppy;   // the reference
  int h, w;
  int64_t offset;
  float inv_far, step;
  int planes, radius, truncation, keep, uniqueness, n_sources;
};

struct CheckArgs {
  View src[ACEZ_MVS_MAX_SOURCES];
  float focal, ppx, ppy;
  int h, w;
  int64_t offset;
  float tolerance, depth_unit;
  int need, n_sources;
};

__global__ void __launch_bounds__(MV_THREADS) prefilter_kernel(const uint8_t* __restrict__ grey, uint8_t* __restrict__ out,
                                                               const acez_mvs_frame* __restrict__ frames) {
  const acez_mvs_frame& fr = frames[blockIdx.y];            // uniform address: scalar loads
  const int h = fr.h, w = fr.w;
  const int i = blockIdx.x * MV_THREADS + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  const int x0 = max(x - 4, 0), x1 = min(x + 4, w - 1), y0 = max(y - 4, 0), y1 = min(y + 4, h - 1);
  const uint8_t* img = grey + fr.offset;                     // [offset, offset + h * w): the host checked that range
  int sum = 0;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) sum += img[yy * w + xx];
  const int n = (x1 - x0 + 1) * (y1 - y0 + 1);
  const int m = (sum + n / 2) / n;
  out[fr.offset + i] = (uint8_t)min(max((int)img[i] - m + 128, 0), 255);
}

// steps 2-4 of the header's raw cost: the point (X, Y, Z) of the reference camera in source v. false: not in front of it.
__device__ __forceinline__ bool project(const View& v, float X, float Y, float Z, float& u, float& w_, float& zc) {
  const float xc = ((v.m[0] * X + v.m[1] * Y) + v.m[2] * Z) + v.m[3];
  const float yc = ((v.m[4] * X + v.m[5] * Y) + v.m[6] * Z) + v.m[7];
  zc = ((v.m[8] * X + v.m[9] * Y) + v.m[10] * Z) + v.m[11];
  u = (v.focal * xc) / zc + v.ppx;
  w_ = (v.focal * yc) / zc + v.ppy;
  return zc > 0.0f;
}

// steps 1-7: the LDS entry (raw cost, bit 15 = in view) of a halo pixel with reference value gr (< 0: outside the reference frame)
__device__ __forceinline__ int raw_cost(const uint8_t* __restrict__ g, const View& v, int gr, float rx, float ry, float z, int T) {
  if (gr < 0) return T;
  float u, w_, zc;
  const bool front = project(v, rx * z, ry * z, z, u, w_, zc);
  if (!(front && u >= 0.0f && u <= (float)(v.w - 1) && w_ >= 0.0f && w_ <= (float)(v.h - 1))) return T;
  const int x0 = min(max((int)floorf(u), 0), v.w - 1), y0 = min(max((int)floorf(w_), 0), v.h - 1);   // the clamps only restate the test
  const int x1 = min(x0 + 1, v.w - 1), y1 = min(y0 + 1, v.h - 1);
  const float fx = u - (float)x0, fy = w_ - (float)y0;
  const uint8_t* img = g + v.offset;
  const float a = (float)img[y0 * v.w + x0], b = (float)img[y0 * v.w + x1];
  const float c = (float)img[y1 * v.w + x0], d = (float)img[y1 * v.w + x1];
  const float top = a + fx * (b - a);
  const float bot = c + fx * (d - c);
  const float val = top + fy * (bot - top);
  const int sample = (int)(val + 0.5f);
  return min(abs(gr - sample), T) | MV_IN_VIEW;
}

// VOLUME: write C(p, k) | V(p, k) << 15 of every plane to `volume` ([y][x][k] of the reference frame) and nothing else.
template <bool VOLUME>
__global__ void __launch_bounds__(MV_THREADS) sweep_kernel(const uint8_t* __restrict__ g, const SweepArgs a, float* __restrict__ out_depth,
                                                           int32_t* __restrict__ out_cost, int32_t* __restrict__ out_plane,
                                                           uint16_t* __restrict__ volume) {
  __shared__ uint16_t s_raw[2][MV_MAX_HALO];
  __shared__ View s_view[ACEZ_MVS_MAX_SOURCES];
  const int t = threadIdx.x;
  if (t == 0) {
#pragma unroll
    for (int s = 0; s < ACEZ_MVS_MAX_SOURCES; ++s) s_view[s] = a.src[s];   // constant offsets into the launch arguments
  }
  const int R = a.radius, side = MV_TILE + 2 * R, n_halo = side * side, T = a.truncation;
  const int x_base = blockIdx.x * MV_TILE - R, y_base = blockIdx.y * MV_TILE - R;
  int gr[MV_PER_THREAD];
  float rx[MV_PER_THREAD], ry[MV_PER_THREAD];
#pragma unroll
  for (int j = 0; j < MV_PER_THREAD; ++j) {
    const int e = t + j * MV_THREADS;
    const int hy = y_base + e / side, hx = x_base + e % side;
    const bool inside = e < n_halo && hx >= 0 && hx < a.w && hy >= 0 && hy < a.h;
    gr[j] = inside ? (int)g[a.offset + (int64_t)hy * a.w + hx] : -1;
    rx[j] = ((float)hx - a.ppx) / a.focal;
    ry[j] = ((float)hy - a.ppy) / a.focal;
  }
  __syncthreads();
  const int centre = ((t >> 4) + R) * side + (t & 15) + R;   // this thread's pixel in the halo tile; its window stays inside the tile
  int v0 = INT32_MAX, v1 = INT32_MAX, v2 = INT32_MAX, v3 = INT32_MAX;   // the four smallest (C, k), ascending, ties by k
  int k0 = -1, k1 = -1, k2 = -1, k3 = -1;
  int c_before = 0, c_after = 0, c_prev = 0, n_star = 0;
  int buf = 0;
  const int px = blockIdx.x * MV_TILE + (t & 15), py = blockIdx.y * MV_TILE + (t >> 4);
  const bool in_frame = px < a.w && py < a.h;
  const int64_t cell = ((int64_t)py * a.w + px) * a.planes;   // this pixel's run of the volume
  for (int k = 0; k < a.planes; ++k) {
    const float inv_k = a.inv_far + (float)k * a.step;
    const float z = 1.0f / inv_k;
    int A[ACEZ_MVS_MAX_SOURCES];                               // A_s in ascending order; only constant indices
#pragma unroll
    for (int i = 0; i < ACEZ_MVS_MAX_SOURCES; ++i) A[i] = MV_NO_COST;
    int n_in = 0;
    for (int s = 0; s < a.n_sources; ++s) {                   // uniform over the grid
      const View v = s_view[s];                               // one address for the whole wave: broadcast reads
#pragma unroll
      for (int j = 0; j < MV_PER_THREAD; ++j) {
        const int e = t + j * MV_THREADS;
        if (e < n_halo) s_raw[buf][e] = (uint16_t)raw_cost(g, v, gr[j], rx[j], ry[j], z, T);
      }
      __syncthreads();
      int sum = 0;
      for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) sum += s_raw[buf][centre + dy * side + dx] & (MV_IN_VIEW - 1);
      n_in += s_raw[buf][centre] >> 15;
      buf ^= 1;                                               // the next step writes the other tile: one barrier per step
#pragma unroll
      for (int i = 0; i < ACEZ_MVS_MAX_SOURCES; ++i) {        // insert into the ascending list
        const int lo = min(A[i], sum);
        sum = max(A[i], sum);
        A[i] = lo;
      }
    }
    int C = 0;
#pragma unroll
    for (int i = 0; i < ACEZ_MVS_MAX_SOURCES; ++i)
      if (i < a.keep) C += A[i];
    if constexpr (VOLUME) {
      if (in_frame) volume[cell + k] = (uint16_t)(C | (n_in >= a.keep ? MV_IN_VIEW : 0));   // the host checked C <= 32767
      continue;
    }
    if (k0 == k - 1) c_after = C;                             // (k0 = -1 at k = 0: c_after is only read for an interior k*)
    if (C < v0) {
      c_before = c_prev;
      n_star = n_in;
    }
    c_prev = C;
    if (C < v3) {
      v3 = C, k3 = k;
      if (v3 < v2) {
        int tv = v2, tk = k2;
        v2 = v3, k2 = k3, v3 = tv, k3 = tk;
        if (v2 < v1) {
          tv = v1, tk = k1;
          v1 = v2, k1 = k2, v2 = tv, k2 = tk;
          if (v1 < v0) {
            tv = v0, tk = k0;
            v0 = v1, k0 = k1, v1 = tv, k1 = tk;
          }
        }
      }
    }
  }
  if (VOLUME || !in_frame) return;                            // (after the last barrier)
  const int x = px, y = py;
  const int best = v0, ks = k0, D = a.planes;
  bool unique = true;                                         // no plane outside the neighbourhood (D <= 3)
  if (k1 >= 0 && abs(k1 - ks) > 1) unique = v1 > 0 && 100 * best <= (100 - a.uniqueness) * v1;
  else if (k2 >= 0 && abs(k2 - ks) > 1) unique = v2 > 0 && 100 * best <= (100 - a.uniqueness) * v2;
  else if (k3 >= 0 && abs(k3 - ks) > 1) unique = v3 > 0 && 100 * best <= (100 - a.uniqueness) * v3;
  float delta = 0.0f;
  if (ks > 0 && ks < D - 1) {
    const int den = c_before - 2 * best + c_after;
    if (den > 0) delta = (float)(c_before - c_after) / (float)(2 * den);
  }
  float depth = 1.0f / (a.inv_far + ((float)ks + delta) * a.step);
  if (n_star < a.keep || !unique || (D > 2 && (ks == 0 || ks == D - 1))) depth = 0.0f;
  const int64_t at = a.offset + (int64_t)y * a.w + x;
  out_depth[at] = depth;
  if (out_cost) out_cost[at] = best;
  if (out_plane) out_plane[at] = ks;
}

__global__ void __launch_bounds__(MV_THREADS) check_kernel(const float* __restrict__ depth, const CheckArgs a, uint16_t* __restrict__ out) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= a.w || y >= a.h) return;
  const int64_t at = a.offset + (int64_t)y * a.w + x;
  const float d = depth[at];
  uint16_t result = 0;
  if (d > 0.0f) {
    const float rx = ((float)x - a.ppx) / a.focal, ry = ((float)y - a.ppy) / a.focal;
    const float X = rx * d, Y = ry * d;
    int agree = 0;
#pragma unroll
    for (int s = 0; s < ACEZ_MVS_MAX_SOURCES; ++s) {
      if (s < a.n_sources) {
        const View& v = a.src[s];
        float u, w_, zc;
        const bool front = project(v, X, Y, d, u, w_, zc);
        if (front && u >= -0.5f && u < (float)v.w - 0.5f && w_ >= -0.5f && w_ < (float)v.h - 0.5f) {
          const int ix = min(max((int)floorf(u + 0.5f), 0), v.w - 1), iy = min(max((int)floorf(w_ + 0.5f), 0), v.h - 1);
          const float ds = depth[v.offset + (int64_t)iy * v.w + ix];
          if (ds > 0.0f && fabsf(ds - zc) <= a.tolerance * zc) ++agree;
        }
      }
    }
    const float qd = floorf(d / a.depth_unit + 0.5f);
    if (agree >= a.need && qd <= 65535.0f) result = (uint16_t)qd;
  }
  out[at] = result;
}

// ------------------------------------------------------------------------------------------------- section M: aggregate, select
constexpr int AG_INF = 1 << 29;          // an absent plane: above any L_r (<= 65534), and AG_INF + P1 does not overflow
constexpr int AG_LINES = MV_THREADS / 64;   // scanlines (wavefronts) per workgroup
constexpr int AG_AHEAD = 4;              // pixels of a scanline whose costs are requested before they are needed
constexpr int SEL_LANES = 16;            // lanes per pixel of the select kernel

struct AggArgs {
  int h, w, planes, p1, p2, n_dirs;
  int dy[8], dx[8];
  int first[9];                          // first[i] .. first[i + 1] - 1: the scanlines of the call's i-th direction
};

// lane l's value of lane (l - 1) mod 64 / (l + 1) mod 64: one DPP move over the whole wave (wave_ror:1 = 0x13C, wave_rol:1 = 0x134)
__device__ __forceinline__ int from_lane_below(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x13C, 0xF, 0xF, false); }
__device__ __forceinline__ int from_lane_above(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x134, 0xF, 0xF, false); }

// the minimum over the wave's 64 lanes as a scalar: xor 1, xor 2 inside a quad, mirror inside 8, mirror inside 16, then the four rows
__device__ __forceinline__ int wave_min(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));    // quad_perm [1, 0, 3, 2]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));    // quad_perm [2, 3, 0, 1]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// NPL: planes per lane; the host picks the smallest with 64 * NPL >= D
template <int NPL>
__global__ void __launch_bounds__(MV_THREADS) aggregate_kernel(const uint16_t* __restrict__ volume, uint32_t* __restrict__ S, const AggArgs a) {
  const int lane = threadIdx.x & 63;
  const int line = __builtin_amdgcn_readfirstlane((int)blockIdx.x * AG_LINES + (int)(threadIdx.x >> 6));
  if (line >= a.first[8]) return;   // (first[8] = the call's scanlines) whole waves leave: every DPP move below sees 64 active lanes
  int dy = a.dy[0], dx = a.dx[0], base = 0;
#pragma unroll
  for (int i = 1; i < 8; ++i)
    if (i < a.n_dirs && line >= a.first[i]) dy = a.dy[i], dx = a.dx[i], base = a.first[i];
  // the scanline's first pixel: the pixels whose predecessor is outside the frame, the edge dy enters through first, then dx's edge
  const int i = line - base, h = a.h, w = a.w, D = a.planes, P1 = a.p1, P2 = a.p2;
  int x, y;
  if (dy != 0 && i < w) {
    x = i, y = dy > 0 ? 0 : h - 1;
  } else {
    const int j = i - (dy != 0 ? w : 0);
    y = dy == 0 ? j : (dy > 0 ? j + 1 : h - 2 - j);
    x = dx > 0 ? 0 : w - 1;
  }
  auto inside = [&](int px, int py) { return px >= 0 && px < w && py >= 0 && py < h; };   // uniform over the wave
  auto load = [&](int (&dst)[NPL], int px, int py) {
    const int64_t at = ((int64_t)min(max(py, 0), h - 1) * w + min(max(px, 0), w - 1)) * D;   // past the scanline's end: a pixel nobody uses
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int k = j * 64 + lane;
      dst[j] = volume[at + min(k, D - 1)];   // raw, and read by every lane: whatever uses the value next to the read waits for it there
    }
  };
  // The raw costs of the next AG_AHEAD pixels of the scanline are in flight or in registers. For a read to stay in flight it must
  // not sit under a branch (so every lane reads, at clamped plane and pixel) and its value must first be touched in the step that
  // consumes it: otherwise the wait for it is placed right behind the read. The waits then sit once per unrolled round of AG_AHEAD steps.
  int ahead[AG_AHEAD][NPL], L[NPL];
#pragma unroll
  for (int s = 0; s < AG_AHEAD; ++s)
    load(ahead[s], x + s * dx, y + s * dy);
  int m = 0;
  bool first = true;
  while (true) {
#pragma unroll
    for (int s = 0; s < AG_AHEAD; ++s) {                      // constant indices into `ahead`
      const int64_t at = ((int64_t)y * w + x) * D;
      int c[NPL];
#pragma unroll
      for (int j = 0; j < NPL; ++j) c[j] = j * 64 + lane < D ? (ahead[s][j] & (MV_IN_VIEW - 1)) : AG_INF;
      load(ahead[s], x + AG_AHEAD * dx, y + AG_AHEAD * dy);
      if (first) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) L[j] = c[j];
        first = false;
      } else {
        int below[NPL], above[NPL];
#pragma unroll
        for (int j = 0; j < NPL; ++j) below[j] = from_lane_below(L[j]), above[j] = from_lane_above(L[j]);
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
          // plane k - 1 is the lane below, for lane 0 lane 63 of the register before; k + 1 alike. AG_INF: absent
          const int prev = lane == 0 ? (j > 0 ? below[j > 0 ? j - 1 : 0] : AG_INF) : below[j];
          const int next = lane == 63 ? (j < NPL - 1 ? above[j < NPL - 1 ? j + 1 : 0] : AG_INF) : above[j];
          const int best = min(min(L[j], min(prev, next) + P1), m + P2);
          c[j] = c[j] < AG_INF ? c[j] + (best - m) : AG_INF;
        }
#pragma unroll
        for (int j = 0; j < NPL; ++j) L[j] = c[j];
      }
      int lowest = L[0];
#pragma unroll
      for (int j = 1; j < NPL; ++j) lowest = min(lowest, L[j]);
      m = wave_min(lowest);
#pragma unroll
      for (int j = 0; j < NPL; ++j) {
        const int k = j * 64 + lane;
        if (k < D) atomicAdd(&S[at + k], (uint32_t)L[j]);      // the result is not read: an atomic without return
      }
      x += dx, y += dy;
      if (!inside(x, y)) return;
    }
  }
}

struct SelectArgs {
  int h, w, planes, uniqueness;
  int64_t offset;
  float inv_far, step;
};

// X = S, or C of the volume where S is null. 16 lanes share a pixel; a workgroup has 16 pixels.
__global__ void __launch_bounds__(MV_THREADS) select_kernel(const uint16_t* __restrict__ volume, const uint32_t* __restrict__ S, const SelectArgs a,
                                                            float* __restrict__ out_depth, int32_t* __restrict__ out_cost,
                                                            int32_t* __restrict__ out_plane) {
  const int sub = threadIdx.x & (SEL_LANES - 1), D = a.planes;
  const int64_t pixel = (int64_t)blockIdx.x * (MV_THREADS / SEL_LANES) + (threadIdx.x / SEL_LANES);
  if (pixel >= (int64_t)a.h * a.w) return;                    // all 16 lanes of a pixel leave together
  const int64_t at = pixel * D;
  auto X = [&](int k) { return S ? (int)S[at + k] : (int)(volume[at + k] & (MV_IN_VIEW - 1)); };
  int key = INT32_MAX;                                        // X * 1024 + k: X <= 8 * 65534 < 2^19, k < 2^10; its minimum is the first minimum
  for (int k = sub; k < D; k += SEL_LANES) key = min(key, X(k) * 1024 + k);
#pragma unroll
  for (int d = SEL_LANES / 2; d >= 1; d >>= 1) key = min(key, __shfl_xor(key, d, SEL_LANES));
  const int ks = key & 1023, best = key >> 10;
  int c2 = INT32_MAX;                                         // INT32_MAX: no plane outside the neighbourhood
  for (int k = sub; k < D; k += SEL_LANES)
    if (abs(k - ks) > 1) c2 = min(c2, X(k));
#pragma unroll
  for (int d = SEL_LANES / 2; d >= 1; d >>= 1) c2 = min(c2, __shfl_xor(c2, d, SEL_LANES));
  if (sub != 0) return;
  const bool unique = c2 == INT32_MAX || (c2 > 0 && 100 * best <= (100 - a.uniqueness) * c2);
  float delta = 0.0f;
  if (ks > 0 && ks < D - 1) {
    const int before = X(ks - 1), after = X(ks + 1);
    const int den = before - 2 * best + after;
    if (den > 0) delta = (float)(before - after) / (float)(2 * den);
  }
  float depth = 1.0f / (a.inv_far + ((float)ks + delta) * a.step);
  const bool in_view = (volume[at + ks] & MV_IN_VIEW) != 0;
  if (!in_view || !unique || (D > 2 && (ks == 0 || ks == D - 1))) depth = 0.0f;
  const int64_t out = a.offset + pixel;
  out_depth[out] = depth;
  if (out_cost) out_cost[out] = best;
  if (out_plane) out_plane[out] = ks;
}

void relative(const acez_mvs_frame& r, const acez_mvs_frame& s, float* out12) {
  for (int i = 0; i < 3; ++i) {
    double R[3];
    for (int j = 0; j < 3; ++j)
      R[j] = ((double)s.m[4 * i] * (double)r.m[4 * j] + (double)s.m[4 * i + 1] * (double)r.m[4 * j + 1]) + (double)s.m[4 * i + 2] * (double)r.m[4 * j + 2];
    const double t = (double)s.m[4 * i + 3] - ((R[0] * (double)r.m[3] + R[1] * (double)r.m[7]) + R[2] * (double)r.m[11]);
    out12[4 * i] = (float)R[0];
    out12[4 * i + 1] = (float)R[1];
    out12[4 * i + 2] = (float)R[2];
    out12[4 * i + 3] = (float)t;
  }
}

View view_of(const acez_mvs_frame& r, const acez_mvs_frame& s) {
  View v;
  relative(r, s, v.m);
  v.focal = s.focal, v.ppx = s.ppx, v.ppy = s.ppy, v.h = s.h, v.w = s.w, v.offset = s.offset;
  return v;
}

}  // namespace

// the rows a sweep or a check touches: the reference and its sources
#define MV_REQUIRE_VIEWS()                                                                                               \
  ACEZ_REQUIRE(n_pixels >= 0, "negative buffer length");                                                                 \
  ACEZ_REQUIRE(n_frames >= 1, "frame count must be at least 1");                                                         \
  ACEZ_REQUIRE(ref >= 0 && ref < n_frames, "reference index outside the frame table");                                   \
  ACEZ_REQUIRE(n_sources >= 1 && n_sources <= ACEZ_MVS_MAX_SOURCES, "source count out of range (1 .. 8)");                \
  if (int rc = acez::check_frame(h_frames[ref], n_pixels)) return rc;                                                    \
  for (int s = 0; s < n_sources; ++s) {                                                                                  \
    ACEZ_REQUIRE(h_sources[s] >= 0 && h_sources[s] < n_frames, "source index outside the frame table");                  \
    if (int rc = acez::check_frame(h_frames[h_sources[s]], n_pixels)) return rc;                                         \
  }

extern "C" int acez_mvs_prefilter(const uint8_t* d_grey, uint8_t* d_out, int64_t n_pixels, const acez_mvs_frame* h_frames, int n_frames,
                                  acez_mvs_frame* d_frames, void* stream) {
  ACEZ_REQUIRE(d_grey && d_out && h_frames && d_frames, "null pointer");
  ACEZ_REQUIRE(n_pixels >= 0, "negative buffer length");
  ACEZ_REQUIRE(n_frames >= 1 && n_frames <= 65535, "frame count out of range (1 .. 65535)");
  int64_t largest = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (int rc = acez::check_frame(h_frames[f], n_pixels)) return rc;
    largest = largest > (int64_t)h_frames[f].h * h_frames[f].w ? largest : (int64_t)h_frames[f].h * h_frames[f].w;
  }
  if (int rc = acez::require_device("the stereo prefilter runs on a gfx950 GPU")) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = acez::upload_frames(d_frames, h_frames, n_frames, s)) return rc;
  const dim3 grid((unsigned)((largest + MV_THREADS - 1) / MV_THREADS), (unsigned)n_frames);
  hipLaunchKernelGGL(prefilter_kernel, grid, dim3(MV_THREADS), 0, s, d_grey, d_out, (const acez_mvs_frame*)d_frames);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_mvs_relative(const acez_mvs_frame* ref, const acez_mvs_frame* src, float* out12) {
  ACEZ_REQUIRE(ref && src && out12, "null pointer");
  ACEZ_REQUIRE(acez::finite_all(ref->m, 12) && acez::finite_all(src->m, 12), "non-finite pose or intrinsics in the frame table");
  relative(*ref, *src, out12);
  return ACEZ_OK;
}

// the argument checks and the launch arguments the sweep and the volume share
static int sweep_args(const uint8_t* d_filtered, int64_t n_pixels, const acez_mvs_frame* h_frames, int n_frames, int ref,
                      const int32_t* h_sources, int n_sources, float z_near, float z_far, int planes, int radius, int truncation, int keep,
                      int uniqueness, const void* d_out, SweepArgs& a) {
  ACEZ_REQUIRE(d_filtered && h_frames && h_sources && d_out, "null pointer");
  MV_REQUIRE_VIEWS();
  ACEZ_REQUIRE(isfinite(z_near) && isfinite(z_far) && z_near > 0.0f && z_near < z_far, "the depth range needs 0 < near < far");
  ACEZ_REQUIRE(planes >= 2 && planes <= 1024, "plane count out of range (2 .. 1024)");
  ACEZ_REQUIRE(radius >= 0 && radius <= MV_MAX_RADIUS, "window radius out of range (0 .. 4)");
  ACEZ_REQUIRE(truncation >= 1 && truncation <= 255, "cost truncation out of range (1 .. 255)");
  ACEZ_REQUIRE(keep >= 1 && keep <= n_sources, "keep out of range (1 .. sources)");
  ACEZ_REQUIRE(uniqueness >= 0 && uniqueness <= 100, "uniqueness percentage out of range (0 .. 100)");
  const acez_mvs_frame& r = h_frames[ref];
  for (int s = 0; s < ACEZ_MVS_MAX_SOURCES; ++s) a.src[s] = view_of(r, h_frames[h_sources[s < n_sources ? s : 0]]);
  a.focal = r.focal, a.ppx = r.ppx, a.ppy = r.ppy, a.h = r.h, a.w = r.w, a.offset = r.offset;
  const float inv_near = 1.0f / z_near;
  a.inv_far = 1.0f / z_far;
  a.step = (inv_near - a.inv_far) / (float)(planes - 1);
  a.planes = planes, a.radius = radius, a.truncation = truncation, a.keep = keep, a.uniqueness = uniqueness, a.n_sources = n_sources;
  return ACEZ_OK;
}

extern "C" int acez_mvs_sweep(const uint8_t* d_filtered, int64_t n_pixels, const acez_mvs_frame* h_frames, int n_frames, int ref,
                              const int32_t* h_sources, int n_sources, float z_near, float z_far, int planes, int radius, int truncation,
                              int keep, int uniqueness, float* d_out_depth, int32_t* d_out_cost, int32_t* d_out_plane, void* stream) {
  SweepArgs a;
  if (int rc = sweep_args(d_filtered, n_pixels, h_frames, n_frames, ref, h_sources, n_sources, z_near, z_far, planes, radius, truncation, keep,
                          uniqueness, d_out_depth, a))
    return rc;
  if (int rc = acez::require_device("the plane sweep runs on a gfx950 GPU")) return rc;
  const dim3 grid((a.w + MV_TILE - 1) / MV_TILE, (a.h + MV_TILE - 1) / MV_TILE);
  hipLaunchKernelGGL(sweep_kernel<false>, grid, dim3(MV_THREADS), 0, (hipStream_t)stream, d_filtered, a, d_out_depth, d_out_cost, d_out_plane,
                     (uint16_t*)nullptr);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_mvs_check(const float* d_depth, int64_t n_pixels, const acez_mvs_frame* h_frames, int n_frames, int ref,
                              const int32_t* h_sources, int n_sources, float tolerance, int min_consistent, float depth_unit,
                              uint16_t* d_out, void* stream) {
  ACEZ_REQUIRE(d_depth && h_frames && h_sources && d_out, "null pointer");
  MV_REQUIRE_VIEWS();
  ACEZ_REQUIRE(isfinite(tolerance) && tolerance >= 0.0f, "tolerance must be finite and not negative");
  ACEZ_REQUIRE(min_consistent >= 0, "min_consistent must not be negative");
  ACEZ_REQUIRE(isfinite(depth_unit) && depth_unit > 0.0f, "depth unit must be positive");
  CheckArgs a;
  const acez_mvs_frame& r = h_frames[ref];
  for (int s = 0; s < ACEZ_MVS_MAX_SOURCES; ++s) a.src[s] = view_of(r, h_frames[h_sources[s < n_sources ? s : 0]]);
  a.focal = r.focal, a.ppx = r.ppx, a.ppy = r.ppy, a.h = r.h, a.w = r.w, a.offset = r.offset;
  a.tolerance = tolerance, a.depth_unit = depth_unit;
  a.need = min_consistent < n_sources ? min_consistent : n_sources;
  a.n_sources = n_sources;
  if (int rc = acez::require_device("the consistency check runs on a gfx950 GPU")) return rc;
  const dim3 grid((r.w + 63) / 64, (r.h + 3) / 4);
  hipLaunchKernelGGL(check_kernel, grid, dim3(MV_THREADS), 0, (hipStream_t)stream, d_depth, a, d_out);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

// ------------------------------------------------------------------------------------------------------------------ section M
extern "C" int acez_mvs_volume(const uint8_t* d_filtered, int64_t n_pixels, const acez_mvs_frame* h_frames, int n_frames, int ref,
                               const int32_t* h_sources, int n_sources, float z_near, float z_far, int planes, int radius, int truncation,
                               int keep, uint16_t* d_volume, int64_t n_volume, void* stream) {
  SweepArgs a;
  if (int rc = sweep_args(d_filtered, n_pixels, h_frames, n_frames, ref, h_sources, n_sources, z_near, z_far, planes, radius, truncation, keep,
                          0, d_volume, a))
    return rc;
  ACEZ_REQUIRE(keep * (2 * radius + 1) * (2 * radius + 1) * truncation <= 32767, "keep * (2 * radius + 1)^2 * truncation exceeds 32767: the costs do not fit the volume's 15 bits");
  ACEZ_REQUIRE(n_volume >= 0 && (int64_t)a.h * a.w * planes <= n_volume, "volume smaller than h * w * planes elements");
  if (int rc = acez::require_device("the cost volume runs on a gfx950 GPU")) return rc;
  const dim3 grid((a.w + MV_TILE - 1) / MV_TILE, (a.h + MV_TILE - 1) / MV_TILE);
  hipLaunchKernelGGL(sweep_kernel<true>, grid, dim3(MV_THREADS), 0, (hipStream_t)stream, d_filtered, a, (float*)nullptr, (int32_t*)nullptr,
                     (int32_t*)nullptr, d_volume);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_mvs_aggregate(const uint16_t* d_volume, uint32_t* d_s, int64_t n_volume, int h, int w, int planes, int paths, int direction,
                                  int p1, int p2, void* stream) {
  static const int DY[8] = {0, 0, 1, -1, 1, 1, -1, -1}, DX[8] = {1, -1, 0, 0, 1, -1, 1, -1};
  ACEZ_REQUIRE(d_volume && d_s, "null pointer");
  ACEZ_REQUIRE(h >= 1 && w >= 1 && h <= acez::FRAME_MAX_SIDE && w <= acez::FRAME_MAX_SIDE, "frame size out of range (1 .. 32768 px per side)");
  ACEZ_REQUIRE(planes >= 2 && planes <= 1024, "plane count out of range (2 .. 1024)");
  ACEZ_REQUIRE(paths == 4 || paths == 8, "paths must be 4 or 8");
  ACEZ_REQUIRE(direction >= 0 && direction <= paths, "direction out of range (0 = all, 1 .. paths)");
  ACEZ_REQUIRE(p1 >= 1 && p1 <= p2 && p2 <= 32767, "penalties need 1 <= P1 <= P2 <= 32767");
  ACEZ_REQUIRE(n_volume >= 0 && (int64_t)h * w * planes <= n_volume, "volume smaller than h * w * planes elements");
  AggArgs a;
  a.h = h, a.w = w, a.planes = planes, a.p1 = p1, a.p2 = p2;
  a.n_dirs = direction ? 1 : paths;
  a.first[0] = 0;
  for (int i = 0; i < 8; ++i) {
    const int d = direction ? direction - 1 : (i < paths ? i : 0);
    a.dy[i] = DY[d], a.dx[i] = DX[d];
    const int lines = (DY[d] ? w : 0) + (DX[d] ? h : 0) - (DY[d] && DX[d] ? 1 : 0);   // <= 65535
    a.first[i + 1] = a.first[i] + (i < a.n_dirs ? lines : 0);
  }
  if (int rc = acez::require_device("the cost aggregation runs on a gfx950 GPU")) return rc;
  const dim3 grid((a.first[8] + AG_LINES - 1) / AG_LINES), block(MV_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (planes <= 64) hipLaunchKernelGGL(aggregate_kernel<1>, grid, block, 0, s, d_volume, d_s, a);
  else if (planes <= 128) hipLaunchKernelGGL(aggregate_kernel<2>, grid, block, 0, s, d_volume, d_s, a);
  else if (planes <= 256) hipLaunchKernelGGL(aggregate_kernel<4>, grid, block, 0, s, d_volume, d_s, a);
  else if (planes <= 512) hipLaunchKernelGGL(aggregate_kernel<8>, grid, block, 0, s, d_volume, d_s, a);
  else hipLaunchKernelGGL(aggregate_kernel<16>, grid, block, 0, s, d_volume, d_s, a);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_mvs_select(const uint16_t* d_volume, const uint32_t* d_s, int64_t n_volume, int64_t n_pixels, const acez_mvs_frame* h_frames,
                               int n_frames, int ref, float z_near, float z_far, int planes, int uniqueness, float* d_out_depth,
                               int32_t* d_out_cost, int32_t* d_out_plane, void* stream) {
  ACEZ_REQUIRE(d_volume && h_frames && d_out_depth, "null pointer");
  ACEZ_REQUIRE(n_pixels >= 0, "negative buffer length");
  ACEZ_REQUIRE(n_frames >= 1, "frame count must be at least 1");
  ACEZ_REQUIRE(ref >= 0 && ref < n_frames, "reference index outside the frame table");
  if (int rc = acez::check_frame(h_frames[ref], n_pixels)) return rc;
  ACEZ_REQUIRE(isfinite(z_near) && isfinite(z_far) && z_near > 0.0f && z_near < z_far, "the depth range needs 0 < near < far");
  ACEZ_REQUIRE(planes >= 2 && planes <= 1024, "plane count out of range (2 .. 1024)");
  ACEZ_REQUIRE(uniqueness >= 0 && uniqueness <= 100, "uniqueness percentage out of range (0 .. 100)");
  const acez_mvs_frame& r = h_frames[ref];
  ACEZ_REQUIRE(n_volume >= 0 && (int64_t)r.h * r.w * planes <= n_volume, "volume smaller than h * w * planes elements");
  SelectArgs a;
  a.h = r.h, a.w = r.w, a.planes = planes, a.uniqueness = uniqueness, a.offset = r.offset;
  const float inv_near = 1.0f / z_near;
  a.inv_far = 1.0f / z_far;
  a.step = (inv_near - a.inv_far) / (float)(planes - 1);
  if (int rc = acez::require_device("the plane selection runs on a gfx950 GPU")) return rc;
  const int per_block = MV_THREADS / SEL_LANES;
  const dim3 grid((unsigned)(((int64_t)r.h * r.w + per_block - 1) / per_block));
  hipLaunchKernelGGL(select_kernel, grid, dim3(MV_THREADS), 0, (hipStream_t)stream, d_volume, d_s, a, d_out_depth, d_out_cost, d_out_plane);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
