// ingest_api.hip -- image ingest on the device (include/acez.h section I: acez_ingest_coeffs, acez_ingest_frames).
//
// Decoded uint8 RGB frames become what cli.load_frames computes on the host with Pillow: the frame resized by Pillow's 8-bit
// resize(BILINEAR), its grey conversion convert("L"), and the grey value normalised to float32. Everything is integer arithmetic, so
// the device result equals Pillow's bit for bit:
//   tables      per axis (in -> out samples): for every output index the first source index, the tap count and the taps as int32
//               fixed point with 22 fraction bits. Computed here on the host in double, in Pillow's order (precompute_coeffs and
//               normalize_coeffs_8bpc of its Resample.c), cached per (in, out) pair, and copied into the caller's table block on the
//               stream with every call (a few tens of KB);
//   horizontal  one thread per output byte of a row: (2^21 + sum pixel * tap) >> 22, clipped, stored as uint8 -- Pillow runs the
//               horizontal pass first and keeps its result in 8 bits;
//   vertical    one thread per output pixel: the same sum over rows for R, G and B, then L = (R * 19595 + G * 38470 + B * 7471 + 2^15)
//               >> 16 and the float32 looked up in the caller's 256-entry table (the host builds it with load_frames' own numpy
//               expression, so no float arithmetic happens here).
// All taps are non-negative and sum to 2^22 up to rounding, so 255 * (2^22 + ksize) + 2^21 < 2^31: an int32 accumulator is enough.
// The tap count is a loop bound read from the table: a source of any size goes through the same two kernels.
#include <math.h>
#include <stdint.h>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>
#include "acez_common.h"

namespace {

constexpr int IG_THREADS = 256;
constexpr int IG_BITS = 22;                     // fraction bits of a tap (Pillow's PRECISION_BITS = 32 - 8 - 2)
constexpr int IG_MAX_SIDE = 32768;              // pixels per side, source and result
constexpr int IG_MAX_FRAMES = 65535;
constexpr int IG_MAX_GRID_Y = 65535;
constexpr int IG_MAX_SCENE_COORDINATES = 16384; // per frame, as session.check_frame_size refuses it (the DSAC* kernel's limit)

struct AxisTable {
  int ksize = 0;
  std::vector<int32_t> bounds;                  // [out][2]: first source index, tap count
  std::vector<int32_t> taps;                    // [out][ksize], zero past the tap count
};

inline double triangle(double v) {
  if (v < 0.0) v = -v;
  return v < 1.0 ? 1.0 - v : 0.0;
}

void build_axis(int in, int out, AxisTable& t) {
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = fs;                    // the bilinear filter's support is 1
  const int ksize = (int)ceil(support) * 2 + 1;
  t.ksize = ksize;
  t.bounds.assign((size_t)out * 2, 0);
  t.taps.assign((size_t)out * ksize, 0);
  std::vector<double> k((size_t)ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      const double w = triangle((x + xmin - center + 0.5) / fs);
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) k[x] /= ww;
      t.taps[(size_t)xx * ksize + x] = (int32_t)(0.5 + k[x] * (double)(1 << IG_BITS));
    }
    t.bounds[2 * (size_t)xx] = xmin;
    t.bounds[2 * (size_t)xx + 1] = xmax;
  }
}

// The table of one axis; built once per (in, out) pair and kept for the life of the process, so the pointer stays valid.
const AxisTable* axis_table(int in, int out) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, std::unique_ptr<AxisTable>> cache;
  std::lock_guard<std::mutex> lock(mu);
  std::unique_ptr<AxisTable>& slot = cache[std::make_pair(in, out)];
  if (!slot) {
    slot.reset(new AxisTable());
    build_axis(in, out, *slot);
  }
  return slot.get();
}

__device__ __forceinline__ int32_t clip8(int32_t acc) {
  const int32_t v = acc >> IG_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// src uint8 [rows][W][3] -> tmp uint8 [rows][nw][3], rows = n * H. Thread t of a row makes output byte t = 3 * xx + channel.
__global__ void __launch_bounds__(IG_THREADS) ingest_horizontal_kernel(const uint8_t* __restrict__ src, int64_t rows, int W, int nw,
                                                                       const int32_t* __restrict__ bounds, const int32_t* __restrict__ taps,
                                                                       int ksize, uint8_t* __restrict__ tmp) {
  const int t = blockIdx.x * IG_THREADS + threadIdx.x;
  if (t >= nw * 3) return;
  const int xx = t / 3, c = t - 3 * xx;
  const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
  const int32_t* k = taps + (int64_t)xx * ksize;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const uint8_t* s = src + (row * W + xmin) * 3 + c;
    int32_t acc = 1 << (IG_BITS - 1);
    for (int x = 0; x < cnt; ++x) acc += (int32_t)s[3 * x] * k[x];
    tmp[row * nw * 3 + t] = (uint8_t)clip8(acc);
  }
}

// tmp uint8 [n][H][nw][3] -> rgb uint8 [n][nh][nw][3] (may be null) and grey float32 [n][nh][nw]. One thread per output pixel.
__global__ void __launch_bounds__(IG_THREADS) ingest_vertical_kernel(const uint8_t* __restrict__ tmp, int64_t out_rows, int H, int nw, int nh,
                                                                     const int32_t* __restrict__ bounds, const int32_t* __restrict__ taps,
                                                                     int ksize, const float* __restrict__ norm, uint8_t* __restrict__ out_rgb,
                                                                     float* __restrict__ out_grey) {
  const int x = blockIdx.x * IG_THREADS + threadIdx.x;
  if (x >= nw) return;
  const int64_t stride = (int64_t)nw * 3;
  for (int64_t row = blockIdx.y; row < out_rows; row += gridDim.y) {
    const int64_t frame = row / nh;
    const int yy = (int)(row - frame * nh);
    const int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
    const int32_t* k = taps + (int64_t)yy * ksize;
    const uint8_t* s = tmp + (frame * H + ymin) * stride + (int64_t)x * 3;
    int32_t r = 1 << (IG_BITS - 1), g = r, b = r;
    for (int y = 0; y < cnt; ++y) {
      const uint8_t* p = s + y * stride;
      const int32_t w = k[y];
      r += (int32_t)p[0] * w;
      g += (int32_t)p[1] * w;
      b += (int32_t)p[2] * w;
    }
    r = clip8(r);
    g = clip8(g);
    b = clip8(b);
    const int32_t L = (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16;   // Pillow's convert("L"): at most 255
    out_grey[row * nw + x] = norm[L];
    if (out_rgb) {
      uint8_t* o = out_rgb + (row * nw + x) * 3;
      o[0] = (uint8_t)r;
      o[1] = (uint8_t)g;
      o[2] = (uint8_t)b;
    }
  }
}

inline bool side_ok(int v) { return v >= 1 && v <= IG_MAX_SIDE; }

}  // namespace

extern "C" int acez_ingest_coeffs(int in_size, int out_size, int* out_ksize, int32_t* out_bounds, int32_t* out_taps) {
  ACEZ_REQUIRE(out_ksize, "null pointer");
  ACEZ_REQUIRE(side_ok(in_size) && side_ok(out_size), "axis length out of range (1 .. 32768 samples)");
  const AxisTable* t = axis_table(in_size, out_size);
  *out_ksize = t->ksize;
  if (out_bounds) for (size_t i = 0; i < t->bounds.size(); ++i) out_bounds[i] = t->bounds[i];
  if (out_taps) for (size_t i = 0; i < t->taps.size(); ++i) out_taps[i] = t->taps[i];
  return ACEZ_OK;
}

extern "C" int acez_ingest_frames(const uint8_t* d_src, int n, int H, int W, int nh, int nw, uint8_t* d_tmp, int32_t* d_tables,
                                  int64_t table_bytes, const float* d_norm, uint8_t* d_out_rgb, float* d_out_grey, void* stream) {
  ACEZ_REQUIRE(d_src && d_tmp && d_tables && d_norm && d_out_grey, "null pointer");
  ACEZ_REQUIRE(n >= 1 && n <= IG_MAX_FRAMES, "frame count out of range (1 .. 65535)");
  ACEZ_REQUIRE(side_ok(H) && side_ok(W), "source size out of range (1 .. 32768 px per side)");
  ACEZ_REQUIRE(side_ok(nh) && side_ok(nw), "resized size out of range (1 .. 32768 px per side)");
  int oh = 0, ow = 0;
  if (int rc = acez_encoder_output_size(nh, nw, &oh, &ow)) return rc;
  ACEZ_REQUIRE((int64_t)oh * ow <= IG_MAX_SCENE_COORDINATES, "resized frame gives more than 16384 scene coordinates (lower the resolution)");
  const AxisTable* tx = axis_table(W, nw);
  const AxisTable* ty = axis_table(H, nh);
  // the caller's table block: [x bounds][x taps][y bounds][y taps], int32
  const size_t nbx = tx->bounds.size(), ntx = tx->taps.size(), nby = ty->bounds.size(), nty = ty->taps.size();
  ACEZ_REQUIRE(table_bytes >= (int64_t)((nbx + ntx + nby + nty) * sizeof(int32_t)),
               "table block too small: 4 * (nw * (2 + ksize_x) + nh * (2 + ksize_y)) bytes are needed (acez_ingest_coeffs gives ksize)");
  if (int rc = acez::require_device("image ingest runs on a gfx950 GPU")) return rc;
  hipStream_t s = (hipStream_t)stream;
  int32_t* d_bx = d_tables;
  int32_t* d_tx = d_bx + nbx;
  int32_t* d_by = d_tx + ntx;
  int32_t* d_ty = d_by + nby;
  ACEZ_HIP_CHECK(hipMemcpyAsync(d_bx, tx->bounds.data(), nbx * sizeof(int32_t), hipMemcpyHostToDevice, s));
  ACEZ_HIP_CHECK(hipMemcpyAsync(d_tx, tx->taps.data(), ntx * sizeof(int32_t), hipMemcpyHostToDevice, s));
  ACEZ_HIP_CHECK(hipMemcpyAsync(d_by, ty->bounds.data(), nby * sizeof(int32_t), hipMemcpyHostToDevice, s));
  ACEZ_HIP_CHECK(hipMemcpyAsync(d_ty, ty->taps.data(), nty * sizeof(int32_t), hipMemcpyHostToDevice, s));
  const int64_t rows = (int64_t)n * H, out_rows = (int64_t)n * nh;
  const dim3 gh((unsigned)((nw * 3 + IG_THREADS - 1) / IG_THREADS), (unsigned)(rows < IG_MAX_GRID_Y ? rows : IG_MAX_GRID_Y));
  hipLaunchKernelGGL(ingest_horizontal_kernel, gh, dim3(IG_THREADS), 0, s, d_src, rows, W, nw, (const int32_t*)d_bx, (const int32_t*)d_tx,
                     tx->ksize, d_tmp);
  ACEZ_HIP_CHECK(hipGetLastError());
  const dim3 gv((unsigned)((nw + IG_THREADS - 1) / IG_THREADS), (unsigned)(out_rows < IG_MAX_GRID_Y ? out_rows : IG_MAX_GRID_Y));
  hipLaunchKernelGGL(ingest_vertical_kernel, gv, dim3(IG_THREADS), 0, s, (const uint8_t*)d_tmp, out_rows, H, nw, nh, (const int32_t*)d_by,
                     (const int32_t*)d_ty, ty->ksize, d_norm, d_out_rgb, d_out_grey);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
