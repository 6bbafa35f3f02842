// buffer_api.hip -- creation of the training buffer around the encoder (include/acez.h: acez_buffer_*): the augmented views in front of
// it (acez_buffer_warp_views) and the sampling of its feature maps into buffer rows (acez_buffer_sample_views, _table).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/acez.h"
#include "acez_common.h"
#include "ordered_sum.h"

namespace acez {

// ---------------------------------------------------------------------------------------------------
// Augmented views (acez_buffer_warp_views, include/acez.h): the batched affine warp in front of the encoder when the buffer is filled with
// augmentation (dataset.py:283-343). HBM-bound by construction: 4 B read (gathered, cache-friendly: a rotation of a few degrees) + 4 B
// written per output pixel; the framework version moved an 8 B sampling-grid entry three times per pixel on top.
// Arithmetic follows ATen's grid sampler (GridSampler.h): unnormalise ((g + 1) * size - 1) / 2, reflect about -0.5 / size - 0.5, clip,
// four taps with bounds checks; the mask is "the zero-padded lookup into an all-ones image is positive" = source coordinate in (-1, size).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float warp_reflect(float x, int size) {   // reflect_coordinates(x, -1, 2 size - 1) then clip_coordinates
  const float mn = -0.5f, span = (float)size;
  x = fabsf(x - mn);
  const float extra = fmodf(x, span);
  const int flips = (int)floorf(x / span);
  x = (flips & 1) ? span - extra + mn : extra + mn;
  return fminf((float)(size - 1), fmaxf(x, 0.f));
}
__device__ __forceinline__ float warp_jitter(float v, float br, float ct, float m) {   // ColorJitter on the de-normalised grey value
  float g = fminf(fmaxf((v * 0.25f + 0.4f) * br, 0.f), 1.f);
  g = fminf(fmaxf((g - m) * ct + m, 0.f), 1.f);
  return (g - 0.4f) / 0.25f;
}
// mean over the frame of clamp((v * 0.25 + 0.4) * brightness, 0, 1): torchvision's adjust_contrast blends with the mean of the image it is
// given (the brightness-adjusted one). One workgroup per view, fixed summation order.
__global__ __launch_bounds__(1024) void warp_mean_kernel(const float* __restrict__ images, const int32_t* __restrict__ index, const float* __restrict__ jitter,
                                                         int hw, float* __restrict__ out_mean) {
  __shared__ float part[16];
  const int v = blockIdx.x, t = threadIdx.x;
  const float* img = images + (size_t)index[v] * hw;
  const float br = jitter[2 * v];
  float acc = 0.f;
  for (int i = t; i < hw; i += 1024) acc += fminf(fmaxf((img[i] * 0.25f + 0.4f) * br, 0.f), 1.f);
  acc = wave_sum(acc);
  if ((t & 63) == 0) part[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    float s = 0.f;
    for (int i = 0; i < 16; ++i) s += part[i];
    out_mean[v] = s / (float)hw;
  }
}
__global__ __launch_bounds__(256) void warp_views_kernel(const float* __restrict__ images, const int32_t* __restrict__ index, const float* __restrict__ theta,
                                                         const float* __restrict__ jitter, const float* __restrict__ mean, int H, int W, int hs, int ws,
                                                         float* __restrict__ out) {
  const int v = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= hs * ws) return;
  const int y = p / ws, x = p - y * ws;
  const float* th = theta + 6 * v;
  const float xn = (2.f * x + 1.f) / ws - 1.f, yn = (2.f * y + 1.f) / hs - 1.f;     // affine_grid's base grid, align_corners = False
  const float gx = xn * th[0] + yn * th[1] + th[2], gy = xn * th[3] + yn * th[4] + th[5];
  const float ix = warp_reflect(((gx + 1.f) * W - 1.f) * 0.5f, W), iy = warp_reflect(((gy + 1.f) * H - 1.f) * 0.5f, H);
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
  const float wx1 = ix - fx, wy1 = iy - fy, wx0 = (fx + 1.f) - ix, wy0 = (fy + 1.f) - iy;
  const float* img = images + (size_t)index[v] * H * W;
  float br = 1.f, ct = 1.f, m = 0.f;
  const bool jit = jitter != nullptr;
  if (jit) { br = jitter[2 * v]; ct = jitter[2 * v + 1]; m = mean[v]; }
  auto tap = [&](int yy, int xx) -> float {
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) return 0.f;
    const float val = img[(size_t)yy * W + xx];
    return jit ? warp_jitter(val, br, ct, m) : val;
  };
  out[((size_t)v * hs + y) * ws + x] = tap(y0, x0) * (wx0 * wy0) + tap(y0, x1) * (wx1 * wy0) + tap(y1, x0) * (wx0 * wy1) + tap(y1, x1) * (wx1 * wy1);
}
// the validity mask at feature resolution: cell (my, mx) reads view pixel (floor(my * hs / map_h), floor(mx * ws / map_w)) (the nearest-
// neighbour resize, ace_trainer.py:373-374), whose source coordinate must lie inside (-1, W) x (-1, H)
__global__ __launch_bounds__(256) void warp_mask_kernel(const float* __restrict__ theta, int H, int W, int hs, int ws, int mh, int mw, uint8_t* __restrict__ mask) {
  const int v = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= mh * mw) return;
  const int my = c / mw, mx = c - my * mw;
  const float sy = (float)hs / (float)mh, sx = (float)ws / (float)mw;
  const int y = min((int)floorf(my * sy), hs - 1), x = min((int)floorf(mx * sx), ws - 1);
  const float* th = theta + 6 * v;
  const float xn = (2.f * x + 1.f) / ws - 1.f, yn = (2.f * y + 1.f) / hs - 1.f;
  const float gx = xn * th[0] + yn * th[1] + th[2], gy = xn * th[3] + yn * th[4] + th[5];
  const float ix = ((gx + 1.f) * W - 1.f) * 0.5f, iy = ((gy + 1.f) * H - 1.f) * 0.5f;
  mask[(size_t)v * mh * mw + c] = (ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------
// Training-buffer sampling (ace_trainer.py:404-431): per view, `samples` feature rows are drawn uniformly WITH replacement
// among the pixels whose mask is set (torch.multinomial(mask, n, replacement=True) on equal weights) and appended to the
// buffer together with their target pixel 8 * (x + 0.5, y + 0.5) (ace_util.py:7-13) and the view index.
// The draw is a counter-based stream keyed by (seed, view id, sample): reproducible and independent of batching
// (torch's multinomial stream cannot be reproduced). One workgroup = one view x a slice of its samples:
// inclusive prefix counts of the mask in LDS, one wave per sample (binary search, then a 1 KiB row copy).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sample_draw(uint64_t seed, uint64_t view_id, uint32_t s) {
  return (uint32_t)(mix64(mix64(seed ^ (view_id * 0xD1342543DE82EF95ull)) + s) >> 32);
}

constexpr int SAMPLE_MAX_HW = 24576;   // feature-map pixels per view the LDS prefix array holds (e.g. 128 x 192)

// One view of a sampling launch: `feat` points at the view's first feature row, `mk` at its mask (NULL: every pixel valid), v is
// the view's position in the launch (keys its draws together with first_view_id and numbers its output rows).
__device__ __forceinline__ void sample_one_view(uint16_t* pref, int* part, const uint16_t* __restrict__ feat, const uint8_t* __restrict__ mk,
                                                int hw, int ow, int channels, int samples, uint64_t seed, uint64_t first_view_id, int v,
                                                int view_index_base, uint16_t* __restrict__ out_feat, float* __restrict__ out_px,
                                                int32_t* __restrict__ out_view, int32_t* __restrict__ out_pix) {
  const int t = threadIdx.x;
  const int per = (hw + 255) / 256;
  const int lo = t * per, hi = min(hw, lo + per);
  int cnt = 0;
  for (int p = lo; p < hi; ++p) cnt += mk ? (mk[p] != 0) : 1;
  part[t] = cnt;
  __syncthreads();
  // exclusive scan of the 256 partial counts (Hillis-Steele, 8 rounds)
  for (int off = 1; off < 256; off <<= 1) {
    const int x = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  const int nvalid = part[255];
  int run = part[t] - cnt;
  for (int p = lo; p < hi; ++p) {
    run += mk ? (mk[p] != 0) : 1;
    pref[p] = (uint16_t)run;
  }
  __syncthreads();
  if (nvalid == 0) return;   // the host never passes such a view (ace_trainer.py:377-378 skips it)
  const int lane = t & 63, wave = t >> 6;
  const int per_block = (samples + gridDim.y - 1) / gridDim.y;
  const int s_lo = blockIdx.y * per_block, s_hi = min(samples, s_lo + per_block);
  for (int s = s_lo + wave; s < s_hi; s += 4) {
    const uint32_t r = sample_draw(seed, first_view_id + v, (uint32_t)s);
    const uint32_t k = (uint32_t)(((uint64_t)r * (uint32_t)nvalid) >> 32);   // uniform in [0, nvalid)
    // smallest p with pref[p] > k  == the (k+1)-th valid pixel
    int a = 0, b = hw - 1;
    while (a < b) {
      const int m = (a + b) >> 1;
      if (pref[m] > k) b = m; else a = m + 1;
    }
    const int pix = a;
    const size_t dst = (size_t)v * samples + s;
    const uint16_t* src = feat + (size_t)pix * channels;
    for (int c = lane * 8; c < channels; c += 512)
      *reinterpret_cast<uint4*>(out_feat + dst * channels + c) = *reinterpret_cast<const uint4*>(src + c);
    if (lane == 0) {
      const int y = pix / ow, x = pix - y * ow;
      out_px[dst * 2 + 0] = 8.0f * ((float)x + 0.5f);
      out_px[dst * 2 + 1] = 8.0f * ((float)y + 0.5f);
      out_view[dst] = view_index_base + v;
      if (out_pix) out_pix[dst] = pix;
    }
  }
}

__global__ __launch_bounds__(256) void sample_views_kernel(const uint16_t* __restrict__ feat, const uint8_t* __restrict__ mask, int hw, int ow,
                                                           int channels, int samples, uint64_t seed, uint64_t first_view_id,
                                                           int view_index_base, uint16_t* __restrict__ out_feat, float* __restrict__ out_px,
                                                           int32_t* __restrict__ out_view, int32_t* __restrict__ out_pix) {
  __shared__ uint16_t pref[SAMPLE_MAX_HW];   // inclusive count of valid pixels up to p (hw <= 24576 < 65536)
  __shared__ int part[256];
  const int v = blockIdx.x;
  sample_one_view(pref, part, feat + (size_t)v * hw * channels, mask ? mask + (size_t)v * hw : nullptr, hw, ow, channels, samples, seed,
                  first_view_id, v, view_index_base, out_feat, out_px, out_view, out_pix);
}

// The same draws for views of any sizes in one launch, read in place from a resident feature store: view v's map starts at row
// table[v].row of `feat`, is table[v].map_h x table[v].map_w, and its mask starts at byte table[v].mask of `mask` (< 0: no mask).
// A view whose map would not fit max_hw (<= SAMPLE_MAX_HW), the n_rows of the store or the mask_bytes of the masks is skipped
// rather than read out of bounds (the host never builds one).
__global__ __launch_bounds__(256) void sample_views_table_kernel(const uint16_t* __restrict__ feat, int64_t n_rows, const uint8_t* __restrict__ mask,
                                                                 int64_t mask_bytes, const int64_t* __restrict__ table, int max_hw, int channels, int samples,
                                                                 uint64_t seed, uint64_t first_view_id, int view_index_base,
                                                                 uint16_t* __restrict__ out_feat, float* __restrict__ out_px,
                                                                 int32_t* __restrict__ out_view, int32_t* __restrict__ out_pix) {
  __shared__ uint16_t pref[SAMPLE_MAX_HW];
  __shared__ int part[256];
  const int v = blockIdx.x;
  const int64_t row = table[v * 4 + 0], mh = table[v * 4 + 1], mw = table[v * 4 + 2], moff = table[v * 4 + 3];
  // (uniform over the workgroup: no barrier is skipped by part of it)
  if (row < 0 || mh <= 0 || mw <= 0 || mh * mw > max_hw || row + mh * mw > n_rows) return;
  if (mask && moff >= 0 && moff + mh * mw > mask_bytes) return;
  const int hw = (int)(mh * mw);
  sample_one_view(pref, part, feat + (size_t)row * channels, (mask && moff >= 0) ? mask + moff : nullptr, hw, (int)mw, channels, samples, seed,
                  first_view_id, v, view_index_base, out_feat, out_px, out_view, out_pix);
}

}  // namespace acez

using namespace acez;

extern "C" int acez_buffer_warp_views(const float* d_images, int n_images, int H, int W, const int32_t* d_image_index, const float* d_theta,
                                      const float* d_jitter, int n_views, int hs, int ws, float* d_out_views, uint8_t* d_out_mask, int map_h,
                                      int map_w, float* d_scratch, void* stream) {
  ACEZ_REQUIRE(d_images && d_image_index && d_theta && d_out_views, "null pointer");
  ACEZ_REQUIRE(n_images > 0 && H > 0 && W > 0 && n_views > 0 && hs > 0 && ws > 0, "bad shape");
  ACEZ_REQUIRE(!d_jitter || d_scratch, "jitter needs the per-view scratch");
  ACEZ_REQUIRE(!d_out_mask || (map_h > 0 && map_w > 0), "bad mask shape");
  if (int rc = acez::require_device("the view warp runs on a gfx950 GPU")) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (d_jitter) hipLaunchKernelGGL(warp_mean_kernel, dim3(n_views), dim3(1024), 0, s, d_images, d_image_index, d_jitter, H * W, d_scratch);
  hipLaunchKernelGGL(warp_views_kernel, dim3((hs * ws + 255) / 256, n_views), dim3(256), 0, s, d_images, d_image_index, d_theta, d_jitter, d_scratch, H, W,
                     hs, ws, d_out_views);
  if (d_out_mask)
    hipLaunchKernelGGL(warp_mask_kernel, dim3((map_h * map_w + 255) / 256, n_views), dim3(256), 0, s, d_theta, H, W, hs, ws, map_h, map_w, d_out_mask);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_buffer_sample_views(const void* d_view_features, const uint8_t* d_masks, int n_views, int map_h, int map_w, int channels,
                                        int samples_per_view, uint64_t seed, uint64_t first_view_id, int32_t view_index_base,
                                        void* d_out_features, float* d_out_target_px, int32_t* d_out_view_idx, int32_t* d_out_pixel,
                                        void* stream) {
  ACEZ_REQUIRE(d_view_features && d_out_features && d_out_target_px && d_out_view_idx, "null pointer");
  ACEZ_REQUIRE(n_views > 0 && map_h > 0 && map_w > 0 && samples_per_view > 0, "bad shape");
  ACEZ_REQUIRE(map_h * map_w <= SAMPLE_MAX_HW, "feature map too large for the sampling kernel (24576 pixels)");
  ACEZ_REQUIRE(channels > 0 && channels % 8 == 0, "channels must be a multiple of 8");
  if (int rc = acez::require_device("buffer sampling runs on a gfx950 GPU")) return rc;
  const int hw = map_h * map_w;
  int split = (samples_per_view + 255) / 256;   // ~256 samples per workgroup
  if (split > 64) split = 64;
  hipLaunchKernelGGL(sample_views_kernel, dim3(n_views, split), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)d_view_features, d_masks, hw, map_w,
                     channels, samples_per_view, seed, first_view_id, (int)view_index_base, (uint16_t*)d_out_features, d_out_target_px,
                     d_out_view_idx, d_out_pixel);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_buffer_sample_views_table(const void* d_features, int64_t n_feature_rows, const uint8_t* d_masks, int64_t mask_bytes,
                                              const int64_t* d_view_table, int n_views, int max_hw, int channels, int samples_per_view, uint64_t seed, uint64_t first_view_id,
                                              int32_t view_index_base, void* d_out_features, float* d_out_target_px,
                                              int32_t* d_out_view_idx, int32_t* d_out_pixel, void* stream) {
  ACEZ_REQUIRE(d_features && d_view_table && d_out_features && d_out_target_px && d_out_view_idx, "null pointer");
  ACEZ_REQUIRE(n_views > 0 && max_hw > 0 && samples_per_view > 0 && n_feature_rows > 0, "bad shape");
  ACEZ_REQUIRE(!d_masks || mask_bytes > 0, "mask_bytes must give the size of d_masks");
  ACEZ_REQUIRE(max_hw <= SAMPLE_MAX_HW, "feature map too large for the sampling kernel (24576 pixels)");
  ACEZ_REQUIRE(channels > 0 && channels % 8 == 0, "channels must be a multiple of 8");
  if (int rc = acez::require_device("buffer sampling runs on a gfx950 GPU")) return rc;
  int split = (samples_per_view + 255) / 256;   // as acez_buffer_sample_views: ~256 samples per workgroup
  if (split > 64) split = 64;
  hipLaunchKernelGGL(sample_views_table_kernel, dim3(n_views, split), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)d_features, n_feature_rows,
                     d_masks, mask_bytes, d_view_table, max_hw, channels, samples_per_view, seed, first_view_id, (int)view_index_base, (uint16_t*)d_out_features,
                     d_out_target_px, d_out_view_idx, d_out_pixel);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
