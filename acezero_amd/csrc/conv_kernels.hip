// conv_kernels.hip -- the encoder's convolution kernels and their launchers (conv_launch.h; head_api.hip links against launch_convgemm too).
//
// Data layout: activations NHWC 16-bit ([frame][y][x][channel]; a pixel's channels are contiguous, so a pixel is a "row" of
// an implicit GEMM and the final [F*h*w][512] tensor is exactly the row layout of the training buffer / acez_head_forward).
// Weights: 16-bit [Co][Kp], k = (ky*3 + kx) * Ci + ci, Kp = K rounded up to 64 (zero padded).
// Every kernel is instantiated on the element trait of gemm_common.h: EltBf16 (v_mfma_f32_*_bf16) and EltF16 (v_mfma_f32_*_f16: the
// operand format the reference's autocast runs this network in, ace_trainer.py:366-367, register_mapping.py:209-210); fp32 accumulation,
// one rounding per layer output in both.
//
//   conv1 + conv2           conv12p_kernel: both layers in one launch, the conv1 map never leaves LDS
//   3 x 3, stride 1         conv3x3r_kernel (conv3x3r.h): 256 x 256 tiles, the input kept as an LDS patch (85 % of the encoder's FLOPs)
//   every other layer       implicit GEMM Out[p][co] = act(sum_k In[pix(p, tap(k))][ci(k)] * W[co][k] + b): convgemm512_kernel
//                           (256 x 256 tiles), convgemm256_kernel (256 x 128), convgemm_kernel (80-row x NT-column tiles, 4 multiplier
//                           waves + 4 loader waves, same structure as rowgemm80 in head_kernels.hip), chosen by size. 4-slot LDS-DMA
//                           ring of 64-wide K stages. The im2col never exists in memory: a loader lane computes, per stage, the
//                           source address of its 16-byte chunk (8 input channels of one tap of one pixel) or points at a zero page
//                           for the padding border / K padding / rows past the end (Im2colRows, conv_tiles.h).
// What the tiled kernels share -- tile decode, im2col rows, epilogue -- is in conv_tiles.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "conv3x3r.h"
#include "conv_launch.h"
#include "conv_tiles.h"
#include "gemm_common.h"

namespace acez {

// ---------------------------------------------------------------------------------------------------
// conv12p: conv1 (1 -> 32, stride 1) and conv2 (32 -> 64, stride 2) fused, persistent over 4 x 32 output tiles of conv2 and
// software-pipelined across tiles. As separate kernels these two layers cost 27 % of the encoder's time for 5 % of its FLOPs:
// conv1's 32-channel map (19.7 MB per 480 x 640 frame) is written and read back, and conv2's 3 x 3 taps re-read it nine times from
// L2 into a GEMM that is only 64 columns wide. Here a workgroup keeps the conv1 patch of its tile in LDS:
//   1. image patch 11 x 67 (grey, fp32 as in memory, by LDS-DMA; rounded to 16 bits where conv1 gathers its taps);
//   2. conv1 on the matrix cores: 32-pixel fragments of the 9 x 65 patch, B = the 9 taps gathered from the image patch (K = 16),
//      A = conv1's weights (one register quad), bias + ReLU + 16-bit -> conv1 patch [2 column-parity planes][9][33][32 ch] in LDS
//      (zero outside the image: that is conv2's padding);
//   3. conv2: wave w owns output row w of the tile (32 pixels x 64 channels); its B fragments are read straight from the patch
//      (tap (ky, kx) of output x = plane kx & 1, column x + (kx >> 1): unit stride, swizzled 16-byte chunks), its A fragments (all
//      of conv2's 64 x 288 weights) live in 144 registers for the whole kernel;
//   4. bias + ReLU + 16-bit through a wave-private staging row, 4 KiB contiguous store per output row.
// The two layers of DIFFERENT tiles run beside each other: waves 4 .. 7 compute conv1 of tile i + 1 into one of two LDS patches while
// waves 0 .. TR-1 run conv2 of tile i from the other (and stage the image patch of tile i + 2); waves w and w + 4 share a SIMD, so every
// SIMD has one MFMA-bound and one VALU-bound wave. One s_barrier per tile. (Round 1's phase-by-phase kernel on 8 x 32 tiles -- 7.1 us per
// tile for 1.1 us of MFMA time, 545 us per 64 frames against 352 -- is in the git history; this kernel's output is bit-identical to it.)
// ---------------------------------------------------------------------------------------------------
constexpr int C12_IMG_PITCH = 68;

// 16-byte chunk swizzle of conv12p's conv1 patch (a pixel = 32 channels = four chunks; q = column index inside a parity plane). conv2's
// B-fragment reads take 16 consecutive q with one chunk index: conflict free iff the swizzle differs between q, q + 4, q + 8, q + 12;
// conv1's epilogue writes 8 consecutive pixels = 4 consecutive q x 2 planes per lane group: conflict poor iff it also differs between
// q .. q + 3. (q >> 2) & 3 (round 1) does the first only -- the writes were 4-way conflicts, 180 of the kernel's 573 us (ablation, round
// 5); ((q >> 2) + q) & 3 does both.
__device__ __forceinline__ int c12p_swz(int q) { return ((q >> 2) + q) & 3; }

template <class E, int TR>
__global__ __launch_bounds__(512) void conv12p_kernel(Conv12Args a) {
  typedef typename E::frag frag;
  constexpr int PR = 2 * TR + 1;                 // conv1 patch rows
  constexpr int IMG_N = (PR + 2) * C12_IMG_PITCH;   // image patch: PR + 2 rows of 67 (+ 1 pad) grey values
  constexpr int PLANE = PR * 33 * 32;            // elements per column-parity plane of a conv1 patch
  constexpr int NF = (PR * 65 + 31) / 32;        // 32-pixel conv1 fragments per tile
  static_assert(IMG_N <= 3 * 256, "three image entries per staging thread");
  __shared__ __attribute__((aligned(16))) float s_img[2][3 * 256];   // fp32 as in memory (LDS-DMA); rounded to bf16 where conv1 gathers its taps
  __shared__ __attribute__((aligned(16))) uint16_t s_patch[2][2 * PLANE];
  __shared__ __attribute__((aligned(16))) uint16_t s_out[TR * 32 * 64];
  __shared__ __attribute__((aligned(16))) float s_bias[32 + 64];   // b1 | b2
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int fr = l & 31, fh = l >> 5;
  if (t < 96) s_bias[t] = t < 32 ? a.b1[t] : a.b2[t - 32];   // visible after the first barrier
  const int tiles_y = (a.H2 + TR - 1) / TR, tiles_x = (a.W2 + 31) / 32, tpf = tiles_y * tiles_x;
  const int n_tiles = a.F * tpf;
  const int K = ((int)blockIdx.x < n_tiles) ? (n_tiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;   // tiles of this workgroup
  auto tile_of = [&](int k) { return (int)blockIdx.x + k * (int)gridDim.x; };

  if (w < 4) {
    // ------------------------------------------------------------------ conv2 waves (w < TR multiply; all four stage the image patches)
    frag a2[9][2][2];
    if (w < TR) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            a2[tap][kk][i] = *reinterpret_cast<const frag*>(a.w2 + (size_t)(i * 32 + fr) * a.Kp2 + tap * 32 + kk * 16 + 8 * fh);
    }
    // image patch staging by LDS-DMA, one dword per lane: entries t, t + 256, t + 512 of the [PR + 2][68] patch (coordinates are tile
    // independent); outside the image (and past the patch) the source is a zero word. No registers, no conversion here, and the
    // transfers are OLDER than this iteration's output stores, so a counted wait certifies them without draining the stores.
    int epy[3], epx[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = t + 256 * i;
      epy[i] = min(e, IMG_N - 1) / C12_IMG_PITCH;
      epx[i] = (e < IMG_N) ? e - epy[i] * C12_IMG_PITCH : 67;   // 67 = the pad column: never valid
    }
    auto stage_img = [&](int k) {   // tile k of this workgroup -> s_img[k & 1]
      const int tl = tile_of(k);
      const int f = tl / tpf, r = tl - f * tpf;
      const int ty = r / tiles_x, tx = r - ty * tiles_x;
      const float* base = a.img + (size_t)f * a.H * a.W;
      float* dst = s_img[k & 1] + w * 64;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int iy = 2 * TR * ty - 2 + epy[i], ix = 64 * tx - 2 + epx[i];
        const bool ok = epx[i] < 67 && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const float* g = ok ? base + (size_t)iy * a.W + ix : a.zero;
        __builtin_amdgcn_global_load_lds((gvoid_t*)g, (lvoid_t*)(dst + 256 * i), 4, 0, 0);
      }
    };
    if (0 < K) stage_img(0);
    for (int j = -2; j < K; ++j) {
      // ---- image patch of tile j + 2 -> s_img[j & 1] (read by conv1 of tile j, one iteration ago); tile 0's went out above
      int n_stores = 0;
      if (j + 2 < K && j + 2 > 0) stage_img(j + 2);
      // ---- conv2 of tile j: output row w, pixels x = fr, channels 2 x 32
      if (j >= 0 && w < TR) {
        const int tile = tile_of(j);
        const int f = tile / tpf, r = tile - f * tpf;
        const int ty = r / tiles_x, tx = r - ty * tiles_x;
        const uint16_t* sp = s_patch[j & 1];
        f32x16 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int q = fr + (kx >> 1);
            const uint16_t* src = sp + (kx & 1) * PLANE + ((2 * w + ky) * 33 + q) * 32;
            const int sw = c12p_swz(q);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
              const frag b = *reinterpret_cast<const frag*>(src + (((kk * 2 + fh) ^ sw) << 3));
#pragma unroll
              for (int i = 0; i < 2; ++i) acc[i] = E::mfma32(a2[ky * 3 + kx][kk][i], b, acc[i]);
            }
          }
        // bias + ReLU -> wave-private staging row [32 px][64 ch] -> 4 KiB contiguous store
        uint16_t* so = s_out + w * (32 * 64);
        float4 b2v[2][4];   // (all eight LDS reads in flight before the first is used: as eight read-wait pairs they were eight serial round trips per tile)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int g = 0; g < 4; ++g) b2v[i][g] = *reinterpret_cast<const float4*>(s_bias + 32 + i * 32 + 8 * g + 4 * fh);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int ch = i * 32 + 8 * g + 4 * fh;
            const float4 b = b2v[i][g];
            const uint2 y = E::pk4(fmaxf(acc[i][4 * g + 0] + b.x, 0.f), fmaxf(acc[i][4 * g + 1] + b.y, 0.f), fmaxf(acc[i][4 * g + 2] + b.z, 0.f),
                                  fmaxf(acc[i][4 * g + 3] + b.w, 0.f));
            *reinterpret_cast<uint2*>(so + fr * 64 + ((((ch >> 3) ^ (fr & 7)) << 3) | (ch & 7))) = y;
          }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int oy = TR * ty + w, ox0 = 32 * tx;
        if (oy < a.H2) {
          n_stores = min(4, max(0, (a.W2 - ox0 + 7) >> 3));   // store instructions with at least one active lane (the others are branched over)
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            const int pxl = it * 8 + (l >> 3), chk = l & 7;
            const int ox = ox0 + pxl;
            if (ox < a.W2)
              *reinterpret_cast<uint4*>(a.out + (((size_t)f * a.H2 + oy) * a.W2 + ox) * 64 + chk * 8) =
                  *reinterpret_cast<const uint4*>(so + pxl * 64 + ((chk ^ (pxl & 7)) << 3));
          }
        }
      }
      // the image patch requested at the top of this iteration must have landed before conv1 reads it in the next one; it is older than
      // this tile's output stores, which may stay in flight (in-order completion). Raw barrier: __syncthreads() would drain them.
      wait_vmcnt_dyn(n_stores);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  } else {
    // ------------------------------------------------------------------ conv1 waves: tile j + 1 while the others run conv2 of tile j
    const int lw = w - 4;
    const frag a1 = *reinterpret_cast<const frag*>(a.w1 + fr * 16 + 8 * fh);
    // this lane's sixteen conv1 bias values, in registers for the whole kernel (read from LDS inside the fragment loop each of the four
    // reads was followed by a full lgkmcnt(0) wait: four serial LDS round trips per 32-pixel fragment -- found in the ISA, round 5)
    float4 b1v[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) b1v[g] = *reinterpret_cast<const float4*>(a.b1 + 8 * g + 4 * fh);
    // per-lane constants of this wave's fragments fg = lw, lw + 4, ... (tile independent): patch pixel p = fg * 32 + fr -> (py, px), the
    // offset of its taps in the image patch and of its 64-byte record in the conv1 patch (the division by 65 and the address arithmetic
    // ran once per fragment and tile)
    constexpr int NFW = (NF + 3) / 4;
    int f_py[NFW], f_px[NFW], f_ip[NFW], f_dst[NFW], f_sw[NFW];
#pragma unroll
    for (int u = 0; u < NFW; ++u) {
      const int p = (lw + 4 * u) * 32 + fr;
      const int py = min(p / 65, PR - 1), px = p - (p / 65) * 65, q = px >> 1;
      f_py[u] = (lw + 4 * u < NF && p < PR * 65) ? py : -1;   // -1: no such pixel (nothing is written)
      f_px[u] = px;
      f_ip[u] = py * C12_IMG_PITCH + px;
      f_dst[u] = (px & 1) * PLANE + (py * 33 + q) * 32 + 4 * fh;
      f_sw[u] = c12p_swz(q);
    }
    for (int j = -2; j < K; ++j) {
      const int c = j + 1;
      if (c >= 0 && c < K) {
        const int tile = tile_of(c);
        const int f = tile / tpf, r = tile - f * tpf;
        const int ty = r / tiles_x, tx = r - ty * tiles_x;
        (void)f;
        const float* si = s_img[c & 1];
        uint16_t* sp = s_patch[c & 1];
        const int cy0 = 2 * TR * ty - 1, cx0 = 64 * tx - 1;          // conv1 pixel of patch position (0, 0)
        // a tile whose whole patch lies inside the image (all but the border tiles) needs no zeroing of outside pixels
        const bool interior = cy0 >= 0 && cy0 + PR <= a.H && cx0 >= 0 && cx0 + 65 <= a.W;
        auto fragment = [&](int u, auto chk) {
          constexpr bool CHECK = decltype(chk)::value;
          const float* ip = si + f_ip[u];   // taps: ip[ky * 68 + kx], rounded to 16 bits here (round to nearest even)
          float tp[9];
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) tp[ky * 3 + kx] = ip[ky * C12_IMG_PITCH + kx];
          uint32_t bw[4];
          if (fh == 0) {
            bw[0] = E::pk2(tp[0], tp[1]); bw[1] = E::pk2(tp[2], tp[3]); bw[2] = E::pk2(tp[4], tp[5]); bw[3] = E::pk2(tp[6], tp[7]);
          } else {
            bw[0] = E::pk2(tp[8], 0.f); bw[1] = 0u; bw[2] = 0u; bw[3] = 0u;
          }
          const uint4 bq = make_uint4(bw[0], bw[1], bw[2], bw[3]);
          f32x16 c1;
#pragma unroll
          for (int q = 0; q < 16; ++q) c1[q] = 0.f;
          c1 = E::mfma32(a1, __builtin_bit_cast(frag, bq), c1);
          // conv1 pixel (cy, cx) of this lane; outside the image the map is ZERO (conv2's padding)
          bool inside = true;
          if (CHECK) {
            const int cy = cy0 + f_py[u], cx = cx0 + f_px[u];
            inside = cy >= 0 && cy < a.H && cx >= 0 && cx < a.W;
          }
          if (f_py[u] >= 0) {
            uint16_t* dst = sp + f_dst[u];
#pragma unroll
            for (int g = 0; g < 4; ++g) {   // channels 8g + 4 fh .. +3 = half of logical chunk g
              const float4 b = b1v[g];
              float v0 = fmaxf(c1[4 * g + 0] + b.x, 0.f), v1 = fmaxf(c1[4 * g + 1] + b.y, 0.f);
              float v2 = fmaxf(c1[4 * g + 2] + b.z, 0.f), v3 = fmaxf(c1[4 * g + 3] + b.w, 0.f);
              if (CHECK && !inside) v0 = v1 = v2 = v3 = 0.f;
              *reinterpret_cast<uint2*>(dst + ((g ^ f_sw[u]) << 3)) = E::pk4(v0, v1, v2, v3);
            }
          }
        };
        if (interior) {
#pragma unroll
          for (int u = 0; u < NFW; ++u)
            if (lw + 4 * u < NF) fragment(u, std::integral_constant<bool, false>{});
        } else {
#pragma unroll
          for (int u = 0; u < NFW; ++u)
            if (lw + 4 * u < NF) fragment(u, std::integral_constant<bool, true>{});
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }
}

template <class E, int NT, bool RELU, bool HAS_ADD>
__global__ __launch_bounds__(512) void convgemm_kernel(ConvGemmArgs a) {
  typedef typename E::frag frag;
  static_assert(NT == 64 || NT == 128, "column tile");
  static_assert(!(HAS_ADD && NT == 64), "the residual epilogue exists for 128-column tiles only");
  constexpr int CF = NT / 64;                 // 16-column fragments per multiplier wave
  constexpr int WI = NT / 32;                 // W DMA instructions per loader and stage (8 rows each)
  constexpr int IPS = WI + 3;                 // DMA instructions per loader and stage
  constexpr int STAGE = (NT + 96) * 64;       // elements per ring slot
  __shared__ __attribute__((aligned(16))) uint16_t smem[4 * STAGE + 80 * NT];
  uint16_t* const stO = smem + 4 * STAGE;     // `add` in / output tile
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int M = a.M, Kp = a.Kp;
  int mt, n0, m0;
  if (!tile_decode<80, NT>(M, a.Co, mt, n0, m0)) return;
  const int KT = Kp >> 6;

  if (w >= 4) {
    // ------------------------------------------------------------------ loader waves
    const int lw = w - 4;
    if (HAS_ADD) {
      // residual / skip tile -> staging (oldest DMA of this wave: complete before any stage it could be confused with)
#pragma unroll
      for (int j = 0; j < 5; ++j) residual_dma<128>(a, stO, lw * 5 + j, m0, n0, l);
    }
    const uint16_t* gW[WI];
#pragma unroll
    for (int j = 0; j < WI; ++j) {
      const int row = (lw * WI + j) * 8 + (l >> 3);
      gW[j] = a.W + (size_t)(n0 + row) * Kp + stage_chunk<64>(row, l & 7) * 8;
    }
    Im2colRows<3, 64> in;   // this lane's three rows of the In tile (the four loaders cover 96 rows: those past the tile's 80 read zeros)
    in.init(a, m0, min(M, m0 + 80), lw, l);
    auto issue = [&](int kt) {
      uint16_t* slot = smem + (kt & 3) * STAGE;
#pragma unroll
      for (int j = 0; j < WI; ++j)
        __builtin_amdgcn_global_load_lds((gvoid_t*)(gW[j] + kt * 64), (lvoid_t*)(slot + (lw * WI + j) * 8 * 64), 16, 0, 0);
#pragma unroll
      for (int j = 0; j < 3; ++j)
        __builtin_amdgcn_global_load_lds((gvoid_t*)in.src(a, j, kt * 64), (lvoid_t*)(slot + NT * 64 + (lw * 3 + j) * 8 * 64), 16, 0, 0);
    };
    for (int kt = 0; kt < 4 && kt < KT; ++kt) issue(kt);
    for (int kt = 0; kt < KT; ++kt) {
      // stages issued so far: 0..3 at kt = 0, 0..kt+2 afterwards (in-order completion)
      const int later = (kt == 0) ? min(3, KT - 1) : min(2, KT - 1 - kt);
      if (later >= 3) ACEZ_VMCNT_C(3 * IPS);
      else if (later == 2) ACEZ_VMCNT_C(2 * IPS);
      else if (later == 1) ACEZ_VMCNT_C(IPS);
      else ACEZ_VMCNT(0);
      __builtin_amdgcn_s_barrier();   // stage kt has landed; the multipliers are done with stage kt - 1
      if (kt >= 1 && kt + 3 < KT) issue(kt + 3);
    }
    __builtin_amdgcn_s_barrier();     // the multipliers have left the K loop (ring free)
    __builtin_amdgcn_s_barrier();     // ... and have written the output tile
  } else {
    // ------------------------------------------------------------------ multiplier waves
    f32x4 acc[CF][5];
#pragma unroll
    for (int i = 0; i < CF; ++i)
#pragma unroll
      for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
    const int fr = l & 15, fq = l >> 4;
    float4 bias[CF];
#pragma unroll
    for (int i = 0; i < CF; ++i) bias[i] = *reinterpret_cast<const float4*>(a.bias + n0 + w * (NT / 4) + i * 16 + 4 * fq);
    for (int kt = 0; kt < KT; ++kt) {
      __builtin_amdgcn_s_barrier();
      const uint16_t* sW = smem + (kt & 3) * STAGE;
      const uint16_t* sI = sW + NT * 64;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int c = kk * 4 + fq;
        frag fa[CF], fb[5];
#pragma unroll
        for (int i = 0; i < CF; ++i) fa[i] = *reinterpret_cast<const frag*>(&sW[swz(w * (NT / 4) + i * 16 + fr, c)]);
#pragma unroll
        for (int j = 0; j < 5; ++j) fb[j] = *reinterpret_cast<const frag*>(&sI[swz(j * 16 + fr, c)]);
#pragma unroll
        for (int i = 0; i < CF; ++i)
#pragma unroll
          for (int j = 0; j < 5; ++j) acc[i][j] = E::mfma16(fa[i], fb[j], acc[i][j]);
      }
    }
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int ml = j * 16 + fr;
#pragma unroll
      for (int i = 0; i < CF; ++i) {
        const int nl = w * (NT / 4) + i * 16 + 4 * fq;
        epilogue_quad<E, RELU, HAS_ADD>(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3], bias[i], &stO[st_off_n<NT>(ml, nl)], a.round_before_add);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  // ------------------------------------------------------------------ all eight waves: copy the tile out, full rows
  constexpr int NQ = 80 * NT / 8;   // 16-byte chunks of the tile
#pragma unroll
  for (int it = 0; it < (NQ + 511) / 512; ++it)
    if (t + 512 * it < NQ) copy_out_chunk<NT>(a, stO, t + 512 * it, m0, n0);
}

// ---------------------------------------------------------------------------------------------------
// convgemm256: the large-M variant (encoder layers with >= 128 output channels, i.e. 97 % of its FLOPs). 256 rows x 128
// columns per workgroup halves the L2->LDS bytes per FLOP of the 80-row tile (the measured bound of that kernel at
// ~50-70 GB/s of LDS-DMA fill per CU). 16 waves: 8 multipliers (4 x 2 grid of 64 x 64 sub-tiles, 2 x 2
// v_mfma_f32_32x32x16_bf16 fragments: 4 ds_read_b128 feed 4 MFMAs) and 8 loaders (6 DMA instructions each per 64-wide
// K stage: 2 for the W tile, 4 for the In tile). 3-slot ring of 48 KiB stages; the slot rotation is chosen so that the
// LAST stage sits in slot 2, which leaves slots 0-1 free for the [256][128] epilogue tile one stage early: the loaders
// fetch the residual / skip tile into it while the multipliers work on the last stage.
// ---------------------------------------------------------------------------------------------------
template <class E, bool RELU, bool HAS_ADD>
__global__ __launch_bounds__(1024) void convgemm256_kernel(ConvGemmArgs a) {
  typedef typename E::frag frag;
  constexpr int STAGE = (128 + 256) * 64;     // elements per ring slot
  __shared__ __attribute__((aligned(16))) uint16_t smem[3 * STAGE];
  uint16_t* const stO = smem;                 // epilogue tile [256][128] (slots 0-1)
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int M = a.M, Kp = a.Kp;
  int mt, n0, m0;
  if (!tile_decode<256, 128>(M, a.Co, mt, n0, m0)) return;
  const int KT = Kp >> 6;
  const int rot = (3 - (KT % 3)) % 3;         // slot(kt) = (kt + rot) % 3 with slot(KT - 1) == 2

  if (w >= 8) {
    // ------------------------------------------------------------------ loader waves
    const int lw = w - 8;
    const uint16_t* gW[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = (lw * 2 + j) * 8 + (l >> 3);
      gW[j] = a.W + (size_t)(n0 + row) * Kp + stage_chunk<64>(row, l & 7) * 8;
    }
    Im2colRows<4, 64> in;
    in.init(a, m0, M, lw, l);
    auto issue = [&](int kt) {
      uint16_t* slot = smem + ((kt + rot) % 3) * STAGE;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        __builtin_amdgcn_global_load_lds((gvoid_t*)(gW[j] + kt * 64), (lvoid_t*)(slot + (lw * 2 + j) * 8 * 64), 16, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_global_load_lds((gvoid_t*)in.src(a, j, kt * 64), (lvoid_t*)(slot + 128 * 64 + (lw * 4 + j) * 8 * 64), 16, 0, 0);
    };
    for (int kt = 0; kt < 3 && kt < KT; ++kt) issue(kt);
    for (int kt = 0; kt < KT; ++kt) {
      // issued so far: 0..2 at kt = 0, 0..kt+1 afterwards; 6 DMA instructions per stage, in-order completion
      const int later = (kt == 0) ? min(2, KT - 1) : min(1, KT - 1 - kt);
      if (later >= 2) ACEZ_VMCNT(12);
      else if (later == 1) ACEZ_VMCNT(6);
      else ACEZ_VMCNT(0);
      __builtin_amdgcn_s_barrier();   // stage kt has landed; the multipliers are done with stage kt - 1
      if (kt >= 1 && kt + 2 < KT) issue(kt + 2);
      if (HAS_ADD && kt == KT - 1) {
        // slots 0-1 are free from here on (KT >= 3 for every layer that has a residual input): residual tile -> stO
#pragma unroll
        for (int j = 0; j < 8; ++j) residual_dma<128>(a, stO, lw * 8 + j, m0, n0, l);
      }
    }
    ACEZ_VMCNT(0);
    __builtin_amdgcn_s_barrier();     // K loop finished, residual tile landed
    __builtin_amdgcn_s_barrier();     // output tile written
  } else {
    // ------------------------------------------------------------------ multiplier waves
    const int wm = w >> 1, wn = w & 1;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int fr = l & 31, fh = l >> 5;
    for (int kt = 0; kt < KT; ++kt) {
      __builtin_amdgcn_s_barrier();
      const uint16_t* sW = smem + ((kt + rot) % 3) * STAGE;
      const uint16_t* sI = sW + 128 * 64;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int c = kk * 2 + fh;
        frag fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const frag*>(&sW[swz(wn * 64 + i * 32 + fr, c)]);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const frag*>(&sI[swz(wm * 64 + j * 32 + fr, c)]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = E::mfma32(fa[i], fb[j], acc[i][j]);
      }
    }
    __builtin_amdgcn_s_barrier();
    float4 bv[2][4];
    load_bias_quads(bv, a.bias + n0, wn, fh);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ml = wm * 64 + j * 32 + fr;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int nl = wn * 64 + i * 32 + 8 * q + 4 * fh;
          // epilogue_quad of conv_tiles.h written out on its own helpers, the staging address formed BEHIND the bias pass: with the address
          // as the helper's argument the <RELU, no add> form takes 110 registers instead of 109
          float v[4] = {acc[i][j][4 * q + 0], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
          bias_act<RELU>(v, bv[i][q]);
          uint16_t* po = &stO[st_off_n<128>(ml, nl)];
          if (HAS_ADD) {
            float ad[4];
            E::un4(*reinterpret_cast<const uint2*>(po), ad);
            if (a.round_before_add) round16<E>(v);
            v[0] += ad[0]; v[1] += ad[1]; v[2] += ad[2]; v[3] += ad[3];
          }
          *reinterpret_cast<uint2*>(po) = E::pk4(v[0], v[1], v[2], v[3]);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  // ------------------------------------------------------------------ all sixteen waves: copy the tile out, full rows
#pragma unroll
  for (int it = 0; it < 4; ++it) copy_out_chunk<128>(a, stO, t + 1024 * it, m0, n0);
}

// ---------------------------------------------------------------------------------------------------
// convgemm512: 256 rows x 256 columns per workgroup for the layers with >= 256 output channels when there are enough
// tiles to fill the chip several times. Why: every GEMM kernel of this package ends up with ~96 KiB of LDS-DMA in flight per
// CU (the ring is bounded by the 160 KiB LDS) and measures ~70-77 GB/s of fill per CU, i.e. ~1.3 us of latency under load
// (Little's law) -- loads-only and MFMA-only ablations of convgemm256 take the same time and ADD. The only lever left is
// FLOP per byte: 256 x 256 needs 1.5x fewer bytes per FLOP than 256 x 128 (131 FLOP/B: 75 GB/s per CU then feeds the full
// MFMA rate) and its 128 x 64 wave tiles need 0.75 KiB of fragment reads per MFMA instead of 1 KiB.
// 12 waves: 8 multipliers (2 x 4 grid of 128-row x 64-column sub-tiles = 2 x 4 fragments of v_mfma_f32_32x32x16_bf16,
// 128 accumulator registers) and 4 loaders (8 DMA instructions each per stage). K stages are 32 wide (32 KiB), 4-slot ring.
// The [256][256] bf16 epilogue tile needs the whole ring, so a residual input is fetched after the K loop.
// ---------------------------------------------------------------------------------------------------

template <class E, bool RELU, bool HAS_ADD>
__global__ __launch_bounds__(768) void convgemm512_kernel(ConvGemmArgs a) {
  typedef typename E::frag frag;
  constexpr int STAGE = 512 * 32;             // elements per ring slot: [W 256 x 32 | In 256 x 32]
  __shared__ __attribute__((aligned(16))) uint16_t smem[4 * STAGE];
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int M = a.M, Kp = a.Kp;
  const int KT = Kp >> 5;
  // One workgroup per tile. A PERSISTENT walk over the tiles (one workgroup per CU, the next tile's first stages requested as soon as the
  // output tile is out of LDS) was measured in round 5 (tools/conv_trace.py: a tile is 3.8 us to its first stage, 13.2 us of K loop, 1.6 us
  // of epilogue, 2.4 us until its stores are acknowledged = 21.1 us of a 26.7 us period): bit-identical and 9 % SLOWER (2.55 against 2.34 ms
  // for the head's eight layers) -- behind a tile's own 128 KiB of stores the next first stage lands after 6 us, and the hardware's
  // overlap of one workgroup's drain with the next one's start is better than the in-workgroup sequence.
  int mt, n0, m0;
  if (!tile_decode<256, 256>(M, a.Co, mt, n0, m0)) return;
#ifdef ACEZ_DIAG   // tools/conv_trace.py: stamp i of this tile (slot 4 + i for the first loader wave)
#define CG_STAMP(i) do { if (a.trace && (t == 0 || t == 512)) a.trace[((size_t)(mt * (a.Co >> 8) + (n0 >> 8))) * 8 + (t ? 4 : 0) + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define CG_STAMP(i) do { } while (0)
#endif
  CG_STAMP(0);

  if (w >= 8) {
    // ------------------------------------------------------------------ loader waves
    const int lw = w - 8;
    const int lrow = l >> 2, lch = l & 3;     // a DMA instruction covers 16 rows x 64 bytes
    const uint16_t* gW[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = (lw * 4 + j) * 16 + lrow;
      gW[j] = a.W + (size_t)(n0 + row) * Kp + stage_chunk<32>(row, lch) * 8;
    }
    Im2colRows<4, 32> in;
    in.init(a, m0, M, lw, l);
    auto issue = [&](int kt) {
      uint16_t* slot = smem + (kt & 3) * STAGE;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_global_load_lds((gvoid_t*)(gW[j] + kt * 32), (lvoid_t*)(slot + (lw * 4 + j) * 16 * 32), 16, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_global_load_lds((gvoid_t*)in.src(a, j, kt * 32), (lvoid_t*)(slot + 256 * 32 + (lw * 4 + j) * 16 * 32), 16, 0, 0);
    };
    for (int kt = 0; kt < 4 && kt < KT; ++kt) issue(kt);
    for (int kt = 0; kt < KT; ++kt) {
      const int later = (kt == 0) ? min(3, KT - 1) : min(2, KT - 1 - kt);
      if (later >= 3) ACEZ_VMCNT(24);
      else if (later == 2) ACEZ_VMCNT(16);
      else if (later == 1) ACEZ_VMCNT(8);
      else ACEZ_VMCNT(0);
      __builtin_amdgcn_s_barrier();   // stage kt has landed; the multipliers are done with stage kt - 1
      if (kt == 0) CG_STAMP(1);
      if (kt >= 1 && kt + 3 < KT) issue(kt + 3);
    }
    __builtin_amdgcn_s_barrier();     // the multipliers have left the K loop: the ring is free
    CG_STAMP(2);
    if (HAS_ADD) {
      // residual tile [256][256] -> ring space, 128 DMA instructions of 2 rows x 512 bytes (32 per loader)
      for (int j = 0; j < 32; ++j) residual_dma<256>(a, smem, lw * 32 + j, m0, n0, l);
      ACEZ_VMCNT(0);
      __builtin_amdgcn_s_barrier();   // residual tile landed
    }
    __builtin_amdgcn_s_barrier();     // output tile written
  } else {
    // ------------------------------------------------------------------ multiplier waves
    const int wm = w >> 2, wn = w & 3;
    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int fr = l & 31, fh = l >> 5;
    for (int kt = 0; kt < KT; ++kt) {
      __builtin_amdgcn_s_barrier();
      const uint16_t* sW = smem + (kt & 3) * STAGE;
      const uint16_t* sI = sW + 256 * 32;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int c = kk * 2 + fh;
        frag fa[2], fb[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const frag*>(&sW[swz32(wn * 64 + i * 32 + fr, c)]);
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const frag*>(&sI[swz32(wm * 128 + j * 32 + fr, c)]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = E::mfma32(fa[i], fb[j], acc[i][j]);
      }
    }
    __builtin_amdgcn_s_barrier();     // ring free
    CG_STAMP(1);
    if (HAS_ADD) __builtin_amdgcn_s_barrier();
    float4 bv[2][4];
    load_bias_quads(bv, a.bias + n0, wn, fh);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ml = wm * 128 + j * 32 + fr;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int nl = wn * 64 + i * 32 + 8 * q + 4 * fh;
          epilogue_quad<E, RELU, HAS_ADD>(acc[i][j][4 * q + 0], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3], bv[i][q], &smem[st_off_n<256>(ml, nl)],
                                          a.round_before_add);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  // ------------------------------------------------------------------ all twelve waves: copy the tile out, full 512-byte rows
  CG_STAMP(2 + (t ? 1 : 0));   // (multiplier slot 2 / loader slot 3: the epilogue tile is complete)
  for (int q = t; q < 256 * 32; q += 768) copy_out_chunk<256>(a, smem, q, m0, n0);
#ifdef ACEZ_DIAG
  if (a.trace && t == 0) { ACEZ_VMCNT(0); CG_STAMP(3); }   // this wave's stores acknowledged
#endif
}

#ifdef ACEZ_DIAG
static unsigned long long* g_conv_trace = nullptr;
extern "C" void diagz_conv_trace(void* buf) { g_conv_trace = static_cast<unsigned long long*>(buf); }   // tools/conv_trace.py (not an acez_ symbol: the two builds export the same C ABI)
#endif
// the kernel instantiation of the context's 16-bit operand format (ConvGemmArgs::f16)
#define ACEZ_CONV_LAUNCH(kern, grid, blk, ...)                                                    \
  do {                                                                                            \
    if (g.f16) hipLaunchKernelGGL((kern<EltF16, __VA_ARGS__>), grid, blk, 0, s, g);               \
    else hipLaunchKernelGGL((kern<EltBf16, __VA_ARGS__>), grid, blk, 0, s, g);                    \
  } while (0)
// the three epilogue forms of an implicit-GEMM kernel: launch(RELU, HAS_ADD) for residual add (always with ReLU) / ReLU / plain
template <class F>
static void launch_form(const ConvGemmArgs& g, bool relu, F&& launch) {
  using T = std::true_type;
  using Fl = std::false_type;
  if (g.add) {
    if (!relu) abort();
    launch(T{}, T{});
  } else if (relu) {
    launch(T{}, Fl{});
  } else {
    launch(Fl{}, Fl{});
  }
}
// tile_mode: 0 = choose by size; 3 / 512 / 256 / 80 = force conv3x3r / convgemm512 / convgemm256 / the 80-row kernel where the layer shape
// allows it (ACEZ_CONV_TILE, tests)
void launch_convgemm(const ConvGemmArgs& g_in, bool relu, hipStream_t s, int tile_mode) {
  ConvGemmArgs g = g_in;
#ifdef ACEZ_DIAG
  g.trace = g_conv_trace;
#endif
  const bool patch_ok = g.ksize == 3 && g.stride == 1 && g.pad == 1 && g.Hi == g.Ho && g.Wi == g.Wo && g.Wi <= (P3_ROWS - 258) / 2 &&
                        g.Ci % 32 == 0 && g.Co % 256 == 0 && g.K == g.Kp;
  // the patch kernel pays from one tile per CU on (16 frames of 480x640 at Co = 256: 0.0925 -> 0.0775 ms per frame against the
  // 80-row / 256 x 128 kernels; 32 frames: 0.0715 -> 0.067); round 1's conv3x3p needed four waves of tiles to win
  const bool use_patch = patch_ok && (tile_mode == 3 || (tile_mode == 0 && (int64_t)((g.M + 255) / 256) * (g.Co / 256) >= 256));
  if (g.W2 && !g.In2) {
    // a pointwise Co -> Co layer behind this one (res1_conv1 + res1_conv2): back to back on conv3x3r's finished tile where the layer runs
    // there and one tile holds a whole output row; else two launches through the scratch map
    if (use_patch && g.Co == 256 && g.Kp2 >= 256 && relu && !g.add) {
      // (launched below with the other conv3x3r forms)
    } else {
      if (!g.skip_scratch || g.add) abort();
      ConvGemmArgs k = g;
      k.W2 = nullptr; k.bias2 = nullptr; k.out = g.skip_scratch;
      launch_convgemm(k, relu, s, tile_mode);
      ConvGemmArgs p = g;
      p.In = g.skip_scratch; p.W = g.W2; p.bias = g.bias2; p.W2 = nullptr; p.bias2 = nullptr;
      p.Hi = g.Ho; p.Wi = g.Wo; p.Ci = g.Co; p.ci_shift = __builtin_ctz(g.Co); p.ksize = 1; p.stride = 1; p.pad = 0; p.K = g.Co; p.Kp = g.Kp2;
      launch_convgemm(p, true, s, tile_mode);
      return;
    }
  }
  if (g.In2 && !(use_patch && g.Ci >= 64 && g.Ci2 % 128 == 0 && g.Kp2 >= g.Ci2 && relu)) {
    // the unfused form: the pointwise skip as its own launch into the scratch map, added by the main layer's epilogue
    if (!g.skip_scratch || g.add) abort();
    ConvGemmArgs k = g;
    k.In = g.In2; k.W = g.W2; k.bias = g.bias2; k.add = nullptr; k.out = g.skip_scratch; k.In2 = nullptr; k.W2 = nullptr; k.bias2 = nullptr;
    k.Hi = g.Ho; k.Wi = g.Wo; k.Ci = g.Ci2; k.ci_shift = __builtin_ctz(g.Ci2); k.ksize = 1; k.stride = 1; k.pad = 0; k.K = g.Ci2; k.Kp = g.Kp2;
    launch_convgemm(k, false, s, tile_mode);
    g.add = g.skip_scratch; g.In2 = nullptr; g.W2 = nullptr; g.bias2 = nullptr;
  }
  if (use_patch) {
    const dim3 grid = tile_grid(g.M, g.Co, 256, 256), blkq(512);
    if (!relu) abort();
    if (g.In2) ACEZ_CONV_LAUNCH(conv3x3r_kernel, grid, blkq, true, false, true);
    else if (g.W2) ACEZ_CONV_LAUNCH(conv3x3r_kernel, grid, blkq, true, false, false, true);
    else if (g.add) ACEZ_CONV_LAUNCH(conv3x3r_kernel, grid, blkq, true, true);
    else ACEZ_CONV_LAUNCH(conv3x3r_kernel, grid, blkq, true, false);
    return;
  }
  const bool huge_ok = g.Co % 256 == 0 && g.Kp >= 256;
  if (huge_ok && (tile_mode == 512 || (tile_mode == 0 && (int64_t)((g.M + 255) / 256) * (g.Co / 256) >= 4 * 256))) {
    const dim3 grid = tile_grid(g.M, g.Co, 256, 256), blk(768);
    launch_form(g, relu, [&](auto r, auto ad) { ACEZ_CONV_LAUNCH(convgemm512_kernel, grid, blk, decltype(r)::value, decltype(ad)::value); });
    return;
  }
  const bool big_ok = g.Co % 128 == 0 && g.Kp >= 192;
  if (big_ok && (tile_mode == 256 || (tile_mode == 0 && g.M >= 256 * 128))) {
    // enough rows to fill the chip with 256-row tiles
    const dim3 grid = tile_grid(g.M, g.Co, 256, 128), blk(1024);
    launch_form(g, relu, [&](auto r, auto ad) { ACEZ_CONV_LAUNCH(convgemm256_kernel, grid, blk, decltype(r)::value, decltype(ad)::value); });
    return;
  }
  const int nt = (g.Co % 128 == 0) ? 128 : 64;
  const dim3 grid = tile_grid(g.M, g.Co, 80, nt), blk(512);
  if (nt == 64) {
    if (g.add || !relu) abort();
    ACEZ_CONV_LAUNCH(convgemm_kernel, grid, blk, 64, true, false);
  } else {
    launch_form(g, relu, [&](auto r, auto ad) { ACEZ_CONV_LAUNCH(convgemm_kernel, grid, blk, 128, decltype(r)::value, decltype(ad)::value); });
  }
}

// conv1 + conv2 in one launch, software-pipelined over 4 x 32 output tiles (conv1 of tile i + 1 beside conv2 of tile i)
void launch_conv12p(const Conv12Args& c, bool f16, hipStream_t s) {
  const int nt4 = c.F * ((c.H2 + 3) / 4) * c.tiles_x;
  const dim3 grid(nt4 < 256 ? nt4 : 256), blk(512);
  if (f16) hipLaunchKernelGGL((conv12p_kernel<EltF16, 4>), grid, blk, 0, s, c);
  else hipLaunchKernelGGL((conv12p_kernel<EltBf16, 4>), grid, blk, 0, s, c);
}

}  // namespace acez
