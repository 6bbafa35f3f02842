// conv_tiles.h -- the pieces the tiled convolution kernels share (conv_kernels.hip, conv3x3r.h), each written once: workgroup -> tile
// decode and its host twin, the im2col row set of the implicit-GEMM loaders, and the epilogue (bias pre-load, bias / ReLU / rounding /
// residual add into the 16-bit staging tile, residual-tile DMA, row-wise copy-out). Loop shapes (how many DMA instructions or output
// chunks a wave walks, unrolled or not) depend on a kernel's wave count and stay with the kernel; what one step does is here.
#pragma once
#include "conv_launch.h"
#include "gemm_common.h"

namespace acez {

// ---- workgroup -> tile of TM rows x TN columns (TN a power of two). blockIdx.x & 7 is the XCD the workgroup lands on: the column tiles
// of a row tile share an XCD (and its L2). False: a padding workgroup of the last round (the grid is a multiple of 8 row-tile groups).
template <int TM, int TN>
__device__ __forceinline__ bool tile_decode(int M, int Co, int& mt, int& n0, int& m0) {
  static_assert((TN & (TN - 1)) == 0, "column tile");
  const int ntiles = Co >> __builtin_ctz(TN);
  const int mtiles = (TM & (TM - 1)) == 0 ? (M + TM - 1) >> __builtin_ctz(TM) : (M + TM - 1) / TM;
  const int per_xcd = (mtiles + 7) >> 3;
  const int jx = blockIdx.x >> 3;
  mt = (blockIdx.x & 7) * per_xcd + jx / ntiles;
  if (mt >= mtiles) return false;
  n0 = (jx % ntiles) * TN;
  m0 = mt * TM;
  return true;
}
inline dim3 tile_grid(int M, int Co, int TM, int TN) {   // the grid tile_decode<TM, TN> expects
  const int ntiles = Co / TN, mtiles = (M + TM - 1) / TM;
  return dim3(8 * ntiles * ((mtiles + 7) / 8));
}

// 16-byte chunk swizzle of a [row][KW] K-stage tile (swz / swz32 of the fragment reads), applied to the per-lane SOURCE chunk of the LDS-DMA
template <int KW>
__device__ __forceinline__ int stage_chunk(int row, int chunk) {
  static_assert(KW == 64 || KW == 32, "stage width");
  return KW == 64 ? chunk ^ ((row >> 1) & 7) : chunk ^ ((row >> 2) & 3);
}

// ---- the im2col row set of a loader lane: R rows of the In tile, K stages KW wide. A DMA instruction covers 64 / (KW / 8) rows (8 rows
// of 128 bytes or 16 rows of 64 bytes); instruction j of loader wave lw brings rows (lw * R + j) * RPI .. + RPI - 1. init() maps this
// lane's rows (output pixels) to the top-left input pixel of their receptive fields; src() gives, per stage, the source of the lane's
// 16-byte chunk (8 input channels of one tap of one pixel) or the zero page for the padding border / K padding / rows at or past m_end.
template <int R, int KW>
struct Im2colRows {
  static constexpr int CPR = KW / 8, RPI = 64 / CPR;
  const uint16_t* ibase[R];
  const uint16_t* zp;
  int iy0[R], ix0[R], kc[R];
  bool pv[R];
  __device__ __forceinline__ void init(const ConvGemmArgs& a, int m0, int m_end, int lw, int l) {
    const int hw = a.Ho * a.Wo;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int row = (lw * R + j) * RPI + (l >> __builtin_ctz(CPR));
      const int p = m0 + row;
      pv[j] = p < m_end;
      const int pp = pv[j] ? p : 0;
      const int f = pp / hw, r = pp - f * hw;
      const int y = r / a.Wo, x = r - y * a.Wo;
      iy0[j] = y * a.stride - a.pad;
      ix0[j] = x * a.stride - a.pad;
      ibase[j] = a.In + (size_t)f * a.Hi * a.Wi * a.Ci;
      kc[j] = stage_chunk<KW>(row, l & (CPR - 1)) * 8;   // logical K offset of this lane's chunk inside a stage
    }
    zp = a.zeros + (l & (CPR - 1)) * 8;
  }
  __device__ __forceinline__ const uint16_t* src(const ConvGemmArgs& a, int j, int kbase) const {   // kbase = first k of the stage
    const int k0 = kbase + kc[j];
    const int tap = k0 >> a.ci_shift, ci = k0 & (a.Ci - 1);
    const int ky = (a.ksize == 3) ? (tap * 11) >> 5 : 0;   // tap / 3 for tap < 12
    const int kx = tap - 3 * ky;
    const int iy = iy0[j] + ky, ix = ix0[j] + kx;
    const bool ok = pv[j] && k0 < a.K && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
    return ok ? ibase[j] + (((size_t)iy * a.Wi + ix) << a.ci_shift) + ci : zp;
  }
};

// ---- epilogue. [rows][NT] 16-bit staging tile, NT = 64 / 128 / 256: chunk index XOR row & (NT / 8 - 1) (conflict-free for the
// accumulator layout and for the row-wise copy; st_off of gemm_common.h is the NT = 128 case)
template <int NT>
__device__ __forceinline__ int st_off_n(int row, int col) { return row * NT + ((((col >> 3) ^ (row & (NT / 8 - 1))) << 3) | (col & 7)); }

// bias (+ ReLU) on four accumulator values / their rounding to the 16-bit format and back
template <bool RELU>
__device__ __forceinline__ void bias_act(float (&v)[4], const float4 b) {
  v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  if (RELU) {
    v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
  }
}
template <class E>
__device__ __forceinline__ void round16(float (&v)[4]) { E::un4(E::pk4(v[0], v[1], v[2], v[3]), v); }

// four accumulator values -> staging tile at po. HAS_ADD: po holds the residual quad (residual_dma below); it is added in fp32 after the
// activation -- round_before_add: after the activation was rounded to 16 bits, as a layer that stores it would have -- and the sum is
// rounded once. A change of this rule has three places: here, convgemm256_kernel's written-out copy of this body (conv_kernels.hip: it
// forms the staging address behind the bias pass, which saves it a register) and conv3x3r's SKIP in-register pass (bias_act / round16 only).
template <class E, bool RELU, bool HAS_ADD>
__device__ __forceinline__ void epilogue_quad(float x0, float x1, float x2, float x3, const float4 b, uint16_t* po, int round_before_add) {
  float v[4] = {x0, x1, x2, x3};
  bias_act<RELU>(v, b);
  if (HAS_ADD) {
    float ad[4];
    E::un4(*reinterpret_cast<const uint2*>(po), ad);
    if (round_before_add) round16<E>(v);
    v[0] += ad[0]; v[1] += ad[1]; v[2] += ad[2]; v[3] += ad[3];
  }
  *reinterpret_cast<uint2*>(po) = E::pk4(v[0], v[1], v[2], v[3]);
}

// the eight bias vectors of a lane of the 32 x 32 fragment layout (columns i * 32 + 8 q + 4 fh of wave wn's 64; `bias` points at the
// tile's first column), fetched once before the tile is touched (inside the loops every one of the 16-32 loads was followed by a full
// wait: as many serial L2 round trips per tile)
__device__ __forceinline__ void load_bias_quads(float4 (&bv)[2][4], const float* bias, int wn, int fh) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) bv[i][q] = *reinterpret_cast<const float4*>(bias + wn * 64 + i * 32 + 8 * q + 4 * fh);
}

// DMA instruction `idx` of the residual / skip tile -> staging tile: 64 / (NT / 8) rows of NT columns (4 rows x 256 bytes or 2 rows x
// 512 bytes), source chunks swizzled as st_off_n; rows past the end repeat row M - 1 (never copied out)
template <int NT>
__device__ __forceinline__ void residual_dma(const ConvGemmArgs& a, uint16_t* st, int idx, int m0, int n0, int l) {
  constexpr int CH = NT / 8, RPI = 64 / CH;
  const int row = idx * RPI + (l >> __builtin_ctz(CH));
  const uint16_t* g = a.add + (size_t)min(m0 + row, a.M - 1) * a.Co + n0 + (((l & (CH - 1)) ^ (row & (CH - 1))) << 3);
  __builtin_amdgcn_global_load_lds((gvoid_t*)g, (lvoid_t*)(st + idx * RPI * NT), 16, 0, 0);
}

// 16-byte chunk q of the finished staging tile -> out (full rows: consecutive lanes write consecutive chunks of a row)
template <int NT>
__device__ __forceinline__ void copy_out_chunk(const ConvGemmArgs& a, const uint16_t* st, int q, int m0, int n0) {
  constexpr int CH = NT / 8;
  const int row = q >> __builtin_ctz(CH), ch = q & (CH - 1), m = m0 + row;
  if (m < a.M) *reinterpret_cast<uint4*>(a.out + (size_t)m * a.Co + n0 + ch * 8) = *reinterpret_cast<const uint4*>(&st[row * NT + ((ch ^ (row & (CH - 1))) << 3)]);
}

}  // namespace acez
