// ransac_rgbd.h -- the stages of DSAC* RGB-D registration that the forward kernel (ransac_rgbd.hip) and the backward kernel
// (ransac_grad.hip) share: the valid-cell compaction, the hypothesis sampling, the scoring and the Kabsch refinement, all on one
// 512-thread workgroup per frame with fp64 geometry. The including units are compiled with -ffp-contract=off; each stage is the
// forward kernel's code, so both kernels draw, score and refine with the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "ordered_sum.h"
#include "ransac_math.h"
#include "ransac_ctx.h"
#include "svd3.h"

namespace acez_rgbd {

constexpr int THREADS = acez_rs::RGBD_THREADS;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_ROWS = 32;          // valid-list entries per thread (flags in one 32-bit word): N <= 16384
static_assert(THREADS * MAX_ROWS == acez_rs::MAX_CELLS, "check_frames' limit is this layout's");
constexpr int RED_STRIDE = 16;        // doubles per wavefront in the reduction scratch

// The inputs both kernels take.
struct RgbdIn {
  const float* sc;      // [n][3][H][W] scene coordinates, metres
  const float* cc;      // [n][3][H][W] camera coordinates, metres
  const acez_rs::FrameParam* fp;  // frame ids
  float* big;           // [n][7][Npad] compacted lists of frames that do not fit the LDS (GC instantiation)
  int H, W, N, Npad, hyps, max_tries, max_ref_steps;
  uint32_t h_magic;     // ceil(2^32 / H): p / H == __umulhi(p, h_magic) for p < 2^16 (H >= 2)
  float thr, alpha, max_dist;
  uint64_t seed;
  double* hyp_poses;    // [n][hyps][6] (rvec, tvec)
  double* scores;       // [n][hyps]
  int* samples;         // [n][hyps][3] map indices y * W + x of the kept triple
};

inline RgbdIn make_in(const float* sc, const float* cc, const acez_rs::FrameParam* fp, const acez_rs::Workspace& ws,
                      const acez_rs::Geometry& g, int h, int w, const acez_ransac_params* params, uint64_t seed) {
  RgbdIn a;
  a.sc = sc; a.cc = cc; a.fp = fp; a.big = ws.d_list;
  a.H = h; a.W = w; a.N = g.N; a.Npad = g.Npad; a.hyps = params->hypotheses; a.max_tries = params->max_tries;
  a.max_ref_steps = params->max_ref_steps;
  a.h_magic = g.h_magic;
  a.thr = params->inlier_threshold; a.alpha = params->inlier_alpha; a.max_dist = params->max_reproj; a.seed = seed;
  a.hyp_poses = ws.d_hyp_poses; a.scores = ws.d_scores; a.samples = ws.d_samples;
  return a;
}

// The frame's compacted valid list (LDS or HBM) and the LDS region after it.
struct Frame {
  float *sx, *sy, *sz, *ex, *ey, *ez;
  uint16_t* cell;
  double* sScores;  // [hyps]
  double* sHyp;     // [hyps][6]
  double* sRed;     // [WAVES][RED_STRIDE]
  int* sIdx;        // [hyps][3]
  int* sCnt;        // [MAX_ROWS][WAVES]
  int* sInt;        // [8]
  unsigned char* tail;   // LDS after the region (the backward kernel's own arrays)
  int nv;
};

using acez::wave_sum;   // ordered_sum.h

// get3DDistErrs for one cell: transform() rounds R X + t to float (cv::Point3f), the difference is a float vector, cv::norm
// its fp64 length; (float) length * 100, clamped (a NaN length takes the clamp value)
__device__ __forceinline__ float dist_err(const double R[9], const double t[3], float X, float Y, float Z, float ex, float ey, float ez,
                                          float max_dist) {
  const float px = (float)(((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]);
  const float py = (float)(((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]);
  const float pz = (float)(((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]);
  const float dx = ex - px, dy = ey - py, dz = ez - pz;
  const float l = (float)sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz) * 100.f;
  return l < max_dist ? l : max_dist;
}

// Kabsch: the rotation R (row-major) and translation t with eye ~ R X + t from the centred covariance C = sum Xc Ec^T and the
// centroids. false if C has rank < 2 (the rotation is not determined). svd3 returns proper U, V with a signed third singular value,
// so R = V U^T is the sign-corrected Kabsch rotation. d (optional) receives the SVD.
__host__ __device__ __forceinline__ bool kabsch(const double C[9], const double mX[3], const double mE[3], double rv[3], double t[3],
                                                acez::Svd3* dout = nullptr) {
  acez::Svd3 d;
  acez::svd3(C, d);
  if (dout) *dout = d;
  if (!(d.s[0] > 0.0) || !(d.s[1] >= 1e-12 * d.s[0])) return false;
  double R[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = d.v[0][r] * d.u[0][c] + d.v[1][r] * d.u[1][c] + d.v[2][r] * d.u[2][c];
  for (int r = 0; r < 3; ++r) t[r] = mE[r] - ((R[r * 3 + 0] * mX[0] + R[r * 3 + 1] * mX[1]) + R[r * 3 + 2] * mX[2]);
  rsm::rodrigues_inv(R, rv);   // the hypothesis is kept as (rvec, tvec), as cv::Rodrigues stores it (dsacstar_util_rgbd.h:290-302)
  return true;
}

// K sums over the workgroup: per-thread sums in list order, wavefront butterflies, the wavefronts added in index order
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* sRed, int lane, int wave) {
#pragma unroll
  for (int q = 0; q < K; ++q) v[q] = wave_sum(v[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < K; ++q) sRed[wave * RED_STRIDE + q] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < K; ++q) {
    double s = sRed[q];
    for (int w = 1; w < WAVES; ++w) s = s + sRed[w * RED_STRIDE + q];
    v[q] = s;
  }
  __syncthreads();
}

__host__ __device__ inline size_t region_bytes(int hyps) {
  return 8 * (size_t)(7 * hyps + RED_STRIDE * WAVES) + 4 * (size_t)(3 * hyps + MAX_ROWS * WAVES + 8);
}

// LDS: [6][Npad] float list coordinates + [Npad] uint16 map indices (LDS instantiation only), then the region:
//   scores [hyps] f64, sampled poses [hyps][6] f64, reduction scratch [WAVES][16] f64, sampled triples [hyps][3] int,
//   compaction counts [MAX_ROWS][WAVES] int, [8] int; then the caller's tail.
template <bool GC>
__device__ __forceinline__ Frame frame_layout(const RgbdIn& a, unsigned char* smem_raw, int frame) {
  Frame f;
  const int Npad = a.Npad;
  f.sx = GC ? a.big + (size_t)frame * 7 * Npad : reinterpret_cast<float*>(smem_raw);
  f.sy = f.sx + Npad;
  f.sz = f.sy + Npad;
  f.ex = f.sz + Npad;
  f.ey = f.ex + Npad;
  f.ez = f.ey + Npad;
  f.cell = reinterpret_cast<uint16_t*>(f.ez + Npad);
  unsigned char* reg = smem_raw + (GC ? 0 : 26 * (size_t)Npad);
  f.sScores = reinterpret_cast<double*>(reg);
  f.sHyp = f.sScores + a.hyps;
  f.sRed = f.sHyp + 6 * a.hyps;
  f.sIdx = reinterpret_cast<int*>(f.sRed + RED_STRIDE * WAVES);
  f.sCnt = f.sIdx + 3 * a.hyps;
  f.sInt = f.sCnt + MAX_ROWS * WAVES;
  f.tail = reg + ((region_bytes(a.hyps) + 7) & ~(size_t)7);   // 8-byte aligned
  f.nv = 0;
  return f;
}

// ---- valid cells in scan order p = x * H + y; thread tid owns p = tid + THREADS i. Invalid cells get mask 0 if mk.
__device__ __forceinline__ void compact_valid(const RgbdIn& a, Frame& f, int frame, uint8_t* mk) {
  const int N = a.N, H = a.H, W = a.W;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* sc = a.sc + (size_t)frame * 3 * N;
  const float* cc = a.cc + (size_t)frame * 3 * N;
  const int rows = (N + THREADS - 1) / THREADS;
  uint32_t vflags = 0;
  for (int i = 0; i < rows; ++i) {
    const int p = tid + THREADS * i;
    if (p >= N) break;
    const int x = rsm::div_h(p, H, a.h_magic), y = p - x * H;
    const int m = y * W + x;
    const float cx = cc[m], cy = cc[N + m], cz = cc[2 * N + m];
    if (cz != 0.f && isfinite(cx) && isfinite(cy) && isfinite(cz)) vflags |= 1u << i;
    else if (mk) mk[m] = 0;   // invalid cells are never inliers (valid ones are written once, below)
  }
  for (int i = 0; i < rows; ++i) {
    const unsigned long long m = __ballot((vflags >> i) & 1u);
    if (lane == 0) f.sCnt[i * WAVES + wave] = __popcll(m);
  }
  __syncthreads();
  int nv = 0;
  for (int i = 0; i < rows; ++i) {
    const bool fl = (vflags >> i) & 1u;
    const unsigned long long bm = __ballot(fl);
    int base = nv, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const int c = f.sCnt[i * WAVES + w];
      base += w < wave ? c : 0;
      tot += c;
    }
    if (fl) {
      const int j = base + __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u));
      const int p = tid + THREADS * i;
      const int x = rsm::div_h(p, H, a.h_magic), y = p - x * H;
      const int m = y * W + x;
      f.sx[j] = sc[m]; f.sy[j] = sc[N + m]; f.sz[j] = sc[2 * N + m];
      f.ex[j] = cc[m]; f.ey[j] = cc[N + m]; f.ez[j] = cc[2 * N + m];
      f.cell[j] = (uint16_t)m;
    }
    nv += tot;
  }
  __syncthreads();
  f.nv = nv;
}

// The centred covariance and centroids of a triple, in the sampling's summation order.
__host__ __device__ __forceinline__ void triple_moments(const double X[3][3], const double E[3][3], double mX[3], double mE[3], double C[9]) {
  for (int r = 0; r < 3; ++r) {
    mX[r] = ((X[0][r] + X[1][r]) + X[2][r]) / 3.0;
    mE[r] = ((E[0][r] + E[1][r]) + E[2][r]) / 3.0;
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      C[r * 3 + c] = ((X[0][r] - mX[r]) * (E[0][c] - mE[c]) + (X[1][r] - mX[r]) * (E[1][c] - mE[c])) + (X[2][r] - mX[r]) * (E[2][c] - mE[c]);
}

// ---- sample: hypothesis h = wave + WAVES (8 pass + slot), try t0 + tr on lane 8 slot + tr. Needs nv >= 3.
__device__ __forceinline__ void sample_hyps(const RgbdIn& a, Frame& f, uint64_t frame_id) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nv = f.nv;
  for (int pass = 0; wave + WAVES * (8 * pass) < a.hyps; ++pass) {
    const int slot = lane >> 3, tr = lane & 7;
    const int h = wave + WAVES * (8 * pass + slot);
    bool settled = h >= a.hyps;
    for (int t0 = 0; t0 < a.max_tries; t0 += 8) {
      if (__ballot(!settled) == 0ull) break;
      const int t = t0 + tr;
      double rv[3] = {0, 0, 0}, tv[3] = {0, 0, 0};
      int idx[3] = {0, 0, 0};
      int status = 0;   // 0: rank-deficient triple (zero pose), 1: fitted but a point is not reproduced, 2: accepted
      if (!settled && t < a.max_tries) {
        const uint64_t key = rsm::try_key(a.seed, frame_id, (uint32_t)h, (uint32_t)t);
        double X[3][3], E[3][3];
        for (int j = 0; j < 3; ++j) {
          idx[j] = rsm::irand(key, j, nv);
          X[j][0] = f.sx[idx[j]]; X[j][1] = f.sy[idx[j]]; X[j][2] = f.sz[idx[j]];
          E[j][0] = f.ex[idx[j]]; E[j][1] = f.ey[idx[j]]; E[j][2] = f.ez[idx[j]];
        }
        double mX[3], mE[3], C[9];
        triple_moments(X, E, mX, mE, C);
        if (kabsch(C, mX, mE, rv, tv)) {
          status = 2;
          double R[9];
          rsm::rodrigues(rv, R, nullptr);
          for (int j = 0; j < 3; ++j) {
            const float px = (float)(((R[0] * X[j][0] + R[1] * X[j][1]) + R[2] * X[j][2]) + tv[0]);
            const float py = (float)(((R[3] * X[j][0] + R[4] * X[j][1]) + R[5] * X[j][2]) + tv[1]);
            const float pz = (float)(((R[6] * X[j][0] + R[7] * X[j][1]) + R[8] * X[j][2]) + tv[2]);
            const float dx = (float)E[j][0] - px, dy = (float)E[j][1] - py, dz = (float)E[j][2] - pz;
            if (sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz) * 100 < (double)a.thr) continue;
            status = 1;
            break;
          }
        } else {
          rv[0] = rv[1] = rv[2] = tv[0] = tv[1] = tv[2] = 0.0;
        }
      }
      const unsigned long long ok = __ballot(status == 2);
      if (!settled) {
        const unsigned g = (unsigned)(ok >> (slot * 8)) & 0xffu;
        int src = -1;
        if (g) src = __ffs((int)g) - 1;                                  // first accepted try of this batch
        else if (t0 + 8 >= a.max_tries) src = a.max_tries - 1 - t0;      // every try failed: the last one stands
        if (src >= 0) {
          settled = true;
          if (tr == src) {
            for (int i = 0; i < 3; ++i) {
              f.sHyp[h * 6 + i] = rv[i];
              f.sHyp[h * 6 + 3 + i] = tv[i];
              f.sIdx[h * 3 + i] = f.cell[idx[i]];
            }
          }
        }
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();   // a wavefront scores the hypotheses its own lanes sampled
}

// ---- score: hypothesis h on wavefront h % WAVES, lanes over the valid list; writes sScores and the diagnostics.
__device__ __forceinline__ void score_hyps(const RgbdIn& a, Frame& f, int frame) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nv = f.nv;
  const float inlierBeta = 5 / a.thr;
  const float score_scale = a.alpha / (float)a.W / (float)a.H;
  double inv_term = 0.0;             // an invalid cell's term: its error is max_dist
  {
    const float be = inlierBeta * (a.max_dist - a.thr);
    if (!(be > 40.f)) inv_term = 1 - 1 / (1 + detm::exp_(-(double)be));
  }
  for (int h = wave; h < a.hyps; h += WAVES) {
    double prm[6], R[9];
    for (int i = 0; i < 6; ++i) prm[i] = f.sHyp[h * 6 + i];
    rsm::rodrigues(prm, R, nullptr);
    double acc = 0;
    for (int j = lane; j < nv; j += 64) {
      const float e = dist_err(R, prm + 3, f.sx[j], f.sy[j], f.sz[j], f.ex[j], f.ey[j], f.ez[j], a.max_dist);
      const float beta_e = inlierBeta * (e - a.thr);
      if (beta_e > 40.f) continue;   // 1 + exp(-40) == 1 in fp64: the term is exactly +0
      acc += 1 - 1 / (1 + detm::exp_(-(double)beta_e));
    }
    double score = wave_sum(acc) + (double)(a.N - nv) * inv_term;
    score *= score_scale;
    if (lane == 0) {
      f.sScores[h] = score;
      const size_t o = (size_t)frame * a.hyps + h;
      for (int i = 0; i < 6; ++i) a.hyp_poses[o * 6 + i] = prm[i];
      for (int i = 0; i < 3; ++i) a.samples[o * 3 + i] = f.sIdx[h * 3 + i];
      a.scores[o] = score;
    }
  }
  __syncthreads();
}

struct Refined {
  uint32_t acc_flags;  // bit k: list entry tid + THREADS k is an inlier of the last accepted step
  int inliers;         // its size (3 if no step was accepted)
  bool have_map;       // a step was accepted
};

// ---- refine (refineHypRGBD): thread tid owns list entries j = tid + THREADS k. param: in the hypothesis, out the refined pose.
__device__ __forceinline__ Refined refine(const RgbdIn& a, const Frame& f, double param[6]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nv = f.nv;
  const int vrows = (nv + THREADS - 1) / THREADS;
  auto classify = [&](const double* prm) -> uint32_t {
    double R[9];
    rsm::rodrigues(prm, R, nullptr);
    uint32_t fl = 0;
    for (int k = 0; k < vrows; ++k) {
      const int j = tid + THREADS * k;
      if (j >= nv) break;
      if (dist_err(R, prm + 3, f.sx[j], f.sy[j], f.sz[j], f.ex[j], f.ey[j], f.ez[j], a.max_dist) < a.thr) fl |= 1u << k;
    }
    return fl;
  };
  uint32_t flags = classify(param), acc_flags = 0;
  int bestInliers = 3;
  bool have_map = false;
  const int max_ref = a.max_ref_steps > 0 ? a.max_ref_steps : 100;
  for (int rStep = 0; rStep < max_ref; ++rStep) {
    double s1[7] = {0, 0, 0, 0, 0, 0, 0};   // count, sum X, sum E
    for (int k = 0; k < vrows; ++k) {
      if (!((flags >> k) & 1u)) continue;
      const int j = tid + THREADS * k;
      s1[0] += 1.0;
      s1[1] += f.sx[j]; s1[2] += f.sy[j]; s1[3] += f.sz[j];
      s1[4] += f.ex[j]; s1[5] += f.ey[j]; s1[6] += f.ez[j];
    }
    block_sum(s1, f.sRed, lane, wave);
    const int cnt = (int)s1[0];
    if (cnt <= bestInliers) break;   // converged
    const double mX[3] = {s1[1] / s1[0], s1[2] / s1[0], s1[3] / s1[0]};
    const double mE[3] = {s1[4] / s1[0], s1[5] / s1[0], s1[6] / s1[0]};
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < vrows; ++k) {
      if (!((flags >> k) & 1u)) continue;
      const int j = tid + THREADS * k;
      const double xc[3] = {f.sx[j] - mX[0], f.sy[j] - mX[1], f.sz[j] - mX[2]};
      const double ec[3] = {f.ex[j] - mE[0], f.ey[j] - mE[1], f.ez[j] - mE[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[r * 3 + c] += xc[r] * ec[c];
    }
    block_sum(C, f.sRed, lane, wave);
    double rv[3], tv[3];
    if (!kabsch(C, mX, mE, rv, tv)) break;   // rank-deficient inlier set: keep the last accepted step
    bestInliers = cnt;
    for (int i = 0; i < 3; ++i) {
      param[i] = rv[i];
      param[3 + i] = tv[i];
    }
    acc_flags = flags;
    have_map = true;
    flags = classify(param);
  }
  return Refined{acc_flags, bestInliers, have_map};
}

}  // namespace acez_rgbd
