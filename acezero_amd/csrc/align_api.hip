// align_api.hip -- pose evaluation against ground truth on the device (eval_poses.py / eval_poses_util.py of the reference).
//
// estimate_alignment (eval_poses_util.py:70-180): RANSAC over similarity transforms fitted to three camera centres, each
// hypothesis scored on every confident frame (translation AND rotation test), the best `refine_max_hyp` refined on their
// inlier sets, then the per-frame errors of eval_poses.py:140-170 under the winning alignment.  Everything is fp64.
//
// Launches (one stream, no host round trip in between):
//   align_hyp_kernel     256 threads = 4 waves, ALIGN_HPB hypotheses per workgroup.  Lanes 0..ALIGN_HPB-1 each solve one
//                        minimal sample (lane per hypothesis) into LDS; then every wave takes one hypothesis at a time (uniform
//                        transform, lanes over frames) while the frames' GT / estimate SoA rows are staged through LDS in tiles
//                        of ALIGN_TILE.  __ballot turns 64 inlier tests into one uint64 word of the hypothesis' mask.
//   align_refine_kernel  one workgroup per shortlisted hypothesis: the shortlist is the stable top-k of the valid scores (ties
//                        keep ascending hypothesis index, Python's sorted(reverse=True)); the workgroup re-solves on its inlier
//                        set until the score stops improving.
//   align_eval_kernel    grid over all frames: pick the refined winner (stable re-sort), per-frame t_err / r_err.
//
// Kabsch (eval_poses_util.py:20-45) with the 3x3 SVD done by one-sided (Hestenes) Jacobi on the covariance C: plane rotations of
// the columns of B = C V until they are orthogonal; S_i = |b_i|, u_i = b_i / S_i.  The third pair is taken as v1 x v2, u1 x u2,
// which makes R = V diag(1,1,d) U^T and d*S2 come out without sign bookkeeping (d = sign(det(V U^T)) and the sign of u3 cancel).
// Rotation angles (scipy's Rotation.from_matrix(M).magnitude() and the cv2.Rodrigues angle) take the orthogonal polar factor
// U V^T of M with the same SVD, then Markley's quaternion and 2 atan2(|v|, |w|): the angle does not depend on a scale of M.
// Every reduction runs in a fixed order; this unit is compiled with -ffp-contract=off.
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "acez_common.h"
#include "ransac_math.h"
#include "svd3.h"

namespace acez {

constexpr int ALIGN_THREADS = 256;
constexpr int ALIGN_WAVES = ALIGN_THREADS / 64;
constexpr int ALIGN_HPB = 16;      // hypotheses per workgroup of align_hyp_kernel (4 per wave)
constexpr int ALIGN_TILE = 128;    // frames per LDS tile
constexpr int ALIGN_G = 16;        // GT cam->world, all 4 rows (h_T @ poses_gt is a full 4x4 product)
constexpr int ALIGN_E = 12;        // estimate cam->world, rows 0..2
constexpr int ALIGN_REC = 16;      // per-hypothesis record: T rows 0..2 (12), scale, flags, score, pad
constexpr int ALIGN_MAX_REFINE = 64;

struct AlignDev {
  const double* g;       // [16][nc] SoA, confident frames
  const double* e;       // [12][nc]
  int nc;
  int words;             // ceil(nc / 64)
  double thr_t, thr_r;   // metres, radians
  int estimate_scale;
};

// ---------------------------------------------------------------------------------------------------- 3x3 algebra: svd3.h
// angle (radians) of the orthogonal polar factor of M (row-major): Markley's quaternion as scipy 1.15 builds it, normalised,
// 2 atan2(|v|, |w|).  Non-finite input or det(M) <= 0 -> NaN (scipy raises there; every comparison with NaN is false).
__host__ __device__ inline double rot_angle(const double M[9]) {
  double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
  if (!(det > 0.0) || !isfinite(det)) return NAN;
  Svd3 d;
  svd3(M, d);
  double Q[9];   // U V^T, rows r, cols c: sum_i u_i[r] v_i[c]
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Q[r * 3 + c] = d.u[0][r] * d.v[0][c] + d.u[1][r] * d.v[1][c] + d.u[2][r] * d.v[2][c];
  const double tr = Q[0] + Q[4] + Q[8];
  double dec[4] = {Q[0], Q[4], Q[8], tr};
  int ch = 0;
  for (int i = 1; i < 4; ++i)
    if (dec[i] > dec[ch]) ch = i;
  double q[4];
  if (ch != 3) {
    const int i = ch, j = (i + 1) % 3, k = (j + 1) % 3;
    q[i] = 1.0 - tr + 2.0 * Q[i * 3 + i];
    q[j] = Q[j * 3 + i] + Q[i * 3 + j];
    q[k] = Q[k * 3 + i] + Q[i * 3 + k];
    q[3] = Q[k * 3 + j] - Q[j * 3 + k];
  } else {
    q[0] = Q[7] - Q[5];
    q[1] = Q[2] - Q[6];
    q[2] = Q[3] - Q[1];
    q[3] = 1.0 + tr;
  }
  const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) q[i] /= qn;
  return 2.0 * atan2(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), fabs(q[3]));
}

// kabsch() of eval_poses_util.py:20-45 from the centred sums: cov = sum c1^T c2 / n, var2 = mean |c2|^2.  Writes rec[0..11]
// (rows 0..2 of T), rec[12] = scale, rec[13] = 1 if the sample is rank deficient (S1 < 1e-12 S0).
__host__ __device__ inline void kabsch_solve(const double cov[9], double var2, const double m1[3], const double m2[3], int estimate_scale,
                                             double* rec) {
  Svd3 d;
  svd3(cov, d);
  const double scale = estimate_scale ? var2 / (d.s[0] + d.s[1] + d.s[2]) : 1.0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) rec[r * 4 + c] = scale * (d.v[0][r] * d.u[0][c] + d.v[1][r] * d.u[1][c] + d.v[2][r] * d.u[2][c]);
    rec[r * 4 + 3] = m2[r] - (rec[r * 4 + 0] * m1[0] + rec[r * 4 + 1] * m1[1] + rec[r * 4 + 2] * m1[2]);
  }
  rec[12] = scale;
  rec[13] = (d.s[1] < 1e-12 * d.s[0] || d.s[0] == 0.0) ? 1.0 : 0.0;
}

// T (rows 0..2, row-major 3x4) applied to GT frame f of SoA rows with leading dimension LD; returns |t| error (aligned frame) and fills M = (T G)_R R_est^T.
__device__ __forceinline__ double frame_delta(const double* T, const double* g, const double* e, int LD, int f, double M[9]) {
  double A[3][4];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c)
      A[r][c] = T[r * 4 + 0] * g[(0 * 4 + c) * LD + f] + T[r * 4 + 1] * g[(1 * 4 + c) * LD + f] + T[r * 4 + 2] * g[(2 * 4 + c) * LD + f] +
                T[r * 4 + 3] * g[(3 * 4 + c) * LD + f];
  const double dx = A[0][3] - e[3 * LD + f], dy = A[1][3] - e[7 * LD + f], dz = A[2][3] - e[11 * LD + f];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      M[r * 3 + c] = A[r][0] * e[(c * 4 + 0) * LD + f] + A[r][1] * e[(c * 4 + 1) * LD + f] + A[r][2] * e[(c * 4 + 2) * LD + f];
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// get_inliers (eval_poses_util.py:55-67) for one (hypothesis, frame).  The rotation is only evaluated where translation passes.
__device__ __forceinline__ bool is_inlier(const double* T, const double* g, const double* e, int ld, int f, double thr_t, double thr_r) {
  double M[9];
  const double dt = frame_delta(T, g, e, ld, f, M);
  if (!(dt < thr_t)) return false;
  return rot_angle(M) < thr_r;
}

// the three distinct sample indices of hypothesis h (counter-based stream keyed (seed, h), or the replay table)
__device__ __forceinline__ void draw_sample(uint64_t seed, int h, int n, const int32_t* table, int s[3]) {
  if (table) {
    s[0] = table[h * 3 + 0]; s[1] = table[h * 3 + 1]; s[2] = table[h * 3 + 2];
    return;
  }
  const uint64_t key = rsm::try_key(seed, 0x45564131ull, (uint32_t)h, 0u);   // "EVA1": its own stream, apart from the DSAC* draws
  int a = rsm::irand(key, 0, n), b = rsm::irand(key, 1, n - 1), c = rsm::irand(key, 2, n - 2);
  if (b >= a) ++b;                          // a uniform draw of 3 distinct indices without a retry loop
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  if (c >= lo) ++c;
  if (c >= hi) ++c;
  s[0] = a; s[1] = b; s[2] = c;
}

// ---------------------------------------------------------------------------------------------------- launch 1: hypotheses
__global__ __launch_bounds__(ALIGN_THREADS) void align_hyp_kernel(AlignDev a, int H, uint64_t seed, const int32_t* __restrict__ table,
                                                                 uint64_t* __restrict__ masks, double* __restrict__ recs,
                                                                 int32_t* __restrict__ scores, int32_t* __restrict__ valid) {
  __shared__ double s_g[ALIGN_G * ALIGN_TILE];
  __shared__ double s_e[ALIGN_E * ALIGN_TILE];
  __shared__ double s_rec[ALIGN_HPB][ALIGN_REC];
  __shared__ int s_smp[ALIGN_HPB][3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h0 = blockIdx.x * ALIGN_HPB;
  if (t < ALIGN_HPB && h0 + t < H) {
    const int h = h0 + t;
    int s[3];
    draw_sample(seed, h, a.nc, table, s);
    double p1[3][3], p2[3][3], m1[3], m2[3];
    for (int k = 0; k < 3; ++k)
      for (int r = 0; r < 3; ++r) {
        p1[k][r] = a.g[(r * 4 + 3) * a.nc + s[k]];
        p2[k][r] = a.e[(r * 4 + 3) * a.nc + s[k]];
      }
    for (int r = 0; r < 3; ++r) {
      m1[r] = (p1[0][r] + p1[1][r] + p1[2][r]) / 3.0;
      m2[r] = (p2[0][r] + p2[1][r] + p2[2][r]) / 3.0;
    }
    double cov[9], var2 = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double acc = 0.0;
        for (int k = 0; k < 3; ++k) acc += (p1[k][i] - m1[i]) * (p2[k][j] - m2[j]);
        cov[i * 3 + j] = acc / 3.0;
      }
    for (int k = 0; k < 3; ++k) {
      const double x = p2[k][0] - m2[0], y = p2[k][1] - m2[1], z = p2[k][2] - m2[2];
      var2 += x * x + y * y + z * z;
    }
    kabsch_solve(cov, var2 / 3.0, m1, m2, a.estimate_scale, s_rec[t]);
    for (int k = 0; k < 3; ++k) s_smp[t][k] = s[k];
  }
  __syncthreads();
  int score[ALIGN_HPB / ALIGN_WAVES], hits[ALIGN_HPB / ALIGN_WAVES];
  for (int j = 0; j < ALIGN_HPB / ALIGN_WAVES; ++j) score[j] = hits[j] = 0;
  for (int f0 = 0; f0 < a.nc; f0 += ALIGN_TILE) {
    const int nt = min(ALIGN_TILE, a.nc - f0);
    __syncthreads();
    for (int i = t; i < ALIGN_G * ALIGN_TILE; i += ALIGN_THREADS) {
      const int row = i / ALIGN_TILE, f = i % ALIGN_TILE;
      s_g[i] = f < nt ? a.g[row * a.nc + f0 + f] : 0.0;
    }
    for (int i = t; i < ALIGN_E * ALIGN_TILE; i += ALIGN_THREADS) {
      const int row = i / ALIGN_TILE, f = i % ALIGN_TILE;
      s_e[i] = f < nt ? a.e[row * a.nc + f0 + f] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < ALIGN_HPB / ALIGN_WAVES; ++j) {
      const int hl = wave * (ALIGN_HPB / ALIGN_WAVES) + j, h = h0 + hl;
      if (h >= H) break;   // wave-uniform
      double T[12];
      for (int k = 0; k < 12; ++k) T[k] = s_rec[hl][k];
      for (int w0 = 0; w0 < nt; w0 += 64) {
        const int f = w0 + lane;
        const bool in = f < nt && is_inlier(T, s_g, s_e, ALIGN_TILE, f, a.thr_t, a.thr_r);
        const uint64_t word = __ballot(in);
        const int wi = (f0 + w0) >> 6;
        if (lane == 0) masks[(size_t)h * a.words + wi] = word;
        score[j] += __popcll(word);
        for (int k = 0; k < 3; ++k) {
          const int sk = s_smp[hl][k];
          if ((sk >> 6) == wi) hits[j] += (int)((word >> (sk & 63)) & 1ull);
        }
      }
    }
  }
  if (lane == 0)
    for (int j = 0; j < ALIGN_HPB / ALIGN_WAVES; ++j) {
      const int hl = wave * (ALIGN_HPB / ALIGN_WAVES) + j, h = h0 + hl;
      if (h >= H) break;
      for (int k = 0; k < ALIGN_REC; ++k) recs[(size_t)h * ALIGN_REC + k] = k < 14 ? s_rec[hl][k] : 0.0;
      scores[h] = score[j];
      valid[h] = hits[j] >= 3 ? 1 : 0;   // inliers[samples].sum() >= 3
    }
}

// ---------------------------------------------------------------------------------------------------- launch 2: refinement
__device__ __forceinline__ double block_sum(double v, double* part) {
  // fixed-order: per-thread partial in LDS, then a binary tree over the 256 slots
  const int t = threadIdx.x;
  __syncthreads();
  part[t] = v;
  __syncthreads();
  for (int off = ALIGN_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) part[t] += part[t + off];
    __syncthreads();
  }
  return part[0];
}
__device__ __forceinline__ uint64_t block_max_u64(uint64_t v, uint64_t* part) {
  const int t = threadIdx.x;
  __syncthreads();
  part[t] = v;
  __syncthreads();
  for (int off = ALIGN_THREADS / 2; off > 0; off >>= 1) {
    if (t < off && part[t + off] > part[t]) part[t] = part[t + off];
    __syncthreads();
  }
  return part[0];
}

// one workgroup per shortlist rank k.  out_rec[k] = refined record (rec[14] = score, -1 if rank k is empty), mask scratch [2][words].
__global__ __launch_bounds__(ALIGN_THREADS) void align_refine_kernel(AlignDev a, int H, int max_it, const int32_t* __restrict__ scores,
                                                                    const int32_t* __restrict__ valid, const uint64_t* __restrict__ masks,
                                                                    const double* __restrict__ recs, uint64_t* __restrict__ scratch,
                                                                    double* __restrict__ out_rec) {
  __shared__ uint64_t s_key[ALIGN_THREADS];
  __shared__ double s_part[ALIGN_THREADS];
  __shared__ double s_rec[ALIGN_REC];
  __shared__ int s_cnt[ALIGN_THREADS];
  const int t = threadIdx.x, k = blockIdx.x;
  // stable top-k: key = score << 32 | (2^32 - 1 - h); the k-th largest key is the k-th entry of sorted(reverse=True)
  uint64_t prev = ~0ull, key = 0;
  for (int r = 0; r <= k; ++r) {
    uint64_t best = 0;
    for (int h = t; h < H; h += ALIGN_THREADS) {
      if (!valid[h]) continue;
      const uint64_t kk = ((uint64_t)(uint32_t)scores[h] << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)h);
      if (kk < prev && kk > best) best = kk;
    }
    key = block_max_u64(best, s_key);
    prev = key;
    if (key == 0) break;
  }
  double* out = out_rec + (size_t)k * ALIGN_REC;
  if (key == 0) {
    if (t == 0) out[14] = -1.0;
    return;
  }
  const int h = (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
  int cur_score = scores[h];
  uint64_t* cur = scratch + (size_t)k * 2 * a.words;
  uint64_t* nxt = cur + a.words;
  for (int w = t; w < a.words; w += ALIGN_THREADS) cur[w] = masks[(size_t)h * a.words + w];
  if (t < ALIGN_REC) s_rec[t] = recs[(size_t)h * ALIGN_REC + t];
  const int per = (a.nc + ALIGN_THREADS - 1) / ALIGN_THREADS;   // thread t owns frames [t*per, t*per+per): a fixed summation order
  const int lo = min(a.nc, t * per), hi = min(a.nc, lo + per);
  for (int it = 0; it < max_it; ++it) {
    __syncthreads();
    // re-solve on the inlier set: two passes (means, then centred sums), as kabsch() centres before it multiplies
    double sx[6] = {0, 0, 0, 0, 0, 0};
    int cnt = 0;
    for (int f = lo; f < hi; ++f) {
      if (!((cur[f >> 6] >> (f & 63)) & 1ull)) continue;
      ++cnt;
      for (int r = 0; r < 3; ++r) {
        sx[r] += a.g[(r * 4 + 3) * a.nc + f];
        sx[3 + r] += a.e[(r * 4 + 3) * a.nc + f];
      }
    }
    double tot[6];
    for (int r = 0; r < 6; ++r) tot[r] = block_sum(sx[r], s_part);
    const double n = block_sum((double)cnt, s_part);
    double m1[3], m2[3];
    for (int r = 0; r < 3; ++r) { m1[r] = tot[r] / n; m2[r] = tot[3 + r] / n; }
    double cx[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int f = lo; f < hi; ++f) {
      if (!((cur[f >> 6] >> (f & 63)) & 1ull)) continue;
      double c1[3], c2[3];
      for (int r = 0; r < 3; ++r) {
        c1[r] = a.g[(r * 4 + 3) * a.nc + f] - m1[r];
        c2[r] = a.e[(r * 4 + 3) * a.nc + f] - m2[r];
      }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) cx[i * 3 + j] += c1[i] * c2[j];
      cx[9] += c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2];
    }
    double cov[9], var2;
    for (int i = 0; i < 9; ++i) cov[i] = block_sum(cx[i], s_part) / n;
    var2 = block_sum(cx[9], s_part) / n;
    double rec[ALIGN_REC];
    kabsch_solve(cov, var2, m1, m2, a.estimate_scale, rec);
    // recount: one bit per frame; each wave writes whole 64-bit words
    int c = 0;
    const int lane = t & 63, wave = t >> 6;
    for (int w = wave; w < a.words; w += ALIGN_WAVES) {
      const int f = w * 64 + lane;
      const bool in = f < a.nc && is_inlier(rec, a.g, a.e, a.nc, f, a.thr_t, a.thr_r);
      const uint64_t word = __ballot(in);
      if (lane == 0) nxt[w] = word;
      c += __popcll(word);
    }
    __syncthreads();
    s_cnt[t] = (lane == 0) ? c : 0;
    __syncthreads();
    for (int off = ALIGN_THREADS / 2; off > 0; off >>= 1) {
      if (t < off) s_cnt[t] += s_cnt[t + off];
      __syncthreads();
    }
    const int refined = s_cnt[0];
    if (!(refined > cur_score)) break;   // block-uniform
    cur_score = refined;
    __syncthreads();
    for (int w = t; w < a.words; w += ALIGN_THREADS) cur[w] = nxt[w];
    if (t < 14) s_rec[t] = rec[t];
    __threadfence_block();
  }
  __syncthreads();
  if (t < 14) out[t] = s_rec[t];
  if (t == 0) { out[14] = (double)cur_score; out[15] = (double)h; }
}

// ---------------------------------------------------------------------------------------------------- launch 3: evaluation
// out_sel[0..11] = T rows 0..2, [12] = scale, [13] = status (0 ok, 1 failed), [14] = winning score, [15] = winning hypothesis
__global__ __launch_bounds__(ALIGN_THREADS) void align_eval_kernel(const double* __restrict__ g_all, const double* __restrict__ e_all, int n,
                                                                  const double* __restrict__ ref_rec, int kref, int fixed,
                                                                  double* __restrict__ out_sel, double* __restrict__ t_err,
                                                                  double* __restrict__ r_err) {
  __shared__ double s_T[16];
  const int t = threadIdx.x;
  if (t == 0) {
    double T[16];
    for (int i = 0; i < 16; ++i) T[i] = 0.0;
    if (fixed) {   // --estimate_alignment False: identity, scale 1
      T[0] = T[5] = T[10] = 1.0;
      T[12] = 1.0;
      T[15] = -1.0;
    } else {
      int best = -1;
      for (int k = 0; k < kref; ++k)   // stable re-sort: the first of the largest scores in shortlist order
        if (ref_rec[k * ALIGN_REC + 14] >= 0.0 && (best < 0 || ref_rec[k * ALIGN_REC + 14] > ref_rec[best * ALIGN_REC + 14])) best = k;
      if (best >= 0) {
        for (int i = 0; i < 13; ++i) T[i] = ref_rec[best * ALIGN_REC + i];
        T[14] = ref_rec[best * ALIGN_REC + 14];
        T[15] = ref_rec[best * ALIGN_REC + 15];
      } else {
        T[13] = 1.0;
        T[12] = 1.0;
        T[15] = -1.0;
      }
    }
    for (int i = 0; i < 16; ++i) s_T[i] = T[i];
    if (blockIdx.x == 0)
      for (int i = 0; i < 16; ++i) out_sel[i] = T[i];
  }
  __syncthreads();
  const int f = blockIdx.x * ALIGN_THREADS + t;
  if (f >= n) return;
  if (s_T[13] != 0.0) {
    t_err[f] = INFINITY;
    r_err[f] = INFINITY;
    return;
  }
  double T[12];
  for (int i = 0; i < 12; ++i) T[i] = s_T[i];
  double A[3][4];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c)
      A[r][c] = T[r * 4 + 0] * g_all[(0 * 4 + c) * n + f] + T[r * 4 + 1] * g_all[(1 * 4 + c) * n + f] +
                T[r * 4 + 2] * g_all[(2 * 4 + c) * n + f] + T[r * 4 + 3] * g_all[(3 * 4 + c) * n + f];
  const double dx = A[0][3] - e_all[3 * n + f], dy = A[1][3] - e_all[7 * n + f], dz = A[2][3] - e_all[11 * n + f];
  t_err[f] = sqrt(dx * dx + dy * dy + dz * dz) / s_T[12];
  double M[9];   // R_est (T G)_R^T (eval_poses.py:157)
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      M[r * 3 + c] = e_all[(r * 4 + 0) * n + f] * A[c][0] + e_all[(r * 4 + 1) * n + f] * A[c][1] + e_all[(r * 4 + 2) * n + f] * A[c][2];
  r_err[f] = rot_angle(M) * 180.0 / M_PI;
}

}  // namespace acez

using namespace acez;

struct acez_align {
  int device;
  int max_frames, max_hyp;
  double* d_in;       // [28][max_frames] confident SoA, then [28][max_frames] all-frames SoA
  int32_t* d_table;   // [max_hyp][3]
  uint64_t* d_masks;  // [max_hyp][words]
  uint64_t* d_scratch;
  double* d_recs;     // [max_hyp][16]
  int32_t* d_scores;  // [2][max_hyp]: scores, valid
  double* d_out;      // [16 sel][max_frames t][max_frames r][MAX_REFINE][16]
  double* h_stage;    // pinned: inputs
  void* h_out;        // pinned: outputs
  hipStream_t stream;
};

static size_t out_doubles(int max_frames) { return 16 + 2 * (size_t)max_frames + (size_t)ALIGN_MAX_REFINE * ALIGN_REC; }

extern "C" int acez_align_create(acez_align** out, int max_frames, int max_hyp, int device) {
  ACEZ_REQUIRE(out, "null pointer");
  *out = nullptr;
  ACEZ_REQUIRE(max_frames > 0 && max_hyp > 0, "sizes must be positive");
  ACEZ_REQUIRE(max_frames <= (1 << 24) && max_hyp <= (1 << 24), "at most 2^24 frames and hypotheses");
  if (int rc = acez::require_device("pose evaluation runs on a gfx950 GPU")) return rc;
  if (device >= 0) ACEZ_HIP_CHECK(hipSetDevice(device));
  acez_align* c = new (std::nothrow) acez_align();
  ACEZ_REQUIRE(c, "out of host memory");
  ACEZ_HIP_CHECK(hipGetDevice(&c->device));
  c->max_frames = max_frames;
  c->max_hyp = max_hyp;
  const size_t words = ((size_t)max_frames + 63) / 64;
  const size_t in_bytes = (size_t)2 * (ALIGN_G + ALIGN_E) * max_frames * sizeof(double);
  const size_t out_bytes = out_doubles(max_frames) * sizeof(double) + (size_t)2 * max_hyp * sizeof(int32_t);
  int rc = ACEZ_OK;
  auto A = [&](void** p, size_t bytes) {
    if (rc == ACEZ_OK && hipMalloc(p, bytes) != hipSuccess) {
      acez::set_error("hipMalloc(%zu) failed", bytes);
      rc = ACEZ_ERR_HIP;
    }
  };
  A((void**)&c->d_in, in_bytes);
  A((void**)&c->d_table, (size_t)max_hyp * 3 * sizeof(int32_t));
  A((void**)&c->d_masks, (size_t)max_hyp * words * sizeof(uint64_t));
  A((void**)&c->d_scratch, (size_t)ALIGN_MAX_REFINE * 2 * words * sizeof(uint64_t));
  A((void**)&c->d_recs, (size_t)max_hyp * ALIGN_REC * sizeof(double));
  A((void**)&c->d_scores, (size_t)2 * max_hyp * sizeof(int32_t));
  A((void**)&c->d_out, out_doubles(max_frames) * sizeof(double));
  if (rc == ACEZ_OK && hipHostMalloc((void**)&c->h_stage, in_bytes + (size_t)max_hyp * 3 * sizeof(int32_t), 0) != hipSuccess) rc = ACEZ_ERR_HIP;
  if (rc == ACEZ_OK && hipHostMalloc(&c->h_out, out_bytes, 0) != hipSuccess) rc = ACEZ_ERR_HIP;
  if (rc == ACEZ_OK && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) rc = ACEZ_ERR_HIP;
  if (rc != ACEZ_OK) {
    if (rc == ACEZ_ERR_HIP) acez::set_error("acez_align_create: device or pinned allocation failed");
    acez_align_destroy(c);
    return rc;
  }
  *out = c;
  return ACEZ_OK;
}

extern "C" void acez_align_destroy(acez_align* c) {
  if (!c) return;
  (void)hipFree(c->d_in);
  (void)hipFree(c->d_table);
  (void)hipFree(c->d_masks);
  (void)hipFree(c->d_scratch);
  (void)hipFree(c->d_recs);
  (void)hipFree(c->d_scores);
  (void)hipFree(c->d_out);
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  if (c->h_out) (void)hipHostFree(c->h_out);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

static bool finite16(const double* p) {
  for (int i = 0; i < 16; ++i)
    if (!isfinite(p[i])) return false;
  return true;
}

// rows 0..R-1 of n 4x4 matrices (selected by idx) -> SoA [R*4][n]
static void to_soa(const double* poses, const std::vector<int>& idx, int rows, double* dst) {
  const int n = (int)idx.size();
  for (int f = 0; f < n; ++f) {
    const double* p = poses + (size_t)idx[f] * 16;
    for (int i = 0; i < rows * 4; ++i) dst[(size_t)i * n + f] = p[i];
  }
}

extern "C" int acez_align_evaluate(acez_align* c, const double* gt_c2w, const double* est_c2w, const double* confidence, int n_frames,
                                   const acez_align_params* prm, const int32_t* samples, double* out_T, double* out_scale,
                                   int32_t* out_status, int32_t* out_scores, int32_t* out_valid, double* out_t_err, double* out_r_err,
                                   int32_t* out_accurate) {
  ACEZ_REQUIRE(c && gt_c2w && est_c2w && confidence && prm && out_T && out_scale && out_status && out_t_err && out_r_err && out_accurate,
               "null pointer");
  ACEZ_REQUIRE(n_frames > 0 && n_frames <= c->max_frames, "n_frames outside [1, max_frames]");
  ACEZ_REQUIRE(prm->estimate_alignment == 0 || (prm->ransac_iterations > 0 && prm->ransac_iterations <= c->max_hyp),
               "ransac_iterations outside [1, max_hyp]");
  ACEZ_REQUIRE(prm->refinement_max_hyp >= 1 && prm->refinement_max_hyp <= ALIGN_MAX_REFINE, "refinement_max_hyp outside [1, 64]");
  ACEZ_REQUIRE(prm->refinement_max_it >= 0, "refinement_max_it < 0");
  ACEZ_HIP_CHECK(hipSetDevice(c->device));
  // confident frames (eval_poses_util.py:85-87): finite GT, confidence strictly above the threshold
  std::vector<int> conf, all(n_frames);
  for (int f = 0; f < n_frames; ++f) {
    all[f] = f;
    if (finite16(gt_c2w + (size_t)f * 16) && confidence[f] > prm->confidence_threshold) conf.push_back(f);
  }
  const int nc = (int)conf.size();
  const int H = prm->ransac_iterations;
  const bool fixed = prm->estimate_alignment == 0;
  const bool run_ransac = !fixed && nc >= prm->min_confident_estimates && nc >= 3;
  const int words = (nc + 63) / 64;
  const size_t mf = (size_t)c->max_frames;
  double* st = c->h_stage;
  double* st_all = st + (ALIGN_G + ALIGN_E) * mf;
  int32_t* st_tab = (int32_t*)(st + 2 * (ALIGN_G + ALIGN_E) * mf);
  to_soa(gt_c2w, all, 4, st_all);
  to_soa(est_c2w, all, 3, st_all + (size_t)ALIGN_G * n_frames);
  if (run_ransac) {
    to_soa(gt_c2w, conf, 4, st);
    to_soa(est_c2w, conf, 3, st + (size_t)ALIGN_G * nc);
    if (samples) {
      for (int i = 0; i < 3 * H; ++i) ACEZ_REQUIRE(samples[i] >= 0 && samples[i] < nc, "sample index outside the confident frames");
      for (int h = 0; h < H; ++h)
        ACEZ_REQUIRE(samples[3 * h] != samples[3 * h + 1] && samples[3 * h] != samples[3 * h + 2] && samples[3 * h + 1] != samples[3 * h + 2],
                     "a sample triple repeats an index");
      memcpy(st_tab, samples, (size_t)3 * H * sizeof(int32_t));
    }
  }
  hipStream_t s = c->stream;
  double* d_conf = c->d_in;
  double* d_all = c->d_in + (ALIGN_G + ALIGN_E) * mf;
  double* d_sel = c->d_out;
  double* d_t = d_sel + 16;
  double* d_r = d_t + mf;
  double* d_ref = d_r + mf;
  ACEZ_HIP_CHECK(hipMemcpyAsync(d_all, st_all, (size_t)(ALIGN_G + ALIGN_E) * n_frames * sizeof(double), hipMemcpyHostToDevice, s));
  const int kref = prm->refinement_max_hyp;
  if (run_ransac) {
    ACEZ_HIP_CHECK(hipMemcpyAsync(d_conf, st, (size_t)(ALIGN_G + ALIGN_E) * nc * sizeof(double), hipMemcpyHostToDevice, s));
    if (samples) ACEZ_HIP_CHECK(hipMemcpyAsync(c->d_table, st_tab, (size_t)3 * H * sizeof(int32_t), hipMemcpyHostToDevice, s));
    AlignDev a{d_conf, d_conf + (size_t)ALIGN_G * nc, nc, words, prm->threshold_t, prm->threshold_r / 180.0 * M_PI,
               prm->estimate_scale};
    hipLaunchKernelGGL(align_hyp_kernel, dim3((H + ALIGN_HPB - 1) / ALIGN_HPB), dim3(ALIGN_THREADS), 0, s, a, H, prm->seed,
                       samples ? (const int32_t*)c->d_table : nullptr, c->d_masks, c->d_recs, c->d_scores, c->d_scores + c->max_hyp);
    ACEZ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(align_refine_kernel, dim3(kref), dim3(ALIGN_THREADS), 0, s, a, H, prm->refinement_max_it, (const int32_t*)c->d_scores,
                       (const int32_t*)(c->d_scores + c->max_hyp), (const uint64_t*)c->d_masks, (const double*)c->d_recs, c->d_scratch, d_ref);
    ACEZ_HIP_CHECK(hipGetLastError());
  } else if (!fixed) {
    ACEZ_HIP_CHECK(hipMemsetAsync(d_ref, 0xFF, (size_t)kref * ALIGN_REC * sizeof(double), s));   // all-ones bits: NaN, never >= 0 -> failed
  }
  hipLaunchKernelGGL(align_eval_kernel, dim3((n_frames + ALIGN_THREADS - 1) / ALIGN_THREADS), dim3(ALIGN_THREADS), 0, s, (const double*)d_all,
                     (const double*)(d_all + (size_t)ALIGN_G * n_frames), n_frames, (const double*)d_ref, kref, fixed ? 1 : 0, d_sel, d_t, d_r);
  ACEZ_HIP_CHECK(hipGetLastError());
  // one copy back and one synchronisation
  double* ho = (double*)c->h_out;
  ACEZ_HIP_CHECK(hipMemcpyAsync(ho, d_sel, (16 + 2 * mf) * sizeof(double), hipMemcpyDeviceToHost, s));
  int32_t* hs = (int32_t*)(ho + out_doubles(c->max_frames));
  const bool want_scores = out_scores && run_ransac;
  if (want_scores) ACEZ_HIP_CHECK(hipMemcpyAsync(hs, c->d_scores, (size_t)2 * c->max_hyp * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ACEZ_HIP_CHECK(hipStreamSynchronize(s));
  const bool failed = ho[13] != 0.0;
  for (int i = 0; i < 16; ++i) out_T[i] = 0.0;
  if (!failed) {
    for (int i = 0; i < 12; ++i) out_T[i] = ho[i];
    out_T[15] = 1.0;
  }
  *out_scale = failed ? 1.0 : ho[12];
  *out_status = failed ? 1 : 0;
  int acc = 0;
  const double thr_r = prm->threshold_r, thr_t = prm->threshold_t;
  for (int f = 0; f < n_frames; ++f) {
    out_t_err[f] = ho[16 + f];
    out_r_err[f] = ho[16 + mf + f];
    acc += (out_r_err[f] < thr_r && out_t_err[f] < thr_t) ? 1 : 0;   // eval_poses.py:166-167
  }
  *out_accurate = acc;
  if (out_scores) {
    for (int h = 0; h < H; ++h) {
      out_scores[h] = want_scores ? hs[h] : 0;
      if (out_valid) out_valid[h] = want_scores ? hs[c->max_hyp + h] : 0;
    }
  }
  return ACEZ_OK;
}
