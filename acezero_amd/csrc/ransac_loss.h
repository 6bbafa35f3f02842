// ransac_loss.h -- the DSAC* pose loss (dsacstar_loss.h: loss, dLoss), the small fp64 helpers and the stages both backward kernels
// share (ransac_api.hip for RGB, ransac_grad.hip for RGB-D): soft-max and entropy, the expected loss, the support-term scatter and
// the zeroing / flushing of a frame's fp64 accumulator. The including units are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include "ransac_math.h"
#include "svd3.h"

namespace acez_loss {

constexpr double PROB_THRESH = 0.001;   // dsacstar_derivative.h:36
constexpr double MAXLOSS = 10000000.0;  // dsacstar_loss.h:35
constexpr double FD_EPS = 0.001;        // dKabschFD's eps
constexpr double PI_D = 3.141592653589793;

__device__ __forceinline__ void cross(const double* a, const double* b, double* c) { acez::cross3(a, b, c); }

// x = M^-1 b for a 3x3 row-major M (cofactors); false if M is singular
__device__ __forceinline__ bool solve3(const double M[9], const double b[3], double x[3]) {
  const double c0 = M[4] * M[8] - M[5] * M[7], c1 = M[5] * M[6] - M[3] * M[8], c2 = M[3] * M[7] - M[4] * M[6];
  const double det = M[0] * c0 + M[1] * c1 + M[2] * c2;
  if (!(fabs(det) > 1e-300)) return false;
  const double inv[9] = {c0, M[2] * M[7] - M[1] * M[8], M[1] * M[5] - M[2] * M[4],
                         c1, M[0] * M[8] - M[2] * M[6], M[2] * M[3] - M[0] * M[5],
                         c2, M[1] * M[6] - M[0] * M[7], M[0] * M[4] - M[1] * M[3]};
  for (int r = 0; r < 3; ++r) x[r] = ((inv[r * 3] * b[0] + inv[r * 3 + 1] * b[1]) + inv[r * 3 + 2] * b[2]) / det;
  return true;
}

// Jr (row-major): column k = vee(R^T dR/dr_k), so that a change dr of the Rodrigues vector turns R into R [Jr dr]x
__device__ __forceinline__ void body_jacobian(const double R[9], const double J[27], double Jr[9]) {
  for (int k = 0; k < 3; ++k) {
    const double* d = J + k * 9;
    double M[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) M[r * 3 + c] = (R[0 * 3 + r] * d[0 * 3 + c] + R[1 * 3 + r] * d[1 * 3 + c]) + R[2 * 3 + r] * d[2 * 3 + c];
    Jr[0 * 3 + k] = 0.5 * (M[7] - M[5]);
    Jr[1 * 3 + k] = 0.5 * (M[2] - M[6]);
    Jr[2 * 3 + k] = 0.5 * (M[3] - M[1]);
  }
}

// dsacstar::loss(pose2trans(hyp), gt) and, if g, its gradient with respect to (rvec, tvec)
__device__ double pose_loss(const double prm[6], const float* G, float w_rot, float w_trans, float cut, double* g) {
  double R[9], J[27];
  rsm::rodrigues(prm, R, J);
  double Rg[9], cg[3];   // ground truth world->camera rotation, camera centre
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rg[r * 3 + c] = (double)G[c * 4 + r];
    cg[r] = (double)G[r * 4 + 3];
  }
  double tr = 0;
  for (int q = 0; q < 9; ++q) tr += R[q] * Rg[q];
  const double trc = tr < -1.0 ? -1.0 : tr > 3.0 ? 3.0 : tr;
  const double rotErr = 180 * acos((trc - 1.0) / 2.0) / PI_D;
  double c[3], u[3];
  for (int r = 0; r < 3; ++r) c[r] = -((R[0 * 3 + r] * prm[3] + R[1 * 3 + r] * prm[4]) + R[2 * 3 + r] * prm[5]);
  for (int r = 0; r < 3; ++r) u[r] = c[r] - cg[r];
  const double tErr = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  const double l = (double)w_rot * rotErr + (double)w_trans * tErr;
  double L = l > (double)cut ? sqrt((double)cut * l) : l;
  L = L < MAXLOSS ? L : MAXLOSS;
  if (!g) return L;
  for (int i = 0; i < 6; ++i) g[i] = 0.0;
  if (!(L < MAXLOSS) || !(tErr + rotErr > 0.0)) return L;
  // dl/dR = w_rot drot/dtr Rg - w_trans t u^T / |u|;  dl/dt = -w_trans R u / |u|
  const double dtr = (tr > -1.0 && tr < 3.0) ? (double)w_rot * (-180 / PI_D) / sqrt(3 - tr * tr + 2 * tr) : 0.0;
  if (tErr > 0.0)
    for (int r = 0; r < 3; ++r) u[r] /= tErr;
  else
    u[0] = u[1] = u[2] = 0.0;
  double gR[9];
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) gR[r * 3 + q] = dtr * Rg[r * 3 + q] - (double)w_trans * prm[3 + r] * u[q];
  for (int k = 0; k < 3; ++k) {
    double s = 0;
    for (int q = 0; q < 9; ++q) s += gR[q] * J[k * 9 + q];
    g[k] = s;
  }
  for (int r = 0; r < 3; ++r) g[3 + r] = -(double)w_trans * ((R[r * 3 + 0] * u[0] + R[r * 3 + 1] * u[1]) + R[r * 3 + 2] * u[2]);
  const double sc = l > (double)cut ? 0.5 * sqrt((double)cut / l) : 1.0;
  bool finite = true;
  for (int i = 0; i < 6; ++i) {
    g[i] *= sc;
    finite = finite && isfinite(g[i]);
  }
  if (!finite)
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
  return L;
}

// ---- the stages of a backward kernel that do not depend on its kind

// Zero the frame's fp64 accumulator gacc [3][N] and the mask words of all its hypotheses (every thread of the workgroup).
__device__ __forceinline__ void zero_frame(double* gacc, int N, unsigned long long* mw, int words, int tid, int threads) {
  for (int m = tid; m < N; m += threads) gacc[m] = gacc[N + m] = gacc[2 * N + m] = 0.0;
  for (int i = tid; i < words; i += threads) mw[i] = 0ull;
}

// The caller's gradient og [3][N] += the accumulator, rounded once (every thread of the workgroup).
__device__ __forceinline__ void flush_grad(float* og, const double* gacc, int N, int tid, int threads) {
  for (int i = tid; i < 3 * N; i += threads) og[i] += (float)gacc[i];
}

// dsacstar::softMax and dsacstar::entropy of a frame's scores (one lane): p_h to sProb and probs_out, the entropy to *entropy_out.
__device__ __forceinline__ void softmax_entropy(const double* scores, int hyps, double* sProb, double* probs_out, double* entropy_out) {
  double maxScore = 0;
  for (int i = 0; i < hyps; i++)
    if (i == 0 || scores[i] > maxScore) maxScore = scores[i];
  double sum = 0.0;
  for (int i = 0; i < hyps; i++) {
    sProb[i] = detm::exp_(scores[i] - maxScore);
    sum += sProb[i];
  }
  double ent = 0.0;
  for (int i = 0; i < hyps; i++) {
    sProb[i] /= sum;
    probs_out[i] = sProb[i];
    if (sProb[i] > 0) ent -= sProb[i] * log2(sProb[i]);
  }
  *entropy_out = ent;
}

// E = sum_h p_h loss_h in index order (one lane)
__device__ __forceinline__ double expected_loss(const double* sProb, const double* sLoss, int hyps) {
  double E = 0;
  for (int h = 0; h < hyps; ++h) E += sProb[h] * sLoss[h];
  return E;
}

// The hypothesis' dependence on its minimal set (one lane): gacc[c][cells[i]] += sum_q S[q] cols[3 i + c][q] for the three
// differentiated points i, S = d score-path / d hypothesis, cols = d hypothesis / d coordinate c of point i.
__device__ __forceinline__ void scatter_support(double* gacc, int N, const int cells[3], const double S[6], const double (*cols)[6]) {
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 3; ++c) {
      double v = 0;
      for (int q = 0; q < 6; ++q) v += S[q] * cols[i * 3 + c][q];
      gacc[c * N + cells[i]] += v;
    }
}

}  // namespace acez_loss
