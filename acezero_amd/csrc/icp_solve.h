// icp_solve.h -- the UPDATE step of the ICP loop (include/acez.h section N, ICP): from the 18 totals of one iteration to the record,
// the stopping rules and the Umeyama step on the device-resident state. Host + device, so that tests/icp_probe.hip can run it on the
// CPU; the including units are compiled with -ffp-contract=off. Every expression is evaluated in the order written.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "device_loop.h"
#include "svd3.h"

namespace acez {

constexpr int ICP_TERMS = 18;        // 1, a (3), b (3), b (x) a (9, row r of b, column c of a at 7 + 3 r + c), |a|^2, d2
constexpr int ICP_STATE = 34;        // doubles: device_loop.h's 16 (T, status, iterations, previous fitness, previous rmse), last totals (18)
constexpr int ICP_RECORD = LOOP_RECORD;   // T (12), count, sum d2, fitness, rmse
constexpr int ICP_PREV_FITNESS = 14, ICP_PREV_RMSE = 15;

// The Umeyama step on the totals s: T <- Delta * T with Delta(x') = scale R (x' - pivot - mean a) + mean b + pivot. false, and T
// untouched, if the correspondences do not determine it: fewer than 3, a total that is not finite, the covariance's second singular
// value <= 1e-12 x its first, or (with_scale) a scale that is not a positive finite number.
__host__ __device__ inline bool icp_solve(const double* s, const double* pivot, int with_scale, double* T) {
  const double count = s[0];
  if (!(count >= 3.0)) return false;
  for (int i = 0; i < ICP_TERMS; ++i)
    if (!isfinite(s[i])) return false;
  double C[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[r * 3 + c] = s[7 + 3 * r + c] - s[4 + r] * s[1 + c] / count;
  Svd3 d;
  svd3(C, d);   // u2 = u0 x u1, v2 = v0 x v1, s[2] signed: U V^T is U diag(1, 1, sign) V^T of the unsigned SVD, s[2] is sign * sigma2
  if (!(d.s[1] > 1e-12 * d.s[0])) return false;
  double scale = 1.0;
  if (with_scale) {
    const double var = s[16] - ((s[1] * s[1] + s[2] * s[2]) + s[3] * s[3]) / count;
    scale = ((d.s[0] + d.s[1]) + d.s[2]) / var;
    if (!(isfinite(scale) && scale > 0.0)) return false;
  }
  double M[9], shift[3], Tn[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[r * 3 + c] = scale * ((d.u[0][r] * d.v[0][c] + d.u[1][r] * d.v[1][c]) + d.u[2][r] * d.v[2][c]);
  const double am[3] = {s[1] / count + pivot[0], s[2] / count + pivot[1], s[3] / count + pivot[2]};
  const double bm[3] = {s[4] / count + pivot[0], s[5] / count + pivot[1], s[6] / count + pivot[2]};
  for (int r = 0; r < 3; ++r) shift[r] = bm[r] - ((M[r * 3] * am[0] + M[r * 3 + 1] * am[1]) + M[r * 3 + 2] * am[2]);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      const double v = (M[r * 3] * T[c] + M[r * 3 + 1] * T[4 + c]) + M[r * 3 + 2] * T[8 + c];
      Tn[r * 4 + c] = c == 3 ? v + shift[r] : v;
    }
  for (int i = 0; i < 12; ++i)
    if (!isfinite(Tn[i])) return false;
  for (int i = 0; i < 12; ++i) T[i] = Tn[i];
  return true;
}

// One UPDATE on a running state (the caller has checked status and iteration count): the record, rule (a), rule (b), the step.
__host__ __device__ inline void icp_update(double* state, const double* totals, int64_t n, const double* pivot, int with_scale,
                                           double rel_fitness, double rel_rmse, double* history) {
  const int64_t it = (int64_t)state[LOOP_COUNT];
  const double count = totals[0], sum_d2 = totals[17];
  const double fitness = count / (double)n, rmse = sqrt(sum_d2 / count);
  double* rec = history + it * ICP_RECORD;
  for (int i = 0; i < 12; ++i) rec[i] = state[i];
  rec[12] = count;
  rec[13] = sum_d2;
  rec[14] = fitness;
  rec[15] = rmse;
  const double prev_fitness = state[ICP_PREV_FITNESS], prev_rmse = state[ICP_PREV_RMSE];
  state[LOOP_COUNT] = (double)(it + 1);
  state[ICP_PREV_FITNESS] = fitness;
  state[ICP_PREV_RMSE] = rmse;
  for (int i = 0; i < ICP_TERMS; ++i) state[LOOP_TOTALS + i] = totals[i];
  if (it >= 1 && fabs(fitness - prev_fitness) < rel_fitness && fabs(rmse - prev_rmse) < rel_rmse) {
    state[LOOP_STATUS] = LOOP_CONVERGED;
    return;
  }
  if (!icp_solve(totals, pivot, with_scale, state)) state[LOOP_STATUS] = LOOP_DEGENERATE;
}

}  // namespace acez
