// track_solve.h -- the UPDATE step of the frame-to-model tracking loop (include/acez.h section K3): from the 29 totals of one iteration
// of one frame to the record, the stopping rules and the damped Gauss-Newton step on the device-resident state. Host + device, so that
// tests/track_probe.hip can run it on the CPU; the including units are compiled with -ffp-contract=off. Every expression is evaluated
// in the order written, and only +, -, *, / and sqrt occur: the device, the host and numpy give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "device_loop.h"

namespace acez {

constexpr int TRACK_TERMS = 29;      // 1, the upper triangle of J J^T row-major (21), J r (6), r^2
constexpr int TRACK_STATE = 45;      // doubles: device_loop.h's 16 (pose, status, records, previous count, previous rms), last totals (29)
constexpr int TRACK_RECORD = LOOP_RECORD;   // pose (12), count, sum r^2, rms, the status after this update
constexpr int TRACK_PREV_COUNT = 14, TRACK_PREV_RMS = 15;
constexpr int TRACK_H = 1, TRACK_B = 22, TRACK_R2 = 28;

// The step on the totals s: pose <- (R_delta R, t + u) with (u, omega) = -(H + damping * (trace(H) / 6) * I)^-1 b. false, and the pose
// untouched, if a pivot of the Cholesky factorisation is <= 1e-12 x the largest diagonal entry, or the new pose is not finite.
__host__ __device__ inline bool track_solve(const double* s, double damping, double* pose) {
  double L[6][6];
  int at = TRACK_H;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      L[i][j] = s[at];
      L[j][i] = s[at];
      ++at;
    }
  const double trace = ((((L[0][0] + L[1][1]) + L[2][2]) + L[3][3]) + L[4][4]) + L[5][5];
  const double lambda = damping * (trace / 6.0);
  double largest = 0.0;
  for (int i = 0; i < 6; ++i) {
    L[i][i] = L[i][i] + lambda;
    largest = L[i][i] > largest ? L[i][i] : largest;
  }
  // Cholesky in place, column by column: L[i][j], i >= j, becomes the factor
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
    for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
    if (!(d > 1e-12 * largest)) return false;
    const double root = sqrt(d);
    L[j][j] = root;
    for (int i = j + 1; i < 6; ++i) {
      double v = L[i][j];
      for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
      L[i][j] = v / root;
    }
  }
  double y[6], x[6];
  for (int i = 0; i < 6; ++i) {
    double v = s[TRACK_B + i];
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
    x[i] = v / L[i][i];
  }
  const double u[3] = {-x[0], -x[1], -x[2]};
  // Cayley: the unit quaternion (1, omega / 2) / |(1, omega / 2)|
  const double hx = -x[3] / 2.0, hy = -x[4] / 2.0, hz = -x[5] / 2.0;
  const double norm = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
  const double qw = 1.0 / norm, qx = hx / norm, qy = hy / norm, qz = hz / norm;
  const double D[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                       2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                       2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
  double out[12];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[4 * r + c] = (D[3 * r] * pose[c] + D[3 * r + 1] * pose[4 + c]) + D[3 * r + 2] * pose[8 + c];
    out[4 * r + 3] = pose[4 * r + 3] + u[r];
  }
  for (int i = 0; i < 12; ++i)
    if (!isfinite(out[i])) return false;
  for (int i = 0; i < 12; ++i) pose[i] = out[i];
  return true;
}

// One UPDATE on a running state (the caller has checked status and record count): the record, rule (a), rule (b), the step.
__host__ __device__ inline void track_update(double* state, const double* totals, double rel_rms, double damping, double min_count,
                                             double* history) {
  const int64_t it = (int64_t)state[LOOP_COUNT];
  const double count = totals[0], sum_r2 = totals[TRACK_R2];
  const double rms = count > 0.0 ? sqrt(sum_r2 / count) : 0.0;
  double* rec = history + it * TRACK_RECORD;
  for (int i = 0; i < 12; ++i) rec[i] = state[i];
  rec[12] = count;
  rec[13] = sum_r2;
  rec[14] = rms;
  const double prev_rms = state[TRACK_PREV_RMS];
  state[LOOP_COUNT] = (double)(it + 1);
  state[TRACK_PREV_COUNT] = count;
  state[TRACK_PREV_RMS] = rms;
  for (int i = 0; i < TRACK_TERMS; ++i) state[LOOP_TOTALS + i] = totals[i];
  double status = LOOP_RUNNING;
  bool finite = true;
  for (int i = 0; i < TRACK_TERMS; ++i) finite = finite && isfinite(totals[i]);
  if (it >= 1 && fabs(rms - prev_rms) < rel_rms)
    status = LOOP_CONVERGED;
  else if (!finite || count < min_count || !track_solve(totals, damping, state))
    status = LOOP_DEGENERATE;
  state[LOOP_STATUS] = status;
  rec[15] = status;
}

}  // namespace acez
