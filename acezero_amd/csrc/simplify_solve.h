// simplify_solve.h -- the PLACEMENT step of the mesh simplification (include/acez.h section Q, step 6): from a cluster's quadric
// (A, b) and its mean to the cluster's vertex. Host + device, so that tests/simplify_probe.hip can run it on the CPU; the including
// units are compiled with -ffp-contract=off. Every expression is evaluated in the order written. All coordinates are relative to the
// cluster's cell centre.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "svd3.h"

namespace acez {

constexpr int SIMPLIFY_TERMS = 9;                  // A: xx, xy, xz, yy, yz, zz (0 .. 5), b: x, y, z (6 .. 8)
constexpr double SIMPLIFY_RANK_RATIO = 1e-3;       // a direction counts if its singular value exceeds this fraction of the largest

// One corner's term: the plane quadric of the face (a, b, c), its vertices relative to the cell centre of the cluster that takes it.
// n = (b - a) x (c - a), unnormalised (|n|^2 = 4 area^2 is the weight); A += n n^T, b += -(n . a) n, added to q in the order 0 .. 8.
__host__ __device__ inline void simplify_add_corner(const double* a, const double* b, const double* c, double* q) {
  const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  double n[3];
  cross3(e1, e2, n);
  const double d = -dot3(n, a);
  q[0] = q[0] + n[0] * n[0];
  q[1] = q[1] + n[0] * n[1];
  q[2] = q[2] + n[0] * n[2];
  q[3] = q[3] + n[1] * n[1];
  q[4] = q[4] + n[1] * n[2];
  q[5] = q[5] + n[2] * n[2];
  q[6] = q[6] + d * n[0];
  q[7] = q[7] + d * n[1];
  q[8] = q[8] + d * n[2];
}

// x = mean + sum over the kept directions i (s_i > 1e-3 s_0, in the order 0, 1, 2) of v_i (v_i . (-b - A mean)) / s_i. false, and x =
// mean, if A is zero (or not a number), if x is not finite, or if a component of x lies more than `cell` from the centre.
__host__ __device__ inline bool simplify_solve(const double* q, const double* mean, double cell, double* x) {
  x[0] = mean[0]; x[1] = mean[1]; x[2] = mean[2];
  const double A[9] = {q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5]};
  Svd3 d;
  svd3(A, d);
  if (!(d.s[0] > 0.0)) return false;
  double r[3];
  for (int j = 0; j < 3; ++j) r[j] = -q[6 + j] - ((A[3 * j] * mean[0] + A[3 * j + 1] * mean[1]) + A[3 * j + 2] * mean[2]);
  const double least = SIMPLIFY_RANK_RATIO * d.s[0];
  double y[3] = {mean[0], mean[1], mean[2]};
  for (int i = 0; i < 3; ++i) {
    if (!(d.s[i] > least)) continue;
    const double step = dot3(d.v[i], r) / d.s[i];
    for (int j = 0; j < 3; ++j) y[j] = y[j] + d.v[i][j] * step;
  }
  for (int j = 0; j < 3; ++j)
    if (!isfinite(y[j]) || fabs(y[j]) > cell) return false;
  x[0] = y[0]; x[1] = y[1]; x[2] = y[2];
  return true;
}

}  // namespace acez
