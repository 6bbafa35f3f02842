// svd3.h -- the deterministic 3x3 SVD shared by the pose evaluation (align_api.hip) and the RGB-D registration
// (ransac_rgbd.hip). Host + device; the including units are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace acez {

struct Svd3 {
  double u[3][3];  // columns u_i (u[i] is column i)
  double v[3][3];  // columns v_i
  double s[3];     // descending; s[2] is signed: u3 . (C v3) with u3 = u0 x u1, v3 = v0 x v1
};

__host__ __device__ inline void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// A 3-vector orthogonal to unit a (used only when the column space is rank deficient)
__host__ __device__ inline void any_orthogonal(const double* a, double* out) {
  double e[3] = {0.0, 0.0, 0.0};
  const double ax = fabs(a[0]), ay = fabs(a[1]), az = fabs(a[2]);
  e[(ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2)] = 1.0;
  double c[3];
  cross3(a, e, c);
  const double n = sqrt(dot3(c, c));
  out[0] = c[0] / n; out[1] = c[1] / n; out[2] = c[2] / n;
}

// C (row-major 3x3) = U diag(s) V^T, one-sided Jacobi.  Deterministic: a fixed sweep order and a fixed sweep cap.
__host__ __device__ inline void svd3(const double C[9], Svd3& o) {
  double b[3][3], v[3][3];   // b[i] = column i of C V, v[i] = column i of V
  for (int i = 0; i < 3; ++i)
    for (int r = 0; r < 3; ++r) {
      b[i][r] = C[r * 3 + i];
      v[i][r] = (r == i) ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 12; ++sweep) {
    bool rotated = false;
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double al = dot3(b[p], b[p]), be = dot3(b[q], b[q]), ga = dot3(b[p], b[q]);
      if (!(fabs(ga) > 2.220446049250313e-16 * sqrt(al * be))) continue;   // columns orthogonal to working precision
      rotated = true;
      const double zeta = (be - al) / (2.0 * ga);
      const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
      for (int r = 0; r < 3; ++r) {
        const double bp = b[p][r], bq = b[q][r];
        b[p][r] = c * bp - s * bq;
        b[q][r] = s * bp + c * bq;
        const double vp = v[p][r], vq = v[q][r];
        v[p][r] = c * vp - s * vq;
        v[q][r] = s * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  double n[3];
  for (int i = 0; i < 3; ++i) n[i] = sqrt(dot3(b[i], b[i]));
  int ord[3] = {0, 1, 2};   // descending by norm, stable
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (n[ord[j]] < n[ord[j + 1]]) { const int x = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = x; }
  for (int k = 0; k < 2; ++k)
    for (int r = 0; r < 3; ++r) o.v[k][r] = v[ord[k]][r];
  cross3(o.v[0], o.v[1], o.v[2]);
  o.s[0] = n[ord[0]];
  o.s[1] = n[ord[1]];
  if (o.s[0] > 0.0) {
    for (int r = 0; r < 3; ++r) o.u[0][r] = b[ord[0]][r] / o.s[0];
  } else {
    o.u[0][0] = 1.0; o.u[0][1] = 0.0; o.u[0][2] = 0.0;
  }
  if (o.s[1] > 0.0) {
    for (int r = 0; r < 3; ++r) o.u[1][r] = b[ord[1]][r] / o.s[1];
  } else {
    // rank <= 1: LAPACK completes the basis with some orthonormal vector; R is not unique here (a declared deviation)
    if (o.s[0] > 0.0) any_orthogonal(o.u[0], o.u[1]);
    else { o.u[1][0] = 0.0; o.u[1][1] = 1.0; o.u[1][2] = 0.0; }
  }
  cross3(o.u[0], o.u[1], o.u[2]);
  double cv[3];
  for (int r = 0; r < 3; ++r) cv[r] = C[r * 3 + 0] * o.v[2][0] + C[r * 3 + 1] * o.v[2][1] + C[r * 3 + 2] * o.v[2][2];
  o.s[2] = dot3(o.u[2], cv);
}

}  // namespace acez
