// ransac_grad.hip -- the DSAC* RGB-D backward pass on gfx950 (the reference's commented-out dsacstar_rgbd_backward,
// dsacstar/dsacstar.cpp:642-895, with dSMScoreRGBD / dScoreRGBD of dsacstar_derivative.h, loss / dLoss of dsacstar_loss.h and
// kabsch / dKabschFD of dsacstar_util_rgbd.h): the expected pose loss E = sum_h p_h loss_h of a frame and its gradient with respect
// to the scene coordinates. One 512-thread workgroup per frame, frames batched over the grid, fp64 geometry. Build with
// -ffp-contract=off.
//
//   sample, score   ransac_rgbd.h's stages, the forward kernel's code: for the same (seed, frame id) the same triples and poses.
//   soft-max        p_h = exp(s_h - max s) / sum (dsacstar::softMax), entropy - sum p log2 p (one lane).
//   refine          every hypothesis with p_h >= PROB_THRESH (0.001) in index order, with ransac_rgbd.h's refine (refineHypRGBD);
//                   its final inlier set is kept as a bitmask over the valid list (diagnostics). The others keep the sampled pose.
//   loss            loss(pose2trans(refined), gt): angular error in degrees + translation error of the camera centres, the soft
//                   clamp sqrt(cut * l) above cut, MAXLOSS. E = sum_h p_h loss_h in index order.
//   path I          p_h dLoss/dHyp_h dHyp_h/dObj as a vector-Jacobian product through the Kabsch fit of the final inlier set:
//                   the rotation's gradient is carried in the body frame (w = Jr dr, Jr from rodrigues' dR/dr), projected onto the
//                   SVD of the covariance (dR = U Omega V^T, Omega_ij = (G_ij - G_ji) / (s_i + s_j) with the signed third singular
//                   value) and pushed back to each inlier as B (e_k - mean e) - R^T g_t / n. Where s_1 + s_2 <= 1e-6 s_0 the fit is
//                   degenerate and the product is taken from central differences of Kabsch instead (eps 0.001; the covariance is
//                   updated in rank one per coordinate, so each difference costs one 3x3 SVD).
//   path II         dE/ds_h = p_h (loss_h - E), times ds_h/dObj: every valid cell's own error with the hypothesis held fixed, plus the
//                   hypothesis' dependence on its three sampled cells (the 6 x 9 Kabsch Jacobian, forward mode, zeroed when an
//                   entry exceeds 10 as in dScoreRGBD).
//   accumulate      a per-frame fp64 map of [3][H][W] in HBM; each cell is owned by one thread, hypotheses are added in index order
//                   (path I for all, then path II for all), the support cells by lane 0 between barriers: no atomics, the same bits
//                   on every run. The map is added once, rounded to float, into the caller's gradient (the reference's +=).
// Declared deviations from the reference: exact derivatives where the reference's differ from its own loss and score
// (the score's distance is in centimetres, so its derivative carries the factor 100 that dTransformdObj / dTransformdHyp omit; the
// soft clamp's derivative is 0.5 sqrt(cut / l), where dLoss has 0.5 / sqrt(l)); fp64 throughout; the Jacobian of Kabsch is exact
// whenever s_1 + s_2 > 1e-6 s_0 (the reference falls back to differences when any two singular values are within 1e-6); one fp64
// accumulation rounded once instead of a float += per hypothesis.
#include <hip/hip_runtime.h>
#include "ransac_math.h"
#include "acez_common.h"
#include "ransac_ctx.h"
#include "ransac_rgbd.h"
#include "ransac_loss.h"

namespace {

using namespace acez_rgbd;
using namespace acez_loss;

struct GradArgs {
  RgbdIn in;
  acez_rs::GradOut grad;   // the masks are over the valid list
};

__host__ __device__ inline size_t tail_bytes(int hyps) { return 8 * (size_t)(8 * hyps + 16); }
__host__ __device__ inline size_t lds_bytes(int Npad, int hyps, bool lists_in_hbm) {
  return (lists_in_hbm ? 0 : 26 * (size_t)Npad) + ((region_bytes(hyps) + 7) & ~(size_t)7) + tail_bytes(hyps);
}

// The Kabsch fit (rv, t) of covariance C = sum Xc Ec^T and centroids mX, mE, differentiated. Jvp: the change of (rv, t) when point k's
// scene coordinate moves along e_c (k's centred camera coordinate ec, n points). Degenerate (s_1 + s_2 <= 1e-6 s_0): central
// differences of Kabsch with the rank-one update of C. Returns false if the column is not finite or a fit fails.
struct KabschDiff {
  acez::Svd3 d;
  double R[9];       // V U^T
  double Jr[9];      // body Jacobian at rodrigues(rv)
  double C[9], mX[3], mE[3];
  double n;
  bool degenerate;
};

__device__ __forceinline__ bool kabsch_setup(const double C[9], const double mX[3], const double mE[3], double n, KabschDiff& k) {
  double rv[3], t[3];
  if (!kabsch(C, mX, mE, rv, t, &k.d)) return false;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) k.R[r * 3 + c] = k.d.v[0][r] * k.d.u[0][c] + k.d.v[1][r] * k.d.u[1][c] + k.d.v[2][r] * k.d.u[2][c];
  double Rr[9], J[27];
  rsm::rodrigues(rv, Rr, J);
  body_jacobian(Rr, J, k.Jr);
  for (int i = 0; i < 9; ++i) k.C[i] = C[i];
  for (int i = 0; i < 3; ++i) { k.mX[i] = mX[i]; k.mE[i] = mE[i]; }
  k.n = n;
  k.degenerate = !(k.d.s[1] + k.d.s[2] > 1e-6 * k.d.s[0]);
  return true;
}

__device__ __forceinline__ bool kabsch_fd_column(const KabschDiff& k, const double ec[3], int c, double col[6]) {
  double pose[2][6];
  for (int sgn = 0; sgn < 2; ++sgn) {
    const double e = sgn == 0 ? FD_EPS : -FD_EPS;
    double C[9], mX[3] = {k.mX[0], k.mX[1], k.mX[2]};
    for (int i = 0; i < 9; ++i) C[i] = k.C[i];
    for (int q = 0; q < 3; ++q) C[c * 3 + q] += e * ec[q];
    mX[c] += e / k.n;
    if (!kabsch(C, mX, k.mE, pose[sgn], pose[sgn] + 3)) return false;
  }
  bool ok = true;
  for (int i = 0; i < 6; ++i) {
    col[i] = (pose[0][i] - pose[1][i]) / (2 * FD_EPS);
    ok = ok && isfinite(col[i]);
  }
  return ok;
}

__device__ __forceinline__ bool kabsch_jvp(const KabschDiff& k, const double ec[3], int c, double col[6]) {
  if (k.degenerate) return kabsch_fd_column(k, ec, c, col);
  const double* s = k.d.s;
  double a[3], b[3];   // G = a b^T with a = V_c^T ec, b = U_c^T e_c
  for (int i = 0; i < 3; ++i) {
    a[i] = (k.d.v[i][0] * ec[0] + k.d.v[i][1] * ec[1]) + k.d.v[i][2] * ec[2];
    b[i] = k.d.u[i][c];
  }
  const double om[3] = {(a[2] * b[1] - a[1] * b[2]) / (s[2] + s[1]), (a[0] * b[2] - a[2] * b[0]) / (s[0] + s[2]),
                        (a[1] * b[0] - a[0] * b[1]) / (s[1] + s[0])};
  double w[3];
  for (int r = 0; r < 3; ++r) w[r] = (k.d.u[0][r] * om[0] + k.d.u[1][r] * om[1]) + k.d.u[2][r] * om[2];
  if (!solve3(k.Jr, w, col)) return false;
  double wx[3];
  cross(w, k.mX, wx);
  wx[c] += 1.0 / k.n;
  for (int r = 0; r < 3; ++r) col[3 + r] = -((k.R[r * 3 + 0] * wx[0] + k.R[r * 3 + 1] * wx[1]) + k.R[r * 3 + 2] * wx[2]);
  bool ok = true;
  for (int i = 0; i < 6; ++i) ok = ok && isfinite(col[i]);
  return ok;
}

template <bool GC>
__global__ __launch_bounds__(THREADS, 1) void rgbd_grad_kernel(GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const RgbdIn& in = a.in;
  const int frame = blockIdx.x;
  Frame f = frame_layout<GC>(in, smem_raw, frame);
  const int hyps = in.hyps, N = in.N;
  double* sProb = reinterpret_cast<double*>(f.tail);   // [hyps]
  double* sLoss = sProb + hyps;                         // [hyps]
  double* sRef = sLoss + hyps;                          // [hyps][6]
  double* sHand = sRef + 6 * hyps;                      // [16] lane 0 -> workgroup
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t frame_id = in.fp[frame].frame_id;
  const acez_rs::GradOut& go = a.grad;
  const float* G = go.gt + (size_t)frame * 16;
  double* gacc = go.gacc + (size_t)frame * 3 * N;
  unsigned long long* mw = go.masks + (size_t)frame * hyps * go.mwords;

  zero_frame(gacc, N, mw, hyps * go.mwords, tid, THREADS);
  compact_valid(in, f, frame, nullptr);
  const int nv = f.nv;
  const int vrows = (nv + THREADS - 1) / THREADS;

  if (nv < 3) {   // as the forward kernel: zero poses, equal scores, no gradient
    for (int h = tid; h < hyps; h += THREADS) {
      const size_t o = (size_t)frame * hyps + h;
      for (int i = 0; i < 6; ++i) in.hyp_poses[o * 6 + i] = go.ref_poses[o * 6 + i] = 0.0;
      for (int i = 0; i < 3; ++i) in.samples[o * 3 + i] = -1;
      in.scores[o] = 0.0;
    }
    if (tid == 0) {
      const double zero[6] = {0, 0, 0, 0, 0, 0};
      const double L = pose_loss(zero, G, go.w_rot, go.w_trans, go.cut, nullptr);
      for (int h = 0; h < hyps; ++h) {
        go.probs[(size_t)frame * hyps + h] = 1.0 / hyps;
        go.losses[(size_t)frame * hyps + h] = L;
      }
      go.entropy[frame] = log2((double)hyps);
      go.out_loss[frame] = L;
    }
    return;
  }
  sample_hyps(in, f, frame_id);
  score_hyps(in, f, frame);

  // ---- soft-max and entropy
  if (tid == 0) softmax_entropy(f.sScores, hyps, sProb, go.probs + (size_t)frame * hyps, go.entropy + frame);
  __syncthreads();

  // ---- refine, loss, path I: hypothesis by hypothesis
  for (int h = 0; h < hyps; ++h) {
    const double p = sProb[h];
    const bool active = p >= PROB_THRESH;
    double param[6];
    for (int i = 0; i < 6; ++i) param[i] = f.sHyp[h * 6 + i];
    Refined rf{0u, 3, false};
    if (active) rf = refine(in, f, param);
    if (active && rf.have_map) {
      for (int k = 0; k < vrows; ++k) {
        const unsigned long long bits = __ballot((rf.acc_flags >> k) & 1u);
        if (lane == 0) mw[(size_t)h * go.mwords + k * WAVES + wave] = bits;
      }
    }
    double g6[6];
    const double L = pose_loss(param, G, go.w_rot, go.w_trans, go.cut, active ? g6 : nullptr);
    if (tid == 0) {
      sLoss[h] = L;
      const size_t o = (size_t)frame * hyps + h;
      go.losses[o] = L;
      for (int i = 0; i < 6; ++i) go.ref_poses[o * 6 + i] = sRef[h * 6 + i] = param[i];
    }
    if (!(active && rf.have_map)) continue;

    // the Kabsch fit of the final inlier set, differentiated (a uniform branch: every thread holds the same sums)
    double s1[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < vrows; ++k) {
      if (!((rf.acc_flags >> k) & 1u)) continue;
      const int j = tid + THREADS * k;
      s1[0] += 1.0;
      s1[1] += f.sx[j]; s1[2] += f.sy[j]; s1[3] += f.sz[j];
      s1[4] += f.ex[j]; s1[5] += f.ey[j]; s1[6] += f.ez[j];
    }
    block_sum(s1, f.sRed, lane, wave);
    const double mX[3] = {s1[1] / s1[0], s1[2] / s1[0], s1[3] / s1[0]};
    const double mE[3] = {s1[4] / s1[0], s1[5] / s1[0], s1[6] / s1[0]};
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < vrows; ++k) {
      if (!((rf.acc_flags >> k) & 1u)) continue;
      const int j = tid + THREADS * k;
      const double xc[3] = {f.sx[j] - mX[0], f.sy[j] - mX[1], f.sz[j] - mX[2]};
      const double ec[3] = {f.ex[j] - mE[0], f.ey[j] - mE[1], f.ez[j] - mE[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[r * 3 + c] += xc[r] * ec[c];
    }
    block_sum(C, f.sRed, lane, wave);
    KabschDiff kd;
    if (!kabsch_setup(C, mX, mE, s1[0], kd)) continue;
    for (int i = 0; i < 6; ++i) g6[i] *= p;
    // vector-Jacobian product: the body-frame rotation gradient gw = Jr^-T g_r - mX x (R^T g_t)
    double JrT[9], gw[3], Rtg[3], xg[3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) JrT[r * 3 + c] = kd.Jr[c * 3 + r];
    if (!solve3(JrT, g6, gw)) continue;
    for (int r = 0; r < 3; ++r) Rtg[r] = (kd.R[0 * 3 + r] * g6[3] + kd.R[1 * 3 + r] * g6[4]) + kd.R[2 * 3 + r] * g6[5];
    cross(mX, Rtg, xg);
    for (int r = 0; r < 3; ++r) gw[r] -= xg[r];
    double B[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!kd.degenerate) {
      const double* s = kd.d.s;
      double q[3];
      for (int i = 0; i < 3; ++i) q[i] = (kd.d.u[i][0] * gw[0] + kd.d.u[i][1] * gw[1]) + kd.d.u[i][2] * gw[2];
      double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      A[2 * 3 + 1] = q[0] / (s[2] + s[1]); A[1 * 3 + 2] = -A[2 * 3 + 1];
      A[0 * 3 + 2] = q[1] / (s[0] + s[2]); A[2 * 3 + 0] = -A[0 * 3 + 2];
      A[1 * 3 + 0] = q[2] / (s[1] + s[0]); A[0 * 3 + 1] = -A[1 * 3 + 0];
      // B = U_c A^T V_c^T: the gradient of a point is B ec - R^T g_t / n
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          double v = 0;
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) v += kd.d.u[i][r] * A[j * 3 + i] * kd.d.v[j][c];
          B[r * 3 + c] = v;
        }
    }
    for (int k = 0; k < vrows; ++k) {
      if (!((rf.acc_flags >> k) & 1u)) continue;
      const int j = tid + THREADS * k;
      const int m = f.cell[j];
      const double ec[3] = {f.ex[j] - mE[0], f.ey[j] - mE[1], f.ez[j] - mE[2]};
      double gx[3];
      if (!kd.degenerate) {
        for (int r = 0; r < 3; ++r) gx[r] = ((B[r * 3 + 0] * ec[0] + B[r * 3 + 1] * ec[1]) + B[r * 3 + 2] * ec[2]) - Rtg[r] / s1[0];
      } else {
        for (int c = 0; c < 3; ++c) {
          double col[6];
          gx[c] = 0.0;
          if (!kabsch_fd_column(kd, ec, c, col)) continue;
          for (int i = 0; i < 6; ++i) gx[c] += g6[i] * col[i];
        }
      }
      for (int c = 0; c < 3; ++c) gacc[c * N + m] += gx[c];
    }
  }
  __syncthreads();

  // ---- the expected loss
  if (tid == 0) {
    const double E = expected_loss(sProb, sLoss, hyps);
    sHand[0] = E;
    go.out_loss[frame] = E;
  }
  __syncthreads();
  const double E = sHand[0];

  // ---- path II: dE/ds_h = p_h (loss_h - E), through every valid cell's error and the hypothesis' three sampled cells
  const float inlierBeta = 5 / in.thr;
  const float score_scale = in.alpha / (float)in.W / (float)in.H;
  for (int h = 0; h < hyps; ++h) {
    const double p = sProb[h];
    if (!(p >= PROB_THRESH)) continue;
    const double sg = p * (sLoss[h] - E);
    double prm[6], R[9], J[27];
    for (int i = 0; i < 6; ++i) prm[i] = f.sHyp[h * 6 + i];
    rsm::rodrigues(prm, R, J);
    double s6[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < vrows; ++k) {
      const int j = tid + THREADS * k;
      if (j >= nv) break;
      const double X[3] = {f.sx[j], f.sy[j], f.sz[j]};
      double d[3];   // eye - (R X + t) in fp64
      d[0] = (double)f.ex[j] - (((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + prm[3]);
      d[1] = (double)f.ey[j] - (((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + prm[4]);
      d[2] = (double)f.ez[j] - (((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + prm[5]);
      const double err = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      if (!(err * 100 <= (double)in.max_dist) || !(err > 0.0)) continue;   // clamped: no derivative
      const float e = dist_err(R, prm + 3, f.sx[j], f.sy[j], f.sz[j], f.ex[j], f.ey[j], f.ez[j], in.max_dist);
      const float beta_e = inlierBeta * (e - in.thr);
      if (beta_e > 40.f) continue;   // sigma' < 5e-18
      const double st = 1 / (1 + detm::exp_(-(double)beta_e));
      const double dD = -st * (1 - st) * (double)inlierBeta * sg * (double)score_scale;
      double gp[3];   // d err_cm / d (R X + t), times dD
      for (int r = 0; r < 3; ++r) gp[r] = dD * (-100.0 * d[r] / err);
      const int m = f.cell[j];
      for (int c = 0; c < 3; ++c) gacc[c * N + m] += (R[0 * 3 + c] * gp[0] + R[1 * 3 + c] * gp[1]) + R[2 * 3 + c] * gp[2];
      for (int kk = 0; kk < 3; ++kk) {
        const double* Jk = J + kk * 9;
        double v = 0;
        for (int r = 0; r < 3; ++r) v += gp[r] * ((Jk[r * 3 + 0] * X[0] + Jk[r * 3 + 1] * X[1]) + Jk[r * 3 + 2] * X[2]);
        s6[kk] += v;
      }
      for (int r = 0; r < 3; ++r) s6[3 + r] += gp[r];
    }
    block_sum(s6, f.sRed, lane, wave);
    if (tid == 0) {
      const float* sc = in.sc + (size_t)frame * 3 * N;
      const float* cc = in.cc + (size_t)frame * 3 * N;
      double X[3][3], Ec[3][3];
      int ms[3];
      for (int i = 0; i < 3; ++i) {
        ms[i] = f.sIdx[h * 3 + i];
        for (int c = 0; c < 3; ++c) {
          X[i][c] = (double)sc[(size_t)c * N + ms[i]];
          Ec[i][c] = (double)cc[(size_t)c * N + ms[i]];
        }
      }
      double mX[3], mE[3], C[9];
      triple_moments(X, Ec, mX, mE, C);
      KabschDiff kd;
      if (kabsch_setup(C, mX, mE, 3.0, kd)) {
        double cols[9][6];
        bool ok = true;
        double mx = 0;
        for (int i = 0; i < 3 && ok; ++i) {
          const double ec[3] = {Ec[i][0] - mE[0], Ec[i][1] - mE[1], Ec[i][2] - mE[2]};
          for (int c = 0; c < 3 && ok; ++c) {
            ok = kabsch_jvp(kd, ec, c, cols[i * 3 + c]);
            for (int q = 0; q < 6; ++q) mx = fmax(mx, fabs(cols[i * 3 + c][q]));
          }
        }
        if (ok && !(mx > 10)) scatter_support(gacc, N, ms, s6, cols);   // dScoreRGBD: an entry above 10 zeroes the support term
      }
    }
    __syncthreads();
  }

  // ---- the caller's gradient (+=)
  flush_grad(go.out_grad + (size_t)frame * 3 * N, gacc, N, tid, THREADS);
}

}  // namespace

// ====================================================================================================
// C ABI
// ====================================================================================================
extern "C" int acez_register_rgbd_backward_device(acez_ransac* ctx, const float* d_scene_coords, const float* d_camera_coords,
                                                  const float* d_gt_poses, int n_frames, int h, int w, const acez_ransac_params* params,
                                                  float w_loss_rot, float w_loss_trans, float soft_clamp, uint64_t seed,
                                                  const uint64_t* h_frame_ids, float* d_out_grad, double* d_out_loss, void* stream) {
  ACEZ_REQUIRE(ctx && d_scene_coords && d_camera_coords && d_gt_poses && params && d_out_grad && d_out_loss, "null pointer");
  int rc = acez_rs::check_frames(ctx, n_frames, h, w, params, false, "cells");
  if (rc != ACEZ_OK) return rc;
  ACEZ_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  acez_rs::GradWorkspace& gw = ctx->rgbd_grad;
  acez_rs::Geometry g;
  acez_rs::ParamSlot* slot = nullptr;
  rc = acez_rs::ensure_grad(gw, params->hypotheses, h * w);
  if (rc == ACEZ_OK) rc = acez_rs::plan_launch(gw.ws, h, w, params->hypotheses, 7, lds_bytes, &g);
  if (rc == ACEZ_OK) rc = acez_rs::stage_params(ctx, s, n_frames, nullptr, h_frame_ids, &slot);
  if (rc != ACEZ_OK) return rc;
  const GradArgs a{acez_rgbd::make_in(d_scene_coords, d_camera_coords, slot->d, gw.ws, g, h, w, params, seed),
                   acez_rs::make_grad_out(gw, h * w, d_gt_poses, w_loss_rot, w_loss_trans, soft_clamp, d_out_grad, d_out_loss)};
  rc = acez_rs::launch(rgbd_grad_kernel<true>, rgbd_grad_kernel<false>, g, n_frames, THREADS, s, a, *slot);
  if (rc == ACEZ_OK) acez_rs::note_launch(gw, params->hypotheses, h * w);
  return rc;
}

extern "C" int acez_register_rgbd_backward_host(acez_ransac* ctx, const float* h_scene_coords, int64_t sc_stride_c, int64_t sc_stride_h,
                                                int64_t sc_stride_w, const float* h_camera_coords, int64_t cc_stride_c,
                                                int64_t cc_stride_h, int64_t cc_stride_w, const float* h_gt_pose16, int h, int w,
                                                const acez_ransac_params* params, float w_loss_rot, float w_loss_trans,
                                                float soft_clamp, uint64_t seed, uint64_t frame_id, float* h_grad,
                                                int64_t g_stride_c, int64_t g_stride_h, int64_t g_stride_w, double* out_loss) {
  ACEZ_REQUIRE(ctx && h_scene_coords && h_camera_coords && h_gt_pose16 && params && h_grad && out_loss, "null pointer");
  ACEZ_REQUIRE(h > 0 && w > 0 && h <= ctx->max_h && w <= ctx->max_w, "frame larger than the context was created for");
  ACEZ_HIP_CHECK(hipSetDevice(ctx->device));
  acez_rs::GradWorkspace& gw = ctx->rgbd_grad;
  if (!ctx->d_cc) ACEZ_HIP_CHECK(hipMalloc((void**)&ctx->d_cc, (size_t)3 * ctx->max_h * ctx->max_w * sizeof(float)));
  int rc = acez_rs::ensure_grad(gw, params->hypotheses, h * w);
  if (rc == ACEZ_OK) rc = acez_rs::upload_strided(ctx->d_sc, h_scene_coords, sc_stride_c, sc_stride_h, sc_stride_w, h, w);
  if (rc == ACEZ_OK) rc = acez_rs::upload_strided(ctx->d_cc, h_camera_coords, cc_stride_c, cc_stride_h, cc_stride_w, h, w);
  if (rc != ACEZ_OK) return rc;
  auto launch = [&](const float* d_gt, float* d_grad, double* d_loss) {
    return acez_register_rgbd_backward_device(ctx, ctx->d_sc, ctx->d_cc, d_gt, 1, h, w, params, w_loss_rot, w_loss_trans, soft_clamp,
                                              seed, &frame_id, d_grad, d_loss, nullptr);
  };
  return acez_rs::backward_host(gw, h, w, h_gt_pose16, h_grad, g_stride_c, g_stride_h, g_stride_w, out_loss, launch);
}

extern "C" int acez_ransac_rgbd_backward_debug_fetch(acez_ransac* ctx, int n_frames, int hypotheses, int h, int w, int32_t* h_samples,
                                                     double* h_hyp_poses, double* h_scores, double* h_probs, double* h_losses,
                                                     double* h_ref_poses, uint64_t* h_mask_words, double* h_entropy) {
  ACEZ_REQUIRE(ctx && ctx->rgbd_grad.ws.d_best, "no RGB-D backward call on this context");
  return acez_rs::grad_debug_fetch(ctx, ctx->rgbd_grad, n_frames, hypotheses, h, w, h_samples, h_hyp_poses, h_scores, h_probs, h_losses,
                                   h_ref_poses, h_mask_words, h_entropy);
}
