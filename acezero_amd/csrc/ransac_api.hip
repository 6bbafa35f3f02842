// ransac_api.hip -- DSAC* RGB registration on gfx950: one 256-thread workgroup per frame, frames batched over
// the grid. Replaces dsacstar_rgb_forward (dsacstar/dsacstar.cpp:66-186). Build with -ffp-contract=off.
//
// Mapping of the reference's stages onto the workgroup (4 wavefronts):
//   load        the frame's H*W scene coordinates are staged ONCE into LDS (3 x N floats, pixel order
//               p = x*H + y, the reference's x-outer/y-inner scan order) with coalesced global reads
//   sample      sampleHypotheses (dsacstar_util.h:135-221): ONE HYPOTHESIS PER WAVEFRONT, the up-to-max_tries
//               minimal-set draws run 64 at a time on the lanes (each lane: 4 draws -> P3P -> 4-point check);
//               __ballot + first-set-bit picks the first accepted try = what the sequential loop would keep
//   score       getReproErrs + getHypScores (:316-343,:356-446): the same wavefront projects all N pixels of its
//               hypothesis from LDS, lane-strided fp64 partial sums, one butterfly (order 32,16,..,1)
//   select      softMax + draw(argmax) (:684-752) by one lane
//   refine      refineHyp (:522-597): all 256 threads. Every round classifies all pixels against the threshold and
//               COMPACTS the inliers into an LDS list in scan order -- the reference's own localImgPts / localObjPts
//               (:545-560) -- so that the Levenberg-Marquardt passes of solvePnP(ITERATIVE) (cvFindExtrinsicCameraParams2
//               + CvLevMarq) touch inliers only: list entry j belongs to thread j % 256, J^T J / J^T e / |e|^2 are
//               accumulated per thread, reduced inside each wavefront by a TRANSPOSING butterfly (v_permlane32_swap,
//               v_permlane16_swap, DPP: 28 sums cost 29 cross-lane steps instead of 168) and summed over the 4
//               wavefronts in a fixed order through LDS; the 6x6 solve runs on wavefront 0.
// Nothing is written to HBM between stages except the diagnostics (hypothesis poses / scores).
// Roofline: per frame 57.6 KB in, ~5 KB out; the kernel is fp64-VALU/latency bound.
// This unit also defines the registration host side that ransac_rgbd.hip and ransac_grad.hip share (ransac_ctx.h): the context, the
// per-estimator workspaces, the frame-parameter slot ring, the argument checks, the launch geometry, the host-buffer staging of the
// forward and backward entries and the debug fetches.
#include <hip/hip_runtime.h>
#include "ransac_math.h"
#include "acez_common.h"
#include "ransac_ctx.h"
#include "ransac_loss.h"
#include <new>
#include <vector>

namespace {

using rsm::Cam;
using rsm::Pose;
using rsm::div_h;

using acez_rs::FrameParam;

struct RansacArgs {
  const float* sc;  // [n][3][H][W]
  const FrameParam* fp;
  float* big;       // [n][3][Npad] transposed copies, only for frames that do not fit the LDS (GC instantiation)
  int H, W, N, hyps, max_tries, sub, max_ref_steps;
  uint32_t h_magic;  // ceil(2^32 / H): p / H == __umulhi(p, h_magic) for p < 2^16 (H >= 2)
  float thr, alpha, max_reproj;
  uint64_t seed;
  double* hyp_poses;  // [n][hyps][6]
  double* scores;     // [n][hyps]
  int* best;          // [n]
  double* refined;    // [n][6]
  float* out_poses;   // [n][16]
  int* out_inliers;   // [n]
  uint8_t* out_masks; // [n][H][W] or null
  // the backward pass only (GRAD instantiation)
  int* samples;                // [n][hyps][4] scan indices x * H + y of the kept minimal set
  acez_rs::GradOut grad;       // the masks are over all pixels
};

// ---- cross-lane sums of doubles without the LDS crossbar --------------------------------------------------------------------
// All of them realise the butterfly v_l + v_(l ^ off), off = 32, 16, 8, 4, 2, 1 (the order of oracle tree64): IEEE addition is
// commutative, so which partner supplies the left operand does not matter and every lane ends with the same bits.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
// a[32..63] <-> b[0..31]
__device__ __forceinline__ void swap_halves(double& a, double& b) {
  const u32x2 lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const u32x2 hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  a = __hiloint2double((int)hi.x, (int)lo.x);
  b = __hiloint2double((int)hi.y, (int)lo.y);
}
// odd 16-lane rows of a <-> even rows of b
__device__ __forceinline__ void swap_rows(double& a, double& b) {
  const u32x2 lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const u32x2 hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  a = __hiloint2double((int)hi.x, (int)lo.x);
  b = __hiloint2double((int)hi.y, (int)lo.y);
}
template <int CTRL, int BANK>
__device__ __forceinline__ double dpp_d(double old, double v) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, 0xf, BANK, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, 0xf, BANK, false);
  return __hiloint2double(hi, lo);
}
// offsets 8, 4, 2, 1 inside each row of 16 lanes
__device__ __forceinline__ double row_tree(double v) {
  v = v + dpp_d<0x128, 0xf>(v, v);          // row_ror:8 = lane ^ 8
  double t = dpp_d<0x104, 0x5>(v, v);        // row_shl:4 on lanes 0-3, 8-11 (read lane + 4)
  t = dpp_d<0x114, 0xa>(t, v);               // row_shr:4 on lanes 4-7, 12-15 (read lane - 4)  -> lane ^ 4
  v = v + t;
  v = v + dpp_d<0x4E, 0xf>(v, v);            // quad_perm [2,3,0,1] = lane ^ 2
  v = v + dpp_d<0xB1, 0xf>(v, v);            // quad_perm [1,0,3,2] = lane ^ 1
  return v;
}
__device__ __forceinline__ double wave_tree(double v) {
  double a = v, b = v;
  swap_halves(a, b);
  v = a + b;
  a = v; b = v;
  swap_rows(a, b);
  v = a + b;
  return row_tree(v);
}
// 28 sums at once: after the two swap levels row r of the wavefront works on quantities 7r .. 7r+6 only
__device__ __forceinline__ void wave_tree28(const double acc[28], double out7[7]) {
  double h[14];
#pragma unroll
  for (int j = 0; j < 14; ++j) {
    double a = acc[j], b = acc[14 + j];
    swap_halves(a, b);   // lanes < 32: (own acc[j], acc[j] of lane + 32); lanes >= 32: (acc[14 + j] of lane - 32, own acc[14 + j])
    h[j] = a + b;
  }
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    double a = h[j], b = h[7 + j];
    swap_rows(a, b);
    out7[j] = row_tree(a + b);
  }
}

// detm::exp_ with 32-bit integer steps (|x * INV_LN2| < 1100, so the int conversion, k / 2 and the exponent words are the same
// values as the 64-bit ones of det_math.h; every floating-point operation is identical)
__device__ __forceinline__ double exp_dev(double x) {
  if (x != x) return x;
  if (x > 709.0) return __hiloint2double(0x7ff00000, 0);
  if (x < -745.0) return 0.0;
  const double kf = x * detm::INV_LN2;
  const int k = (int)(kf + (kf >= 0 ? 0.5 : -0.5));
  const double kd = (double)k;
  const double r = (x - kd * detm::LN2_HI) - kd * detm::LN2_LO;
  const double p = (0x1.0000000000000p+0 + r * (0x1.0000000000000p+0 + r * (0x1.0000000000000p-1 + r * (0x1.5555555555555p-3 + r * (0x1.555555555555fp-5 + r * (0x1.1111111111114p-7 + r * (0x1.6c16c16c1321dp-10 + r * (0x1.a01a01a018130p-13 + r * (0x1.a01a01b4cf7bbp-16 + r * (0x1.71de3a60775bep-19 + r * (0x1.27e4beb6f974bp-22 + r * (0x1.ae6415b4ca760p-26 + r * (0x1.1f9e46dddd4e5p-29 + r * 0x1.61e0dace500bbp-33)))))))))))));
  const int k1 = k / 2, k2 = k - k1;
  return (p * __hiloint2double((k1 + 1023) << 20, 0)) * __hiloint2double((k2 + 1023) << 20, 0);
}

// reprojection error of one pixel exactly as getReproErrs stores it (float, clamped)
__device__ __forceinline__ float pixel_err(const double R[9], const double t[3], const Cam& k, float X, float Y, float Z, int pxx,
                                           int pyy, float max_reproj) {
  double u, v;
  rsm::project(R, t, k, X, Y, Z, &u, &v, nullptr, nullptr, nullptr);
  const float pu = (float)u, pv = (float)v;
  const float dx = (float)pxx - pu, dy = (float)pyy - pv;
  const double nrm = sqrt((double)dx * dx + (double)dy * dy);
  const float l = (float)nrm;
  return l < max_reproj ? l : max_reproj;
}

struct LMAccum {
  double JtJ[36], JtErr[6], errsq;
};

__device__ bool inv4x4(const double Ain[16], double out[16]) {
  double A[16], Bm[16];
  for (int i = 0; i < 16; ++i) {
    A[i] = Ain[i];
    Bm[i] = (i % 5 == 0) ? 1. : 0.;
  }
  const int m = 4, n = 4;
  for (int i = 0; i < m; i++) {
    int k = i;
    for (int j = i + 1; j < m; j++)
      if (fabs(A[j * m + i]) > fabs(A[k * m + i])) k = j;
    if (fabs(A[k * m + i]) < 2.220446049250313e-16 * 100) return false;
    if (k != i) {
      for (int j = i; j < m; j++) { const double tmp = A[i * m + j]; A[i * m + j] = A[k * m + j]; A[k * m + j] = tmp; }
      for (int j = 0; j < n; j++) { const double tmp = Bm[i * n + j]; Bm[i * n + j] = Bm[k * n + j]; Bm[k * n + j] = tmp; }
    }
    const double d = -1 / A[i * m + i];
    for (int j = i + 1; j < m; j++) {
      const double alpha = A[j * m + i] * d;
      for (int kk = i + 1; kk < m; kk++) A[j * m + kk] += alpha * A[i * m + kk];
      for (int kk = 0; kk < n; kk++) Bm[j * n + kk] += alpha * Bm[i * n + kk];
    }
  }
  for (int i = m - 1; i >= 0; i--)
    for (int j = 0; j < n; j++) {
      double s = Bm[i * n + j];
      for (int k = i + 1; k < m; k++) s -= A[i * m + k] * Bm[k * n + j];
      Bm[i * n + j] = s / A[i * m + i];
    }
  for (int i = 0; i < 16; ++i) out[i] = Bm[i];
  return true;
}

// ---- LDS layout (host and device agree through these helpers) ---------------------------------------------------------------
//   [3][Npad] float   scene coordinates in scan order (LDS instantiation only)
//   [Npad]    uint16  the current inlier list
//   region            one fp64 area used twice: while sampling / scoring / selecting it holds the scores [hyps] and the sampled
//                     poses [hyps][6]; both are dead once the best hypothesis is chosen, and the refinement reuses it for the LM
//                     step hand-over (6 doubles, padded to 8), the double-buffered reduction scratch [2][4][28] and the compaction
//                     counts [64][4] int. Keeping the two apart cost 1.8 KB more and, with 64 hypotheses, the second workgroup
//                     of a CU (round 1: 20 ms vs 12 ms).
//   [8] int           best hypothesis
// 60x80 (7-Scenes): 70.1 KB, 60x93 (Mip-NeRF 360 at 480 px): 81.7 KB with 64 hypotheses -> two workgroups per CU in both cases.
constexpr int MAX_ROWS = 64;                        // pixels per thread (inlier flags are one 64-bit word): N <= 16384
static_assert(acez_rs::RGB_THREADS * MAX_ROWS == acez_rs::MAX_CELLS, "check_frames' limit is this layout's");
constexpr int RED_DOUBLES = 8 + 2 * 4 * 28;         // step hand-over + reduction scratch
constexpr int REGION_MIN = RED_DOUBLES + MAX_ROWS * 4 / 2;
__host__ __device__ inline int region_doubles(int hyps) { return 7 * hyps > REGION_MIN ? 7 * hyps : REGION_MIN; }
__host__ __device__ inline size_t lds_bytes(int Npad, int hyps, bool coords_in_hbm) {
  return (coords_in_hbm ? 0 : 12 * (size_t)Npad) + 2 * (size_t)Npad + 8 * (size_t)region_doubles(hyps) + 8 * sizeof(int);
}
// the backward pass adds probabilities [hyps], losses [hyps] and 64 doubles of hand-over (the 6x6 pseudo-inverse, v, E, a max)
__host__ __device__ inline size_t grad_lds_bytes(int Npad, int hyps, bool coords_in_hbm) {
  return lds_bytes(Npad, hyps, coords_in_hbm) + 8 * (size_t)(2 * hyps + 64);
}

// GC: the frame does not fit the LDS (more than ~11 400 scene coordinates): its scan-order copy lives in an HBM workspace (L2
// resident, 12 N bytes) and every stage reads it from there; same arithmetic, same order, same bits.
// GRAD: the backward pass (dsacstar_rgb_backward) instead of the selection and the single refinement; the sampling, scoring and
// refinement code is the same.
template <bool GC, bool GRAD = false>
__global__ __launch_bounds__(256, 2) void ransac_kernel(RansacArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int N = a.N, H = a.H, W = a.W;
  const int Npad = (N + 3) & ~3;
  const int frame = blockIdx.x;
  float* sX = GC ? a.big + (size_t)frame * 3 * Npad : reinterpret_cast<float*>(smem_raw);
  float* sY = sX + Npad;
  float* sZ = sY + Npad;
  uint16_t* sList = reinterpret_cast<uint16_t*>(smem_raw + (GC ? 0 : 12 * (size_t)Npad));
  double* sRegion = reinterpret_cast<double*>(sList + Npad);
  double* sScores = sRegion;                              // [hyps]
  double* sHyp = sScores + a.hyps;                        // [hyps][6] sampled poses
  double* sRed = sRegion + 8;                             // [2][4][28] (refinement only)
  int* sCnt = reinterpret_cast<int*>(sRegion + RED_DOUBLES);   // [rows][4] (refinement only)
  int* sInt = reinterpret_cast<int*>(sRegion + region_doubles(a.hyps));   // [8]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const FrameParam fp = a.fp[frame];
  const Cam k{(double)fp.focal, (double)fp.focal, (double)fp.ppx, (double)fp.ppy};
  const float* sc = a.sc + (size_t)frame * 3 * N;
  const uint32_t magic = a.h_magic;
  const int half = a.sub / 2;

  // ---- load: memory order i = y*W + x  ->  scan order p = x*H + y
  for (int i = tid; i < N; i += 256) {
    const int y = i / W, x = i - y * W;
    const int p = x * H + y;
    sX[p] = sc[i];
    sY[p] = sc[N + i];
    sZ[p] = sc[2 * N + i];
  }
  __syncthreads();

  // ---- sample + score: hypothesis h on wavefront h % 4
  const float inlierBeta = 5 / a.thr;
  const float score_scale = a.alpha / (float)W / (float)H;
  // Sampling (dsacstar_util.h:135-221): the sequential loop keeps, per hypothesis, the FIRST try whose P3P pose passes the
  // 4-point check. Tries are independent draws of the counter-based stream, so they are evaluated in parallel and the first
  // accepted one is picked with a ballot: a wavefront works on 8 of its hypotheses at once, 8 tries each (lane = 8 * slot +
  // try); almost every hypothesis is settled by the first batch, so the whole workgroup needs ONE P3P latency for 32
  // hypotheses instead of eight. Hypothesis h lives on wavefront h % 4 (as does its scoring below).
  for (int pass = 0; wave + 4 * (8 * pass) < a.hyps; ++pass) {
    const int slot = lane >> 3, tr = lane & 7;
    const int h = wave + 4 * (8 * pass + slot);
    const bool hvalid = h < a.hyps;
    bool settled = !hvalid;   // of this lane's slot
    for (int t0 = 0; t0 < a.max_tries; t0 += 8) {
      if (__ballot(!settled) == 0ull) break;
      const int t = t0 + tr;
      Pose cur;
#pragma unroll
      for (int i = 0; i < 3; ++i) cur.r[i] = cur.t[i] = 0;
      int ps[4] = {0, 0, 0, 0};   // the draw's scan indices (kept by the backward pass)
      int status = 0;  // 0: PnP failed (zero pose), 1: solved but rejected by the 4-point check, 2: accepted
      if (!settled && t < a.max_tries) {
        const uint64_t key = rsm::try_key(a.seed, fp.frame_id, (uint32_t)h, (uint32_t)t);
        float obj[4][3], img[4][2];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int x = rsm::irand(key, 2 * j, W);
          const int y = rsm::irand(key, 2 * j + 1, H);
          img[j][0] = (float)(x * a.sub + half);
          img[j][1] = (float)(y * a.sub + half);
          const int p = x * H + y;
          ps[j] = p;
          obj[j][0] = sX[p];
          obj[j][1] = sY[p];
          obj[j][2] = sZ[p];
        }
        if (rsm::solve_pnp_p3p(obj, img, k, &cur)) {
          status = 2;
          double R[9];
          rsm::rodrigues(cur.r, R, nullptr);
          for (int j = 0; j < 4; j++) {
            double u, v;
            rsm::project(R, cur.t, k, obj[j][0], obj[j][1], obj[j][2], &u, &v, nullptr, nullptr, nullptr);
            const float dx = img[j][0] - (float)u, dy = img[j][1] - (float)v;
            if (sqrt((double)dx * dx + (double)dy * dy) < (double)a.thr) continue;
            status = 1;
            break;
          }
        } else {
#pragma unroll
          for (int i = 0; i < 3; ++i) cur.r[i] = cur.t[i] = 0;
        }
      }
      const unsigned long long ok = __ballot(status == 2);
      if (!settled) {
        const unsigned g = (unsigned)(ok >> (slot * 8)) & 0xffu;
        int src = -1;
        if (g) src = __ffs((int)g) - 1;                                  // first accepted try of this batch
        else if (t0 + 8 >= a.max_tries) src = a.max_tries - 1 - t0;      // every try failed: the last try's pose stays (:157-220)
        if (src >= 0) {
          settled = true;
          if (tr == src) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              sHyp[h * 6 + i] = cur.r[i];
              sHyp[h * 6 + 3 + i] = cur.t[i];
            }
            if constexpr (GRAD)
              for (int j = 0; j < 4; ++j) a.samples[((size_t)frame * a.hyps + h) * 4 + j] = ps[j];
          }
        }
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();   // the poses of this wave's hypotheses are written by its own lanes
  for (int h = wave; h < a.hyps; h += 4) {
    Pose res;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      res.r[i] = sHyp[h * 6 + i];
      res.t[i] = sHyp[h * 6 + 3 + i];
    }
    // score this hypothesis
    double R[9];
    rsm::rodrigues(res.r, R, nullptr);
    double acc = 0;
    for (int p = lane; p < N; p += 64) {
      const int x = div_h(p, H, magic), y = p - x * H;
      const float e = pixel_err(R, res.t, k, sX[p], sY[p], sZ[p], x * a.sub + half, y * a.sub + half, a.max_reproj);
      const float beta_e = inlierBeta * (e - a.thr);
      // beyond 40 the sigmoid is exactly 1 in fp64 (exp(-40) = 4e-18 < 2^-53, so 1 + exp(-x) == 1) and the pixel adds exactly +0:
      // far outliers -- nearly every pixel of a wrong hypothesis -- skip the exponential and the division
      if (beta_e > 40.f) continue;
      double softThreshold = beta_e;
      softThreshold = 1 / (1 + exp_dev(-softThreshold));
      acc += 1 - softThreshold;
    }
    double score = wave_tree(acc);
    score *= score_scale;
    if (lane == 0) {
      sScores[h] = score;
      double* hp = a.hyp_poses + ((size_t)frame * a.hyps + h) * 6;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        hp[i] = res.r[i];
        hp[3 + i] = res.t[i];
      }
      a.scores[(size_t)frame * a.hyps + h] = score;
    }
  }
  __syncthreads();

  const int rows = (N + 255) >> 8;  // thread tid looks at pixels p = tid + 256 i, i < rows (p < N)

  // bit i of the result: pixel tid + 256 i is an inlier of prm (getReproErrs + the threshold test of refineHyp, :536-560)
  auto classify = [&](const double* prm) -> uint64_t {
    double R[9];
    rsm::rodrigues(prm, R, nullptr);
    uint64_t flags = 0;
    for (int i = 0; i < rows; ++i) {
      const int p = tid + 256 * i;
      if (p >= N) break;
      const int x = div_h(p, H, magic), y = p - x * H;
      const float e = pixel_err(R, prm + 3, k, sX[p], sY[p], sZ[p], x * a.sub + half, y * a.sub + half, a.max_reproj);
      if (e < a.thr) flags |= 1ull << i;
    }
    return flags;
  };
  // the inliers in scan order (ascending p): counts per (row, wavefront) through LDS, positions from ballots. Returns their number.
  auto compact = [&](uint64_t flags) -> int {
    for (int i = 0; i < rows; ++i) {
      const unsigned long long m = __ballot((flags >> i) & 1ull);
      if (lane == 0) sCnt[i * 4 + wave] = __popcll(m);
    }
    __syncthreads();
    int run = 0;
    for (int i = 0; i < rows; ++i) {
      const bool f = (flags >> i) & 1ull;
      const unsigned long long m = __ballot(f);
      const int4 c = reinterpret_cast<const int4*>(sCnt)[i];
      const int base = run + (wave > 0 ? c.x : 0) + (wave > 1 ? c.y : 0) + (wave > 2 ? c.z : 0);
      const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      if (f) sList[base + below] = (uint16_t)(tid + 256 * i);
      run += (c.x + c.y) + (c.z + c.w);
    }
    __syncthreads();
    return run;
  };
  int red_parity = 0;
  // sums over the workgroup in the canonical order (oracle tree256); the 27 Jacobian sums are only read by wavefront 0, the one
  // that solves for the step; |e|^2 drives the control flow of every thread
  auto reduce28 = [&](double* acc, LMAccum* out) {
    double* buf = sRed + red_parity * (4 * 28);
    double r7[7];
    wave_tree28(acc, r7);
    if ((lane & 15) == 0) {
#pragma unroll
      for (int j = 0; j < 7; ++j) buf[wave * 28 + 7 * (lane >> 4) + j] = r7[j];
    }
    __syncthreads();
    if (wave == 0) {
      double s[27];
#pragma unroll
      for (int i = 0; i < 27; ++i) s[i] = ((buf[0 * 28 + i] + buf[1 * 28 + i]) + buf[2 * 28 + i]) + buf[3 * 28 + i];
      int q = 0;
#pragma unroll
      for (int aa = 0; aa < 6; ++aa)
#pragma unroll
        for (int bb = aa; bb < 6; ++bb) {
          out->JtJ[aa * 6 + bb] = s[q];
          out->JtJ[bb * 6 + aa] = s[q];
          ++q;
        }
#pragma unroll
      for (int aa = 0; aa < 6; ++aa) out->JtErr[aa] = s[21 + aa];
    }
    out->errsq = ((buf[0 * 28 + 27] + buf[1 * 28 + 27]) + buf[2 * 28 + 27]) + buf[3 * 28 + 27];
    red_parity ^= 1;
  };
  auto reduce1 = [&](double e) -> double {
    double* buf = sRed + red_parity * (4 * 28);
    const double v = wave_tree(e);
    if (lane == 0) buf[wave * 28 + 27] = v;
    __syncthreads();
    red_parity ^= 1;
    return ((buf[0 * 28 + 27] + buf[1 * 28 + 27]) + buf[2 * 28 + 27]) + buf[3 * 28 + 27];
  };
  // J^T J, J^T e and |e|^2 over the inlier list
  auto accumulate_J = [&](const double* prm, int cnt, LMAccum* out) {
    double R[9], dRdr[27];
    rsm::rodrigues(prm, R, dRdr);
    double acc[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0;
    for (int j = tid; j < cnt; j += 256) {
      const int p = sList[j];
      const int x = div_h(p, H, magic), y = p - x * H;
      double u, v, Ju[6], Jv[6];
      rsm::project(R, prm + 3, k, sX[p], sY[p], sZ[p], &u, &v, dRdr, Ju, Jv);
      const double eu = u - (double)(float)(x * a.sub + half), ev = v - (double)(float)(y * a.sub + half);
      int q = 0;
#pragma unroll
      for (int aa = 0; aa < 6; ++aa)
#pragma unroll
        for (int bb = aa; bb < 6; ++bb) {
          acc[q] = acc[q] + Ju[aa] * Ju[bb];
          acc[q] = acc[q] + Jv[aa] * Jv[bb];
          ++q;
        }
#pragma unroll
      for (int aa = 0; aa < 6; ++aa) {
        acc[21 + aa] = acc[21 + aa] + Ju[aa] * eu;
        acc[21 + aa] = acc[21 + aa] + Jv[aa] * ev;
      }
      acc[27] = acc[27] + eu * eu;
      acc[27] = acc[27] + ev * ev;
    }
    reduce28(acc, out);
  };
  // |e|^2 only (CvLevMarq's CHECK_ERR state)
  auto accumulate_E = [&](const double* prm, int cnt) -> double {
    double R[9];
    rsm::rodrigues(prm, R, nullptr);
    double acc = 0;
    for (int j = tid; j < cnt; j += 256) {
      const int p = sList[j];
      const int x = div_h(p, H, magic), y = p - x * H;
      double u, v;
      rsm::project(R, prm + 3, k, sX[p], sY[p], sZ[p], &u, &v, nullptr, nullptr, nullptr);
      const double eu = u - (double)(float)(x * a.sub + half), ev = v - (double)(float)(y * a.sub + half);
      acc = acc + eu * eu;
      acc = acc + ev * ev;
    }
    return reduce1(acc);
  };
  auto lm_step = [&](const LMAccum& acc, const double* prevParam, int lambdaLg10, double* prm) {
    // The 6x6 solve is serial fp64 work with identical inputs on every lane (Cholesky: ~2 us; its eigen fallback ~55 us): only
    // wavefront 0 runs it and hands the step over through LDS, which leaves the other three SIMDs to the second workgroup of
    // this CU (every lm_step is followed by an accumulation, whose block reduction orders the next overwrite of sStep).
    double* sStep = sRegion;   // the scores / sampled poses are dead after the selection
    if (wave == 0) {
      const double lambda = detm::pow10i(lambdaLg10);
      double A[36], x[6];
      for (int i = 0; i < 36; ++i) A[i] = acc.JtJ[i];
      for (int i = 0; i < 6; ++i) A[i * 6 + i] *= 1. + lambda;
      rsm::solve_normal6(A, acc.JtErr, x);
      if (lane == 0)
        for (int i = 0; i < 6; ++i) sStep[i] = x[i];
    }
    __syncthreads();
    for (int i = 0; i < 6; ++i) prm[i] = prevParam[i] - sStep[i];
  };

  // refineHyp of prm: the inlier flags of the last accepted step, whether one was accepted, and its inlier count
  auto refine = [&](double* param, uint64_t& acc_flags, bool& have_map, unsigned& bestInliers) {
  uint64_t flags = classify(param);
  acc_flags = 0;
  bestInliers = 4;
  have_map = false;
  const int max_ref = a.max_ref_steps > 0 ? a.max_ref_steps : 100;
  for (int rStep = 0; rStep < max_ref; rStep++) {
    const int cnt = compact(flags);
    if ((unsigned)cnt <= bestInliers) break;
    bestInliers = (unsigned)cnt;

    // solvePnP(ITERATIVE, useExtrinsicGuess) on the inlier list
    {
      const int max_iter = 20;
      const double epsilon = 1.1920928955078125e-07;
      double prm[6], prevParam[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) prm[i] = param[i];
      int lambdaLg10 = -3, iters = 0;
      double prevErrNorm = 1.7976931348623157e308, errNorm;
      LMAccum acc;
      accumulate_J(prm, cnt, &acc);
      for (;;) {
        for (int i = 0; i < 6; ++i) prevParam[i] = prm[i];
        lm_step(acc, prevParam, lambdaLg10, prm);
        if (iters == 0) prevErrNorm = sqrt(acc.errsq);
        for (;;) {
          errNorm = sqrt(accumulate_E(prm, cnt));
          if (errNorm > prevErrNorm) {
            if (++lambdaLg10 <= 16) {
              lm_step(acc, prevParam, lambdaLg10, prm);
              continue;
            }
          }
          break;
        }
        lambdaLg10 = (lambdaLg10 - 1 > -16) ? lambdaLg10 - 1 : -16;
        double dn = 0, pn = 0;
        for (int i = 0; i < 6; ++i) {
          const double d = prm[i] - prevParam[i];
          dn += d * d;
          pn += prevParam[i] * prevParam[i];
        }
        const double rel = sqrt(dn) / (sqrt(pn) + 2.220446049250313e-16);
        if (++iters >= max_iter || rel < epsilon) break;
        prevErrNorm = errNorm;
        accumulate_J(prm, cnt, &acc);
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) param[i] = prm[i];
    }
    acc_flags = flags;
    have_map = true;
    flags = classify(param);
  }
  };

  if constexpr (GRAD) {
    // ---- the backward pass (dsacstar_rgb_backward, dsacstar.cpp:208-490): probabilities, every hypothesis with p >= PROB_THRESH
    // refined, losses, E, path I through the refinement's normal equations, path II through the scores and P3P
    double* sProb = reinterpret_cast<double*>(sInt + 8);   // [hyps]
    double* sLoss = sProb + a.hyps;                         // [hyps]
    double* sM = sLoss + a.hyps;    // [0,36) (J^T J)^+, [36,42) v = (J^T J)^+ p dLoss, [42] E, [48,52) wavefront maxima
    const acez_rs::GradOut& go = a.grad;
    const float* G = go.gt + (size_t)frame * 16;
    double* gacc = go.gacc + (size_t)frame * 3 * N;
    unsigned long long* mw = go.masks + (size_t)frame * a.hyps * go.mwords;
    acez_loss::zero_frame(gacc, N, mw, a.hyps * go.mwords, tid, 256);
    if (tid == 0) acez_loss::softmax_entropy(sScores, a.hyps, sProb, go.probs + (size_t)frame * a.hyps, go.entropy + frame);
    __syncthreads();
    const double NORM_EPS = 1e-8;   // the reference's max(|e|, EPS)
    // d|e| / d(rvec, tvec) of pixel p at prm (one row of the refinement's Jacobian); false if its error exceeds max_reproj
    auto norm_row = [&](int p, const double* R, const double* dRdr, const double* prm, double row[6]) -> bool {
      const int x = div_h(p, H, magic), y = p - x * H;
      double u, v, Ju[6], Jv[6];
      rsm::project(R, prm + 3, k, sX[p], sY[p], sZ[p], &u, &v, dRdr, Ju, Jv);
      const double du = u - (double)(float)(x * a.sub + half), dv = v - (double)(float)(y * a.sub + half);
      double err = sqrt(du * du + dv * dv);
      err = err > NORM_EPS ? err : NORM_EPS;
      if (err > (double)a.max_reproj) return false;
      for (int q = 0; q < 6; ++q) row[q] = (du * Ju[q] + dv * Jv[q]) / err;
      return true;
    };
    // dProjectdObj: d|e| / dX of pixel p with the pose fixed; zero if the point is behind the camera or its error exceeds max_reproj
    auto dproj_dobj = [&](int p, const double* R, const double* t, double g[3]) {
      g[0] = g[1] = g[2] = 0.0;
      const int x = div_h(p, H, magic), y = p - x * H;
      const double X[3] = {sX[p], sY[p], sZ[p]};
      double c[3];
      for (int r = 0; r < 3; ++r) c[r] = ((R[r * 3 + 0] * X[0] + R[r * 3 + 1] * X[1]) + R[r * 3 + 2] * X[2]) + t[r];
      if (fabs(c[2]) < NORM_EPS) return;
      const double px = k.fx * c[0] / c[2] + k.cx, py = k.fy * c[1] / c[2] + k.cy;
      const double ex = px - (double)(float)(x * a.sub + half), ey = py - (double)(float)(y * a.sub + half);
      double err = sqrt(ex * ex + ey * ey);
      if (err > (double)a.max_reproj) return;
      err += NORM_EPS;
      for (int q = 0; q < 3; ++q) {
        const double pxd = k.fx * R[0 * 3 + q] / c[2] - k.fx * c[0] / (c[2] * c[2]) * R[2 * 3 + q];
        const double pyd = k.fy * R[1 * 3 + q] / c[2] - k.fy * c[1] / (c[2] * c[2]) * R[2 * 3 + q];
        g[q] = (ex * pxd + ey * pyd) / err;
      }
    };
    // the largest value over the workgroup (wavefront butterflies, then the 4 wavefronts through LDS)
    auto block_max = [&](double v) -> double {
      for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
      if (lane == 0) sM[48 + wave] = v;
      __syncthreads();
      const double r = fmax(fmax(sM[48], sM[49]), fmax(sM[50], sM[51]));
      __syncthreads();
      return r;
    };

    // ---- refine, loss, path I
    for (int h = 0; h < a.hyps; ++h) {
      const double p = sProb[h];
      const bool active = p >= acez_loss::PROB_THRESH;
      double param[6];
      for (int i = 0; i < 6; ++i) param[i] = a.hyp_poses[((size_t)frame * a.hyps + h) * 6 + i];
      uint64_t accf = 0;
      bool hm = false;
      unsigned ninl = 0;
      if (active) refine(param, accf, hm, ninl);
      if (active && hm)
        for (int i = 0; i < rows; ++i) {
          const unsigned long long bits = __ballot((accf >> i) & 1ull);
          if (lane == 0) mw[(size_t)h * go.mwords + i * 4 + wave] = bits;
        }
      double g6[6];
      const double L = acez_loss::pose_loss(param, G, go.w_rot, go.w_trans, go.cut, active ? g6 : nullptr);
      if (tid == 0) {
        sLoss[h] = L;
        const size_t o = (size_t)frame * a.hyps + h;
        go.losses[o] = L;
        for (int i = 0; i < 6; ++i) go.ref_poses[o * 6 + i] = param[i];
      }
      if (!(active && hm)) continue;
      // dHyp/dObj = -(J^T J)^+ J^T dN/dObj over the final inliers, J the rows of d|e|/dHyp (dsacstar.cpp:362-420)
      const int cnt = compact(accf);
      double R[9], dRdr[27];
      rsm::rodrigues(param, R, dRdr);
      double acc[28];
      for (int i = 0; i < 28; ++i) acc[i] = 0.0;
      for (int j = tid; j < cnt; j += 256) {
        double row[6];
        if (!norm_row(sList[j], R, dRdr, param, row)) continue;
        int q = 0;
        for (int aa = 0; aa < 6; ++aa)
          for (int bb = aa; bb < 6; ++bb) acc[q++] += row[aa] * row[bb];
      }
      LMAccum S;
      reduce28(acc, &S);
      if (tid == 0) {
        for (int c = 0; c < 6; ++c) {
          double e[6] = {0, 0, 0, 0, 0, 0}, col[6];
          e[c] = 1.0;
          rsm::solve_sym6(S.JtJ, e, col);   // inv(DECOMP_SVD)
          for (int r = 0; r < 6; ++r) sM[r * 6 + c] = col[r];
        }
        for (int r = 0; r < 6; ++r) {
          double v = 0;
          for (int q = 0; q < 6; ++q) v += sM[r * 6 + q] * (p * g6[q]);
          sM[36 + r] = v;
        }
      }
      __syncthreads();
      double mx = 0.0;   // maxJR: the largest entry of (J^T J)^+ J^T
      for (int j = tid; j < cnt; j += 256) {
        double row[6];
        if (!norm_row(sList[j], R, dRdr, param, row)) continue;
        for (int r = 0; r < 6; ++r) {
          double w = 0;
          for (int q = 0; q < 6; ++q) w += sM[r * 6 + q] * row[q];
          mx = fmax(mx, fabs(w));
        }
      }
      if (block_max(mx) > 10) continue;   // clamping for stability (dsacstar.cpp:403-404)
      for (int j = tid; j < cnt; j += 256) {
        const int pp = sList[j];
        double row[6], g[3];
        if (!norm_row(pp, R, dRdr, param, row)) continue;
        double s = 0;
        for (int q = 0; q < 6; ++q) s += sM[36 + q] * row[q];
        dproj_dobj(pp, R, param + 3, g);
        const int x = div_h(pp, H, magic), y = pp - x * H, m = y * W + x;
        for (int c = 0; c < 3; ++c) gacc[c * N + m] += -s * g[c];
      }
      __syncthreads();
    }
    __syncthreads();
    if (tid == 0) {
      const double E = acez_loss::expected_loss(sProb, sLoss, a.hyps);
      sM[42] = E;
      go.out_loss[frame] = E;
    }
    __syncthreads();
    const double Eexp = sM[42];

    // ---- path II (dSMScore / dScore): every pixel's own error with the hypothesis fixed, and the hypothesis through P3P (dPNP)
    for (int h = 0; h < a.hyps; ++h) {
      const double p = sProb[h];
      if (!(p >= acez_loss::PROB_THRESH)) continue;
      const double sg = p * (sLoss[h] - Eexp);
      double prm[6], R[9], dRdr[27];
      for (int i = 0; i < 6; ++i) prm[i] = a.hyp_poses[((size_t)frame * a.hyps + h) * 6 + i];
      rsm::rodrigues(prm, R, dRdr);
      double acc[28];
      for (int i = 0; i < 28; ++i) acc[i] = 0.0;
      for (int i = 0; i < rows; ++i) {
        const int pp = tid + 256 * i;
        if (pp >= N) break;
        const int x = div_h(pp, H, magic), y = pp - x * H;
        const float e = pixel_err(R, prm + 3, k, sX[pp], sY[pp], sZ[pp], x * a.sub + half, y * a.sub + half, a.max_reproj);
        const float beta_e = inlierBeta * (e - a.thr);
        if (beta_e > 40.f) continue;   // sigma' < 5e-18
        const double st = 1 / (1 + exp_dev(-(double)beta_e));
        const double dD = -st * (1 - st) * (double)inlierBeta * sg * (double)score_scale;
        double row[6], g[3];
        if (!norm_row(pp, R, dRdr, prm, row)) continue;
        dproj_dobj(pp, R, prm + 3, g);
        const int m = y * W + x;
        for (int c = 0; c < 3; ++c) gacc[c * N + m] += dD * g[c];
        for (int q = 0; q < 6; ++q) acc[21 + q] += dD * row[q];
      }
      LMAccum S;
      reduce28(acc, &S);   // wavefront 0: S.JtErr = d score-path / d hypothesis
      if (tid == 0) {
        const int* smp = a.samples + ((size_t)frame * a.hyps + h) * 4;
        float obj[4][3], img[4][2];
        for (int j = 0; j < 4; ++j) {
          const int x = div_h(smp[j], H, magic), y = smp[j] - x * H;
          obj[j][0] = sX[smp[j]]; obj[j][1] = sY[smp[j]]; obj[j][2] = sZ[smp[j]];
          img[j][0] = (float)(x * a.sub + half);
          img[j][1] = (float)(y * a.sub + half);
        }
        // dPNP: central differences (eps 0.001, in float as the reference perturbs cv::Point3f) of P3P in the first three points
        double cols[9][6];
        bool ok = true;
        double mxc = 0.0;
        for (int i = 0; i < 3 && ok; ++i)
          for (int c = 0; c < 3 && ok; ++c) {
            float o[4][3];
            for (int j = 0; j < 4; ++j)
              for (int q = 0; q < 3; ++q) o[j][q] = obj[j][q];
            Pose fw, bw;
            o[i][c] = obj[i][c] + 0.001f;
            ok = rsm::solve_pnp_p3p(o, img, k, &fw);
            o[i][c] = o[i][c] - 2 * 0.001f;
            ok = ok && rsm::solve_pnp_p3p(o, img, k, &bw);
            for (int q = 0; q < 3 && ok; ++q) {
              cols[i * 3 + c][q] = (fw.r[q] - bw.r[q]) / (double)(2 * 0.001f);
              cols[i * 3 + c][3 + q] = (fw.t[q] - bw.t[q]) / (double)(2 * 0.001f);
            }
            for (int q = 0; q < 6 && ok; ++q) {
              ok = isfinite(cols[i * 3 + c][q]);
              mxc = fmax(mxc, fabs(cols[i * 3 + c][q]));
            }
          }
        if (ok && !(mxc > 10)) {   // a failed solve or an entry above 10 zeroes the support term (dPNP, dScore)
          int ms[3];
          for (int i = 0; i < 3; ++i) {
            const int x = div_h(smp[i], H, magic), y = smp[i] - x * H;
            ms[i] = y * W + x;
          }
          acez_loss::scatter_support(gacc, N, ms, S.JtErr, cols);
        }
      }
      __syncthreads();
    }
    acez_loss::flush_grad(go.out_grad + (size_t)frame * 3 * N, gacc, N, tid, 256);
    return;
  }

  // ---- select: softMax + draw(argmax)
  if (tid == 0) {
    double maxScore = 0;
    for (int i = 0; i < a.hyps; i++)
      if (i == 0 || sScores[i] > maxScore) maxScore = sScores[i];
    double sum = 0.0;
    for (int i = 0; i < a.hyps; i++) sum += detm::exp_(sScores[i] - maxScore);
    double maxProb = -1;
    int maxIdx = 0;
    for (int idx = 0; idx < a.hyps; idx++) {
      const double pr = detm::exp_(sScores[idx] - maxScore) / sum;
      if (pr < 0.00000001) continue;
      if (maxProb < 0 || pr > maxProb) {
        maxProb = pr;
        maxIdx = idx;
      }
    }
    sInt[0] = maxIdx;
    a.best[frame] = maxIdx;
  }
  __syncthreads();

  // ---- refine
  const int bestIdx = sInt[0];
  double param[6];
  {
    const double* hp = a.hyp_poses + ((size_t)frame * a.hyps + bestIdx) * 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) param[i] = hp[i];
  }
  uint64_t acc_flags;
  unsigned bestInliers;
  bool have_map;
  refine(param, acc_flags, have_map, bestInliers);

  // ---- outputs
  if (a.out_masks) {
    uint8_t* mk = a.out_masks + (size_t)frame * N;
    for (int i = 0; i < rows; ++i) {
      const int p = tid + 256 * i;
      if (p >= N) break;
      const int x = div_h(p, H, magic), y = p - x * H;
      mk[y * W + x] = (have_map && ((acc_flags >> i) & 1ull)) ? 1 : 0;
    }
  }
  if (tid == 0) {
    double R[9], T[16], Ti[16];
    rsm::rodrigues(param, R, nullptr);
    for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1. : 0.;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T[r * 4 + c] = R[r * 3 + c];
      T[r * 4 + 3] = param[3 + r];
    }
    if (!inv4x4(T, Ti))
      for (int i = 0; i < 16; ++i) Ti[i] = 0;
    for (int i = 0; i < 16; ++i) a.out_poses[(size_t)frame * 16 + i] = (float)Ti[i];
    for (int i = 0; i < 6; ++i) a.refined[(size_t)frame * 6 + i] = param[i];
    a.out_inliers[frame] = have_map ? (int)bestInliers : 0;
  }
}

}  // namespace

// ====================================================================================================
// The registration host side shared with ransac_rgbd.hip (declared in ransac_ctx.h)
// ====================================================================================================
namespace acez_rs {

int ensure_hyps(Workspace& ws, int hyps) {
  if (!ws.d_best) ACEZ_HIP_CHECK(hipMalloc((void**)&ws.d_best, (size_t)ws.frames * sizeof(int)));
  if (!ws.d_refined) ACEZ_HIP_CHECK(hipMalloc((void**)&ws.d_refined, (size_t)ws.frames * 6 * sizeof(double)));
  if (hyps <= ws.hyps) return ACEZ_OK;
  ACEZ_HIP_CHECK(hipDeviceSynchronize());   // earlier launches may still write the old buffers
  if (ws.d_hyp_poses) (void)hipFree(ws.d_hyp_poses);
  if (ws.d_scores) (void)hipFree(ws.d_scores);
  if (ws.d_samples) (void)hipFree(ws.d_samples);
  ws.d_hyp_poses = nullptr; ws.d_scores = nullptr; ws.d_samples = nullptr;
  ws.hyps = 0;
  ACEZ_HIP_CHECK(hipMalloc((void**)&ws.d_hyp_poses, (size_t)ws.frames * hyps * 6 * sizeof(double)));
  ACEZ_HIP_CHECK(hipMalloc((void**)&ws.d_scores, (size_t)ws.frames * hyps * sizeof(double)));
  if (ws.sample_width)
    ACEZ_HIP_CHECK(hipMalloc((void**)&ws.d_samples, (size_t)ws.frames * hyps * ws.sample_width * sizeof(int)));
  ws.hyps = hyps;
  return ACEZ_OK;
}

int ensure_list_floats(Workspace& ws, size_t floats) {
  if (floats <= ws.list_floats) return ACEZ_OK;
  ACEZ_HIP_CHECK(hipDeviceSynchronize());
  if (ws.d_list) (void)hipFree(ws.d_list);
  ws.d_list = nullptr;
  ws.list_floats = 0;
  ACEZ_HIP_CHECK(hipMalloc((void**)&ws.d_list, floats * sizeof(float)));
  ws.list_floats = floats;
  return ACEZ_OK;
}

void release(Workspace& ws) {
  for (void* p : {(void*)ws.d_hyp_poses, (void*)ws.d_scores, (void*)ws.d_samples, (void*)ws.d_best, (void*)ws.d_refined, (void*)ws.d_list})
    if (p) (void)hipFree(p);
  ws = Workspace();
}

int ensure_grad(GradWorkspace& g, int hyps, int cells) {
  int rc = ensure_hyps(g.ws, hyps);
  if (rc != ACEZ_OK) return rc;
  const int frames = g.ws.frames, mw = mask_words(g, cells);
  if (!g.d_entropy) {
    ACEZ_HIP_CHECK(hipMalloc((void**)&g.d_entropy, (size_t)frames * sizeof(double)));
    ACEZ_HIP_CHECK(hipMalloc((void**)&g.d_loss, (size_t)frames * sizeof(double)));
    ACEZ_HIP_CHECK(hipMalloc((void**)&g.d_gt, (size_t)frames * 16 * sizeof(float)));
  }
  if (hyps <= g.hyps && cells <= g.cells && mw <= g.mwords) return ACEZ_OK;
  ACEZ_HIP_CHECK(hipDeviceSynchronize());   // earlier launches may still write the old buffers
  for (void* p : {(void*)g.d_probs, (void*)g.d_losses, (void*)g.d_ref_poses, (void*)g.d_masks, (void*)g.d_gacc, (void*)g.d_grad})
    if (p) (void)hipFree(p);
  g.d_probs = g.d_losses = g.d_ref_poses = g.d_gacc = nullptr;
  g.d_masks = nullptr;
  g.d_grad = nullptr;
  g.hyps = g.cells = g.mwords = 0;
  const int H = hyps > g.ws.hyps ? hyps : g.ws.hyps;
  ACEZ_HIP_CHECK(hipMalloc((void**)&g.d_probs, (size_t)frames * H * sizeof(double)));
  ACEZ_HIP_CHECK(hipMalloc((void**)&g.d_losses, (size_t)frames * H * sizeof(double)));
  ACEZ_HIP_CHECK(hipMalloc((void**)&g.d_ref_poses, (size_t)frames * H * 6 * sizeof(double)));
  ACEZ_HIP_CHECK(hipMalloc((void**)&g.d_masks, (size_t)frames * H * mw * sizeof(unsigned long long)));
  ACEZ_HIP_CHECK(hipMalloc((void**)&g.d_gacc, (size_t)frames * 3 * cells * sizeof(double)));
  ACEZ_HIP_CHECK(hipMalloc((void**)&g.d_grad, (size_t)3 * cells * sizeof(float)));
  g.hyps = H; g.cells = cells; g.mwords = mw;
  return ACEZ_OK;
}

void release_grad(GradWorkspace& g) {
  release(g.ws);
  for (void* p : {(void*)g.d_probs, (void*)g.d_losses, (void*)g.d_ref_poses, (void*)g.d_masks, (void*)g.d_gacc, (void*)g.d_entropy,
                  (void*)g.d_gt, (void*)g.d_grad, (void*)g.d_loss})
    if (p) (void)hipFree(p);
  g = GradWorkspace();
}

GradOut make_grad_out(const GradWorkspace& g, int cells, const float* gt, float w_rot, float w_trans, float cut, float* out_grad,
                      double* out_loss) {
  return GradOut{gt, w_rot, w_trans, cut, g.d_probs, g.d_losses, g.d_ref_poses, g.d_masks, mask_words(g, cells), g.d_gacc, g.d_entropy,
                 out_grad, out_loss};
}

int check_frames(const acez_ransac* ctx, int n_frames, int h, int w, const acez_ransac_params* params, bool needs_subsampling,
                 const char* noun) {
  ACEZ_REQUIRE(n_frames > 0 && n_frames <= ctx->max_frames, "n_frames exceeds the context's max_frames");
  ACEZ_REQUIRE(h > 0 && w > 0 && h <= ctx->max_h && w <= ctx->max_w, "frame larger than the context was created for");
  if ((int64_t)h * w > MAX_CELLS) {
    acez::set_error("invalid argument: at most 16384 %s per frame", noun);
    return ACEZ_ERR_INVALID;
  }
  ACEZ_REQUIRE(params->hypotheses > 0 && params->max_tries > 0, "hypotheses and max_tries must be positive");
  if (needs_subsampling)
    ACEZ_REQUIRE(params->subsampling > 0 && params->inlier_threshold > 0.f, "subsampling and inlier_threshold must be positive");
  else
    ACEZ_REQUIRE(params->inlier_threshold > 0.f, "inlier_threshold must be positive");
  return ACEZ_OK;
}

int plan_launch(Workspace& ws, int h, int w, int hyps, int list_floats_per_cell, size_t (*lds_bytes)(int, int, bool), Geometry* g) {
  g->N = h * w;
  g->Npad = (g->N + 3) & ~3;
  g->h_magic = h > 1 ? (uint32_t)(((1ull << 32) + (uint64_t)h - 1) / (uint64_t)h) : 0u;
  g->hbm = lds_bytes(g->Npad, hyps, false) > 160 * 1024;
  g->lds = lds_bytes(g->Npad, hyps, g->hbm);
  ACEZ_REQUIRE(g->lds <= 160 * 1024, "too many hypotheses for the 160 KB LDS of a CU");
  return g->hbm ? ensure_list_floats(ws, (size_t)ws.frames * list_floats_per_cell * g->Npad) : ACEZ_OK;
}

int stage_params(acez_ransac* ctx, hipStream_t s, int n, const acez_intrinsics* h_intrinsics, const uint64_t* h_frame_ids,
                 ParamSlot** out) {
  ParamSlot& slot = ctx->slot[ctx->next_slot];
  ctx->next_slot = (ctx->next_slot + 1) % PARAM_SLOTS;
  if (slot.in_flight) ACEZ_HIP_CHECK(hipEventSynchronize(slot.done));
  for (int i = 0; i < n; ++i) {
    const acez_intrinsics k = h_intrinsics ? h_intrinsics[i] : acez_intrinsics{0.f, 0.f, 0.f};
    slot.h[i] = FrameParam{k.focal, k.ppx, k.ppy, 0.f, h_frame_ids ? h_frame_ids[i] : (uint64_t)i};
  }
  ACEZ_HIP_CHECK(hipMemcpyAsync(slot.d, slot.h, (size_t)n * sizeof(FrameParam), hipMemcpyHostToDevice, s));
  *out = &slot;
  return ACEZ_OK;
}

int upload_strided(float* d_dst, const float* h_src, int64_t stride_c, int64_t stride_h, int64_t stride_w, int h, int w) {
  std::vector<float> packed((size_t)3 * h * w);
  for (int c = 0; c < 3; ++c)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) packed[((size_t)c * h + y) * w + x] = h_src[c * stride_c + y * stride_h + x * stride_w];
  ACEZ_HIP_CHECK(hipMemcpy(d_dst, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice));
  return ACEZ_OK;
}

// upload_strided's counterpart: adds a packed [3][h][w] gradient to the caller's strided host tensor
static void add_strided(float* h_dst, int64_t stride_c, int64_t stride_h, int64_t stride_w, const float* packed, int h, int w) {
  for (int c = 0; c < 3; ++c)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) h_dst[c * stride_c + y * stride_h + x * stride_w] += packed[((size_t)c * h + y) * w + x];
}

int download_result(const acez_ransac* ctx, int h, int w, float* h_out_pose16, int32_t* out_inliers, uint8_t* h_out_mask) {
  ACEZ_HIP_CHECK(hipMemcpy(h_out_pose16, ctx->d_pose, 16 * sizeof(float), hipMemcpyDeviceToHost));
  ACEZ_HIP_CHECK(hipMemcpy(out_inliers, ctx->d_inl, sizeof(int), hipMemcpyDeviceToHost));
  if (h_out_mask) ACEZ_HIP_CHECK(hipMemcpy(h_out_mask, ctx->d_mask, (size_t)h * w, hipMemcpyDeviceToHost));
  return ACEZ_OK;
}

int debug_fetch(const acez_ransac* ctx, const Workspace& ws, int n_frames, int hypotheses, int32_t* h_samples, double* h_hyp_poses,
                double* h_scores, int32_t* h_best, double* h_refined) {
  ACEZ_REQUIRE(n_frames > 0 && n_frames <= ws.frames && hypotheses == ws.last_hyps, "shape does not match the last call");
  ACEZ_HIP_CHECK(hipSetDevice(ctx->device));
  ACEZ_HIP_CHECK(hipDeviceSynchronize());
  const size_t nh = (size_t)n_frames * hypotheses;
  if (h_samples) ACEZ_HIP_CHECK(hipMemcpy(h_samples, ws.d_samples, nh * ws.sample_width * sizeof(int), hipMemcpyDeviceToHost));
  if (h_hyp_poses) ACEZ_HIP_CHECK(hipMemcpy(h_hyp_poses, ws.d_hyp_poses, nh * 6 * sizeof(double), hipMemcpyDeviceToHost));
  if (h_scores) ACEZ_HIP_CHECK(hipMemcpy(h_scores, ws.d_scores, nh * sizeof(double), hipMemcpyDeviceToHost));
  if (h_best) ACEZ_HIP_CHECK(hipMemcpy(h_best, ws.d_best, (size_t)n_frames * sizeof(int), hipMemcpyDeviceToHost));
  if (h_refined) ACEZ_HIP_CHECK(hipMemcpy(h_refined, ws.d_refined, (size_t)n_frames * 6 * sizeof(double), hipMemcpyDeviceToHost));
  return ACEZ_OK;
}

int backward_host(GradWorkspace& g, int h, int w, const float* h_gt_pose16, float* h_grad, int64_t g_stride_c, int64_t g_stride_h,
                  int64_t g_stride_w, double* out_loss, const std::function<int(const float*, float*, double*)>& launch) {
  const size_t cells = (size_t)h * w;
  ACEZ_HIP_CHECK(hipMemcpy(g.d_gt, h_gt_pose16, 16 * sizeof(float), hipMemcpyHostToDevice));
  ACEZ_HIP_CHECK(hipMemset(g.d_grad, 0, 3 * cells * sizeof(float)));
  const int rc = launch(g.d_gt, g.d_grad, g.d_loss);
  if (rc != ACEZ_OK) return rc;
  std::vector<float> grad(3 * cells);
  ACEZ_HIP_CHECK(hipMemcpy(grad.data(), g.d_grad, grad.size() * sizeof(float), hipMemcpyDeviceToHost));
  ACEZ_HIP_CHECK(hipMemcpy(out_loss, g.d_loss, sizeof(double), hipMemcpyDeviceToHost));
  add_strided(h_grad, g_stride_c, g_stride_h, g_stride_w, grad.data(), h, w);
  return ACEZ_OK;
}

int grad_debug_fetch(const acez_ransac* ctx, const GradWorkspace& g, int n_frames, int hypotheses, int h, int w, int32_t* h_samples,
                     double* h_hyp_poses, double* h_scores, double* h_probs, double* h_losses, double* h_ref_poses,
                     uint64_t* h_mask_words, double* h_entropy) {
  ACEZ_REQUIRE(h * w == g.last_cells, "shape does not match the last call");
  int rc = debug_fetch(ctx, g.ws, n_frames, hypotheses, h_samples, h_hyp_poses, h_scores, nullptr, nullptr);
  if (rc != ACEZ_OK) return rc;
  const size_t nh = (size_t)n_frames * hypotheses;
  if (h_probs) ACEZ_HIP_CHECK(hipMemcpy(h_probs, g.d_probs, nh * sizeof(double), hipMemcpyDeviceToHost));
  if (h_losses) ACEZ_HIP_CHECK(hipMemcpy(h_losses, g.d_losses, nh * sizeof(double), hipMemcpyDeviceToHost));
  if (h_ref_poses) ACEZ_HIP_CHECK(hipMemcpy(h_ref_poses, g.d_ref_poses, nh * 6 * sizeof(double), hipMemcpyDeviceToHost));
  if (h_mask_words)
    ACEZ_HIP_CHECK(hipMemcpy(h_mask_words, g.d_masks, nh * mask_words(g, h * w) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (h_entropy) ACEZ_HIP_CHECK(hipMemcpy(h_entropy, g.d_entropy, (size_t)n_frames * sizeof(double), hipMemcpyDeviceToHost));
  return ACEZ_OK;
}

}  // namespace acez_rs

namespace {
// The forward fields of the kernel's arguments (the backward fields stay zero).
RansacArgs make_args(const float* d_scene_coords, const acez_rs::ParamSlot& slot, const acez_rs::Workspace& ws, const acez_rs::Geometry& g,
                     int h, int w, const acez_ransac_params* params, uint64_t seed) {
  RansacArgs a{};
  a.sc = d_scene_coords; a.fp = slot.d; a.big = ws.d_list; a.H = h; a.W = w; a.N = g.N; a.hyps = params->hypotheses;
  a.h_magic = g.h_magic;
  a.max_tries = params->max_tries; a.sub = params->subsampling; a.max_ref_steps = params->max_ref_steps;
  a.thr = params->inlier_threshold; a.alpha = params->inlier_alpha; a.max_reproj = params->max_reproj; a.seed = seed;
  a.hyp_poses = ws.d_hyp_poses; a.scores = ws.d_scores; a.best = ws.d_best; a.refined = ws.d_refined;
  return a;
}
}  // namespace

// ====================================================================================================
// C ABI
// ====================================================================================================
extern "C" void acez_ransac_destroy(acez_ransac* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  for (acez_rs::ParamSlot& s : ctx->slot) {
    if (s.d) (void)hipFree(s.d);
    if (s.h) (void)hipHostFree(s.h);
    if (s.done) (void)hipEventDestroy(s.done);
  }
  acez_rs::release(ctx->rgb);
  acez_rs::release(ctx->rgbd);
  acez_rs::release_grad(ctx->rgbd_grad);
  acez_rs::release_grad(ctx->rgb_grad);
  for (void* p : {(void*)ctx->d_sc, (void*)ctx->d_cc, (void*)ctx->d_pose, (void*)ctx->d_inl, (void*)ctx->d_mask})
    if (p) (void)hipFree(p);
  delete ctx;
}

extern "C" int acez_ransac_create(acez_ransac** out, int max_frames, int max_h, int max_w, int device) {
  ACEZ_REQUIRE(out, "null pointer");
  ACEZ_REQUIRE(max_frames > 0 && max_h > 0 && max_w > 0, "sizes must be positive");
  if ((int64_t)max_h * max_w > 256 * MAX_ROWS) {
    acez::set_error("%d x %d = %lld scene coordinates per frame: the DSAC* kernel handles at most %d (e.g. 96 x 170, a 768 x 1360 image "
                    "at output stride 8); lower the image resolution (ace_zero.py --image_resolution, dataset.py:40) -- the reference's "
                    "CPU loop has no such limit", max_h, max_w, (long long)max_h * max_w, 256 * MAX_ROWS);
    return ACEZ_ERR_INVALID;
  }
  if (int rc = acez::require_device("the DSAC* kernels need a gfx950 GPU")) return rc;
  if (device >= 0) ACEZ_HIP_CHECK(hipSetDevice(device));
  acez_ransac* ctx = new (std::nothrow) acez_ransac();
  ACEZ_REQUIRE(ctx, "out of host memory");
  ACEZ_HIP_CHECK(hipGetDevice(&ctx->device));
  ctx->max_frames = max_frames;
  ctx->max_h = max_h;
  ctx->max_w = max_w;
  ctx->rgb.frames = ctx->rgbd.frames = ctx->rgbd_grad.ws.frames = ctx->rgb_grad.ws.frames = max_frames;
  ctx->rgbd.sample_width = ctx->rgbd_grad.ws.sample_width = 3;   // the RGB-D triple
  ctx->rgb_grad.ws.sample_width = 4;                             // the P3P minimal set
  ctx->rgb_grad.row_words = acez_rs::RGB_THREADS / 64;
  ctx->rgbd_grad.row_words = acez_rs::RGBD_THREADS / 64;
  int rc = ACEZ_OK;
  auto A = [&](void** p, size_t bytes) {
    if (rc == ACEZ_OK && hipMalloc(p, bytes) != hipSuccess) {
      acez::set_error("hipMalloc(%zu) failed", bytes);
      rc = ACEZ_ERR_HIP;
    }
  };
  for (acez_rs::ParamSlot& s : ctx->slot) {
    A((void**)&s.d, (size_t)max_frames * sizeof(FrameParam));
    if (rc == ACEZ_OK && (hipHostMalloc((void**)&s.h, (size_t)max_frames * sizeof(FrameParam)) != hipSuccess ||
                          hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess)) {
      acez::set_error("hipHostMalloc / hipEventCreate failed");
      rc = ACEZ_ERR_HIP;
    }
  }
  A((void**)&ctx->d_sc, (size_t)3 * max_h * max_w * sizeof(float));
  A((void**)&ctx->d_pose, 16 * sizeof(float));
  A((void**)&ctx->d_inl, sizeof(int));
  A((void**)&ctx->d_mask, (size_t)max_h * max_w);
  if (rc == ACEZ_OK) rc = acez_rs::ensure_hyps(ctx->rgb, 64);
  if (rc != ACEZ_OK) {
    acez_ransac_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return ACEZ_OK;
}

extern "C" int acez_register_rgb_device(acez_ransac* ctx, const float* d_scene_coords, int n_frames, int h, int w,
                                        const acez_ransac_params* params, const acez_intrinsics* h_intrinsics, uint64_t seed,
                                        const uint64_t* h_frame_ids, float* d_out_poses, int32_t* d_out_inliers,
                                        uint8_t* d_out_masks, void* stream) {
  ACEZ_REQUIRE(ctx && d_scene_coords && params && h_intrinsics && d_out_poses && d_out_inliers, "null pointer");
  int rc = acez_rs::check_frames(ctx, n_frames, h, w, params, true, "scene coordinates");
  if (rc != ACEZ_OK) return rc;
  ACEZ_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  acez_rs::Workspace& ws = ctx->rgb;
  acez_rs::Geometry g;
  acez_rs::ParamSlot* slot = nullptr;
  rc = acez_rs::ensure_hyps(ws, params->hypotheses);
  if (rc == ACEZ_OK) rc = acez_rs::plan_launch(ws, h, w, params->hypotheses, 3, lds_bytes, &g);
  if (rc == ACEZ_OK) rc = acez_rs::stage_params(ctx, s, n_frames, h_intrinsics, h_frame_ids, &slot);
  if (rc != ACEZ_OK) return rc;
  RansacArgs a = make_args(d_scene_coords, *slot, ws, g, h, w, params, seed);
  a.out_poses = d_out_poses; a.out_inliers = d_out_inliers; a.out_masks = d_out_masks;
  rc = acez_rs::launch(ransac_kernel<true>, ransac_kernel<false>, g, n_frames, 256, s, a, *slot);
  if (rc == ACEZ_OK) ws.last_hyps = params->hypotheses;
  return rc;
}

extern "C" int acez_register_rgb_host(acez_ransac* ctx, const float* h_scene_coords, int64_t stride_c, int64_t stride_h,
                                      int64_t stride_w, int h, int w, const acez_ransac_params* params,
                                      const acez_intrinsics* intr, uint64_t seed, uint64_t frame_id, float* h_out_pose16,
                                      int32_t* out_inliers, uint8_t* h_out_mask) {
  ACEZ_REQUIRE(ctx && h_scene_coords && params && intr && h_out_pose16 && out_inliers, "null pointer");
  ACEZ_REQUIRE(h > 0 && w > 0 && h <= ctx->max_h && w <= ctx->max_w, "frame larger than the context was created for");
  ACEZ_HIP_CHECK(hipSetDevice(ctx->device));
  int rc = acez_rs::upload_strided(ctx->d_sc, h_scene_coords, stride_c, stride_h, stride_w, h, w);
  if (rc == ACEZ_OK)
    rc = acez_register_rgb_device(ctx, ctx->d_sc, 1, h, w, params, intr, seed, &frame_id, ctx->d_pose, ctx->d_inl,
                                  h_out_mask ? ctx->d_mask : nullptr, nullptr);
  return rc == ACEZ_OK ? acez_rs::download_result(ctx, h, w, h_out_pose16, out_inliers, h_out_mask) : rc;
}

extern "C" int acez_ransac_debug_fetch(acez_ransac* ctx, int n_frames, int hypotheses, double* h_hyp_poses, double* h_scores,
                                       int32_t* h_best, double* h_refined) {
  ACEZ_REQUIRE(ctx, "null context");
  return acez_rs::debug_fetch(ctx, ctx->rgb, n_frames, hypotheses, nullptr, h_hyp_poses, h_scores, h_best, h_refined);
}

extern "C" int acez_register_rgb_backward_device(acez_ransac* ctx, const float* d_scene_coords, const float* d_gt_poses, int n_frames,
                                                 int h, int w, const acez_ransac_params* params, const acez_intrinsics* h_intrinsics,
                                                 float w_loss_rot, float w_loss_trans, float soft_clamp, uint64_t seed,
                                                 const uint64_t* h_frame_ids, float* d_out_grad, double* d_out_loss, void* stream) {
  ACEZ_REQUIRE(ctx && d_scene_coords && d_gt_poses && params && h_intrinsics && d_out_grad && d_out_loss, "null pointer");
  int rc = acez_rs::check_frames(ctx, n_frames, h, w, params, true, "scene coordinates");
  if (rc != ACEZ_OK) return rc;
  ACEZ_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  acez_rs::GradWorkspace& gw = ctx->rgb_grad;
  acez_rs::Geometry g;
  acez_rs::ParamSlot* slot = nullptr;
  rc = acez_rs::ensure_grad(gw, params->hypotheses, h * w);
  if (rc == ACEZ_OK) rc = acez_rs::plan_launch(gw.ws, h, w, params->hypotheses, 3, grad_lds_bytes, &g);
  if (rc == ACEZ_OK) rc = acez_rs::stage_params(ctx, s, n_frames, h_intrinsics, h_frame_ids, &slot);
  if (rc != ACEZ_OK) return rc;
  RansacArgs a = make_args(d_scene_coords, *slot, gw.ws, g, h, w, params, seed);
  a.samples = gw.ws.d_samples;
  a.grad = acez_rs::make_grad_out(gw, h * w, d_gt_poses, w_loss_rot, w_loss_trans, soft_clamp, d_out_grad, d_out_loss);
  rc = acez_rs::launch(ransac_kernel<true, true>, ransac_kernel<false, true>, g, n_frames, 256, s, a, *slot);
  if (rc == ACEZ_OK) acez_rs::note_launch(gw, params->hypotheses, h * w);
  return rc;
}

extern "C" int acez_register_rgb_backward_host(acez_ransac* ctx, const float* h_scene_coords, int64_t stride_c, int64_t stride_h,
                                               int64_t stride_w, const float* h_gt_pose16, int h, int w, const acez_ransac_params* params,
                                               const acez_intrinsics* intr, float w_loss_rot, float w_loss_trans, float soft_clamp,
                                               uint64_t seed, uint64_t frame_id, float* h_grad, int64_t g_stride_c, int64_t g_stride_h,
                                               int64_t g_stride_w, double* out_loss) {
  ACEZ_REQUIRE(ctx && h_scene_coords && h_gt_pose16 && params && intr && h_grad && out_loss, "null pointer");
  ACEZ_REQUIRE(h > 0 && w > 0 && h <= ctx->max_h && w <= ctx->max_w, "frame larger than the context was created for");
  ACEZ_HIP_CHECK(hipSetDevice(ctx->device));
  acez_rs::GradWorkspace& gw = ctx->rgb_grad;
  int rc = acez_rs::ensure_grad(gw, params->hypotheses, h * w);
  if (rc == ACEZ_OK) rc = acez_rs::upload_strided(ctx->d_sc, h_scene_coords, stride_c, stride_h, stride_w, h, w);
  if (rc != ACEZ_OK) return rc;
  auto launch = [&](const float* d_gt, float* d_grad, double* d_loss) {
    return acez_register_rgb_backward_device(ctx, ctx->d_sc, d_gt, 1, h, w, params, intr, w_loss_rot, w_loss_trans, soft_clamp, seed,
                                             &frame_id, d_grad, d_loss, nullptr);
  };
  return acez_rs::backward_host(gw, h, w, h_gt_pose16, h_grad, g_stride_c, g_stride_h, g_stride_w, out_loss, launch);
}

extern "C" int acez_ransac_rgb_backward_debug_fetch(acez_ransac* ctx, int n_frames, int hypotheses, int h, int w, int32_t* h_samples,
                                                    double* h_hyp_poses, double* h_scores, double* h_probs, double* h_losses,
                                                    double* h_ref_poses, uint64_t* h_mask_words, double* h_entropy) {
  ACEZ_REQUIRE(ctx && ctx->rgb_grad.ws.d_best, "no RGB backward call on this context");
  return acez_rs::grad_debug_fetch(ctx, ctx->rgb_grad, n_frames, hypotheses, h, w, h_samples, h_hyp_poses, h_scores, h_probs, h_losses,
                                   h_ref_poses, h_mask_words, h_entropy);
}
