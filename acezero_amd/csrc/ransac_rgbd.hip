// ransac_rgbd.hip -- DSAC* RGB-D registration on gfx950 (the reference's commented-out dsacstar_rgbd_forward,
// dsacstar/dsacstar.cpp:493-640, with sampleHypothesesRGBD / get3DDistErrs / refineHypRGBD of dsacstar_util.h): a pose
// from 3D-3D correspondences (camera coordinates back-projected from measured depth <-> predicted scene coordinates), no PnP.
// One 512-thread workgroup per frame, frames batched over the grid, fp64 geometry. Build with -ffp-contract=off.
//
//   valid    a cell is valid when its camera coordinate is finite with z != 0. The reference tests channel 0 three times
//            (dsacstar.cpp:530-533); with the principal point at the image centre no cell centre 8x+4 lies on the principal
//            column, so x == 0 exactly when z == 0 and both tests select the same cells.
//   compact  the valid cells, in the reference's x-outer / y-inner scan order, are compacted (ballot + per-wave counts) into a
//            list of (scene xyz, camera xyz, map index) -- in LDS, or for frames too large for it in an HBM workspace.
//   sample   one hypothesis per wavefront slot as in the RGB kernel: 8 hypotheses x 8 tries per wavefront pass, each lane
//            draws three list entries uniformly with replacement from the counter-based stream (seed, frame id, hypothesis,
//            try, draw), fits Kabsch in fp64 (centroids, 3x3 covariance, svd3 of svd3.h, sign-corrected rotation) and checks
//            that the three points are reproduced within the threshold (cm); a ballot keeps the first accepted try, else the
//            last try. A triple whose covariance has rank < 2 is redrawn (a try; as the last try it leaves the zero pose).
//   score    get3DDistErrs + getHypScores: err = min(|eye - (R X + t)| * 100, max_dist) per valid cell (invalid cells carry
//            max_dist), soft inlier count with beta = 5 / thr, lane-strided fp64 sums and a fixed butterfly per wavefront.
//   select   the first maximum of the scores (the reference's argmax of the soft-max; equal up to scores within an ulp).
//   refine   refineHypRGBD: all threads classify the valid cells, count the inliers and stop unless the count exceeds the best
//            so far (starting at 3); otherwise Kabsch on every inlier (two passes: means, then centred covariance), reduced in
//            a fixed order, and the errors are recomputed. A rank-deficient inlier set stops the refinement.
// The host side (workspaces, frame-parameter slots, launch geometry, staging, debug fetch) is ransac_api.hip's, declared in
// ransac_ctx.h; this unit keeps the kernel, its LDS layout and its entry points.
#include <hip/hip_runtime.h>
#include "ransac_math.h"
#include "acez_common.h"
#include "ransac_ctx.h"
#include "svd3.h"

namespace {

using acez_rs::FrameParam;
using rsm::div_h;

constexpr int THREADS = 512;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_ROWS = 32;          // valid-list entries per thread (flags in one 32-bit word): N <= 16384
constexpr int RED_STRIDE = 16;        // doubles per wavefront in the reduction scratch

struct RgbdArgs {
  const float* sc;      // [n][3][H][W] scene coordinates, metres
  const float* cc;      // [n][3][H][W] camera coordinates, metres
  const FrameParam* fp; // frame ids
  float* big;           // [n][7][Npad] compacted lists of frames that do not fit the LDS (GC instantiation)
  int H, W, N, Npad, hyps, max_tries, max_ref_steps;
  uint32_t h_magic;     // ceil(2^32 / H): p / H == __umulhi(p, h_magic) for p < 2^16 (H >= 2)
  float thr, alpha, max_dist;
  uint64_t seed;
  double* hyp_poses;    // [n][hyps][6] (rvec, tvec)
  double* scores;       // [n][hyps]
  int* samples;         // [n][hyps][3] map indices y * W + x of the kept triple
  int* best;            // [n]
  double* refined;      // [n][6]
  float* out_poses;     // [n][16]
  int* out_inliers;     // [n]
  uint8_t* out_masks;   // [n][H][W] or null
};

// butterfly v_l + v_(l ^ off), off = 32, 16, .., 1: every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

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
// so R = V U^T is the sign-corrected Kabsch rotation.
__device__ __forceinline__ bool kabsch(const double C[9], const double mX[3], const double mE[3], double rv[3], double t[3]) {
  acez::Svd3 d;
  acez::svd3(C, d);
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
__host__ __device__ inline size_t lds_bytes(int Npad, int hyps, bool lists_in_hbm) {
  return (lists_in_hbm ? 0 : 26 * (size_t)Npad) + region_bytes(hyps);
}

// LDS: [6][Npad] float list coordinates + [Npad] uint16 map indices (LDS instantiation only), then the region:
//   scores [hyps] f64, sampled poses [hyps][6] f64, reduction scratch [WAVES][16] f64, sampled triples [hyps][3] int,
//   compaction counts [MAX_ROWS][WAVES] int, [8] int.
template <bool GC>
__global__ __launch_bounds__(THREADS, 1) void rgbd_kernel(RgbdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int N = a.N, H = a.H, W = a.W, Npad = a.Npad;
  const int frame = blockIdx.x;
  float* sx = GC ? a.big + (size_t)frame * 7 * Npad : reinterpret_cast<float*>(smem_raw);
  float* sy = sx + Npad;
  float* sz = sy + Npad;
  float* ex = sz + Npad;
  float* ey = ex + Npad;
  float* ez = ey + Npad;
  uint16_t* cell = reinterpret_cast<uint16_t*>(ez + Npad);
  unsigned char* reg = smem_raw + (GC ? 0 : 26 * (size_t)Npad);
  double* sScores = reinterpret_cast<double*>(reg);
  double* sHyp = sScores + a.hyps;
  double* sRed = sHyp + 6 * a.hyps;
  int* sIdx = reinterpret_cast<int*>(sRed + RED_STRIDE * WAVES);
  int* sCnt = sIdx + 3 * a.hyps;
  int* sInt = sCnt + MAX_ROWS * WAVES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t frame_id = a.fp[frame].frame_id;
  const float* sc = a.sc + (size_t)frame * 3 * N;
  const float* cc = a.cc + (size_t)frame * 3 * N;
  uint8_t* mk = a.out_masks ? a.out_masks + (size_t)frame * N : nullptr;

  // ---- valid cells in scan order p = x * H + y; thread tid owns p = tid + THREADS i
  const int rows = (N + THREADS - 1) / THREADS;
  uint32_t vflags = 0;
  for (int i = 0; i < rows; ++i) {
    const int p = tid + THREADS * i;
    if (p >= N) break;
    const int x = div_h(p, H, a.h_magic), y = p - x * H;
    const int m = y * W + x;
    const float cx = cc[m], cy = cc[N + m], cz = cc[2 * N + m];
    if (cz != 0.f && isfinite(cx) && isfinite(cy) && isfinite(cz)) vflags |= 1u << i;
    else if (mk) mk[m] = 0;   // invalid cells are never inliers (valid ones are written once, below)
  }
  for (int i = 0; i < rows; ++i) {
    const unsigned long long m = __ballot((vflags >> i) & 1u);
    if (lane == 0) sCnt[i * WAVES + wave] = __popcll(m);
  }
  __syncthreads();
  int nv = 0;
  for (int i = 0; i < rows; ++i) {
    const bool f = (vflags >> i) & 1u;
    const unsigned long long bm = __ballot(f);
    int base = nv, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const int c = sCnt[i * WAVES + w];
      base += w < wave ? c : 0;
      tot += c;
    }
    if (f) {
      const int j = base + __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u));
      const int p = tid + THREADS * i;
      const int x = div_h(p, H, a.h_magic), y = p - x * H;
      const int m = y * W + x;
      sx[j] = sc[m]; sy[j] = sc[N + m]; sz[j] = sc[2 * N + m];
      ex[j] = cc[m]; ey[j] = cc[N + m]; ez[j] = cc[2 * N + m];
      cell[j] = (uint16_t)m;
    }
    nv += tot;
  }
  __syncthreads();

  if (nv < 3) {   // declared deviation: the reference would call irand(0, 0); identity pose, no inliers
    for (int h = tid; h < a.hyps; h += THREADS) {
      double* hp = a.hyp_poses + ((size_t)frame * a.hyps + h) * 6;
      for (int i = 0; i < 6; ++i) hp[i] = 0.0;
      a.scores[(size_t)frame * a.hyps + h] = 0.0;
      for (int i = 0; i < 3; ++i) a.samples[((size_t)frame * a.hyps + h) * 3 + i] = -1;
    }
    if (mk && tid < nv) mk[cell[tid]] = 0;
    if (tid == 0) {
      for (int i = 0; i < 16; ++i) a.out_poses[(size_t)frame * 16 + i] = (i % 5 == 0) ? 1.f : 0.f;
      for (int i = 0; i < 6; ++i) a.refined[(size_t)frame * 6 + i] = 0.0;
      a.best[frame] = 0;
      a.out_inliers[frame] = 0;
    }
    return;
  }

  // ---- sample: hypothesis h = wave + WAVES (8 pass + slot), try t0 + tr on lane 8 slot + tr
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
          X[j][0] = sx[idx[j]]; X[j][1] = sy[idx[j]]; X[j][2] = sz[idx[j]];
          E[j][0] = ex[idx[j]]; E[j][1] = ey[idx[j]]; E[j][2] = ez[idx[j]];
        }
        double mX[3], mE[3], C[9];
        for (int r = 0; r < 3; ++r) {
          mX[r] = ((X[0][r] + X[1][r]) + X[2][r]) / 3.0;
          mE[r] = ((E[0][r] + E[1][r]) + E[2][r]) / 3.0;
        }
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c)
            C[r * 3 + c] = ((X[0][r] - mX[r]) * (E[0][c] - mE[c]) + (X[1][r] - mX[r]) * (E[1][c] - mE[c])) + (X[2][r] - mX[r]) * (E[2][c] - mE[c]);
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
              sHyp[h * 6 + i] = rv[i];
              sHyp[h * 6 + 3 + i] = tv[i];
              sIdx[h * 3 + i] = cell[idx[i]];
            }
          }
        }
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();   // a wavefront scores the hypotheses its own lanes sampled

  // ---- score: hypothesis h on wavefront h % WAVES, lanes over the valid list
  const float inlierBeta = 5 / a.thr;
  const float score_scale = a.alpha / (float)W / (float)H;
  double inv_term = 0.0;             // an invalid cell's term: its error is max_dist
  {
    const float be = inlierBeta * (a.max_dist - a.thr);
    if (!(be > 40.f)) inv_term = 1 - 1 / (1 + detm::exp_(-(double)be));
  }
  for (int h = wave; h < a.hyps; h += WAVES) {
    double prm[6], R[9];
    for (int i = 0; i < 6; ++i) prm[i] = sHyp[h * 6 + i];
    rsm::rodrigues(prm, R, nullptr);
    double acc = 0;
    for (int j = lane; j < nv; j += 64) {
      const float e = dist_err(R, prm + 3, sx[j], sy[j], sz[j], ex[j], ey[j], ez[j], a.max_dist);
      const float beta_e = inlierBeta * (e - a.thr);
      if (beta_e > 40.f) continue;   // 1 + exp(-40) == 1 in fp64: the term is exactly +0
      acc += 1 - 1 / (1 + detm::exp_(-(double)beta_e));
    }
    double score = wave_sum(acc) + (double)(N - nv) * inv_term;
    score *= score_scale;
    if (lane == 0) {
      sScores[h] = score;
      const size_t o = (size_t)frame * a.hyps + h;
      for (int i = 0; i < 6; ++i) a.hyp_poses[o * 6 + i] = prm[i];
      for (int i = 0; i < 3; ++i) a.samples[o * 3 + i] = sIdx[h * 3 + i];
      a.scores[o] = score;
    }
  }
  __syncthreads();

  // ---- select: the first maximum
  if (tid == 0) {
    int b = 0;
    for (int i = 1; i < a.hyps; ++i)
      if (sScores[i] > sScores[b]) b = i;
    sInt[0] = b;
    a.best[frame] = b;
  }
  __syncthreads();

  // ---- refine: thread tid owns list entries j = tid + THREADS k
  double param[6];
  for (int i = 0; i < 6; ++i) param[i] = sHyp[sInt[0] * 6 + i];
  const int vrows = (nv + THREADS - 1) / THREADS;
  auto classify = [&](const double* prm) -> uint32_t {
    double R[9];
    rsm::rodrigues(prm, R, nullptr);
    uint32_t f = 0;
    for (int k = 0; k < vrows; ++k) {
      const int j = tid + THREADS * k;
      if (j >= nv) break;
      if (dist_err(R, prm + 3, sx[j], sy[j], sz[j], ex[j], ey[j], ez[j], a.max_dist) < a.thr) f |= 1u << k;
    }
    return f;
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
      s1[1] += sx[j]; s1[2] += sy[j]; s1[3] += sz[j];
      s1[4] += ex[j]; s1[5] += ey[j]; s1[6] += ez[j];
    }
    block_sum(s1, sRed, lane, wave);
    const int cnt = (int)s1[0];
    if (cnt <= bestInliers) break;   // converged
    const double mX[3] = {s1[1] / s1[0], s1[2] / s1[0], s1[3] / s1[0]};
    const double mE[3] = {s1[4] / s1[0], s1[5] / s1[0], s1[6] / s1[0]};
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < vrows; ++k) {
      if (!((flags >> k) & 1u)) continue;
      const int j = tid + THREADS * k;
      const double xc[3] = {sx[j] - mX[0], sy[j] - mX[1], sz[j] - mX[2]};
      const double ec[3] = {ex[j] - mE[0], ey[j] - mE[1], ez[j] - mE[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[r * 3 + c] += xc[r] * ec[c];
    }
    block_sum(C, sRed, lane, wave);
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

  // ---- outputs
  if (mk) {
    for (int k = 0; k < vrows; ++k) {
      const int j = tid + THREADS * k;
      if (j >= nv) break;
      mk[cell[j]] = (have_map && ((acc_flags >> k) & 1u)) ? 1 : 0;
    }
  }
  if (tid == 0) {
    double R[9];
    rsm::rodrigues(param, R, nullptr);
    float* o = a.out_poses + (size_t)frame * 16;
    // pose2trans: the inverse of [R | t], written in closed form (R^T, -R^T t)
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) o[r * 4 + c] = (float)R[c * 3 + r];
      o[r * 4 + 3] = (float)(-((R[0 * 3 + r] * param[3] + R[1 * 3 + r] * param[4]) + R[2 * 3 + r] * param[5]));
    }
    o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
    for (int i = 0; i < 6; ++i) a.refined[(size_t)frame * 6 + i] = param[i];
    a.out_inliers[frame] = have_map ? bestInliers : 0;
  }
}

}  // namespace

// ====================================================================================================
// C ABI
// ====================================================================================================
extern "C" int acez_register_rgbd_device(acez_ransac* ctx, const float* d_scene_coords, const float* d_camera_coords, int n_frames, int h,
                                         int w, const acez_ransac_params* params, uint64_t seed, const uint64_t* h_frame_ids,
                                         float* d_out_poses, int32_t* d_out_inliers, uint8_t* d_out_masks, void* stream) {
  ACEZ_REQUIRE(ctx && d_scene_coords && d_camera_coords && params && d_out_poses && d_out_inliers, "null pointer");
  ACEZ_REQUIRE(n_frames > 0 && n_frames <= ctx->max_frames, "n_frames exceeds the context's max_frames");
  ACEZ_REQUIRE(h > 0 && w > 0 && h <= ctx->max_h && w <= ctx->max_w, "frame larger than the context was created for");
  ACEZ_REQUIRE((int64_t)h * w <= THREADS * MAX_ROWS, "at most 16384 cells per frame");
  ACEZ_REQUIRE(params->hypotheses > 0 && params->max_tries > 0, "hypotheses and max_tries must be positive");
  ACEZ_REQUIRE(params->inlier_threshold > 0.f, "inlier_threshold must be positive");
  ACEZ_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  acez_rs::Workspace& ws = ctx->rgbd;
  acez_rs::Geometry g;
  acez_rs::ParamSlot* slot = nullptr;
  int rc = acez_rs::ensure_hyps(ws, params->hypotheses, true);
  if (rc == ACEZ_OK) rc = acez_rs::plan_launch(ws, h, w, params->hypotheses, 7, lds_bytes, &g);
  if (rc == ACEZ_OK) rc = acez_rs::stage_params(ctx, s, n_frames, nullptr, h_frame_ids, &slot);
  if (rc != ACEZ_OK) return rc;
  RgbdArgs a;
  a.sc = d_scene_coords; a.cc = d_camera_coords; a.fp = slot->d; a.big = ws.d_list;
  a.H = h; a.W = w; a.N = g.N; a.Npad = g.Npad; a.hyps = params->hypotheses; a.max_tries = params->max_tries;
  a.max_ref_steps = params->max_ref_steps;
  a.h_magic = g.h_magic;
  a.thr = params->inlier_threshold; a.alpha = params->inlier_alpha; a.max_dist = params->max_reproj; a.seed = seed;
  a.hyp_poses = ws.d_hyp_poses; a.scores = ws.d_scores; a.samples = ws.d_samples; a.best = ws.d_best; a.refined = ws.d_refined;
  a.out_poses = d_out_poses; a.out_inliers = d_out_inliers; a.out_masks = d_out_masks;
  rc = acez_rs::launch(rgbd_kernel<true>, rgbd_kernel<false>, g, n_frames, THREADS, s, a, *slot);
  if (rc == ACEZ_OK) ws.last_hyps = params->hypotheses;
  return rc;
}

extern "C" int acez_register_rgbd_host(acez_ransac* ctx, const float* h_scene_coords, int64_t sc_stride_c, int64_t sc_stride_h,
                                       int64_t sc_stride_w, const float* h_camera_coords, int64_t cc_stride_c, int64_t cc_stride_h,
                                       int64_t cc_stride_w, int h, int w, const acez_ransac_params* params, uint64_t seed,
                                       uint64_t frame_id, float* h_out_pose16, int32_t* out_inliers, uint8_t* h_out_mask) {
  ACEZ_REQUIRE(ctx && h_scene_coords && h_camera_coords && params && h_out_pose16 && out_inliers, "null pointer");
  ACEZ_REQUIRE(h > 0 && w > 0 && h <= ctx->max_h && w <= ctx->max_w, "frame larger than the context was created for");
  ACEZ_HIP_CHECK(hipSetDevice(ctx->device));
  if (!ctx->d_cc) ACEZ_HIP_CHECK(hipMalloc((void**)&ctx->d_cc, (size_t)3 * ctx->max_h * ctx->max_w * sizeof(float)));
  int rc = acez_rs::upload_strided(ctx->d_sc, h_scene_coords, sc_stride_c, sc_stride_h, sc_stride_w, h, w);
  if (rc == ACEZ_OK) rc = acez_rs::upload_strided(ctx->d_cc, h_camera_coords, cc_stride_c, cc_stride_h, cc_stride_w, h, w);
  if (rc == ACEZ_OK)
    rc = acez_register_rgbd_device(ctx, ctx->d_sc, ctx->d_cc, 1, h, w, params, seed, &frame_id, ctx->d_pose, ctx->d_inl,
                                   h_out_mask ? ctx->d_mask : nullptr, nullptr);
  return rc == ACEZ_OK ? acez_rs::download_result(ctx, h, w, h_out_pose16, out_inliers, h_out_mask) : rc;
}

extern "C" int acez_ransac_rgbd_debug_fetch(acez_ransac* ctx, int n_frames, int hypotheses, int32_t* h_samples, double* h_hyp_poses,
                                            double* h_scores, int32_t* h_best, double* h_refined) {
  ACEZ_REQUIRE(ctx && ctx->rgbd.d_best, "no RGB-D call on this context");
  return acez_rs::debug_fetch(ctx, ctx->rgbd, n_frames, hypotheses, h_samples, h_hyp_poses, h_scores, h_best, h_refined);
}
