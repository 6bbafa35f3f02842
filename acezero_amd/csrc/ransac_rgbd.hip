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
// ransac_ctx.h. The stages (compaction, sampling, scoring, refinement) are ransac_rgbd.h's, shared with the backward kernel of
// ransac_grad.hip; this unit keeps the forward kernel, its LDS size and its entry points, and the launch that makes the camera
// coordinates from depth (acez_camera_coordinates).
#include <hip/hip_runtime.h>
#include "ransac_math.h"
#include "acez_common.h"
#include "ransac_ctx.h"
#include "ransac_rgbd.h"

namespace {

using namespace acez_rgbd;

struct RgbdArgs {
  RgbdIn in;
  int* best;            // [n]
  double* refined;      // [n][6]
  float* out_poses;     // [n][16]
  int* out_inliers;     // [n]
  uint8_t* out_masks;   // [n][H][W] or null
};

__host__ __device__ inline size_t lds_bytes(int Npad, int hyps, bool lists_in_hbm) {
  return (lists_in_hbm ? 0 : 26 * (size_t)Npad) + region_bytes(hyps);
}

// LDS: frame_layout of ransac_rgbd.h
template <bool GC>
__global__ __launch_bounds__(THREADS, 1) void rgbd_kernel(RgbdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const RgbdIn& in = a.in;
  const int frame = blockIdx.x;
  Frame f = frame_layout<GC>(in, smem_raw, frame);
  const int tid = threadIdx.x;
  const uint64_t frame_id = in.fp[frame].frame_id;
  uint8_t* mk = a.out_masks ? a.out_masks + (size_t)frame * in.N : nullptr;

  compact_valid(in, f, frame, mk);
  const int nv = f.nv;
  if (nv < 3) {   // declared deviation: the reference would call irand(0, 0); identity pose, no inliers
    for (int h = tid; h < in.hyps; h += THREADS) {
      double* hp = in.hyp_poses + ((size_t)frame * in.hyps + h) * 6;
      for (int i = 0; i < 6; ++i) hp[i] = 0.0;
      in.scores[(size_t)frame * in.hyps + h] = 0.0;
      for (int i = 0; i < 3; ++i) in.samples[((size_t)frame * in.hyps + h) * 3 + i] = -1;
    }
    if (mk && tid < nv) mk[f.cell[tid]] = 0;
    if (tid == 0) {
      for (int i = 0; i < 16; ++i) a.out_poses[(size_t)frame * 16 + i] = (i % 5 == 0) ? 1.f : 0.f;
      for (int i = 0; i < 6; ++i) a.refined[(size_t)frame * 6 + i] = 0.0;
      a.best[frame] = 0;
      a.out_inliers[frame] = 0;
    }
    return;
  }
  sample_hyps(in, f, frame_id);
  score_hyps(in, f, frame);

  // ---- select: the first maximum
  if (tid == 0) {
    int b = 0;
    for (int i = 1; i < in.hyps; ++i)
      if (f.sScores[i] > f.sScores[b]) b = i;
    f.sInt[0] = b;
    a.best[frame] = b;
  }
  __syncthreads();

  double param[6];
  for (int i = 0; i < 6; ++i) param[i] = f.sHyp[f.sInt[0] * 6 + i];
  const Refined rf = refine(in, f, param);

  // ---- outputs
  if (mk) {
    const int vrows = (nv + THREADS - 1) / THREADS;
    for (int k = 0; k < vrows; ++k) {
      const int j = tid + THREADS * k;
      if (j >= nv) break;
      mk[f.cell[j]] = (rf.have_map && ((rf.acc_flags >> k) & 1u)) ? 1 : 0;
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
    a.out_inliers[frame] = rf.have_map ? rf.inliers : 0;
  }
}

// Camera coordinates of the feature-map cell centres (stride x + stride / 2) from measured depth: one thread per cell, one launch for
// all frames. The operations and their order are dsacstar.camera_coordinates' (the mapping buffer's formula, dataset.py:347-388):
// ((px - ppx) / f) * d, ((py - ppy) / f) * d, d in float32, IEEE division, nothing contracted; a cell without depth (d == 0) is +0.
__global__ __launch_bounds__(256) void camera_coords_kernel(const float* __restrict__ depth, const float* __restrict__ focal, float ppx,
                                                            float ppy, int h, int w, int stride, float* __restrict__ out) {
  const int hw = h * w;
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= hw) return;
  const size_t frame = blockIdx.y;
  const float d = depth[frame * hw + cell];
  const float f = focal[frame];
  const float px = (float)((cell % w) * stride + stride / 2), py = (float)((cell / w) * stride + stride / 2);
  const bool none = d == 0.f;
  float* o = out + frame * 3 * hw + cell;
  o[0] = none ? 0.f : (px - ppx) / f * d;
  o[hw] = none ? 0.f : (py - ppy) / f * d;
  o[2 * (size_t)hw] = none ? 0.f : d;
}

}  // namespace

// ====================================================================================================
// C ABI
// ====================================================================================================
extern "C" int acez_register_rgbd_device(acez_ransac* ctx, const float* d_scene_coords, const float* d_camera_coords, int n_frames, int h,
                                         int w, const acez_ransac_params* params, uint64_t seed, const uint64_t* h_frame_ids,
                                         float* d_out_poses, int32_t* d_out_inliers, uint8_t* d_out_masks, void* stream) {
  ACEZ_REQUIRE(ctx && d_scene_coords && d_camera_coords && params && d_out_poses && d_out_inliers, "null pointer");
  int rc = acez_rs::check_frames(ctx, n_frames, h, w, params, false, "cells");
  if (rc != ACEZ_OK) return rc;
  ACEZ_HIP_CHECK(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  acez_rs::Workspace& ws = ctx->rgbd;
  acez_rs::Geometry g;
  acez_rs::ParamSlot* slot = nullptr;
  rc = acez_rs::ensure_hyps(ws, params->hypotheses);
  if (rc == ACEZ_OK) rc = acez_rs::plan_launch(ws, h, w, params->hypotheses, 7, lds_bytes, &g);
  if (rc == ACEZ_OK) rc = acez_rs::stage_params(ctx, s, n_frames, nullptr, h_frame_ids, &slot);
  if (rc != ACEZ_OK) return rc;
  RgbdArgs a;
  a.in = acez_rgbd::make_in(d_scene_coords, d_camera_coords, slot->d, ws, g, h, w, params, seed);
  a.best = ws.d_best; a.refined = ws.d_refined;
  a.out_poses = d_out_poses; a.out_inliers = d_out_inliers; a.out_masks = d_out_masks;
  rc = acez_rs::launch(rgbd_kernel<true>, rgbd_kernel<false>, g, n_frames, THREADS, s, a, *slot);
  if (rc == ACEZ_OK) ws.last_hyps = params->hypotheses;
  return rc;
}

extern "C" int acez_camera_coordinates(const float* d_depth, const float* d_focal, float ppx, float ppy, int n_frames, int h, int w,
                                       int stride, float* d_out_coords, void* stream) {
  ACEZ_REQUIRE(d_depth && d_focal && d_out_coords, "null pointer");
  ACEZ_REQUIRE(n_frames > 0 && n_frames <= 65535 && h > 0 && w > 0 && stride > 0 && (int64_t)h * w <= (1 << 24), "bad shape");
  if (int rc = acez::require_device("camera coordinates are computed on a gfx950 GPU")) return rc;
  hipLaunchKernelGGL(camera_coords_kernel, dim3((h * w + 255) / 256, n_frames), dim3(256), 0, (hipStream_t)stream, d_depth, d_focal, ppx, ppy,
                     h, w, stride, d_out_coords);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
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
