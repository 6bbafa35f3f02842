// ransac_ctx.h -- the registration context (acez_ransac) shared by the four DSAC* entry families: RGB forward and backward
// (ransac_api.hip), RGB-D forward (ransac_rgbd.hip) and RGB-D backward (ransac_grad.hip), and the host helpers their entry points
// use. Every helper declared here is defined in ransac_api.hip; each unit keeps its kernel, its LDS layout (lds_bytes) and its
// extern "C" entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <functional>
#include "acez_common.h"

namespace acez_rs {

struct FrameParam {
  float focal, ppx, ppy, pad;
  uint64_t frame_id;
};

// Workgroup sizes of the two kernel families; either way a frame has at most MAX_CELLS cells (256 x 64 rows, 512 x 32 rows).
constexpr int RGB_THREADS = 256, RGBD_THREADS = 512;
constexpr int MAX_CELLS = 16384;

constexpr int PARAM_SLOTS = 4;
// One pinned + device copy of the per-frame parameter block per call in flight: a device entry point never waits for the
// stream it launches on (only for the call PARAM_SLOTS launches ago, whose kernel has long finished in any pipelined use).
struct ParamSlot {
  FrameParam* h = nullptr;  // pinned
  FrameParam* d = nullptr;
  hipEvent_t done = nullptr;
  bool in_flight = false;
};

// The device workspaces of one estimator. Each kind keeps its own, so a debug fetch sees the last call of its kind.
struct Workspace {
  double* d_hyp_poses = nullptr;  // [frames][hyps][6] (rvec, tvec)
  double* d_scores = nullptr;     // [frames][hyps]
  int* d_samples = nullptr;       // [frames][hyps][sample_width] the kept sample (RGB-D: 3 map indices; RGB backward: 4 scan indices)
  int* d_best = nullptr;          // [frames]
  double* d_refined = nullptr;    // [frames][6]
  float* d_list = nullptr;        // lists of frames that do not fit the LDS, allocated on first use
  size_t list_floats = 0;
  int frames = 0, hyps = 0;       // capacity
  int sample_width = 0;           // ints per kept sample, set at acez_ransac_create: 0 RGB forward (none kept), 3 RGB-D, 4 RGB backward
  int last_hyps = 0;              // hypotheses of the last launch
};

// Allocate best / refined on first use and regrow the per-hypothesis buffers (samples: sample_width ints each) / the list buffer;
// both synchronise the device before freeing buffers that earlier launches may still write. release: the caller has synchronised.
int ensure_hyps(Workspace& ws, int hyps);
int ensure_list_floats(Workspace& ws, size_t floats);
void release(Workspace& ws);

struct Geometry {
  int N, Npad;
  uint32_t h_magic;  // ceil(2^32 / H): p / H == __umulhi(p, h_magic) for p < 2^16 (H >= 2)
  size_t lds;        // dynamic LDS bytes
  bool hbm;          // the lists go to ws.d_list (kernel<true>)
};
// The geometry of an h x w frame for a unit's LDS layout lds_bytes(Npad, hyps, lists_in_hbm): the lists go to HBM when the frame
// does not fit the 160 KB LDS of a CU, and then ws's list buffer grows to list_floats_per_cell floats per cell and frame.
int plan_launch(Workspace& ws, int h, int w, int hyps, int list_floats_per_cell, size_t (*lds_bytes)(int, int, bool), Geometry* g);

// Fills the next slot of the ring for n frames (intrinsics null: zeros; frame ids null: 0, 1, ..) after waiting for the call that
// used it last, and copies it to the device on s. launch() records the slot's event.
int stage_params(acez_ransac* ctx, hipStream_t s, int n, const acez_intrinsics* h_intrinsics, const uint64_t* h_frame_ids,
                 ParamSlot** out);

// Sets the dynamic-LDS attribute, launches kernel<true> (lists in HBM) or kernel<false> (lists in LDS), one workgroup per frame,
// and records the slot's event behind the launch.
template <class Args>
int launch(void (*hbm_kernel)(Args), void (*lds_kernel)(Args), const Geometry& g, int n_frames, int threads, hipStream_t s,
           const Args& a, ParamSlot& slot) {
  void (*kernel)(Args) = g.hbm ? hbm_kernel : lds_kernel;
  ACEZ_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
  hipLaunchKernelGGL(kernel, dim3(n_frames), dim3(threads), g.lds, s, a);
  ACEZ_HIP_CHECK(hipGetLastError());
  ACEZ_HIP_CHECK(hipEventRecord(slot.done, s));
  slot.in_flight = true;
  return ACEZ_OK;
}

// The host-buffer entry points: pack a [3][h][w] host tensor with the caller's accessor strides (dsacstar.cpp:83-84) into the
// staging buffer d_dst; after the device call, copy the pose, the inlier count and, if asked for, the mask back.
int upload_strided(float* d_dst, const float* h_src, int64_t stride_c, int64_t stride_h, int64_t stride_w, int h, int w);
int download_result(const acez_ransac* ctx, int h, int w, float* h_out_pose16, int32_t* out_inliers, uint8_t* h_out_mask);

// The argument checks every device entry makes after its null checks. noun: what the kind calls a cell in its messages.
int check_frames(const acez_ransac* ctx, int n_frames, int h, int w, const acez_ransac_params* params, bool needs_subsampling,
                 const char* noun);

// The per-hypothesis results of ws's last launch (h_samples: sample_width ints per hypothesis); every output may be null.
int debug_fetch(const acez_ransac* ctx, const Workspace& ws, int n_frames, int hypotheses, int32_t* h_samples, double* h_hyp_poses,
                double* h_scores, int32_t* h_best, double* h_refined);

// A backward pass's buffers beyond a Workspace (one per kind: RGB in ransac_api.hip, RGB-D in ransac_grad.hip): per-hypothesis
// probabilities, losses, refined poses and inlier bitmasks, the per-frame fp64 gradient accumulator and entropy, and the host
// entry's staging.
struct GradWorkspace {
  Workspace ws;                           // sampled poses, scores, samples, HBM lists (best / refined unused)
  double* d_probs = nullptr;              // [frames][hyps]
  double* d_losses = nullptr;             // [frames][hyps]
  double* d_ref_poses = nullptr;          // [frames][hyps][6]
  unsigned long long* d_masks = nullptr;  // [frames][hyps][mask_words]
  double* d_gacc = nullptr;               // [frames][3][cells]
  double* d_entropy = nullptr;            // [frames]
  float* d_gt = nullptr;                  // [frames][16] host-entry staging
  float* d_grad = nullptr;                // [3][cells] host-entry staging
  double* d_loss = nullptr;               // [frames] host-entry staging
  int row_words = 0;                      // the kernel's mask layout, set at acez_ransac_create: one 64-bit word per wavefront and
                                          // row of threads (4 per 256 cells for RGB, 8 per 512 for RGB-D)
  int hyps = 0, mwords = 0, cells = 0;    // capacity
  int last_cells = 0;                     // cells per frame of the last launch
};
// The mask words of one hypothesis for a frame of `cells` cells: the stride g's kernel indexes with and the size ensure_grad allocates.
inline int mask_words(const GradWorkspace& g, int cells) { return (cells + 64 * g.row_words - 1) / (64 * g.row_words) * g.row_words; }
// ensure_grad: every buffer for hyps hypotheses and frames of up to `cells` cells; release_grad: the caller has synchronised.
int ensure_grad(GradWorkspace& g, int hyps, int cells);
void release_grad(GradWorkspace& g);
// After a successful launch: the shape the debug fetch is checked against.
inline void note_launch(GradWorkspace& g, int hyps, int cells) {
  g.ws.last_hyps = hyps;
  g.last_cells = cells;
}

// What a backward kernel reads and writes beyond its forward inputs; embedded in each kind's kernel arguments.
struct GradOut {
  const float* gt;             // [n][16] row-major cam->world ground truth
  float w_rot, w_trans, cut;
  double* probs;               // [n][hyps]
  double* losses;              // [n][hyps]
  double* ref_poses;           // [n][hyps][6]
  unsigned long long* masks;   // [n][hyps][mwords]: bit j % 64 of word j / 64 = entry j (scan order) is a final inlier
  int mwords;
  double* gacc;                // [n][3][N] fp64 accumulator
  double* entropy;             // [n]
  float* out_grad;             // [n][3][H][W], added to
  double* out_loss;            // [n]
};
GradOut make_grad_out(const GradWorkspace& g, int cells, const float* gt, float w_rot, float w_trans, float cut, float* out_grad,
                      double* out_loss);

// The host-buffer backward entries after their inputs are uploaded: stage the ground truth, zero the staged gradient, call
// launch(d_gt, d_grad, d_loss) (the kind's device entry on one frame), download, and add the gradient to the strided h_grad.
int backward_host(GradWorkspace& g, int h, int w, const float* h_gt_pose16, float* h_grad, int64_t g_stride_c, int64_t g_stride_h,
                  int64_t g_stride_w, double* out_loss, const std::function<int(const float*, float*, double*)>& launch);

// The per-hypothesis results of g's last launch, which must have been of h x w frames; every output may be null.
int grad_debug_fetch(const acez_ransac* ctx, const GradWorkspace& g, int n_frames, int hypotheses, int h, int w, int32_t* h_samples,
                     double* h_hyp_poses, double* h_scores, double* h_probs, double* h_losses, double* h_ref_poses,
                     uint64_t* h_mask_words, double* h_entropy);

}  // namespace acez_rs

struct acez_ransac {
  int device = 0;
  int max_frames = 0, max_h = 0, max_w = 0;
  acez_rs::ParamSlot slot[acez_rs::PARAM_SLOTS];
  int next_slot = 0;
  acez_rs::Workspace rgb;   // allocated at acez_ransac_create (64 hypotheses)
  acez_rs::Workspace rgbd;  // allocated at the first RGB-D call
  acez_rs::GradWorkspace rgbd_grad;  // allocated at the first RGB-D backward call
  acez_rs::GradWorkspace rgb_grad;   // allocated at the first RGB backward call
  // staging for the host-buffer entry points
  float* d_sc = nullptr;
  float* d_cc = nullptr;    // RGB-D camera coordinates, allocated at the first RGB-D host call
  float* d_pose = nullptr;
  int* d_inl = nullptr;
  uint8_t* d_mask = nullptr;
};
