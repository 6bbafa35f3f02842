// ransac_ctx.h -- the registration context (acez_ransac) shared by the RGB (ransac_api.hip) and RGB-D (ransac_rgbd.hip)
// DSAC* kernels: one ring of per-call frame-parameter slots, the RGB workspaces, and the RGB-D workspaces hung off it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace acez_rs {

struct FrameParam {
  float focal, ppx, ppy, pad;
  uint64_t frame_id;
};

constexpr int PARAM_SLOTS = 4;
// One pinned + device copy of the per-frame parameter block per call in flight: a device entry point never waits for the
// stream it launches on (only for the call PARAM_SLOTS launches ago, whose kernel has long finished in any pipelined use).
struct ParamSlot {
  FrameParam* h = nullptr;  // pinned
  FrameParam* d = nullptr;
  hipEvent_t done = nullptr;
  bool in_flight = false;
};

struct RgbdState;                 // ransac_rgbd.hip: created on the first RGB-D call
void rgbd_release(RgbdState* s);  // frees its buffers (the caller has synchronised the device)

}  // namespace acez_rs

struct acez_ransac {
  int device = 0;
  int max_frames = 0, max_h = 0, max_w = 0, max_hyps = 0;
  acez_rs::ParamSlot slot[acez_rs::PARAM_SLOTS];
  int next_slot = 0;
  double* d_hyp_poses = nullptr;
  double* d_scores = nullptr;
  int* d_best = nullptr;
  double* d_refined = nullptr;
  float* d_big = nullptr;      // scan-order copies of frames that do not fit the LDS, allocated on first use
  size_t big_floats = 0;
  // staging for the host-buffer entry point
  float* d_sc = nullptr;
  float* d_pose = nullptr;
  int* d_inl = nullptr;
  uint8_t* d_mask = nullptr;
  int last_hyps = 0;
  acez_rs::RgbdState* rgbd = nullptr;
};
