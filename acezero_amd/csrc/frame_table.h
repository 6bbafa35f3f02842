// frame_table.h -- the frame table of the fusion and the stereo entry points (include/acez.h: acez_tsdf_frame, which acez_mvs_frame is a
// typedef of) on the host: the checks of a row and the copy to the device. fusion_api.hip, mvs_api.hip.
#pragma once
#include <math.h>
#include <stdint.h>

#include "acez_common.h"

namespace acez {

constexpr int FRAME_MAX_SIDE = 32768;

inline bool finite_all(const float* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!isfinite(p[i])) return false;
  return true;
}

// one row against the packed buffer of n_pixels elements its offset points into: what bounds every index a kernel forms from it
inline int check_frame(const acez_tsdf_frame& fr, int64_t n_pixels) {
  ACEZ_REQUIRE(fr.h >= 1 && fr.w >= 1 && fr.h <= FRAME_MAX_SIDE && fr.w <= FRAME_MAX_SIDE, "frame size out of range (1 .. 32768 px per side)");
  ACEZ_REQUIRE(finite_all(fr.m, 12) && isfinite(fr.focal) && isfinite(fr.ppx) && isfinite(fr.ppy), "non-finite pose or intrinsics in the frame table");
  ACEZ_REQUIRE(fr.focal > 0.0f, "focal length must be positive");
  ACEZ_REQUIRE(fr.offset >= 0 && fr.offset <= n_pixels && (int64_t)fr.h * fr.w <= n_pixels - fr.offset, "frame past the end of the buffer");
  return ACEZ_OK;
}

// the first n rows into the caller's device scratch, in stream order before whatever is launched next
inline int upload_frames(acez_tsdf_frame* d_frames, const acez_tsdf_frame* h_frames, int n, hipStream_t stream) {
  ACEZ_HIP_CHECK(hipMemcpyAsync(d_frames, h_frames, sizeof(acez_tsdf_frame) * (size_t)n, hipMemcpyHostToDevice, stream));
  ACEZ_HIP_CHECK(hipStreamSynchronize(stream));   // h_frames is the caller's again
  return ACEZ_OK;
}

}  // namespace acez
