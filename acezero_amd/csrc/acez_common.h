// acez_common.h -- error plumbing shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include "../../include/acez.h"

namespace acez {
void set_error(const char* fmt, ...);
// ACEZ_OK if a HIP device is visible; else ACEZ_ERR_NODEVICE with the error "no HIP device visible: <what> (there is no CPU fallback)"
int require_device(const char* what);
}

#define ACEZ_HIP_CHECK(expr)                                                                   \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      acez::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return ACEZ_ERR_HIP;                                                                     \
    }                                                                                          \
  } while (0)

#define ACEZ_REQUIRE(cond, msg)                          \
  do {                                                   \
    if (!(cond)) {                                       \
      acez::set_error("invalid argument: %s", msg);      \
      return ACEZ_ERR_INVALID;                           \
    }                                                    \
  } while (0)

// Diagnostics build (-DACEZ_DIAG; acezero_amd/build.py builds it as libacez_diag.so for tests/ and tools/): the switches to the reference
// flows the tests compare against, the side-stream pose launches of round 2, the device timelines and the fault-injection hooks exist only
// there (the measured-and-rejected kernels of rounds 1-5 -- chain_kernel, headfwd_kernel, headinfer_kernel, the 128-row rowgemm tiling,
// wgrad256_kernel, conv12_kernel, conv3x3p_kernel -- and the timing-only ablation switches live in the git history and in
// DESIGN_HISTORY.md, not in the tree). In the product library ACEZ_DIAG_ENV() is a null constant -- every
// `if (const char* e = ACEZ_DIAG_ENV("..."))` folds away -- and no environment variable can change a result. The product reads exactly three
// variables (head_api.hip): ACEZ_SEQ=0 (per-layer launches instead of the one-launch chains; bit-identical results), ACEZ_LOSS_IN_CHAIN=0
// (the fused step's loss as a launch of its own instead of stage -1 of the input-gradient launch; bit-identical results) and
// ACEZ_SEQ_SPIN_US (the hand-off poll budget).
#ifdef ACEZ_DIAG
#include <stdlib.h>
#define ACEZ_DIAG_ENV(name) getenv(name)
constexpr bool kAcezDiag = true;
#else
#define ACEZ_DIAG_ENV(name) (static_cast<const char*>(nullptr))
constexpr bool kAcezDiag = false;
#endif
