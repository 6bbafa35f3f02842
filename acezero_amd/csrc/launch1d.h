// launch1d.h -- what the units that launch one lane per row share (geometry_api.hip, surface_api.hip, mesh_api.hip, simplify_api.hip):
// the largest row count, the grid of a launch and the count requirements with their messages. Host code only.
#pragma once
#include <stdint.h>
#include <initializer_list>

#include "acez_common.h"

namespace acez {

constexpr int64_t ACEZ_MAX_COUNT = ((int64_t)1 << 31) - 1;

inline unsigned blocks_for(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

inline bool counts_ok(std::initializer_list<int64_t> counts) {
  for (const int64_t n : counts)
    if (n < 0 || n > ACEZ_MAX_COUNT) return false;
  return true;
}

}  // namespace acez

// every count in 0 .. 2^31 - 1, or ACEZ_ERR_INVALID: rows of any kind, and points
#define ACEZ_REQUIRE_COUNTS(...) ACEZ_REQUIRE(acez::counts_ok({__VA_ARGS__}), "count out of range (0 .. 2^31 - 1)")
#define ACEZ_REQUIRE_POINT_COUNTS(...) ACEZ_REQUIRE(acez::counts_ok({__VA_ARGS__}), "point count out of range (0 .. 2^31 - 1)")
