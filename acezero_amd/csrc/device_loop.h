// device_loop.h -- what the device-resident iterated solvers (icp_solve.h, track_solve.h) share: a loop is enqueued as max_iterations
// ACCUMULATE + UPDATE launches without a host round trip, and a launch after the loop has stopped returns at once. The state starts
// with 16 doubles of one layout (14 and 15, the "previous" values, are each solver's own), then the last totals; a history record is
// 16 doubles that start with the pose. Host + device.
#pragma once
#include <hip/hip_runtime.h>

namespace acez {

constexpr int LOOP_POSE = 0, LOOP_STATUS = 12, LOOP_COUNT = 13, LOOP_TOTALS = 16;     // pose: 12 doubles; count: the records written
constexpr int LOOP_RECORD = 16;      // doubles per history record
constexpr double LOOP_RUNNING = 0.0, LOOP_CONVERGED = 1.0, LOOP_DEGENERATE = 2.0;

// UPDATE runs: the loop has not stopped and has a record left. Written with >= and <, so that a count that is NaN stops it.
__host__ __device__ inline bool loop_live(const double* state, int max_iterations) {
  const double count = state[LOOP_COUNT];
  return state[LOOP_STATUS] == LOOP_RUNNING && count >= 0.0 && count < (double)max_iterations;
}

}  // namespace acez
