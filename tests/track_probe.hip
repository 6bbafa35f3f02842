// track_probe.hip -- TEST INFRASTRUCTURE: exposes the HOST instantiation of the __host__ __device__ tracking update in
// acezero_amd/csrc/track_solve.h so that tests/test_track_cpu.py can compare it with the numpy restatement before anything runs on a
// GPU. Built by the test with `hipcc -ffp-contract=off` (the host pass only is used). Not part of libacez.so.
#include <hip/hip_runtime.h>
#include "../acezero_amd/csrc/track_solve.h"

extern "C" {
int probe_track_solve(const double* totals29, double damping, double* pose12) { return acez::track_solve(totals29, damping, pose12) ? 1 : 0; }
void probe_track_update(double* state45, const double* totals29, double rel_rms, double damping, double min_count, double* history) {
  acez::track_update(state45, totals29, rel_rms, damping, min_count, history);
}
}
