// icp_probe.hip -- TEST INFRASTRUCTURE: exposes the HOST instantiation of the __host__ __device__ ICP update in
// acezero_amd/csrc/icp_solve.h so that tests/test_icp_cpu.py can compare it with the numpy restatement before anything runs on a GPU.
// Built by the test with `hipcc -ffp-contract=off` (the host pass only is used). Not part of libacez.so.
#include <hip/hip_runtime.h>
#include "../acezero_amd/csrc/icp_solve.h"

extern "C" {
int probe_icp_solve(const double* totals18, const double* pivot3, int with_scale, double* T12) {
  return acez::icp_solve(totals18, pivot3, with_scale, T12) ? 1 : 0;
}
void probe_icp_update(double* state34, const double* totals18, int64_t n, const double* pivot3, int with_scale, double rel_fitness,
                      double rel_rmse, double* history) {
  acez::icp_update(state34, totals18, n, pivot3, with_scale, rel_fitness, rel_rmse, history);
}
}
