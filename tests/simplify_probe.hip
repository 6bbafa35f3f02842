// simplify_probe.hip -- TEST INFRASTRUCTURE: exposes the HOST instantiation of the __host__ __device__ placement of the mesh
// simplification (acezero_amd/csrc/simplify_solve.h, with acezero_amd/csrc/svd3.h under it) so that tests/test_simplify_cpu.py can
// compare it with the restatement bit for bit before anything runs on a GPU. Built by the test with `hipcc -ffp-contract=off` (the
// host pass only is used). Not part of libacez.so.
#include <hip/hip_runtime.h>
#include "../acezero_amd/csrc/simplify_solve.h"

extern "C" {
int probe_simplify_solve(const double* q9, const double* mean3, double cell, double* x3) {
  return acez::simplify_solve(q9, mean3, cell, x3) ? 1 : 0;
}
void probe_simplify_add_corner(const double* a3, const double* b3, const double* c3, double* q9) {
  acez::simplify_add_corner(a3, b3, c3, q9);
}
void probe_svd3(const double* C9, double* u9, double* v9, double* s3) {
  acez::Svd3 d;
  acez::svd3(C9, d);
  for (int i = 0; i < 3; ++i) {
    s3[i] = d.s[i];
    for (int r = 0; r < 3; ++r) {
      u9[3 * i + r] = d.u[i][r];
      v9[3 * i + r] = d.v[i][r];
    }
  }
}
}
