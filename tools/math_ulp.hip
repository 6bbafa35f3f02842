// math_ulp.hip -- worst error, in ulps of the fp32 result, of the device math calls of the head's loss stage (head_kernels.hip loss_body:
// expf, log1pf, tanhf, logf, sqrtf, and the fp32 division) against the host's float64 functions, over the argument ranges the cases of
// tests/loss_stage_cases.py reach. The bounds of tests/golden/parity_tolerances.json ("loss_stage_math_ulps") are these figures plus one.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/math_ulp.hip -o tools/math_ulp.bin && tools/math_ulp.bin
// (the flags of acezero_amd/build.py's head units: no fast-math, so hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt holds and
// `/` and sqrtf are IEEE correctly rounded -- what IvArith._pointwise of tests/loss_stage_restated.py relies on, and what the 0.5 ulp
// measured here confirms; contraction as the compiler likes). One JSON line on stdout.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

enum { F_EXP = 0, F_LOG1P, F_TANH, F_LOG, F_SQRT, F_RCP, F_COUNT };

__global__ void eval_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  float r;
  switch (f) {
    case F_EXP: r = expf(v); break;
    case F_LOG1P: r = log1pf(v); break;
    case F_TANH: r = tanhf(v); break;
    case F_LOG: r = logf(v); break;
    case F_SQRT: r = sqrtf(v); break;
    default: r = x[n - 1 - i] / v; break;   // numerator and denominator both sweep the range, in opposite directions
  }
  y[i] = r;
}

static double ref(int f, double v) {
  switch (f) {
    case F_EXP: return exp(v);
    case F_LOG1P: return log1p(v);
    case F_TANH: return tanh(v);
    case F_LOG: return log(v);
    case F_SQRT: return sqrt(v);
    default: return 0.0;   // (the division: main() forms the quotient of the two arguments)
  }
}

int main() {
  // name, range, spacing (0 linear, 1 geometric)
  struct Case { const char* name; int f; double lo, hi; int geometric; };
  const Case cases[] = {
    {"expf", F_EXP, -64.0, 20.0, 0},          // bx = h_beta * s3 below the softplus threshold
    {"log1pf", F_LOG1P, 1e-28, 5e8, 1},       // log1p(exp(bx))
    {"tanhf", F_TANH, 1e-6, 1100.0, 1},       // e / wgt, e <= hard_clamp, wgt >= soft_clamp_min
    {"logf", F_LOG, 1.0, 1e5, 1},             // 1 + wgt * e
    {"sqrtf", F_SQRT, 1e-12, 1e8, 1},         // wgt * e, |target - X|^2
    {"div", F_RCP, 1e-6, 1e6, 1},             // the plain fp32 division x[n - 1 - i] / x[i]: quotients from 1e-12 to 1e12
  };
  const int n = 1 << 22;
  std::vector<float> hx(n), hy(n);
  float *dx = nullptr, *dy = nullptr;
  CHECK(hipMalloc(&dx, n * sizeof(float)));
  CHECK(hipMalloc(&dy, n * sizeof(float)));
  printf("{");
  for (size_t c = 0; c < sizeof(cases) / sizeof(cases[0]); ++c) {
    const Case& k = cases[c];
    for (int i = 0; i < n; ++i) {
      const double t = (i + 0.5) / n;
      hx[i] = (float)(k.geometric ? k.lo * pow(k.hi / k.lo, t) : k.lo + (k.hi - k.lo) * t);
    }
    CHECK(hipMemcpy(dx, hx.data(), n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(eval_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, n, k.f);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(hy.data(), dy, n * sizeof(float), hipMemcpyDeviceToHost));
    double worst = 0.0, at = 0.0;
    for (int i = 0; i < n; ++i) {
      const double r = k.f == F_RCP ? (double)hx[n - 1 - i] / (double)hx[i] : ref(k.f, (double)hx[i]);
      if (!(fabs(r) >= 1.1754943508222875e-38)) continue;   // a result below the smallest normal has no ulp to speak of
      int ex;
      frexp(r, &ex);                                        // |r| in [2^(ex-1), 2^ex): ulp = 2^(ex - 24)
      const double u = fabs((double)hy[i] - r) / ldexp(1.0, ex - 24);
      if (u > worst) { worst = u; at = hx[i]; }
    }
    printf("%s\"%s\": {\"worst_ulps\": %.4f, \"at\": %.9g, \"lo\": %g, \"hi\": %g, \"samples\": %d}", c ? ", " : "", k.name, worst, at, k.lo, k.hi, n);
  }
  printf("}\n");
  (void)hipFree(dx);
  (void)hipFree(dy);
  return 0;
}
