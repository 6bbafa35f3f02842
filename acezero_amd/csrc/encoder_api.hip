// encoder_api.hip -- the ACE feature encoder (ace_network.py:14-59) on gfx950: its context (weights repacked for the kernels, the
// intermediate maps) and its C ABI (include/acez.h). The kernels and their launchers are in conv_kernels.hip (conv_launch.h).
//
// the encoder is the step right before both hot paths (it fills the training buffer and it
// produces the features the head turns into scene coordinates at registration time).
//
// Data layout: activations NHWC 16-bit ([frame][y][x][channel]: the final [F*h*w][512] tensor is exactly the row layout of the training
// buffer / acez_head_forward). Weights: 16-bit [Co][Kp], k = (ky*3 + kx) * Ci + ci, Kp = K rounded up to 64 (zero padded). The context's
// compute_dtype selects the kernels' element type (bf16 or fp16 operands, fp32 accumulation, one rounding per layer output).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/acez.h"
#include "acez_common.h"
#include "conv_launch.h"

using namespace acez;

namespace {

struct LayerDesc {
  const char* name;
  int ci, co, k, stride;
};
// Encoder.__init__ order (ace_network.py:26-40); co of the last two layers is the configurable feature size
const LayerDesc kLayers[ACEZ_ENCODER_LAYERS] = {
    {"conv1", 1, 32, 3, 1},         {"conv2", 32, 64, 3, 2},        {"conv3", 64, 128, 3, 2},       {"conv4", 128, 256, 3, 2},
    {"res1_conv1", 256, 256, 3, 1}, {"res1_conv2", 256, 256, 1, 1}, {"res1_conv3", 256, 256, 3, 1}, {"res2_conv1", 256, 512, 3, 1},
    {"res2_conv2", 512, 512, 1, 1}, {"res2_conv3", 512, 512, 3, 1}, {"res2_skip", 256, 512, 1, 1}};

uint16_t host_f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
// fp32 -> IEEE half, round to nearest even (what torch .half() / v_cvt_f16_f32 do; overflow -> inf)
uint16_t host_f2h(float f) {
  const _Float16 h = (_Float16)f;
  uint16_t u;
  memcpy(&u, &h, 2);
  return u;
}

}  // namespace

struct acez_encoder {
  int device = 0, out_channels = 512, max_frames = 0, max_h = 0, max_w = 0, tile_mode = 0;
  bool f16 = false;                    // 16-bit operand format of every layer: bf16, or fp16 (what the reference's autocast runs the encoder in,
                                       // ace_trainer.py:366-367, register_mapping.py:209-210); fp32 accumulation in both
  uint16_t* w1b = nullptr;             // conv1 weights 16-bit [32][16] (k = tap, zero padded): A operand of conv12p_kernel
  float* bias[ACEZ_ENCODER_LAYERS] = {};
  uint16_t* W[ACEZ_ENCODER_LAYERS] = {};   // 16-bit [co][Kp] (layers 1..10)
  int K[ACEZ_ENCODER_LAYERS] = {}, Kp[ACEZ_ENCODER_LAYERS] = {}, co[ACEZ_ENCODER_LAYERS] = {};
  uint16_t* zeros = nullptr;
  uint16_t *a2 = nullptr, *a3 = nullptr, *r4 = nullptr, *x5 = nullptr, *x6 = nullptr, *r7 = nullptr, *x8 = nullptr,
           *x9 = nullptr, *sk = nullptr;
  std::vector<void*> allocs;
};

extern "C" void acez_encoder_destroy(acez_encoder* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  for (void* p : e->allocs) (void)hipFree(p);
  delete e;
}

extern "C" int acez_encoder_create(acez_encoder** out, const float* const* h_weights, const float* const* h_biases, int out_channels,
                                   int max_frames, int max_h, int max_w, int compute_dtype, int device) {
  ACEZ_REQUIRE(out && h_weights && h_biases, "null pointer");
  ACEZ_REQUIRE(out_channels > 0 && out_channels % 128 == 0, "out_channels must be a positive multiple of 128");
  ACEZ_REQUIRE(max_frames > 0 && max_h >= 8 && max_w >= 8, "bad capacity");
  ACEZ_REQUIRE(compute_dtype == ACEZ_DTYPE_BF16 || compute_dtype == ACEZ_DTYPE_FP16, "compute_dtype must be ACEZ_DTYPE_BF16 or ACEZ_DTYPE_FP16");
  for (int i = 0; i < ACEZ_ENCODER_LAYERS; ++i) ACEZ_REQUIRE(h_weights[i] && h_biases[i], "null layer pointer");
  if (int rc = acez::require_device("the encoder kernels need a gfx950 GPU")) return rc;
  if (device < 0) ACEZ_HIP_CHECK(hipGetDevice(&device));
  ACEZ_HIP_CHECK(hipSetDevice(device));
  acez_encoder* e = new acez_encoder();
  e->device = device; e->out_channels = out_channels; e->max_frames = max_frames; e->max_h = max_h; e->max_w = max_w;
  if (const char* tm = ACEZ_DIAG_ENV("ACEZ_CONV_TILE")) e->tile_mode = atoi(tm);
  e->f16 = compute_dtype == ACEZ_DTYPE_FP16;
  auto cvt = [&](float f) { return e->f16 ? host_f2h(f) : host_f2bf(f); };
  auto A = [&](void** p, size_t bytes) -> hipError_t {
    hipError_t rc = hipMalloc(p, bytes);
    if (rc == hipSuccess) e->allocs.push_back(*p);
    return rc;
  };
#define ACEZ_ENC_ALLOC(ptr, bytes)                                   \
  do {                                                               \
    hipError_t rc_ = A((void**)&(ptr), (bytes));                     \
    if (rc_ != hipSuccess) {                                         \
      acez::set_error("hipMalloc failed: %s", hipGetErrorString(rc_)); \
      acez_encoder_destroy(e);                                       \
      return ACEZ_ERR_HIP;                                           \
    }                                                                \
  } while (0)
  ACEZ_ENC_ALLOC(e->zeros, 256);
  ACEZ_HIP_CHECK(hipMemset(e->zeros, 0, 256));
  for (int i = 0; i < ACEZ_ENCODER_LAYERS; ++i) {
    const LayerDesc& L = kLayers[i];
    const int co = (i >= 9) ? out_channels : L.co;
    e->co[i] = co;
    const int K = L.k * L.k * L.ci;
    e->K[i] = K; e->Kp[i] = (K + 63) / 64 * 64;
    ACEZ_ENC_ALLOC(e->bias[i], (size_t)co * sizeof(float));
    {
      // fp16: autocast hands conv2d its bias in half precision too (the kernels add it in fp32 to the fp32 accumulator, as cuDNN's fused
      // epilogue does); bf16 keeps the fp32 values
      std::vector<float> b(h_biases[i], h_biases[i] + co);
      if (e->f16)
        for (float& v : b) v = (float)(_Float16)v;
      ACEZ_HIP_CHECK(hipMemcpy(e->bias[i], b.data(), (size_t)co * sizeof(float), hipMemcpyHostToDevice));
    }
    if (i == 0) {
      std::vector<uint16_t> wb(32 * 16, 0);   // [co][1][3][3] is already [co][tap]
      for (int o = 0; o < 32; ++o)
        for (int tp = 0; tp < 9; ++tp) wb[o * 16 + tp] = cvt(h_weights[0][o * 9 + tp]);
      ACEZ_ENC_ALLOC(e->w1b, wb.size() * sizeof(uint16_t));
      ACEZ_HIP_CHECK(hipMemcpy(e->w1b, wb.data(), wb.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    } else {
      // torch layout [co][ci][ky][kx] -> [co][(ky*k + kx) * ci_n + ci], zero padded to Kp
      std::vector<uint16_t> w((size_t)co * e->Kp[i], 0);
      const int kk = L.k * L.k;
      for (int o = 0; o < co; ++o)
        for (int c = 0; c < L.ci; ++c)
          for (int tp = 0; tp < kk; ++tp)
            w[(size_t)o * e->Kp[i] + (size_t)tp * L.ci + c] = cvt(h_weights[i][((size_t)o * L.ci + c) * kk + tp]);
      ACEZ_ENC_ALLOC(e->W[i], w.size() * sizeof(uint16_t));
      ACEZ_HIP_CHECK(hipMemcpy(e->W[i], w.data(), w.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
  }
  const size_t F = max_frames;
  const size_t h2 = (max_h + 1) / 2, w2 = (max_w + 1) / 2, h4 = (h2 + 1) / 2, w4 = (w2 + 1) / 2, h8 = (h4 + 1) / 2, w8 = (w4 + 1) / 2;
  ACEZ_ENC_ALLOC(e->a2, F * h2 * w2 * 64 * 2);
  ACEZ_ENC_ALLOC(e->a3, F * h4 * w4 * 128 * 2);
  const size_t px = F * h8 * w8;
  ACEZ_ENC_ALLOC(e->r4, px * 256 * 2);
  ACEZ_ENC_ALLOC(e->x5, px * 256 * 2);
  ACEZ_ENC_ALLOC(e->x6, px * 256 * 2);
  ACEZ_ENC_ALLOC(e->r7, px * 256 * 2);
  ACEZ_ENC_ALLOC(e->x8, px * 512 * 2);
  ACEZ_ENC_ALLOC(e->x9, px * 512 * 2);
  ACEZ_ENC_ALLOC(e->sk, px * (size_t)out_channels * 2);
#undef ACEZ_ENC_ALLOC
  *out = e;
  return ACEZ_OK;
}

extern "C" int acez_encoder_output_size(int h, int w, int* out_h, int* out_w) {
  ACEZ_REQUIRE(out_h && out_w && h > 0 && w > 0, "bad argument");
  int hh = h, ww = w;
  for (int i = 0; i < 3; ++i) { hh = (hh + 1) / 2; ww = (ww + 1) / 2; }   // three 3x3 stride-2 pad-1 convolutions
  *out_h = hh; *out_w = ww;
  return ACEZ_OK;
}

extern "C" int acez_encoder_forward(acez_encoder* e, const float* d_images, int n_frames, int h, int w, void* d_features, void* stream) {
  ACEZ_REQUIRE(e && d_images && d_features, "null pointer");
  ACEZ_REQUIRE(n_frames > 0 && h >= 8 && w >= 8 && h <= e->max_h && w <= e->max_w, "frame size out of the context's capacity");
  ACEZ_HIP_CHECK(hipSetDevice(e->device));
  hipStream_t s = (hipStream_t)stream;
  const int h2 = (h + 1) / 2, w2 = (w + 1) / 2, h4 = (h2 + 1) / 2, w4 = (w2 + 1) / 2, h8 = (h4 + 1) / 2, w8 = (w4 + 1) / 2;
  for (int f0 = 0; f0 < n_frames; f0 += e->max_frames) {
    const int F = (n_frames - f0 < e->max_frames) ? n_frames - f0 : e->max_frames;
    const float* img = d_images + (size_t)f0 * h * w;
    uint16_t* feat = (uint16_t*)d_features + (size_t)f0 * h8 * w8 * e->out_channels;
    {
      Conv12Args c{};
      c.img = img; c.w1 = e->w1b; c.b1 = e->bias[0]; c.w2 = e->W[1]; c.b2 = e->bias[1]; c.out = e->a2;
      c.F = F; c.H = h; c.W = w; c.H2 = h2; c.W2 = w2; c.Kp2 = e->Kp[1]; c.zero = reinterpret_cast<const float*>(e->zeros);
      c.tiles_x = (w2 + 31) / 32;
      launch_conv12p(c, e->f16, s);
    }
    auto conv = [&](int li, const uint16_t* in, int hi, int wi, uint16_t* outp, int ho, int wo, const uint16_t* add, bool relu, int skip_li = -1,
                    const uint16_t* skip_in = nullptr, int next_li = -1) {
      const LayerDesc& L = kLayers[li];
      ConvGemmArgs g{};
      if (next_li >= 0) {
        g.W2 = e->W[next_li]; g.bias2 = e->bias[next_li]; g.Kp2 = e->Kp[next_li]; g.skip_scratch = e->x5;
      }
      if (skip_li >= 0) {
        g.In2 = skip_in; g.W2 = e->W[skip_li]; g.bias2 = e->bias[skip_li]; g.Ci2 = kLayers[skip_li].ci; g.Kp2 = e->Kp[skip_li]; g.skip_scratch = e->sk;
      }
      g.In = in; g.W = e->W[li]; g.bias = e->bias[li]; g.add = add; g.out = outp; g.zeros = e->zeros;
      g.Hi = hi; g.Wi = wi; g.Ci = L.ci; g.ci_shift = __builtin_ctz(L.ci); g.Ho = ho; g.Wo = wo; g.Co = e->co[li];
      g.ksize = L.k; g.stride = L.stride; g.pad = L.k / 2; g.K = e->K[li]; g.Kp = e->Kp[li]; g.M = F * ho * wo; g.f16 = e->f16 ? 1 : 0;
      // fp16 = the reference's arithmetic: relu(conv(x)) is a half tensor BEFORE `res + x` / `skip + x` (ace_network.py:52,58), so the
      // activation is rounded before the residual is added and the sum is rounded again; bf16 keeps its single rounding of the fp32 sum
      g.round_before_add = e->f16 ? 1 : 0;
      launch_convgemm(g, relu, s, e->tile_mode);
    };
    conv(2, e->a2, h2, w2, e->a3, h4, w4, nullptr, true);
    conv(3, e->a3, h4, w4, e->r4, h8, w8, nullptr, true);
    // relu(res1_conv2(relu(res1_conv1(res))))  (ace_network.py:48-49): the pointwise layer back to back on res1_conv1's tiles where that
    // layer runs on conv3x3r (two launches through e->x5 on small inputs)
    conv(4, e->r4, h8, w8, e->x6, h8, w8, nullptr, true, -1, nullptr, 5);
    conv(6, e->x6, h8, w8, e->r7, h8, w8, e->r4, true);     // res = res + relu(res1_conv3(x))      ace_network.py:50-52
    conv(7, e->r7, h8, w8, e->x8, h8, w8, nullptr, true);
    conv(8, e->x8, h8, w8, e->x9, h8, w8, nullptr, true);
    // res2_skip(res) + relu(res2_conv3(x))  (ace_network.py:57-58): the skip rides as extra K stages of res2_conv3 where that layer runs on
    // conv3x3r (launch_convgemm falls back to two launches through e->sk on small inputs)
    conv(9, e->x9, h8, w8, feat, h8, w8, nullptr, true, 10, e->r7);
  }
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
