// conv3x3r.h -- conv3x3r_kernel, included by conv_kernels.hip (one function of 400 lines: it reads better in a file of its own).
// ---------------------------------------------------------------------------------------------------
// The 3 x 3, stride-1 layers (res1_conv1/3, res2_conv1/3 = 85 % of the encoder's FLOPs) with the INPUT kept as an LDS patch (round 1's
// conv3x3p, the first kernel of this shape, is in the git history). In the implicit-GEMM kernels of conv_kernels.hip every tap's K
// stages DMA the same input pixels again (nine times per
// 32-channel chunk); here the loaders bring, per 32-channel chunk, ONE patch of 448 consecutive input pixels (the tile's 256
// output pixels in (frame, y, x) order plus one image row and one pixel on either side: NHWC frames are back to back, so
// "pixel p + (ky-1) * W + (kx-1)" is a plain linear offset and padding is a per-lane validity bit), and the nine tap stages
// of that chunk only stream weights. L2 -> LDS bytes per 32-wide K stage: 16 KiB of weights + 28 KiB / 9 of patch instead
// of 32 KiB. The multipliers read their B fragments straight from the patch (row q = output row + ky * W + kx, 16-byte chunk
// XOR (q >> 2) & 3: conflict free for the unit-stride rows of a fragment; invalid taps read a zero row).
// Tile 256 x 256, 8 multiplier + 4 loader waves, 4-slot weight ring (64 KiB) + 2 patch buffers (56 KiB); the epilogue tile
// takes the whole 128 KiB. Requires W <= 95 (448-row patch), Ci % 32 == 0, Co % 256 == 0.
// ---------------------------------------------------------------------------------------------------
#pragma once
#include <type_traits>

#include "conv_tiles.h"

namespace acez {

constexpr int P3_ROWS = 448;

// ---------------------------------------------------------------------------------------------------
// conv3x3r: the lean stage loop (round 2). Ablation of conv3x3p on MI355X (tools/enc_kstats.sh, git history): with the LDS-DMA AND
// the MFMAs switched off the 3x3 kernels still take 50 % of their time; loads add 10 %, MFMAs 40 %. The "skeleton" is the stage
// loop itself: per 32-wide K stage a wave executes ~180 scalar / vector / branch instructions (tap decode, nine-way validity
// selects, swizzled fragment addresses, the vmcnt switch, slot arithmetic) around its 16 MFMAs -- ~1250 cycles of in-order issue
// against 512 cycles of matrix work. Here everything that does not change is computed once per lane and kept in registers:
//   * tapaddr[tap][j]: LDS byte address of B fragment j for tap `tap` in patch slot 0 (validity folded in: padded taps point at a
//     zero row inside the slot); the second 16-wide K step is `address ^ 32`, the other patch slot `address ^ 0x8000` (the slots
//     are 32 KiB apart, flipped once per chunk);
//   * the nine taps are unrolled, so tap, validity and the vmcnt of a stage are compile-time constants; the last 32-channel chunk
//     has its own copy of the nine stage bodies (no branches on "is there a next stage / a next patch");
//   * DMA source pointers advance by scalar increments.
// A stage is then 16 MFMAs + 12 ds_read_b128 + 2 global_load_lds + ~14 VALU + ~10 SALU + one barrier. Eight waves that multiply and
// load their own operands (2 weight + amortised 0.5 patch DMA instructions per wave and stage), fragments double-buffered in
// registers (while the 8 MFMAs of one 16-wide K step run, the 6 fragment reads of the next are in flight; that alone, on top of
// conv3x3p's loop, measured +1 %: the loop's instruction count was the limiter, not LDS latency). Same tile, same K order, same
// rounding as conv3x3p.
// LDS (bytes): [0, 64 K) four weight slots; [64 K, 96 K) and [96 K, 128 K) patch slots of 512 rows x 64 B (rows 0..447 data, row 511
// zero); the epilogue tile reuses all 128 KiB.
// ---------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) unsigned char lds_byte;
// SKIP (res2_conv3 + res2_skip, ace_network.py:57-58: x = res2_skip(res) + relu(res2_conv3(x))): after the last 3 x 3 stage the bias and
// the ReLU are applied to the accumulators IN REGISTERS, then Ci2 / 32 more stages multiply the skip layer's weights with its input at
// the tile's own 256 pixels onto the same accumulators -- the separate pointwise launch (159 us per 64 frames at 0.20 of the MFMA peak),
// its 16-bit output map and the epilogue's read of it (315 MB each way) are gone for +5.5 % of K. Skip stages live in a ring of four
// 32 KiB slots (16 KiB weights + 16 KiB input rows, the layouts of a weight slot / of patch rows): the patch slot the last chunk does
// not use takes stage 0 while the last chunk still multiplies; stages 1-3 go out behind the K loop's last barrier, under the
// bias / ReLU pass and stage 0's products. The skip product is not rounded on its own (the reference's half tensor is; one rounding less).
// B2B (res1_conv1 + res1_conv2, ace_network.py:48-49): a 256-channel layer's whole output row fits the 256 x 256 tile, so the pointwise
// layer that follows runs back to back on the finished tile -- out = relu(W2 . relu(conv3x3(In) + bias) + bias2): the 16-bit tile in LDS
// (rounded exactly as the unfused layer stores it) is the B operand, W2's fragments come straight from L2 in the MFMA operand layout (a lane's
// eight K elements are 16 contiguous bytes of a weight row; 256 KiB per tile, no ring, no barrier inside the product), the second
// accumulators replace the first. The 157 MB intermediate map is neither written nor read and the 83 us launch is gone.
template <class E, bool RELU, bool HAS_ADD, bool SKIP = false, bool B2B = false>
__global__ __launch_bounds__(512) void conv3x3r_kernel(ConvGemmArgs a) {
  static_assert(!(SKIP && HAS_ADD), "the fused skip replaces the residual add");
  static_assert(!(B2B && (SKIP || HAS_ADD)), "back-to-back pointwise layer: plain 3 x 3 layer in front");
  typedef typename E::frag frag;
  typedef __attribute__((address_space(3))) const frag lds_frag;
  constexpr unsigned WSLOT = 16384, PATCH0 = 65536, PSLOT = 32768, ZROW = 511 * 64;
  __shared__ __attribute__((aligned(16))) uint16_t smem[65536];
  lds_byte* const lds = (lds_byte*)smem;
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int M = a.M, Kp = a.Kp, Wi = a.Wi;
  int mt, n0, m0;
  if (!tile_decode<256, 256>(M, a.Co, mt, n0, m0)) return;
  const int NC = a.Ci >> 5;                   // 32-channel chunks; stage s = 9 * chunk + tap
  // (Round 6: walking the chunks from a workgroup-dependent start -- the rotation that takes the head's whole-frame kernel off its L2-channel
  // queue, head_maps.hip -- was measured here and is 5-6 % SLOWER: 350 -> 370 us (res1_conv1), 1168 -> 1243 us (res2_conv3). These weight
  // panels are 1.2-4.7 MB; in lockstep every workgroup asks for the same lines at the same time and one fill serves all of them.)
  if (t < 32) {                               // the zero rows of both patch slots (visible after the first barrier)
    *(__attribute__((address_space(3))) unsigned*)(lds + PATCH0 + (t >> 4) * PSLOT + ZROW + (t & 15) * 4) = 0u;
    __builtin_amdgcn_s_waitcnt(0xC07F);
  }

  // ---- LDS-DMA: this wave's share. A DMA instruction covers 16 rows x 64 bytes; lane: row l >> 2, 16-byte chunk l & 3
  const int lrow = l >> 2, lch = l & 3;
  const uint16_t* gW[2];                      // running source pointers of the next weight stage to issue
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = (w * 2 + j) * 16 + lrow;
    gW[j] = a.W + (size_t)(n0 + row) * Kp + (lch ^ ((row >> 2) & 3)) * 8;
  }
  const uint16_t* gP[4];                      // running source pointers of the next patch to issue
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (w * 4 + (w == 7 ? 0 : j)) * 16 + lrow;   // wave 7 would cover rows 448..511 (padding + the zero row): it repeats rows 448..463
    const int g = min(max(m0 - Wi - 1 + row, 0), M - 1);
    gP[j] = a.In + ((size_t)g << a.ci_shift) + (lch ^ ((row >> 2) & 3)) * 8;
  }
  unsigned wdst = 0;                          // LDS byte offset of the slot the next weight stage goes to
  int wtap = 0;                               // its tap
  const int w_step = a.Ci, w_wrap = 32 - 8 * a.Ci;   // element increments of the weight pointers: next tap / next chunk
  auto issue_w = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      __builtin_amdgcn_global_load_lds((gvoid_t*)gW[j], (lvoid_t*)(lds + wdst + (w * 2 + j) * 1024), 16, 0, 0);
      gW[j] += (wtap == 8) ? w_wrap : w_step;
    }
    wtap = (wtap == 8) ? 0 : wtap + 1;
    wdst = (wdst + WSLOT) & (4 * WSLOT - 1);
  };
  unsigned pdst = PATCH0;
  auto issue_patch = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      __builtin_amdgcn_global_load_lds((gvoid_t*)gP[j], (lvoid_t*)(lds + pdst + (w * 4 + (w == 7 ? 0 : j)) * 1024), 16, 0, 0);
      gP[j] += 32;
    }
    pdst ^= PSLOT;
  };

  // fused skip: ring of four 32 KiB slots {free patch slot, 0, 32 K, other patch slot}; stage s -> ring[s & 3]
  const unsigned sk_free = PATCH0 + (NC & 1) * PSLOT;   // the patch slot chunk NC - 1 does NOT use
  auto skip_base = [&](int s2) -> unsigned {
    const int k = s2 & 3;
    return k == 0 ? sk_free : (k == 1 ? 0u : (k == 2 ? 32768u : (sk_free ^ PSLOT)));
  };
  auto issue_skip = [&](int s2) {                       // 2 weight + 2 input DMA instructions per wave
    const unsigned base = skip_base(s2);
    // an opaque zero in every address: the compiler cannot hoist this lane arithmetic in front of the K loop (where it was spilled)
    int opq;
    asm volatile("v_mov_b32 %0, 0" : "=v"(opq));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = (w * 2 + j) * 16 + lrow + opq;
      const int sw8 = (lch ^ ((row >> 2) & 3)) * 8 + s2 * 32;
      __builtin_amdgcn_global_load_lds((gvoid_t*)(a.W2 + (size_t)(n0 + row) * a.Kp2 + sw8), (lvoid_t*)(lds + base + (w * 2 + j) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gvoid_t*)(a.In2 + (size_t)min(m0 + row, M - 1) * a.Ci2 + sw8), (lvoid_t*)(lds + base + 16384 + (w * 2 + j) * 1024),
                                       16, 0, 0);
    }
  };
  bool skip0_now = false;                     // set for chunk NC - 2: skip stage 0 goes out where a next patch would

  // ---- per-lane constants of the multiplier side
  const int wm = w >> 2, wn = w & 3;
  const int fr = l & 31, fh = l >> 5;
  unsigned tapaddr[9][4];                     // B fragments, K step 0, patch slot 0
  {
    const int hw = a.Hi * Wi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wm * 128 + j * 32 + fr;     // output row of the tile; patch origin is pixel m0 - Wi - 1
      const int p = m0 + r;
      const int rem = p % hw;
      const int y = rem / Wi, x = rem - y * Wi;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int iy = y + ky - 1, ix = x + kx - 1;
          const bool ok = p < M && iy >= 0 && iy < a.Hi && ix >= 0 && ix < Wi;
          const int q = r + ky * Wi + kx;
          tapaddr[ky * 3 + kx][j] = ok ? PATCH0 + (unsigned)q * 64 + ((unsigned)(fh ^ ((q >> 2) & 3)) << 4) : PATCH0 + ZROW + ((unsigned)fh << 4);
        }
    }
  }
  unsigned wfrag[2];                          // A fragments, K step 0, byte offset inside a weight slot
#pragma unroll
  for (int i = 0; i < 2; ++i) wfrag[i] = (unsigned)swz32(wn * 64 + i * 32 + fr, fh) * 2;
  unsigned wsrc = 0;                          // LDS byte offset of the slot of the stage whose fragments are read next
  f32x16 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  frag faA[2], fbA[4], faB[2], fbB[4];
  auto multiply = [&](const frag (&fa)[2], const frag (&fb)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i][j] = E::mfma32(fa[i], fb[j], acc[i][j]);
  };

  bool pdst_pending = false;                  // set per chunk: is there a patch to issue at the next chunk boundary
  // one stage. Entering: faA / fbA hold K step 0 of (chunk, TAP). LAST: the chunk is the last one.
  auto stage = [&](auto tapc, auto lastc) {
    constexpr int TAP = decltype(tapc)::value;
    constexpr bool LAST = decltype(lastc)::value;
#pragma unroll
    for (int i = 0; i < 2; ++i) faB[i] = *(lds_frag*)(lds + wsrc + (wfrag[i] ^ 32u));
#pragma unroll
    for (int j = 0; j < 4; ++j) fbB[j] = *(lds_frag*)(lds + (tapaddr[TAP][j] ^ 32u));
    multiply(faA, fbA);
    if (LAST && TAP == 8) {                   // the very last stage: nothing to advance to
      multiply(faB, fbB);
      return;
    }
    // advance to the next stage t: wait for this wave's pieces of W(t) (and of everything older). Younger transfers in flight:
    // W(t+1), W(t+2) (2 instructions each; fewer at the end of the last chunk) and, during the first three stages of a chunk that
    // is not the last one, the patch of the next chunk (4), issued right behind W(t+2) at the chunk's start.
    if (LAST) {
      if (SKIP && TAP <= 2) ACEZ_VMCNT(8);      // (+ skip stage 0, issued where a next patch would have been)
      else if (TAP <= 5) ACEZ_VMCNT(4);
      else if (TAP == 6) ACEZ_VMCNT(2);
      else ACEZ_VMCNT(0);
    } else {
      if (TAP <= 2) ACEZ_VMCNT(8);
      else ACEZ_VMCNT(4);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);       // lgkmcnt(0): this wave's reads of the current stage are complete (faB / fbB hold them)
    __builtin_amdgcn_s_barrier();             // W(t) (and its patch) landed everywhere; nobody reads the current stage any more
    if (!LAST || TAP < 5) issue_w();          // W(t+3) into the slot that just became free
    wsrc = (wsrc + WSLOT) & (4 * WSLOT - 1);
    if (TAP == 8) {                           // t is the first stage of the next chunk: the patch slot of this chunk is free
      if (pdst_pending) issue_patch();
      else if (SKIP && skip0_now) issue_skip(0);
#pragma unroll
      for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int j = 0; j < 4; ++j) tapaddr[tp][j] ^= PSLOT;
    }
    constexpr int NT = (TAP == 8) ? 0 : TAP + 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) faA[i] = *(lds_frag*)(lds + wsrc + wfrag[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) fbA[j] = *(lds_frag*)(lds + tapaddr[NT][j]);
    multiply(faB, fbB);
  };

  // ---- prologue: patch 0, W(0..3), patch 1
  issue_patch();
  for (int s = 0; s < 4; ++s) issue_w();      // S >= 9 > 4
  if (NC > 1) {
    issue_patch();
    ACEZ_VMCNT(10);                           // younger than W(0): W(1..3) and patch 1
  } else {
    ACEZ_VMCNT(6);
  }
  __builtin_amdgcn_s_barrier();               // W(0), patch 0 and the zero rows are in place
#pragma unroll
  for (int i = 0; i < 2; ++i) faA[i] = *(lds_frag*)(lds + wsrc + wfrag[i]);
#pragma unroll
  for (int j = 0; j < 4; ++j) fbA[j] = *(lds_frag*)(lds + tapaddr[0][j]);
  using std::integral_constant;
  for (int cc = 0; cc + 1 < NC; ++cc) {
    pdst_pending = cc + 2 < NC;               // at the boundary to chunk cc + 1: patch cc + 2 goes into this chunk's slot
    skip0_now = cc + 2 == NC;
    stage(integral_constant<int, 0>{}, integral_constant<bool, false>{});
    stage(integral_constant<int, 1>{}, integral_constant<bool, false>{});
    stage(integral_constant<int, 2>{}, integral_constant<bool, false>{});
    stage(integral_constant<int, 3>{}, integral_constant<bool, false>{});
    stage(integral_constant<int, 4>{}, integral_constant<bool, false>{});
    stage(integral_constant<int, 5>{}, integral_constant<bool, false>{});
    stage(integral_constant<int, 6>{}, integral_constant<bool, false>{});
    stage(integral_constant<int, 7>{}, integral_constant<bool, false>{});
    stage(integral_constant<int, 8>{}, integral_constant<bool, false>{});
  }
  stage(integral_constant<int, 0>{}, integral_constant<bool, true>{});
  stage(integral_constant<int, 1>{}, integral_constant<bool, true>{});
  stage(integral_constant<int, 2>{}, integral_constant<bool, true>{});
  stage(integral_constant<int, 3>{}, integral_constant<bool, true>{});
  stage(integral_constant<int, 4>{}, integral_constant<bool, true>{});
  stage(integral_constant<int, 5>{}, integral_constant<bool, true>{});
  stage(integral_constant<int, 6>{}, integral_constant<bool, true>{});
  stage(integral_constant<int, 7>{}, integral_constant<bool, true>{});
  stage(integral_constant<int, 8>{}, integral_constant<bool, true>{});

  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();               // everybody has left the K loop: all of LDS is free
  if (SKIP) {
    const int NS = a.Ci2 >> 5;                // skip stages (>= 4: launcher)
    // Everything this section needs per lane is computed HERE: an opaque zero (the compiler cannot see its value) rides in every address,
    // or the lane constants below are hoisted in front of the K loop and spilled (55 dwords of scratch in the first build).
    int opq;
    asm volatile("v_mov_b32 %0, 0" : "=v"(opq));
    issue_skip(1); issue_skip(2); issue_skip(3);
    const int fro = fr + opq;
    unsigned inaddr[4];                       // B fragments of the skip input, K step 0, relative to a slot's input half
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned r = wm * 128 + j * 32 + fro;
      inaddr[j] = 16384u + r * 64 + ((unsigned)(fh ^ ((r >> 2) & 3)) << 4);
    }
    // stage 0 landed long ago (it is older than the K loop's last weight stages): its first fragments are requested before the bias pass
    frag fa0[2], fb0[4], fa1[2], fb1[4];
    {
      const unsigned base = skip_base(0);
#pragma unroll
      for (int i = 0; i < 2; ++i) fa0[i] = *(lds_frag*)(lds + base + wfrag[i]);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb0[j] = *(lds_frag*)(lds + base + inaddr[j]);
    }
    {   // bias + activation of the 3 x 3 layer on the accumulators (what the epilogue does for the unfused layer)
      const float* bp = a.bias + n0 + wn * 64 + 4 * fh + opq;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 b = *reinterpret_cast<const float4*>(bp + i * 32 + 8 * q);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float v[4] = {acc[i][j][4 * q + 0], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
            bias_act<RELU>(v, b);
            if (a.round_before_add) round16<E>(v);   // fp16: relu(conv) is a half tensor before the add
            acc[i][j][4 * q + 0] = v[0]; acc[i][j][4 * q + 1] = v[1]; acc[i][j][4 * q + 2] = v[2]; acc[i][j][4 * q + 3] = v[3];
          }
        }
    }
    // stages in groups of four (NS % 4 == 0: launcher): ring position, wait count and "is there a stage to issue" are compile-time
    // constants of a stage body, and no body has a second exit (early returns inside the loop made the compiler keep copies of the
    // accumulators per exit: 500 dwords of spills)
    auto skip_stage = [&](auto kc, auto vmc, auto morec, int c) {
      constexpr int KR = decltype(kc)::value;   // c & 3
      constexpr int VM = decltype(vmc)::value;  // DMA instructions younger than stage c + 1
      const unsigned base = KR == 0 ? sk_free : (KR == 1 ? 0u : (KR == 2 ? 32768u : (sk_free ^ PSLOT)));
      const unsigned nb = KR == 3 ? sk_free : (KR == 0 ? 0u : (KR == 1 ? 32768u : (sk_free ^ PSLOT)));
#pragma unroll
      for (int i = 0; i < 2; ++i) fa1[i] = *(lds_frag*)(lds + base + (wfrag[i] ^ 32u));
#pragma unroll
      for (int j = 0; j < 4; ++j) fb1[j] = *(lds_frag*)(lds + base + (inaddr[j] ^ 32u));
      multiply(fa0, fb0);
      ACEZ_VMCNT_C(VM);
      __builtin_amdgcn_s_waitcnt(0xC07F);     // this wave's reads of stage c are complete
      __builtin_amdgcn_s_barrier();           // stage c + 1 landed everywhere; nobody reads stage c any more
      if (decltype(morec)::value) issue_skip(c + 4);
#pragma unroll
      for (int i = 0; i < 2; ++i) fa0[i] = *(lds_frag*)(lds + nb + wfrag[i]);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb0[j] = *(lds_frag*)(lds + nb + inaddr[j]);
      multiply(fa1, fb1);
    };
    using IC0 = integral_constant<int, 0>; using IC1 = integral_constant<int, 1>; using IC2 = integral_constant<int, 2>;
    using IC3 = integral_constant<int, 3>; using IC4 = integral_constant<int, 4>; using IC8 = integral_constant<int, 8>;
    using T = integral_constant<bool, true>; using Fl = integral_constant<bool, false>;
    int c = 0;
#pragma clang loop unroll(disable)
    for (; c + 4 < NS; c += 4) {
      skip_stage(IC0{}, IC8{}, T{}, c);
      skip_stage(IC1{}, IC8{}, T{}, c + 1);
      skip_stage(IC2{}, IC8{}, T{}, c + 2);
      skip_stage(IC3{}, IC8{}, T{}, c + 3);
    }
    skip_stage(IC0{}, IC8{}, Fl{}, c);        // the last four stages: nothing left to issue, the waits count down
    skip_stage(IC1{}, IC4{}, Fl{}, c + 1);
    skip_stage(IC2{}, IC0{}, Fl{}, c + 2);
    {                                         // stage NS - 1: ring position 3
      const unsigned base = sk_free ^ PSLOT;
#pragma unroll
      for (int i = 0; i < 2; ++i) fa1[i] = *(lds_frag*)(lds + base + (wfrag[i] ^ 32u));
#pragma unroll
      for (int j = 0; j < 4; ++j) fb1[j] = *(lds_frag*)(lds + base + (inaddr[j] ^ 32u));
      multiply(fa0, fb0);
      multiply(fa1, fb1);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();             // the skip stages are done: all of LDS is free
  }
  if (HAS_ADD) {
    // residual tile [256][256] -> LDS, 128 DMA instructions of 2 rows x 512 bytes (16 per wave)
    // (written out, not residual_dma<256> of conv_tiles.h as in convgemm512: through the helper this form, at 252 registers, takes 254)
    for (int j = 0; j < 16; ++j) {
      const int row = (w * 16 + j) * 2 + (l >> 5);
      const uint16_t* g = a.add + (size_t)min(m0 + row, M - 1) * a.Co + n0 + (((l & 31) ^ (row & 31)) << 3);
      __builtin_amdgcn_global_load_lds((gvoid_t*)g, (lvoid_t*)(smem + (w * 16 + j) * 2 * 256), 16, 0, 0);
    }
    ACEZ_VMCNT(0);
    __builtin_amdgcn_s_barrier();             // residual tile landed
  }
  float4 bv[2][4];
  load_bias_quads(bv, (SKIP ? a.bias2 : a.bias) + n0, wn, fh);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ml = wm * 128 + j * 32 + fr;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nl = wn * 64 + i * 32 + 8 * q + 4 * fh;
        // (SKIP: the activation went onto the accumulators before the skip stages)
        epilogue_quad<E, RELU && !SKIP, HAS_ADD>(acc[i][j][4 * q + 0], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3], bv[i][q],
                                                 &smem[st_off_n<256>(ml, nl)], a.round_before_add);
      }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (B2B) {
    // ---- second product: acc[i][j] = W2[wn*64 + i*32 .. +31][:] . tile[wm*128 + j*32 .. +31][:]  (K = 256 = 16 steps of 16)
    int opq;
    asm volatile("v_mov_b32 %0, 0" : "=v"(opq));   // (keeps this lane arithmetic behind the K loop: see the skip stages)
    const uint16_t* wp[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) wp[i] = a.W2 + (size_t)(wn * 64 + i * 32 + fr + opq) * a.Kp2 + 8 * fh;
    unsigned brow[4], bx[4];                  // B fragment of K step kk: lds + brow[j] + (((2 kk + fh) ^ bx[j]) << 4)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned r = wm * 128 + j * 32 + fr + opq;
      brow[j] = r * 512;
      bx[j] = (r & 31) ^ (unsigned)fh;        // (2 kk) ^ fh ^ (r & 31): fh and r & 31 folded
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    constexpr int PF = 4;                     // weight fragments requested PF steps ahead
    frag wa[PF][2];
#pragma unroll
    for (int k = 0; k < PF; ++k)
#pragma unroll
      for (int i = 0; i < 2; ++i) wa[k][i] = *reinterpret_cast<const frag*>(wp[i] + 16 * k);
    frag fbx[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fbx[0][j] = *(lds_frag*)(lds + brow[j] + (bx[j] << 4));
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      if (kk + 1 < 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) fbx[(kk + 1) & 1][j] = *(lds_frag*)(lds + brow[j] + ((((unsigned)(2 * (kk + 1))) ^ bx[j]) << 4));
      }
      frag cur[2] = {wa[kk % PF][0], wa[kk % PF][1]};
      if (kk + PF < 16) {
#pragma unroll
        for (int i = 0; i < 2; ++i) wa[kk % PF][i] = *reinterpret_cast<const frag*>(wp[i] + 16 * (kk + PF));
      }
      multiply(cur, fbx[kk & 1]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();             // every wave has read what it needs of the first tile
    float4 b2v[2][4];
    load_bias_quads(b2v, a.bias2 + opq, wn, fh);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ml = wm * 128 + j * 32 + fr;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int nl = wn * 64 + i * 32 + 8 * q + 4 * fh;
          epilogue_quad<E, true, false>(acc[i][j][4 * q + 0], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3], b2v[i][q],
                                        &smem[st_off_n<256>(ml, nl)], 0);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  for (int q = t; q < 256 * 32; q += 512) copy_out_chunk<256>(a, smem, q, m0, n0);
}

}  // namespace acez
