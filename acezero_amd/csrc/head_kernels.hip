// head_kernels.hip -- gfx950 kernels of the ACE scene-coordinate head (training + inference): the chain unit. The per-layer GEMM, the
// one-launch chains built from its body, the loss and the group chain. These kernels are ONE family: the code of a chain kernel depends
// on which sibling instantiations of rowgemm80_body<..., SEQ = true> share its module (DESIGN_HISTORY.md, the head unit's split), so none
// of them moves to another unit without tools/isa_diff.py. The optimiser side of the step is head_optim.hip, whole frames head_maps.hip.
//
// What the head computes (reference file:line), and where:
//   gather                ace_trainer.py:485-494   training_buffer['features'][random_batch_indices]          head_gather.h, head_optim.hip
//   rowgemm (fwd)         ace_network.py:122-136   relu(conv1x1(x)) chains, residual adds at :126,:133          here
//   loss kernel           ace_network.py:137-147   fc3 + softplus de-homogenisation + mean                      here
//                         ace_trainer.py:521-613   projection, masks, ReproLoss (ace_loss.py:39-91), loss/B
//                         + the analytic gradient of all of it wrt the fc3 outputs
//   rowgemm (dgrad)       autograd of the 1x1 convs wrt their inputs (+ relu masks, residual fan-in)             here
//   wgrad                 autograd of the 1x1 convs wrt weight and bias, all layers in one launch               head_wgrad.h, head_optim.hip
//   grad_reduce / adamw   ace_schedule.py:106-126 (AdamW step), torch.optim.AdamW semantics                     head_opt.h, head_optim.hip
//   sched                 ace_schedule.py:72-101,115-126 (cool-down trigger, LinearLR / OneCycleLR)             head_sched.h, head_optim.hip
//
// Data layout: activations are row-major [rows][512] bf16 (a row = one patch = 1 KiB); weights are kept as
// fp32 masters plus two bf16 compute copies, W [out][in] and W^T [in][out], so that the forward GEMM and the
// input-gradient GEMM both see a reduction-contiguous second operand. MFMA: v_mfma_f32_32x32x16_bf16, fp32
// accumulate, computed as D[i = output channel][j = row] so that each lane ends up holding 4 consecutive
// channels of one row (an 8-byte row-major store).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "head_kernels.h"
#include "gemm_common.h"
#include "head_gather.h"
#include "head_seq.h"

namespace acez {

// ---------------------------------------------------------------------------------------------------
// rowgemm80: Out[m][n] = epi( sum_k In[m][k] * W[n][k] ), K = 512 (ACEZ_HEAD_CHANNELS) = 8 K-steps of 64, on 80-row x 128-column
// tiles so that a 5120-row batch gives 64 x 4 = 256 workgroups = one per CU (a 128 x 128 tiling -- round 1, in the git history --
// fills only 160 of the 256 CUs). MFMA v_mfma_f32_16x16x32_{bf16,f16}. LDS tiles are [row][64] 16-bit with the 16-byte chunk index
// XOR-swizzled by (row >> 1) & 7 (conflict-free ds_read_b128 fragment reads); rows past M are clamped (never stored).
// Eight waves with fixed roles (waves w and w + 4 share a SIMD):
//   waves 0..3  multiply: wave w owns output columns 32w .. 32w+31 (2 column fragments x 5 row fragments = 10
//               accumulator tiles) and never touches global memory inside the K loop;
//   waves 4..7  only issue LDS-DMA: the 8 K-stages [W 128 x 64 | In 96 x 64] into a 4-slot ring (112 KiB, 7 DMA
//               instructions per loader and stage) and then the epilogue's input tiles (`add`, `mask` / `res`) into two
//               [80][128] staging tiles, so that their latency is hidden behind the K loop too.
// A wave's instruction stream is in-order: when every wave both loaded and multiplied, the time its DMA instructions
// spent getting through the memory pipeline was added to its MFMA time.
// The epilogue exchanges the whole 80 x 128 tile through the staging tiles (16-byte chunk index XOR row & 15: conflict
// free both for the accumulator layout and for the row-wise copy), so every global access is a full 256-byte row.
// ---------------------------------------------------------------------------------------------------

constexpr int RG80_STAGE = (128 + 96) * 64;                        // elements per ring slot
constexpr int RG80_SMEM = 4 * RG80_STAGE + 2 * 80 * 128;           // ring + two staging tiles
constexpr int RG80_SMEM_SEQ = RG80_SMEM + 1024;                    // + the bias-partial combine buffer (the ring is busy in SEQ mode)

template <bool BIAS_RELU, bool HAS_ADD, bool HAS_MASK, int AUX, bool SEQ, class E = EltBf16>
__device__ __forceinline__ void rowgemm80_body(const RowGemmArgs& a, uint16_t* smem, const int active, const int mt, const int n0,
                                               const SeqLink& q) {
  constexpr int STAGE = RG80_STAGE;
  uint16_t* const stA = smem + 4 * STAGE;   // `add` in / aux out
  uint16_t* const stB = stA + 80 * 128;     // mask | res in / main out
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int m0 = mt * 80;
  const int M = a.M, N = a.N;
  constexpr int K = 512, KT = 8;
  constexpr bool HAS_IN2 = AUX == AUX_RESIDUAL;   // (the ReLU mask of an input-gradient layer is a lane-private bit word since round 6, not a tile)
  constexpr int EPI = 5 * ((HAS_ADD ? 1 : 0) + (HAS_IN2 ? 1 : 0));  // epilogue-input DMA instructions per loader

  if (w >= 4) {
    // ------------------------------------------------------------------ loader waves
    const int lw = w - 4;
    // W instructions 4lw .. 4lw+3 (8 rows each), In instructions 3lw .. 3lw+2; lane: row + (l>>3), slot l&7
    const uint16_t* gW[4];
    const uint16_t* gI[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = (lw * 4 + j) * 8 + (l >> 3);
      gW[j] = a.W + (size_t)(n0 + row) * K + ((l & 7) ^ ((row >> 1) & 7)) * 8;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int row = (lw * 3 + j) * 8 + (l >> 3);
      gI[j] = a.In + (size_t)min(m0 + row, M - 1) * K + ((l & 7) ^ ((row >> 1) & 7)) * 8;
    }
    // (Round 6: K stages started at stage (row tile & 7), so that the eight row tiles an XCD holds of one column tile pull eight different
    // weight stages at any moment -- the rotation head_maps.hip gains 15 % from -- measured +3.5 us on the forward chain and +1.5 us on the
    // input-gradient chain (profiles/r06_krot_experiments.log): in lockstep one L2 fill serves every workgroup that shares the stage.)
    auto issueW = [&](int kt) {
      uint16_t* slot = smem + (kt & 3) * STAGE;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_global_load_lds((gvoid_t*)(gW[j] + kt * 64), (lvoid_t*)(slot + (lw * 4 + j) * 8 * 64), 16, 0, 0);
    };
    auto issueI = [&](int kt) {
      uint16_t* slot = smem + (kt & 3) * STAGE;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        __builtin_amdgcn_global_load_lds((gvoid_t*)(gI[j] + kt * 64), (lvoid_t*)(slot + 128 * 64 + (lw * 3 + j) * 8 * 64), 16, 0, 0);
    };
    auto issue = [&](int kt) { issueW(kt); issueI(kt); };
    // epilogue inputs: 4-row groups 5lw .. 5lw+4 of the [80][128] tile; lane: row + (l>>4), physical chunk l&15 receives
    // the logical chunk (l&15) ^ (row & 15)
    auto issue_tile = [&](const uint16_t* src, uint16_t* dst) {
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int row = (lw * 5 + j) * 4 + (l >> 4);
        const uint16_t* g = src + (size_t)min(m0 + row, M - 1) * N + n0 + (((l & 15) ^ (row & 15)) << 3);
        __builtin_amdgcn_global_load_lds((gvoid_t*)g, (lvoid_t*)(dst + (lw * 5 + j) * 4 * 128), 16, 0, 0);
      }
    };
    if (!SEQ) {
      issue(0); issue(1); issue(2); issue(3);
    } else {
      // W stages 0..3 first (requested by the layer before unless this is the first), then -- once the four column tiles
      // of the producing layer have landed in this XCD's L2 -- the In stages
      if (q.first) { issueW(0); issueW(1); issueW(2); issueW(3); }
      if (q.wait && seq_poll_expired(q.flag, t, q.target, q.limit) && l == 0) seq_raise_fault(q.flag - q.flag_index + SEQ_FAULT_WORD, a.st);
      issueI(0); issueI(1); issueI(2); issueI(3);
    }
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      // in-order completion: everything younger than stage kt may still be in flight
      if (SEQ && kt == 0) ACEZ_VMCNT(9);
      else if (SEQ && kt == 1) ACEZ_VMCNT(6);
      else if (SEQ && kt == 2) ACEZ_VMCNT(10);
      else if (kt == 0) ACEZ_VMCNT(21);
      else if (kt <= 4) ACEZ_VMCNT(14);
      else if (kt == 5) ACEZ_VMCNT_C(14 + EPI);
      else if (kt == 6) ACEZ_VMCNT_C(7 + EPI);
      else ACEZ_VMCNT_C(EPI);
      __builtin_amdgcn_s_barrier();   // stage kt has landed; the multipliers are done with stage kt - 1
      if (kt >= 1 && kt + 3 < KT) issue(kt + 3);
      if (kt == 4) {
        if (HAS_ADD) issue_tile(a.add, stA);
        if (HAS_IN2) issue_tile(a.res, stB);
      }
    }
    ACEZ_VMCNT(0);
    __builtin_amdgcn_s_barrier();     // epilogue inputs have landed; the ring is free
    if (SEQ && q.next_W) {            // overlaps the epilogue: 64 KiB of the next layer's 208 KiB (requested behind the hand-off
#pragma unroll                        // instead, so that the loader waves' vmcnt(0) there covers stores only: measured +3 us per chain)
      for (int j = 0; j < 4; ++j) gW[j] += q.next_W - a.W;
      issueW(0); issueW(1); issueW(2); issueW(3);
    }
    if (!SEQ && !active) return;
    __builtin_amdgcn_s_barrier();       // the multipliers have written the output tiles
  } else {
    // ------------------------------------------------------------------ multiplier waves
    f32x4 acc[2][5];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
    const int fr = l & 15, fq = l >> 4;
    // this lane's 40 ReLU mask bits (RowGemmArgs::mask_in): requested now, used after the K loop. Inline asm: a plain load would be sunk
    // to its first use by the scheduler, i.e. into the epilogue, where its round trip would be exposed
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 mb = {0u, 0u};
    if (HAS_MASK) {
      const uint2* mp = a.mask_in + ((size_t)(mt * 4 + (n0 >> 7)) * 4 + w) * 64 + l;
      asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(mb) : "v"(mp) : "memory");
    }
    float4 bias[2];
    if (BIAS_RELU) {
#pragma unroll
      for (int i = 0; i < 2; ++i) bias[i] = *reinterpret_cast<const float4*>(a.bias + n0 + w * 32 + i * 16 + 4 * fq);
    }
    // The K loop is straight-line code: without this the scheduler sinks
    // the second half's MFMAs below the next s_barrier -- their ds_reads would still be in flight when the loader waves, released by
    // that barrier, refill the slot (only the DMA latency protects them: a rare last-bit corruption under two processes on one GPU,
    // found with tools/seq_stress.py). Keep the fragment reads of a stage complete before the wave arrives at the barrier.
    auto stage_barrier = [&]() {
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    };
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      stage_barrier();
      const uint16_t* sW = smem + (kt & 3) * STAGE;
      const uint16_t* sI = sW + 128 * 64;
      if constexpr (!HAS_MASK) {
        // forward instantiations: the scheduler's own order (reads of the second K step behind the first MFMAs) is the better one
        // (A/B, round 5: the explicit order below costs the forward chain 0.5-1.5 us)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int c = kk * 4 + fq;
          typename E::frag fa[2], fb[5];
#pragma unroll
          for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const typename E::frag*>(&sW[swz(w * 32 + i * 16 + fr, c)]);
#pragma unroll
          for (int j = 0; j < 5; ++j) fb[j] = *reinterpret_cast<const typename E::frag*>(&sI[swz(j * 16 + fr, c)]);
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) acc[i][j] = E::mfma16(fa[i], fb[j], acc[i][j]);
        }
      } else {
      // Input-gradient instantiations: all fourteen fragment reads of the stage are requested before its first MFMA and every MFMA
      // waits for exactly the reads it needs. A multiplier wave is ALONE on its SIMD (its neighbour only issues DMA), so every LDS
      // round trip left between two MFMAs is matrix-pipe idle time: left to the scheduler, these instantiations read a fragment, waited
      // for it -- lgkmcnt(0) -- and multiplied, two to three times per stage (60 such read-wait pairs in rowseq_kernel<true>'s K loops
      // against 3 in the forward chain's; ISA scan, round 5: -2.0 ... -2.6 us on the input-gradient chain). Same MFMAs, same order.
      typename E::frag fa[2][2], fb[2][5];
      // The counted waits below assume ONE ds_read_b128 per fragment (fourteen reads in flight): a fragment is 16 bytes at a 16-byte aligned
      // LDS address (swz() returns multiples of eight elements). A wider / split fragment would turn the counts into wrong hints.
      static_assert(sizeof(typename E::frag) == 16 && alignof(typename E::frag) == 16, "one ds_read_b128 per fragment: ACEZ_KSTEP's lgkmcnt ladder");
      // request order = use order: fa[kk][0], fb[kk][0..4], fa[kk][1] for kk = 0, 1 (LDS returns in order)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int c = kk * 4 + fq;
        fa[kk][0] = *reinterpret_cast<const typename E::frag*>(&sW[swz(w * 32 + fr, c)]);
#pragma unroll
        for (int j = 0; j < 5; ++j) fb[kk][j] = *reinterpret_cast<const typename E::frag*>(&sI[swz(j * 16 + fr, c)]);
        fa[kk][1] = *reinterpret_cast<const typename E::frag*>(&sW[swz(w * 32 + 16 + fr, c)]);
      }
      __builtin_amdgcn_sched_barrier(0);
      // each MFMA waits for exactly the reads it needs: 14 in flight, the first needs two of them, ... (counts = reads that may remain)
#define ACEZ_KSTEP(KK, BASE)                                                                                   \
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"((BASE) + 5) : "memory"); acc[0][0] = E::mfma16(fa[KK][0], fb[KK][0], acc[0][0]); \
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"((BASE) + 4) : "memory"); acc[0][1] = E::mfma16(fa[KK][0], fb[KK][1], acc[0][1]); \
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"((BASE) + 3) : "memory"); acc[0][2] = E::mfma16(fa[KK][0], fb[KK][2], acc[0][2]); \
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"((BASE) + 2) : "memory"); acc[0][3] = E::mfma16(fa[KK][0], fb[KK][3], acc[0][3]); \
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"((BASE) + 1) : "memory"); acc[0][4] = E::mfma16(fa[KK][0], fb[KK][4], acc[0][4]); \
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(BASE) : "memory");                                           \
      acc[1][0] = E::mfma16(fa[KK][1], fb[KK][0], acc[1][0]); acc[1][1] = E::mfma16(fa[KK][1], fb[KK][1], acc[1][1]); \
      acc[1][2] = E::mfma16(fa[KK][1], fb[KK][2], acc[1][2]); acc[1][3] = E::mfma16(fa[KK][1], fb[KK][3], acc[1][3]); \
      acc[1][4] = E::mfma16(fa[KK][1], fb[KK][4], acc[1][4]);
      ACEZ_KSTEP(0, 7)
      __builtin_amdgcn_sched_barrier(0);
      ACEZ_KSTEP(1, 0)
#undef ACEZ_KSTEP
      }
    }
    stage_barrier();                    // epilogue inputs have landed
    if (!SEQ && !active) return;
    float amax = 0.f;                   // fp16 gradient layers: largest |value| before the conversion (absmax_publish)
    // The epilogue inputs this lane needs from the staging tiles (`add` values in stA, mask / residual values in stB: up to 2 x 10 eight-byte
    // reads), ALL requested before the first is used: written as read-compute-write per fragment the compiler could not move a read above
    // the previous fragment's write to the same tile (it cannot see that the addresses differ) and followed every read by a full
    // lgkmcnt(0) -- ten to twenty serial LDS round trips per layer in the input-gradient chain (85 read-wait pairs in rowseq_kernel<true>'s
    // ISA against 2 in the forward chain's; found with a scan for load-wait pairs, round 5). Same values, same arithmetic.
    uint2 ra[2][5], rb[2][5];
    if (HAS_ADD || HAS_IN2) {
#pragma unroll
      for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int o = st_off(j * 16 + fr, w * 32 + i * 16 + 4 * fq);
          if (HAS_ADD) ra[i][j] = *reinterpret_cast<const uint2*>(&stA[o]);
          if (HAS_IN2) rb[i][j] = *reinterpret_cast<const uint2*>(&stB[o]);
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (HAS_MASK) asm volatile("s_waitcnt vmcnt(0)" : "+v"(mb)::"memory");   // the mask bits requested before the K loop (long since landed)
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int ml = j * 16 + fr;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int nl = w * 32 + i * 16 + 4 * fq;
        float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
        uint16_t* pa = &stA[st_off(ml, nl)];
        uint16_t* pb = &stB[st_off(ml, nl)];
        if (BIAS_RELU) {
          v[0] += bias[i].x; v[1] += bias[i].y; v[2] += bias[i].z; v[3] += bias[i].w;
        }
        if (HAS_ADD) {
          float ad[4];
          E::un4(ra[i][j], ad);
          v[0] += ad[0]; v[1] += ad[1]; v[2] += ad[2]; v[3] += ad[3];
        }
        if (BIAS_RELU) {
          v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
        }
        if (E::is_f16 && HAS_MASK) amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        uint2 y = E::pk4(v[0], v[1], v[2], v[3]);
        if (AUX == AUX_RESIDUAL) {
          float yf[4], rf[4];
          E::un4(y, yf);
          E::un4(rb[i][j], rf);
          *reinterpret_cast<uint2*>(pa) = E::pk4(yf[0] + rf[0], yf[1] + rf[1], yf[2] + rf[2], yf[3] + rf[3]);
        } else if (AUX == AUX_UNMASKED) {
          *reinterpret_cast<uint2*>(pa) = y;
        }
        const int f = 2 * j + i;   // (compile-time: both loops are unrolled)
        if (HAS_MASK) {
          // keep a half word iff its bit is set: sign-extended one-bit fields -> 0 / ~0, merged per half
          const uint32_t kx = ((uint32_t)__builtin_amdgcn_sbfe((int)mb.x, 9 - f, 1) & 0x0000ffffu) | ((uint32_t)__builtin_amdgcn_sbfe((int)mb.x, 25 - f, 1) & 0xffff0000u);
          const uint32_t ky = ((uint32_t)__builtin_amdgcn_sbfe((int)mb.y, 9 - f, 1) & 0x0000ffffu) | ((uint32_t)__builtin_amdgcn_sbfe((int)mb.y, 25 - f, 1) & 0xffff0000u);
          y.x &= kx; y.y &= ky;
        }
        *reinterpret_cast<uint2*>(pb) = y;
      }
    }
    if (E::is_f16 && HAS_MASK && a.absmax) absmax_publish(a.absmax, amax);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();       // output tiles complete
  }
  // ------------------------------------------------------------------ all eight waves: copy the tiles out
  // All LDS reads first, into distinct registers, then the stores: as a read-store loop the compiler reused one register quadruple
  // and every read waited -- vmcnt(0) -- for the previous store to COMPLETE (its data register must not be overwritten while the
  // store is in flight): 2-5 serial store round trips at the end of each of the step's 15 launches.
  {
    const int q0 = t, q1 = t + 512, q2 = t + 1024;
    const int so0 = (q0 >> 4) * 128 + (((q0 & 15) ^ ((q0 >> 4) & 15)) << 3);
    const int so1 = (q1 >> 4) * 128 + (((q1 & 15) ^ ((q1 >> 4) & 15)) << 3);
    const int so2 = (q2 < 1280) ? (q2 >> 4) * 128 + (((q2 & 15) ^ ((q2 >> 4) & 15)) << 3) : 0;
    const uint4 m0v = *reinterpret_cast<const uint4*>(&stB[so0]);
    const uint4 m1v = *reinterpret_cast<const uint4*>(&stB[so1]);
    const uint4 m2v = *reinterpret_cast<const uint4*>(&stB[so2]);
    uint4 a0v = m0v, a1v = m1v, a2v = m2v;
    if (AUX != AUX_NONE) {
      a0v = *reinterpret_cast<const uint4*>(&stA[so0]);
      a1v = *reinterpret_cast<const uint4*>(&stA[so1]);
      a2v = *reinterpret_cast<const uint4*>(&stA[so2]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (also keeps the reads above this point)
    const int r0 = m0 + (q0 >> 4), r1 = m0 + (q1 >> 4), r2 = m0 + (q2 >> 4);
    const size_t o0 = (size_t)r0 * N + n0 + (q0 & 15) * 8, o1 = (size_t)r1 * N + n0 + (q1 & 15) * 8, o2 = (size_t)r2 * N + n0 + (q2 & 15) * 8;
    // SEQ: the tile the NEXT layer reads goes first -- the main tile, or after a residual add the aux tile (the residual stream is the next
    // block's input) -- and the hand-off follows its acknowledgement; the other tile (pre-residual activation kept for the backward pass /
    // unmasked gradient with its tile-local consumer) and the bias column sums come after the signal
    constexpr bool AUX_FIRST = AUX == AUX_RESIDUAL;
    uint16_t* const first = AUX_FIRST ? a.out_aux : a.out_main;
    uint16_t* const second = AUX_FIRST ? a.out_main : a.out_aux;
    const uint4 f0 = AUX_FIRST ? a0v : m0v, f1v = AUX_FIRST ? a1v : m1v, f2v = AUX_FIRST ? a2v : m2v;
    const uint4 s0 = AUX_FIRST ? m0v : a0v, s1 = AUX_FIRST ? m1v : a1v, s2 = AUX_FIRST ? m2v : a2v;
    if (r0 < M) *reinterpret_cast<uint4*>(first + o0) = f0;
    if (r1 < M) *reinterpret_cast<uint4*>(first + o1) = f1v;
    if (q2 < 1280 && r2 < M) *reinterpret_cast<uint4*>(first + o2) = f2v;
    if (SEQ && q.signal) {
      ACEZ_VMCNT(0);   // this wave's stores are acknowledged by the L2 = visible to the three sibling workgroups (same XCD)
      if (l == 0) seq_post(q.flag + seq_word(n0 >> 7, w), q.post);
    }
    if (AUX != AUX_NONE && second) {   // (null: a training forward does not keep the pre-residual activation -- only its mask bits are read again)
      if (r0 < M) *reinterpret_cast<uint4*>(second + o0) = s0;
      if (r1 < M) *reinterpret_cast<uint4*>(second + o1) = s1;
      if (q2 < 1280 && r2 < M) *reinterpret_cast<uint4*>(second + o2) = s2;
    }
  }
  if (BIAS_RELU && a.mask_out && w < 4) {
    // ReLU mask bits of this launch's output tile, for the input-gradient layer that will need them (RowGemmArgs::mask_out): computed BEHIND
    // the hand-off, from the main-output staging tile, in the time the multiplier waves would otherwise spend waiting for the next layer's
    // first K stage (in the epilogue proper -- 60 instructions per lane in front of the signal -- they cost the forward chain 2 us per
    // step; a store in front of the signal another 1.6 us per LAYER: its acknowledgement was waited for by the signalling vmcnt(0)).
    // The staging tile is intact until the next layer's loaders refill it behind that layer's K stage 4.
    // A 16-bit output is > 0 iff it is non-zero (the ReLU leaves no sign bit: v_max_f32(-0, +0) = +0): the per-half unsigned minimum with
    // 1 is the flag (v_pk_min_u16; inline asm: written as a vector minimum the compiler scalarised it into a dozen 16-bit compares and
    // selects per word); fragment f = 2 j + i ends at bits 9 - f and 25 - f of its word.
    const int fr = l & 15, fq = l >> 4;
    uint2 yv[5][2];
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) yv[j][i] = *reinterpret_cast<const uint2*>(&stB[st_off(j * 16 + fr, w * 32 + i * 16 + 4 * fq)]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    uint2 mbits = make_uint2(0u, 0u);
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        uint32_t fx, fy;
        asm("v_pk_min_u16 %0, %1, %2" : "=v"(fx) : "v"(yv[j][i].x), "s"(0x00010001u));
        asm("v_pk_min_u16 %0, %1, %2" : "=v"(fy) : "v"(yv[j][i].y), "s"(0x00010001u));
        mbits.x = (mbits.x << 1) | fx;
        mbits.y = (mbits.y << 1) | fy;
      }
    a.mask_out[((size_t)(mt * 4 + (n0 >> 7)) * 4 + w) * 64 + l] = mbits;   // 512 contiguous bytes per wave
  }
  if (HAS_MASK && a.bias_partials) {
    // bias gradient partial of this 80-row tile = column sums of the bf16 output tile: four 20-row groups in parallel,
    // combined in a fixed order (the ring is free by now)
    const int col = t & 127, g = t >> 7;
    const int rows = min(80, M - m0);
    // (all twenty reads first, then the adds in row order: as a read-add loop every read was followed by a full lgkmcnt(0) -- twenty serial
    // LDS round trips per layer, found with the same scan as the epilogue reads above)
    uint16_t colv[20];
#pragma unroll
    for (int r = 0; r < 20; ++r) colv[r] = stB[st_off(g * 20 + r, col)];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float sacc = 0.f;
#pragma unroll
    for (int r = 0; r < 20; ++r) {
      const int row = g * 20 + r;
      const float v = E::to_f(colv[r]);
      sacc += (row < rows) ? v : 0.f;
    }
    float* red = reinterpret_cast<float*>(SEQ ? smem + RG80_SMEM : smem);
    red[g * 128 + col] = sacc;
    if (SEQ) {   // not __syncthreads(): its fence would also wait for the next layer's W stages
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    } else {
      __syncthreads();
    }
    if (t < 128) a.bias_partials[(size_t)mt * 512 + n0 + t] = ((red[t] + red[128 + t]) + red[256 + t]) + red[384 + t];
  }
}

template <bool BIAS_RELU, bool HAS_ADD, bool HAS_MASK, int AUX, class E = EltBf16>
__global__ __launch_bounds__(512) void rowgemm80_kernel(RowGemmArgs a) {
  const int active = a.st ? a.st->active : 1;
  __shared__ __attribute__((aligned(16))) uint16_t smem[RG80_SMEM];
  RowTile t;
  if (!row_tile_decode(row_tiles(a.M), t)) return;
  rowgemm80_body<BIAS_RELU, HAS_ADD, HAS_MASK, AUX, false, E>(a, smem, active, t.mt, t.n0(), SeqLink{});
}

// ---------------------------------------------------------------------------------------------------
// rowseq: the layers of a dependent GEMM chain (the 8 forward layers, or the 7 input-gradient layers) in ONE launch with
// rowgemm80's tiling, roles, ring, K order and epilogues -- bit-identical outputs. Layer l + 1 of row tile mt reads layer l's
// 80 x 512 output = the four column tiles of mt, which the grid decode places on ONE XCD, so the hand-off stays inside that
// XCD's L2: every wave posts its progress word in the row tile's line once its stores are acknowledged, the next layer's loader waves
// poll the line past their L1. No agent-scope fence (a buffer_inv sc1 / buffer_wbl2 sc1 pair per seam costs 5 - 40 us: measured with
// tools/seam_proto.hip). Tile-local epilogue inputs (`add`, `res`) were written by the same CU or before the launch; `In` is
// never read before it is produced, so no stale L1 line can exist. What the seam saves over a kernel boundary: the launch
// ramp, and the next layer's first four W stages are in flight while the epilogue runs (tools/seam_proto.hip: 6.13 -> 4.88 us
// per forward layer at 5120 rows). All workgroups must be resident (they wait for their siblings): the host only uses this
// kernel when the grid is not larger than the number of CUs.
// ---------------------------------------------------------------------------------------------------

// What the layers of a chain share: the batch, the trainer's state and counters, and where the chain stands among the launch's hand-offs
struct SeqCtx {
  int M;
  const TrainState* st;
  uint32_t* flags;       // RowSeqArgs::flags
  uint32_t base;         // seams of this row tile completed by earlier launches (RowSeqArgs::base[mt])
  uint32_t seam0;        // hand-offs of THIS launch in front of the chain's layer 0
  uint32_t limit;        // RowSeqArgs::spin_limit
  uint32_t bias;         // RowSeqArgs::poll_bias
};

// The layers of a chain for the workgroup of tile (mt, n0). HEAD (rowseq_loss_kernel, rowstep_kernel's second chain): c.seam0 hand-offs of
// this launch lie in front of layer 0 -- its In is produced inside the launch and its first four W stages have been requested by the
// caller. TAIL (rowstep_kernel's first chain): a consumer follows the last layer inside the launch, so that layer signals too.
template <bool BWD, class E, bool HEAD, bool TAIL = false>
__device__ __forceinline__ void rowseq_layers(const SeqLayer* layers, const int n_layers, const SeqCtx& c, uint16_t* smem, const int mt, const int n0) {
  for (int layer = 0; layer < n_layers; ++layer) {
    // (one table row -> RowGemmArgs, SeqLink, epilogue shape: written out here and in rowseq_group_kernel -- shared as a function, the
    // fill or the dispatch alone, it changed the instruction order or the registers of the chain kernels)
    const SeqLayer& y = layers[layer];
    RowGemmArgs g;
    g.In = y.In; g.W = y.W; g.bias = y.bias; g.add = y.add; g.mask_out = y.mask_out; g.mask_in = y.mask_in; g.res = y.res; g.out_main = y.out_main; g.out_aux = y.out_aux;
    g.bias_partials = y.bias_partials; g.M = c.M; g.N = 512; g.K = 512; g.relu = BWD ? 0 : 1; g.aux_mode = y.aux_mode; g.st = c.st;
    g.absmax = (BWD && c.st) ? const_cast<uint32_t*>(c.st->dz_absmax_slots) : nullptr;
    SeqLink q;
    q.flag = c.flags + mt * 32; q.post = c.base + c.seam0 + (uint32_t)layer + 1u; q.target = q.post - 1u + c.bias;
    q.first = !HEAD && layer == 0; q.wait = HEAD || layer > 0; q.signal = TAIL || layer + 1 < n_layers;
    q.next_W = layer + 1 < n_layers ? layers[layer + 1].W : nullptr;
    q.flag_index = (uint32_t)(mt * 32); q.limit = c.limit;
    if (!BWD) {
      if (y.aux_mode == AUX_RESIDUAL) rowgemm80_body<true, false, false, AUX_RESIDUAL, true, E>(g, smem, 1, mt, n0, q);
      else rowgemm80_body<true, false, false, AUX_NONE, true, E>(g, smem, 1, mt, n0, q);
    } else {
      if (y.add) rowgemm80_body<false, true, true, AUX_UNMASKED, true, E>(g, smem, 1, mt, n0, q);
      else if (y.aux_mode == AUX_UNMASKED) rowgemm80_body<false, false, true, AUX_UNMASKED, true, E>(g, smem, 1, mt, n0, q);
      else rowgemm80_body<false, false, true, AUX_NONE, true, E>(g, smem, 1, mt, n0, q);
    }
  }
}

template <bool BWD, class E = EltBf16>
__global__ __launch_bounds__(512) void rowseq_kernel(RowSeqArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[RG80_SMEM_SEQ];
  RowTile t;
  if (!row_tile_decode(row_tiles(a.M), t)) return;
  const int mt = t.mt;
  seq_record_placement(a, t);
  if (SEQ_DEAD(a.st, a.flags)) {
    if (threadIdx.x == 0) seq_catch_up(a.base[mt] + seq_seams(a.n_layers), a.flags, mt, t.nt());
    return;
  }
  rowseq_layers<BWD, E, false>(a.layer, a.n_layers, SeqCtx{a.M, a.st, a.flags, a.base[mt], 0u, a.spin_limit, a.poll_bias}, smem, mt, t.n0());
}

// Placement probe (acez_trainer_create): a launch with rowseq_kernel's grid, block size and LDS footprint that only records
// which XCD ran tile (mt, nt) under rowseq_kernel's decode. The host enables the one-launch chains only if the four column tiles
// of every row tile report the same XCD. (A probe cannot promise anything about later launches -- HIP makes no placement
// contract -- which is why the hand-off itself is bounded and fault-checked; the probe keeps a part or a partition mode on which
// the mapping does not hold from ever taking the fault path.)
__global__ __launch_bounds__(512) void seq_probe_kernel(uint32_t* rec /*[256]*/, int mtiles) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[RG80_SMEM_SEQ];
  RowTile t;
  const bool has_tile = row_tile_decode(mtiles, t);
  if (threadIdx.x == 0) smem[0] = (uint16_t)blockIdx.x;   // keeps the allocation
  __syncthreads();
  if (!has_tile || threadIdx.x != 0) return;
  const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;   // HW_REG_XCC_ID[3:0]
  rec[t.mt * 4 + t.nt()] = (xcc << 16) | smem[0];
}

// ---------------------------------------------------------------------------------------------------
// loss kernel (32 rows per workgroup, four wavefronts):
//   A  fc3 forward, wave wv: rows 8 wv .. 8 wv + 7, one row per pass, fp32 accumulate
//   B  one thread per row: de-homogenise, project, masks, robust loss and d(loss)/d(fc3 outputs)
//   C  wave wv: channels 128 wv .. +127 of all 32 rows, one thread per channel pair: fc3 weight-gradient partials and the
//      masked input gradient dZ
// ---------------------------------------------------------------------------------------------------
constexpr int LOSS_ROWS = 8;
__device__ __forceinline__ float sgn(float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); }

// [32][512] bf16 activation tile of the LDSACT form of the loss phases below (the row-persistent kernels it was written for,
// headfwd_kernel and chain_kernel, live in the git history only; see the note on ACEZ_DIAG in acez_common.h): 16-byte chunk index XOR
// (row & 15), so that the 16 rows a ds_read_b128 lane group touches land on 16 different slots of a 256-byte bank row
__device__ __forceinline__ int act_off(int row, int ch) { return row * 512 + ((((ch >> 3) ^ (row & 15)) << 3) | (ch & 7)); }

// phase B's per-row inputs sit behind a chain of dependent loads (idx -> view -> image): they are fetched early (at kernel
// entry) so that the latency hides under phase A / under the forward GEMMs of the chain kernel
struct LossPre {
  int64_t p;
  int view, img;
  float tu, tv;
};
__device__ __forceinline__ LossPre loss_prefetch(const LossArgs& a, int m0, int t, int rows = LOSS_ROWS) {
  LossPre q{0, 0, 0, 0.f, 0.f};
  if (a.idx && t < rows && m0 + t < a.n) {
    q.p = a.idx[m0 + t];
    if (a.meta) {   // looked up where the batch was gathered (GatherMeta): one load level instead of three
      const int4 m = a.meta[m0 + t];
      q.view = m.x; q.img = m.y; q.tu = __int_as_float(m.z); q.tv = __int_as_float(m.w);
    } else {
      q.view = a.view_idx[q.p];
      q.img = a.view_image[q.view];
      q.tu = a.target_px[q.p * 2 + 0];
      q.tv = a.target_px[q.p * 2 + 1];
    }
  }
  return q;
}

// LDS scratch of the loss phases, in floats: s_s / s_ds / s_red [4 waves][LOSS_ROWS][4]
constexpr int LOSS_SCRATCH_FLOATS = 3 * 4 * LOSS_ROWS * 4;

// The three phases for the 32 rows of workgroup `block` (four wavefronts wv = 0..3 of 64 lanes t). LDSACT = false: the fc2
// output is read from a.act and dZ goes to a.dZ (loss_kernel). LDSACT = true: both live in the swizzled LDS tile `Xt`
// (act_off) of the chain kernel and dZ overwrites the activations in place (the caller copies the tile to a.dZ). The four waves
// meet once, through `sync` (loss_kernel: __syncthreads; the chain kernel: its flag barrier).
// PRE_INSIDE (loss_kernel): the per-row index chain of phase B (idx -> view -> image) is started here, BEHIND the loads of phase A:
// vmcnt completes in order, so a dependent chain issued first holds every later load behind its three round trips.
// LR rows per wavefront (4 LR per workgroup). The chain kernel's tile is 32 rows (LR = 8); loss_kernel runs LR = 4 by default: 320
// workgroups for a 5120-row batch instead of 160 on 256 CUs, half the serial row loop per wave (the summation order of the
// fc3 / bias partials follows the workgroup size, so the two sizes agree to rounding, not bitwise).
template <bool LDSACT, bool PRE_INSIDE, class E = EltBf16, int LR = 8, class Sync>
__device__ __forceinline__ void loss_body(const LossArgs& a, const int block, const int wv, const int t, uint16_t* Xt, float* scratch,
                                          LossPre pre, Sync sync) {
  constexpr int LOSS_ROWS = LR;
  float (*s_s)[4] = reinterpret_cast<float (*)[4]>(scratch + wv * LOSS_ROWS * 4);
  float (*s_ds)[4] = reinterpret_cast<float (*)[4]>(scratch + (4 + wv) * LOSS_ROWS * 4);
  float (*s_red)[4] = reinterpret_cast<float (*)[4]>(scratch + (8 + wv) * LOSS_ROWS * 4);
  const int l = t;
  const int m0 = (block * 4 + wv) * LOSS_ROWS;
  const int n = a.n, no = a.no;

  // ---- phase A. All of its loads are issued before anything is computed (as written row by row, every row's load was followed by
  // a full wait: twelve serial round trips).
  // (chain kernel, LDSACT: the rows are LDS reads issued where they are used -- batching them costs 60 registers the 768-thread
  // kernel does not have)
  uint4 w3raw[4], xraw[LDSACT ? 1 : LOSS_ROWS];
#pragma unroll
  for (int j = 0; j < 4; ++j) w3raw[j] = *reinterpret_cast<const uint4*>(a.W3 + (size_t)(j < no ? j : 0) * 512 + l * 8);
  if (!LDSACT) {
#pragma unroll
    for (int rr = 0; rr < LOSS_ROWS; ++rr) xraw[LDSACT ? 0 : rr] = *reinterpret_cast<const uint4*>(a.act + (size_t)min(m0 + rr, n - 1) * 512 + l * 8);
  }
  if (PRE_INSIDE) pre = loss_prefetch(a, m0, t, LOSS_ROWS);
  const int64_t pre_p = pre.p;
  const int pre_view = pre.view, pre_img = pre.img;
  const float pre_tu = pre.tu, pre_tv = pre.tv;
  // phase B's per-view / per-image matrices (augmentation, pose, intrinsics: 37 floats of a row's lane): with PRE_INSIDE they are
  // fetched here, as soon as view and image are known, and arrive while phase A computes
  float Am[12], Tm[16], Km[9];
  const bool early_mats = PRE_INSIDE && a.idx && t < LOSS_ROWS && m0 + t < n;
  if (early_mats) {
#pragma unroll
    for (int i = 0; i < 12; ++i) Am[i] = a.view_aug_inv[(size_t)pre_view * 12 + i];
#pragma unroll
    for (int i = 0; i < 16; ++i) Tm[i] = a.image_pose_inv[(size_t)pre_img * 16 + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) Km[i] = a.view_K[(size_t)pre_view * 9 + i];
  }
  // phase C's loads too (training, loss_kernel): the rows come back from the L1 / L2 this workgroup has just pulled them through, but
  // requested behind the workgroup's meeting point they were one more round trip on the kernel's critical path
  constexpr bool EARLY_C = !LDSACT;
  const int chC = wv * 128 + 2 * t;
  uint32_t w3c[4] = {0u, 0u, 0u, 0u}, xv[LDSACT ? 1 : 4 * LOSS_ROWS];
  if (EARLY_C && a.idx) {
    const int mb = block * 4 * LOSS_ROWS;
#pragma unroll
    for (int j = 0; j < 4; ++j) w3c[j] = *reinterpret_cast<const uint32_t*>(a.W3 + (size_t)(j < no ? j : 0) * 512 + chC);
#pragma unroll
    for (int r = 0; r < 4 * LOSS_ROWS; ++r)   // rows past the end carry ds == 0 and are not stored
      xv[LDSACT ? 0 : r] = *reinterpret_cast<const uint32_t*>(a.act + (size_t)min(mb + r, n - 1) * 512 + chC);
  }
  {
    float w3[4][8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      E::un4(make_uint2(w3raw[j].x, w3raw[j].y), &w3[j][0]);
      E::un4(make_uint2(w3raw[j].z, w3raw[j].w), &w3[j][4]);
      if (j >= no) {
#pragma unroll
        for (int e = 0; e < 8; ++e) w3[j][e] = 0.f;
      }
    }
    float b3v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b3v[j] = (j < no) ? a.b3[j] : 0.f;   // (not inside the row loop: a dependent load per row)
#pragma unroll
    for (int rr = 0; rr < LOSS_ROWS; ++rr) {
      const int r = rr, m = m0 + r;
      float x[8];
      const uint4 xr = LDSACT ? *reinterpret_cast<const uint4*>(&Xt[act_off(wv * LOSS_ROWS + r, l * 8)]) : xraw[LDSACT ? 0 : rr];
      E::un4(make_uint2(xr.x, xr.y), &x[0]);
      E::un4(make_uint2(xr.z, xr.w), &x[4]);
      if (!(m < n)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.f;
      }
      float p[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float sacc = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) sacc = fmaf(x[e], w3[j][e], sacc);
        p[j] = sacc;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j] = wave_sum63(p[j]);   // DPP (the 24 ds_bpermute per row of a shuffle butterfly were most of phase A)
      if (l == 63) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s_s[r][j] = (j < no) ? p[j] + b3v[j] : 0.f;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();

  // ---- phase B
  const float gscale = (a.idx && a.st) ? a.st->grad_scale : 1.f;
  if (t < LOSS_ROWS) {
    const int r = t, m = m0 + r;
    float loss = 0.f, inl = 0.f, fgrad = 0.f, ds[4] = {0.f, 0.f, 0.f, 0.f};
    if (m < n) {
      const float s0 = s_s[r][0], s1 = s_s[r][1], s2 = s_s[r][2], s3 = s_s[r][3];
      float X[3], hval = 1.f, bx = 0.f;
      bool hclamped = false;
      if (a.use_homogeneous) {
        bx = a.h_beta * s3;
        const float sp = (bx > 20.f) ? s3 : log1pf(expf(bx)) / a.h_beta;  // F.softplus(beta), ace_network.py:142
        const float hraw = sp + a.max_inv_scale;
        hclamped = hraw > a.min_inv_scale;                                // clamp_(max=min_inv_scale) :143
        hval = hclamped ? a.min_inv_scale : hraw;
        X[0] = s0 / hval + a.mean[0];
        X[1] = s1 / hval + a.mean[1];
        X[2] = s2 / hval + a.mean[2];
      } else {
        X[0] = s0 + a.mean[0];
        X[1] = s1 + a.mean[1];
        X[2] = s2 + a.mean[2];
      }
      if (a.out_xyz) {
        if (a.planar_hw > 0) {   // Regressor.forward's [B,3,H,W] layout (ace_network.py:265-270), what RANSAC reads
          const int64_t mg = (int64_t)a.row_offset + m;
          const int64_t fr = mg / a.planar_hw, px = mg - fr * a.planar_hw;
          float* o = a.out_xyz + fr * 3 * a.planar_hw + px;
          o[0] = X[0];
          o[(size_t)a.planar_hw] = X[1];
          o[(size_t)2 * a.planar_hw] = X[2];
        } else {
          a.out_xyz[(size_t)m * 3 + 0] = X[0];
          a.out_xyz[(size_t)m * 3 + 1] = X[1];
          a.out_xyz[(size_t)m * 3 + 2] = X[2];
        }
      }
      if (a.idx) {  // training: geometry + loss (skipped for pure inference)
        const float tu = pre_tu, tv = pre_tv;
        const int view = pre_view;
        if (!PRE_INSIDE) {
#pragma unroll
          for (int i = 0; i < 12; ++i) Am[i] = a.view_aug_inv[(size_t)view * 12 + i];
#pragma unroll
          for (int i = 0; i < 16; ++i) Tm[i] = a.image_pose_inv[(size_t)pre_img * 16 + i];
#pragma unroll
          for (int i = 0; i < 9; ++i) Km[i] = a.view_K[(size_t)view * 9 + i];
        }
        const float* A = Am;
        const float* T = Tm;
        float K[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) K[i] = Km[i];
        float kscale = 0.f;
        if (a.refine_calibration) {
          // refine_calibration.py:34-53: K[:2,:2] = (1+g) * f0 * (K00/f0) * I2
          kscale = K[0] / a.focal_init;
          const float f = (1.f + (float)a.st->calib_g) * a.focal_init * kscale;
          K[0] = f; K[1] = 0.f; K[3] = 0.f; K[4] = f;
        }
        // P = A(3x4) . T(4x4)    ace_trainer.py:530
        float P[12];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fmaf(A[i * 4 + k], T[k * 4 + j], acc);
            P[i * 4 + j] = acc;
          }
        float Xc[3], pp[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) Xc[i] = fmaf(P[i * 4 + 0], X[0], fmaf(P[i * 4 + 1], X[1], fmaf(P[i * 4 + 2], X[2], P[i * 4 + 3])));
#pragma unroll
        for (int i = 0; i < 3; ++i) pp[i] = fmaf(K[i * 3 + 0], Xc[0], fmaf(K[i * 3 + 1], Xc[1], K[i * 3 + 2] * Xc[2]));
        const bool zclamped = pp[2] < a.depth_min;                 // clamp_(min=depth_min) :545
        const float pz = zclamped ? a.depth_min : pp[2];
        const float u = pp[0] / pz, v = pp[1] / pz;
        const float du = u - tu, dv = v - tv;
        const float e = fabsf(du) + fabsf(dv);                     // L1 norm :552
        bool invalid = (Xc[2] < a.depth_min) || (e > a.hard_clamp) || (Xc[2] > a.depth_max);  // :558-565
        // depth-supervised mapping (use_depth, ace_trainer.py:567-574): a prediction further than 10 cm from an available
        // ground-truth scene coordinate is treated as invalid too
        float tcd[3] = {0.f, 0.f, 0.f}, tdist = 0.f;
        bool tavail = false;
        if (a.target_crds) {
          const float* tc = a.target_crds + pre_p * 3;
          tavail = (fabsf(tc[0]) + fabsf(tc[1]) + fabsf(tc[2])) > 0.00001f;
#pragma unroll
          for (int k = 0; k < 3; ++k) tcd[k] = tc[k] - X[k];
          tdist = sqrtf(tcd[0] * tcd[0] + tcd[1] * tcd[1] + tcd[2] * tcd[2]);
          if (tavail && tdist > 0.1f) invalid = true;
        }
        float dXc[3], dXs[3] = {0.f, 0.f, 0.f};
        if (!invalid) {
          float ge;
          const float wgt = a.st->loss_weight;
          if (a.loss_type == LOSS_TANH || a.loss_type == LOSS_DYNTANH) {
            const float th = tanhf(e / wgt);
            loss = wgt * th;
            ge = 1.f - th * th;
          } else if (a.loss_type == LOSS_L1) {
            const bool big = e > wgt;
            loss = big ? 0.f : e;
            ge = big ? 0.f : 1.f;
          } else if (a.loss_type == LOSS_L1_SQRT) {
            const bool big = e > wgt;
            loss = big ? sqrtf(wgt * e) : e;
            ge = big ? 0.5f * wgt / sqrtf(wgt * e) : 1.f;
          } else {
            const bool big = e > wgt;
            loss = big ? logf(1.f + wgt * e) : e;
            ge = big ? wgt / (1.f + wgt * e) : 1.f;
          }
          inl = (e < a.inlier_px) ? 1.f : 0.f;                      // :585
          const float gu = ge * sgn(du), gv = ge * sgn(dv);
          float dp[3];
          dp[0] = gu / pz;
          dp[1] = gv / pz;
          dp[2] = zclamped ? 0.f : -(gu * pp[0] + gv * pp[1]) / (pz * pz);
          if (a.refine_calibration) fgrad = (dp[0] * Xc[0] + dp[1] * Xc[1]) * a.focal_init * kscale;
#pragma unroll
          for (int j = 0; j < 3; ++j) dXc[j] = K[0 * 3 + j] * dp[0] + K[1 * 3 + j] * dp[1] + K[2 * 3 + j] * dp[2];
        } else if (a.target_crds) {
          // use_depth (ace_trainer.py:601-609): L2 distance to the ground-truth coordinate where there is one, nothing otherwise
          dXc[0] = dXc[1] = dXc[2] = 0.f;
          if (tavail) {
            loss = tdist;
            const float inv = tdist > 0.f ? 1.f / tdist : 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) dXs[k] = -tcd[k] * inv;
          }
        } else {
          // proxy target at constant depth, ace_trainer.py:592-600
          const float* Ki = a.view_Kinv + (size_t)view * 9;
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const float tgt = a.depth_target * fmaf(Ki[i * 3 + 0], tu, fmaf(Ki[i * 3 + 1], tv, Ki[i * 3 + 2]));
            const float d = tgt - Xc[i];
            loss += fabsf(d);
            dXc[i] = -sgn(d);
          }
        }
        const float invB = a.inv_batch;
        if (a.row_dT) {
          // d(loss)/dT[k][j] = sum_i A[i][k] * dXc[i] * Xh[j], k < 3 (row 3 of T is the constant 0 0 0 1)
          const float Xh[4] = {X[0], X[1], X[2], 1.f};
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float ak = (A[0 * 4 + k] * dXc[0] + A[1 * 4 + k] * dXc[1] + A[2 * 4 + k] * dXc[2]) * invB;
#pragma unroll
            for (int j = 0; j < 4; ++j) a.row_dT[(size_t)m * 12 + k * 4 + j] = ak * Xh[j];
          }
          a.row_image[m] = pre_img;
        }
        float dX[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) dX[k] = (P[0 * 4 + k] * dXc[0] + P[1 * 4 + k] * dXc[1] + P[2 * 4 + k] * dXc[2] + dXs[k]) * invB;
        fgrad *= invB;
        if (a.use_homogeneous) {
          ds[0] = dX[0] / hval;
          ds[1] = dX[1] / hval;
          ds[2] = dX[2] / hval;
          float dh = -(dX[0] * s0 + dX[1] * s1 + dX[2] * s2) / (hval * hval);
          if (hclamped) dh = 0.f;
          if (bx > 20.f) ds[3] = dh;
          else {
            const float z = expf(bx);
            ds[3] = dh * z / (z + 1.f);
          }
        } else {
          ds[0] = dX[0]; ds[1] = dX[1]; ds[2] = dX[2]; ds[3] = 0.f;
        }
      }
    }
    // (fp16 operands: the gradient is propagated scaled by grad_scale and un-scaled where it meets the fp32 optimiser; 1 for bf16)
#pragma unroll
    for (int j = 0; j < 4; ++j) s_ds[r][j] = E::is_f16 ? ds[j] * gscale : ds[j];   // (bf16: no multiply at all -- even an exact one changes how
                                                                                 // the compiler contracts the divisions above: last bits of ds)
    s_red[r][0] = loss; s_red[r][1] = inl; s_red[r][2] = fgrad; s_red[r][3] = 0.f;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (!a.idx) return;  // inference: no gradients

  // ---- the four waves meet once: phase C reads every row's ds and, in the chain kernel, overwrites activations that the other
  // waves' phase A has read
  sync();

  // ---- phase C: wave wv owns channels 128 wv .. 128 wv + 127 of ALL 32 rows, lane t two of them; the row sums of the fc3 weight
  // gradient and of the fc2 bias gradient (the bf16-rounded dZ values) run over the rows in order inside one lane, so a workgroup
  // emits ONE partial per 32 rows without any cross-wave combine
  {
    const int ch = wv * 128 + 2 * t;
    const int mb = block * 4 * LOSS_ROWS;
    float w3[4][2], gw[4][2], bsum[2] = {0.f, 0.f};
    float amax = 0.f;   // fp16: largest |dZ| this lane produces (scaled units) -> the gradient-scale control of the schedule wave
    // every load of the phase first (row by row, a load was followed by a full wait: 32 serial round trips); loss_kernel: they were
    // requested in front of phase B already (EARLY_C)
    if (!EARLY_C) {
#pragma unroll
      for (int j = 0; j < 4; ++j) w3c[j] = *reinterpret_cast<const uint32_t*>(a.W3 + (size_t)(j < no ? j : 0) * 512 + ch);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t v = (j < no) ? w3c[j] : 0u;
      E::un2(v, w3[j][0], w3[j][1]);
      gw[j][0] = gw[j][1] = 0.f;
    }
    const float (*ds_all)[4] = reinterpret_cast<const float (*)[4]>(scratch + 4 * LOSS_ROWS * 4);
    constexpr int C_UNROLL = LDSACT ? 4 : 4 * LOSS_ROWS;
#pragma unroll C_UNROLL
    for (int r = 0; r < 4 * LOSS_ROWS; ++r) {
      const int m = min(mb + r, n - 1);
      const uint32_t v = LDSACT ? *reinterpret_cast<const uint32_t*>(&Xt[act_off(r, ch)]) : xv[LDSACT ? 0 : r];
      float x[2];
      E::un2(v, x[0], x[1]);
      float d[2] = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float dsj = ds_all[r][j];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          d[e] = fmaf(dsj, w3[j][e], d[e]);
          gw[j][e] = fmaf(dsj, x[e], gw[j][e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 2; ++e)
        if (!(x[e] > 0.f)) d[e] = 0.f;  // relu mask of the fc2 output
      if (E::is_f16) amax = fmaxf(amax, fmaxf(fabsf(d[0]), fabsf(d[1])));
      const uint32_t pk = E::pk2(d[0], d[1]);
      // chain kernel: the gradient replaces the activations in the LDS tile (rows past the end become zero rows); the tile is
      // copied to a.dZ by the caller
      if (LDSACT) *reinterpret_cast<uint32_t*>(&Xt[act_off(r, ch)]) = pk;
      else if (mb + r < n) *reinterpret_cast<uint32_t*>(a.dZ + (size_t)m * 512 + ch) = pk;
      if (mb + r < n) {
        float r0, r1;
        E::un2(pk, r0, r1);
        bsum[0] += r0;   // bias gradient of fc2: the rounded values, in row order
        bsum[1] += r1;
      }
    }
    if (E::is_f16 && a.absmax) absmax_publish(a.absmax, amax);
    *reinterpret_cast<float2*>(a.bias_partials + (size_t)block * 512 + ch) = make_float2(bsum[0], bsum[1]);
    float* gp = a.fc3_partials + (size_t)block * a.fc3_stride;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < no) *reinterpret_cast<float2*>(gp + (size_t)j * 512 + ch) = make_float2(gw[j][0], gw[j][1]);
    if (wv == 0) {
      // fc3 bias gradient and the statistics: sums over the 32 rows in row order
      const float (*red_all)[4] = reinterpret_cast<const float (*)[4]>(scratch + 8 * LOSS_ROWS * 4);
      if (t < no) {
        float fb3 = 0.f;
        for (int r = 0; r < 4 * LOSS_ROWS; ++r) fb3 += ds_all[r][t];
        gp[(size_t)no * 512 + t] = fb3;
      }
      if (t < 3) {
        float stat = 0.f;
        for (int r = 0; r < 4 * LOSS_ROWS; ++r) stat += red_all[r][t];
        a.stat_partials[(size_t)block * 4 + t] = stat;
      }
    }
  }
}

template <class E = EltBf16, int LR = 8>
__global__ __launch_bounds__(256) void loss_kernel(LossArgs a) {
  if ((a.st && !a.st->active) || (a.fault && *a.fault)) return;
  __shared__ float scratch[LOSS_SCRATCH_FLOATS];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  loss_body<false, true, E, LR>(a, blockIdx.x, wv, t, nullptr, scratch, LossPre{0, 0, 0, 0.f, 0.f}, [] { __syncthreads(); });
}

// loss_kernel's launch with the batch gather of the NEXT step as extra workgroups behind it (acez_train_step_next on the wgrad_opt path:
// the optimiser launch that used to carry the gather no longer exists). The loss kernel is a latency chain that leaves most wave slots
// of the chip empty (320 workgroups of 16 rows on 256 CUs, two fit per CU), the gather another (index -> row -> metadata): the
// two overlap. The rows go to the OTHER of the trainer's two input buffers / metadata tables -- this step's weight-gradient launch
// still reads the current ones. Eight rows per wavefront and pass: the free slots hold the whole batch in one pass.
template <class E = EltBf16, int LR = 8>
__global__ __launch_bounds__(256) void loss_gather_kernel(LossArgs a, int nblk, const uint16_t* __restrict__ feat, const int64_t* __restrict__ idx_next,
                                                          uint16_t* __restrict__ out, int n_next, GatherMeta meta) {
  const int ng = (int)gridDim.x - nblk;   // the gather workgroups come FIRST: three dependent load levels, the longest chain of the launch
  if ((int)blockIdx.x < ng) {
    const int lane = threadIdx.x & 63;
    const int wave = ((int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x) >> 6;
    const int nwaves = (ng * (int)blockDim.x) >> 6;
    gather_rows<8>(feat, idx_next, out, n_next, wave, nwaves, lane, meta);
    return;
  }
  if ((a.st && !a.st->active) || (a.fault && *a.fault)) return;
  __shared__ float scratch[LOSS_SCRATCH_FLOATS];
  const int wv = threadIdx.x >> 6, t = threadIdx.x & 63;
  loss_body<false, true, E, LR>(a, (int)blockIdx.x - ng, wv, t, nullptr, scratch, LossPre{0, 0, 0, 0.f, 0.f}, [] { __syncthreads(); });
}

// ---------------------------------------------------------------------------------------------------
// rowseq_loss: the input-gradient chain (rowseq_kernel<true>) with the loss launch as its stage -1 and the next batch's gather in the
// waves that have nothing to do meanwhile -- the fused step's loss launch sat alone on the critical path between two launches that each
// fill every CU: a 12 us latency chain on 320 small workgroups, plus a kernel boundary on either side.
//   stage -1  An 80-row tile is five of loss_kernel's 16-row blocks: row tile mt owns blocks 5 mt .. 5 mt + 4, so every partial (fc3, fc2
//             bias, statistics) lands in loss_kernel's slot and every sum downstream keeps its order -- bit-identical. A workgroup's two
//             wave quartets are two loss workgroups: column tile 0 runs blocks 5 mt (multiplier waves) and 5 mt + 1 (loader waves), column
//             tiles 1..3 run block 5 mt + 1 + nt on their multiplier waves. loss_body as loss_kernel instantiates it; the four waves of a
//             quartet meet through an LDS counter of their own (a barrier would tie the two quartets together), the scratch lies in the
//             staging tiles, which layer 0 does not touch before its K stage 4.
//   hand-off  dZ of fc2 is the In of the first layer: every wave of a loss block posts its progress word behind the acknowledgement of
//             its stores, exactly as a layer epilogue does -- and in column tiles 1..3, whose loader waves run no block, the word of its
//             loader partner w + 4 with it (lanes 0 and 1 of one store) --; layer 0 then waits for the 32 words like any later layer. A
//             block past the batch's last row stores nothing (and owns no partial slot) and still posts.
//   W stages  the loader waves request the first layer's first four W stages before anything else, as the seam prefetch does.
//   gather    the loader waves of column tiles 1..3 have only a hand-off to wait for: they copy the NEXT batch's rows (gather_rows, three
//             dependent load levels -- shorter than a loss block's chain) into the trainer's other input buffer. Under the fault word
//             nothing is stored (GatherMeta::hold); a launch that returns at entry still gathers, as loss_gather_kernel's workgroups did.
// A poll that expires behind stage -1 is a fault like any other seam's: the partials and dZ written so far are per-step buffers.
// ---------------------------------------------------------------------------------------------------

// Stage -1 for the workgroup of tile (mt, nt), all eight waves: the first layer's W stages, the next batch's gather, the tile's loss
// blocks and their hand-off to layer 0 (`W0`: that layer's weights). `dead`: the launch's entry test -- only the gather runs.
// FWD_SEAM (rowstep_kernel): the blocks' `act` rows are produced inside this launch, by the four workgroups of the row tile: every wave
// that runs a block first waits for the tile's 32 words to reach seam `c.base + c.seam0 - 1`, as a layer's loader waves would. Nothing
// is requested in front of that poll: the four workgroups of a tile run in step, so the poll is usually passed at its first look, and
// whatever sits in front of its vmcnt(0) is a round trip added to the chain, not hidden by it (W3, b3 and the rows' indices and metadata
// touched there, to warm this CU's L1 for loss_body: +0.8 us per step, DESIGN_HISTORY).
template <class E, bool FWD_SEAM>
__device__ __forceinline__ void rowseq_loss_stage(const uint16_t* W0, const SeqLossArgs& x, const SeqCtx& c, const bool dead, uint16_t* smem,
                                                  const int mt, const int nt, const int mtiles) {
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int n0 = nt * 128;
  // the quartets' meeting counters: in the bias-partial combine buffer (first used by layer 0's epilogue)
  uint32_t* const qsync = reinterpret_cast<uint32_t*>(smem + RG80_SMEM);
  if (t < 2) qsync[t] = 0u;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();   // (FWD_SEAM: also every wave's last read of the staging tiles the scratch lies in)
  if (w >= 4) {
    const int lw = w - 4;
    if (!dead) {   // rowgemm80_body's issueW(0 .. 3) for layer 0
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = (lw * 4 + j) * 8 + (l >> 3);
        const uint16_t* g = W0 + (size_t)(n0 + row) * 512 + ((l & 7) ^ ((row >> 1) & 7)) * 8;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          __builtin_amdgcn_global_load_lds((gvoid_t*)(g + kt * 64), (lvoid_t*)(smem + kt * RG80_STAGE + (lw * 4 + j) * 8 * 64), 16, 0, 0);
      }
    }
    if (nt != 0 && x.n_next > 0) gather_rows<8>(x.feat, x.idx_next, x.out_next, x.n_next, (mt * 3 + nt - 1) * 4 + lw, mtiles * 12, l, x.meta);
  }
  if (dead) return;
  if (w < 4 || nt == 0) {
    uint32_t* const flag = c.flags + mt * 32;
    const int quartet = w >> 2;
    const int block = 5 * mt + (nt == 0 ? quartet : nt + 1);
    if (FWD_SEAM && seq_poll_expired(flag, t, c.base + c.seam0 - 1u + c.bias, c.limit) && l == 0) seq_raise_fault(c.flags + SEQ_FAULT_WORD, c.st);
    if (block < x.nblk) {
      float* scratch = reinterpret_cast<float*>(smem + 4 * RG80_STAGE) + quartet * (3 * 4 * 4 * 4);
      uint32_t* const f = qsync + quartet;
      loss_body<false, true, E, 4>(x.loss, block, w & 3, l, nullptr, scratch, LossPre{0, 0, 0, 0.f, 0.f}, [f] { lds_bump(f); lds_wait_ge(f, 4u); });
    }
    ACEZ_VMCNT(0);   // this wave's dZ stores are acknowledged by the L2 the four sibling workgroups share
    if (l < (nt == 0 ? 1 : 2)) seq_post(flag + seq_word(nt, w) + 4 * l, c.base + c.seam0);   // the workgroup's eight words: eight waves, or four with their partners'
  }
}

template <class E = EltBf16>
__global__ __launch_bounds__(512) void rowseq_loss_kernel(RowSeqArgs a, SeqLossArgs x) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[RG80_SMEM_SEQ];
  RowTile t;
  if (!row_tile_decode(row_tiles(a.M), t)) return;
  const int mt = t.mt, nt = t.nt();
  seq_record_placement(a, t);
  const bool dead = SEQ_DEAD(a.st, a.flags);
  const SeqCtx c{a.M, a.st, a.flags, a.base[mt], 1u, a.spin_limit, a.poll_bias};
  rowseq_loss_stage<E, false>(a.layer[0].W, x, c, dead, smem, mt, nt, row_tiles(a.M));
  if (dead) {   // (one seam more than rowseq_kernel's launch)
    if (threadIdx.x == 0) seq_catch_up(a.base[mt] + seq_seams(a.n_layers, 1), a.flags, mt, nt);
    return;
  }
  rowseq_layers<true, E, true>(a.layer, a.n_layers, c, smem, mt, nt * 128);
}

// ---------------------------------------------------------------------------------------------------
// rowstep: the forward chain, the loss stage and the input-gradient chain of a fused step in ONE launch -- rowseq_kernel<false> followed
// by rowseq_loss_kernel on the same grid, decode and LDS. The dependency from the last forward layer to the loss blocks to the first
// input-gradient layer is local to a row tile, whose four workgroups share an XCD in both chains: the kernel boundary between the two
// launches ordered nothing that the row tile's counter does not order, and cost a launch ramp plus the drain of the forward chain's
// dirty lines (which now leave the L2 by eviction, under the input-gradient layers).
//   seams     per launch and row tile: n_fwd - 1 between the forward layers, one from the last forward layer (which signals: TAIL) to the
//             loss blocks, one from the loss blocks to the first input-gradient layer, n_bwd - 1 between those: n_fwd + n_bwd (15 for the
//             default head). One array of lines, one base per row tile; a dead launch leaves the same words.
//   L1        nothing is read through a CU's L1 before it is produced: `act` (fc2's output) has no reader inside the forward chain, the
//             buffers the input-gradient chain and the loss write are none of the forward chain's inputs, the mask bits are written and
//             read by the same lane. No fence, no cache write-back or invalidate anywhere in the launch.
// ---------------------------------------------------------------------------------------------------

template <class E = EltBf16>
__global__ __launch_bounds__(512) void rowstep_kernel(RowStepArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[RG80_SMEM_SEQ];
  RowTile t;
  if (!row_tile_decode(row_tiles(a.M), t)) return;
  const int mt = t.mt, nt = t.nt();
  seq_record_placement(a, t);
  const bool dead = SEQ_DEAD(a.st, a.flags);
  const uint32_t base = a.base[mt];
  if (!dead) rowseq_layers<false, E, false, true>(a.fwd, a.n_fwd, SeqCtx{a.M, a.st, a.flags, base, 0u, a.spin_limit, a.poll_bias}, smem, mt, nt * 128);
  const SeqCtx c{a.M, a.st, a.flags, base, (uint32_t)a.n_fwd + 1u, a.spin_limit, a.poll_bias};
  rowseq_loss_stage<E, true>(a.bwd[0].W, a.x, c, dead, smem, mt, nt, row_tiles(a.M));
  if (dead) {
    if (threadIdx.x == 0) seq_catch_up(base + seq_seams(a.n_fwd + a.n_bwd, 1), a.flags, mt, nt);
    return;
  }
  rowseq_layers<true, E, true>(a.bwd, a.n_bwd, c, smem, mt, nt * 128);
}

// the product's instantiations (head_kernels.h): the host launches them from head_api.hip
ACEZ_CHAIN_KERNELS(template __global__, EltBf16)
ACEZ_CHAIN_KERNELS(template __global__, EltF16)

}  // namespace acez

// ---------------------------------------------------------------------------------------------------
// rowseq_group: the chains of several trainers in one launch (host: head_group.hip, which says why). Its bodies are rowseq_kernel's, so
// it lives beside them; kernel and argument structs are in the global namespace (head_kernels.h).
// ---------------------------------------------------------------------------------------------------
using namespace acez;

template <bool BWD, class E = EltBf16>
__global__ __launch_bounds__(512) void rowseq_group_kernel(RowSeqGroupArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[RG80_SMEM_SEQ];
  __shared__ uint32_t run_mask;
  // rowseq_kernel's decode over the largest member's row tiles: the four column tiles of row tile mt of EVERY member share one XCD
  RowTile t;
  if (!row_tile_decode(a.mtiles, t)) return;
  const int mt = t.mt, n0 = t.n0();
  if (threadIdx.x == 0) {
    // which members this workgroup runs, decided once for the whole workgroup: row tile mt inside the member's batch, its schedule
    // active and its fault word down (rowseq_kernel's entry test, per member). A member that does not run keeps its words in step with
    // the host's bases exactly as rowseq_kernel's early return does; row tiles past a member's batch are not counted (seq_account).
    uint32_t run = 0;
    for (int h = 0; h < a.H; ++h) {
      if (mt >= row_tiles(a.M[h])) continue;
      uint32_t* flags = a.heads[h].flags;
      if (SEQ_DEAD(a.st[h], flags)) {
        seq_catch_up(a.base[h][mt] + seq_seams(a.n_layers), flags, mt, t.nt());
        continue;
      }
      run |= 1u << h;
    }
    run_mask = run;
  }
  __syncthreads();
  const uint32_t run = __builtin_amdgcn_readfirstlane(run_mask);
  if (!run) return;
  auto table = [&](int h, int layer) -> const SeqLayer& {
    const GroupHead& g = a.heads[h];
    return BWD ? g.bwd[a.layer0 + layer] : g.fwd[a.variant[h]][a.layer0 + layer];
  };
  bool first = true;
  for (int layer = 0; layer < a.n_layers; ++layer) {
    for (int h = 0; h < a.H; ++h) {
      if (!((run >> h) & 1u)) continue;
      const SeqLayer& y = table(h, layer);
      // the body this workgroup runs next: the next member of this layer, else the first member of the next layer
      const uint32_t later = run & ~((2u << h) - 1u);
      const uint16_t* next_W = nullptr;
      if (later) next_W = table(__builtin_ctz(later), layer).W;
      else if (layer + 1 < a.n_layers) next_W = table(__builtin_ctz(run), layer + 1).W;
      const TrainState* st = a.st[h];
      RowGemmArgs g;   // (rowseq_layers' row -> RowGemmArgs, SeqLink and epilogue shape, written out: see there)
      g.In = y.In; g.W = y.W; g.bias = y.bias; g.add = y.add; g.mask_out = y.mask_out; g.mask_in = y.mask_in; g.res = y.res; g.out_main = y.out_main; g.out_aux = y.out_aux;
      g.bias_partials = y.bias_partials; g.M = a.M[h]; g.N = 512; g.K = 512; g.relu = BWD ? 0 : 1; g.aux_mode = y.aux_mode; g.st = st;
      g.absmax = (BWD && st) ? const_cast<uint32_t*>(st->dz_absmax_slots) : nullptr;
      SeqLink q;
      // (target and budget are scalar operands of the poll: the table lives in global memory, so say that they are uniform)
      // (... and the line's address, the scalar base of the poll's load)
      const uint64_t line = reinterpret_cast<uint64_t>(a.heads[h].flags + mt * 32);
      q.flag = reinterpret_cast<uint32_t*>((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)line) |
                                           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(line >> 32)) << 32));
      q.post = (uint32_t)__builtin_amdgcn_readfirstlane((int)(a.base[h][mt] + (uint32_t)layer + 1u));
      q.target = q.post - 1u + (uint32_t)__builtin_amdgcn_readfirstlane((int)a.poll_bias[h]);
      q.first = first; q.wait = layer > 0; q.signal = layer + 1 < a.n_layers;
      q.next_W = next_W;
      q.flag_index = (uint32_t)(mt * 32); q.limit = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.heads[h].spin_limit);
      first = false;
      if (!BWD) {
        if (y.aux_mode == AUX_RESIDUAL) rowgemm80_body<true, false, false, AUX_RESIDUAL, true, E>(g, smem, 1, mt, n0, q);
        else rowgemm80_body<true, false, false, AUX_NONE, true, E>(g, smem, 1, mt, n0, q);
      } else {
        if (y.add) rowgemm80_body<false, true, true, AUX_UNMASKED, true, E>(g, smem, 1, mt, n0, q);
        else if (y.aux_mode == AUX_UNMASKED) rowgemm80_body<false, false, true, AUX_UNMASKED, true, E>(g, smem, 1, mt, n0, q);
        else rowgemm80_body<false, false, true, AUX_NONE, true, E>(g, smem, 1, mt, n0, q);
      }
    }
  }
}

ACEZ_GROUP_KERNELS(template __global__, EltBf16)
ACEZ_GROUP_KERNELS(template __global__, EltF16)
