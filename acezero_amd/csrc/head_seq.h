// head_seq.h -- the same-XCD hand-off protocol of the head's one-launch chains, each piece once, for the device and for the host.
#pragma once
#include "head_kernels.h"

namespace acez {

// ---------------------------------------------------------------------------------------------------
// The same-XCD hand-off protocol, each piece once. Its users: the chain kernels (rowseq_kernel,
// rowseq_loss_kernel, rowstep_kernel, rowseq_group_kernel: head_kernels.hip) through rowgemm80_body<..., SEQ> and rowseq_loss_stage, and
// wgrad_opt_kernel's exchange (head_optim.hip). The host's side is seq_account (head_api.hip).
// ---------------------------------------------------------------------------------------------------
constexpr int SEQ_FAULT_WORD = 64 * 32;   // flags[SEQ_FAULT_WORD]: the trainer's sticky fault word, behind its 64 row-tile lines (128 bytes = 32 progress words each)

// Row tiles of an n-row batch, the chain kernels' grid for them (N = 512 -> 4 column tiles of 128; a multiple of 8 row-tile groups) and
// the decode of that grid: blockIdx.x & 7 is the XCD the workgroup lands on, so the four column tiles of a row tile share an XCD and its
// L2 (conv_tiles.h's tile_decode at 80 x 128, from the tile count: the group kernel decodes over its largest member's). False: a padding
// workgroup of the last round.
__host__ __device__ constexpr int row_tiles(int n) { return (n + 79) / 80; }
inline dim3 chain_grid(int mtiles) { return dim3(8 * 4 * ((mtiles + 7) / 8)); }
struct RowTile {
  int mt, jx;   // row tile; workgroup index inside its XCD (the column tile is its two low bits)
  __device__ __forceinline__ int nt() const { return jx & 3; }           // column tile
  __device__ __forceinline__ int n0() const { return (jx & 3) * 128; }   // ... and its first column
};
__device__ __forceinline__ bool row_tile_decode(const int mtiles, RowTile& t) {
  const int per_xcd = (mtiles + 7) >> 3;
  t.jx = blockIdx.x >> 3;
  t.mt = (blockIdx.x & 7) * per_xcd + (t.jx >> 2);
  return t.mt < mtiles;
}

// Seams (hand-offs) a launch adds to each of its row tiles: one between two consecutive stages, a stage being a chain layer or the loss
// stage. rowseq_kernel: n - 1; rowseq_loss_kernel: n; rowstep_kernel: n_fwd + n_bwd; rowseq_group_kernel: cnt - 1 per member. Seams are
// numbered absolutely per row tile: a launch whose base is b completes seams b + 1 .. b + seq_seams, the host advances its bases by as
// much (seq_account), and a launch that returns at entry leaves b + seq_seams in its words (seq_catch_up).
// Progress words: word nt * 8 + w of a row tile's line belongs to wave w of column tile nt -- 4 workgroups x 8 waves, the 32 words of the
// line. A wave stores the number of the seam it has completed into ITS word (seq_post); a consumer reads the whole line and passes when
// none of the 32 is behind its seam (seq_poll_expired). One writer per word, absolute values: no read-modify-write, and nothing queues on
// the line the way the 32 same-line atomics of a shared counter did (11-13 ns each in the L2).
__host__ __device__ constexpr uint32_t seq_seams(int n_layers, int loss_stages = 0) { return (uint32_t)(n_layers + loss_stages - 1); }
__device__ __forceinline__ int seq_word(const int nt, const int w) { return nt * 8 + w; }

// The bounded poll of a row tile's line. True: the budget expired.
// Bounded: a sibling that never arrives (workgroups of one row tile on different XCDs -- every L2 then holds its own copy
// of the line and none of them ever shows all 32 words --, or a sibling that is never dispatched) must not hang the
// stream. When the budget expires the wave raises the sticky fault word (seq_raise_fault) and goes on with whatever is in memory: the
// results of this launch are garbage, the optimiser and schedule kernels of the step see the word and do nothing, and
// the host switches the trainer to per-layer launches at its next state read (head_api.hip).
// The whole poll is ONE asm statement: written as a C loop with a second exit, the compiler re-scheduled the K loops and
// epilogues of the input-gradient instantiation (+3 us per chain, same instruction mix; found by diffing the ISA of a
// build without the bound). sc1: past this CU's L1; the line and the tiles live in the L2 all four workgroups share,
// no L2 invalidate. Lane l loads word l & 31 (one request for the line; the byte offset 4 (l & 31) is formed from `tid`, the thread's index in
// the workgroup, INSIDE the statement: formed outside, it was hoisted out of the layer loop into a register of its own); a lane is behind while
// word - target < 0 as a signed number (a sibling that is a seam AHEAD does not hold anybody up, and the 32-bit seam number may wrap); the
// wave passes when no lane is behind: one compare into vcc, one scalar test of it. The budget is counted in polls
// (>= ~0.5 us each: an L2 round trip + the sleep).
__device__ __forceinline__ bool seq_poll_expired(const uint32_t* line, uint32_t tid, uint32_t target, uint32_t limit) {
  uint32_t vseen, voff, spins, timed;
  asm volatile(
      "v_lshlrev_b32 %[voff], 2, %[tid]\n\t"
      "v_and_b32 %[voff], 0x7c, %[voff]\n\t"
      "s_mov_b32 %[spins], 0\n\t"
      "s_mov_b32 %[timed], 0\n"
      "1:\n\t"
      "global_load_dword %[vseen], %[voff], %[line] sc1\n\t"
      "s_waitcnt vmcnt(0)\n\t"
      "v_subrev_u32 %[vseen], %[target], %[vseen]\n\t"
      "v_cmp_gt_i32 vcc, 0, %[vseen]\n\t"
      "s_cbranch_vccz 2f\n\t"
      "s_sleep 1\n\t"   // 64 clocks between two polls
      "s_add_u32 %[spins], %[spins], 1\n\t"
      "s_cmp_lt_u32 %[spins], %[limit]\n\t"
      "s_cbranch_scc1 1b\n\t"
      "s_mov_b32 %[timed], 1\n"
      "2:"
      : [vseen] "=&v"(vseen), [voff] "=&v"(voff), [spins] "=&s"(spins), [timed] "=&s"(timed)
      : [line] "s"(line), [tid] "v"(tid), [target] "s"(target), [limit] "s"(limit)
      : "memory", "scc", "vcc");
  return timed != 0;
}
// ... and of ONE counter word with several senders (wgrad_opt_kernel's exchange: two waves bump a pair's word, seq_bump): every lane
// loads the same word, the loop condition is scalar.
__device__ __forceinline__ bool seq_poll_word_expired(const uint32_t* flag, uint32_t target, uint32_t limit) {
  uint32_t vseen, sseen, spins, timed;
  asm volatile(
      "s_mov_b32 %[spins], 0\n\t"
      "s_mov_b32 %[timed], 0\n"
      "1:\n\t"
      "global_load_dword %[vseen], %[flag], off sc1\n\t"
      "s_waitcnt vmcnt(0)\n\t"
      "v_readfirstlane_b32 %[sseen], %[vseen]\n\t"
      "s_sub_i32 %[sseen], %[sseen], %[target]\n\t"
      "s_cmp_ge_i32 %[sseen], 0\n\t"
      "s_cbranch_scc1 2f\n\t"
      "s_sleep 1\n\t"   // 64 clocks between two polls
      "s_add_u32 %[spins], %[spins], 1\n\t"
      "s_cmp_lt_u32 %[spins], %[limit]\n\t"
      "s_cbranch_scc1 1b\n\t"
      "s_mov_b32 %[timed], 1\n"
      "2:"
      : [vseen] "=&v"(vseen), [sseen] "=&s"(sseen), [spins] "=&s"(spins), [timed] "=&s"(timed)
      : [flag] "v"(flag), [target] "s"(target), [limit] "s"(limit)
      : "memory", "scc");
  return timed != 0;
}

// An expired poll (one lane of the wave): the fault word goes up and the step is switched off -- every later kernel of this trainer starts
// with `if (!st->active) return`, the chain kernels with SEQ_DEAD.
__device__ __forceinline__ void seq_raise_fault(uint32_t* fault_word, const TrainState* st) {
  __hip_atomic_store(fault_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (st) __hip_atomic_store(const_cast<int*>(&st->active), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A wave's progress word (one lane of the wave, behind the acknowledgement of the wave's stores: ACEZ_VMCNT(0)): a plain vector store of
// the seam number the wave has completed -- the value a consumer of that seam polls for --, no atomic, no fence.
__device__ __forceinline__ void seq_post(uint32_t* word, const uint32_t seam) {
  asm volatile("global_store_dword %0, %1, off" ::"v"(word), "v"(seam) : "memory");
}
// The bump of a counter word that has several senders (wgrad_opt_kernel's exchange; one lane of the wave, behind ACEZ_VMCNT(0)): an
// L2-local atomic without return, no fence.
__device__ __forceinline__ void seq_bump(uint32_t* flag, const uint32_t inc) {
  asm volatile("global_atomic_add %0, %1, off" ::"v"(flag), "v"(inc) : "memory");
}

// The entry test of a launch on a trainer's lines: training has ended on the device (after an expired poll the fault handler has
// cleared `active` too), or a poll of this trainer has expired in an EARLIER launch -- the buffers of the faulted step are left alone
// until the host has fallen back. Both words are wave-uniform loads. A dead launch does no work, but its words keep step with the
// host's bases (seq_catch_up, one lane of the workgroup: the launch's last seam number `last` = base + seq_seams into the workgroup's eight
// words -- the words are absolute, so this is a live launch's end state by construction).
// A macro, not a function: as a function (by value or on the kernel arguments by reference) `flags` was fetched in front of the test of
// `st` and the four chain kernels' registers were allocated anew -- the two loads keep the order they were measured with. Used by the chain
// kernels and by rowseq_group_kernel.
#define SEQ_DEAD(st, flags) (((st) && !(st)->active) || (flags)[SEQ_FAULT_WORD])
__device__ __forceinline__ void seq_catch_up(const uint32_t last, uint32_t* flags, const int mt, const int nt) {
  uint4* const w8 = reinterpret_cast<uint4*>(flags + mt * 32 + seq_word(nt, 0));
  w8[0] = w8[1] = make_uint4(last, last, last, last);
}

// The placement record of a chain kernel (xcc_dbg: RowSeqArgs; null: none), by thread 0 of the workgroup that owns tile t: which XCD ran
// it. `a`: the kernel arguments by reference, RowSeqArgs or RowStepArgs. (A chain kernel's entry is row_tile_decode and its return --
// a workgroup without a row tile touches no counter; inside a function that return became a predicate over the whole entry --, this
// record, then SEQ_DEAD.)
template <class A>
__device__ __forceinline__ void seq_record_placement(const A& a, const RowTile& t) {
  if (a.xcc_dbg && threadIdx.x == 0) {
    const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;   // HW_REG_XCC_ID[3:0]
    atomicOr(a.xcc_dbg + (blockIdx.x & 7), 1u << xcc);
    a.xcc_dbg[8 + t.mt * 4 + t.nt()] = xcc;
  }
}

// One layer of one workgroup. SEQ = false: the whole of rowgemm80_kernel. SEQ = true: one link of rowseq_kernel (below), where
// the layers of a dependent chain run in ONE launch and the kernel boundary is replaced by a same-XCD hand-off (SeqLink).
struct SeqLink {
  uint32_t* flag;        // the row tile's line of 32 progress words in this XCD's L2, each monotonically increasing
  uint32_t target;       // the seam in front of this layer: in every word once the four column tiles of the layer before have stored their outputs
  uint32_t post;         // the seam behind this layer: what its waves store into their words
  bool first, wait;      // first layer of the launch (requests its own W stages) / In is produced inside this launch
  bool signal;           // another layer follows: post the wave's word after the stores
  const uint16_t* next_W;  // weights of the layer after (null: none): its first four W stages are requested before the epilogue
  uint32_t flag_index;   // flag = flags + flag_index; the trainer's sticky fault word is flags[SEQ_FAULT_WORD]: set when the bounded poll
                         // below expires (the host then falls back to per-layer launches, head_api.hip seq_fault_check)
  uint32_t limit;        // the poll budget (a number of polls), a kernel argument
};

// LDS counters through which the waves of one workgroup meet without s_barrier (the wave quartets of rowseq_loss_stage; wgrad_opt_kernel's
// multiplier and loader waves after the K loop: a barrier would make the loader waves' arithmetic wait for the multiplier waves'
// small-parameter work and vice versa). Ahead of their first user, the loss stage.
// spin until an LDS counter of this workgroup reaches `target`
__device__ __forceinline__ void lds_wait_ge(uint32_t* f, uint32_t target) {
  while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) __builtin_amdgcn_s_sleep(1);
  asm volatile("" ::: "memory");
}
__device__ __forceinline__ void lds_bump(uint32_t* f) {   // after this wave's earlier LDS operations (the LDS executes a wave's operations in order)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

}  // namespace acez
