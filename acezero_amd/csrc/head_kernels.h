// head_kernels.h -- argument structs shared by the head kernels and their host-side launcher.
#pragma once
#include <stdint.h>

#include "gemm_common.h"

namespace acez {

constexpr int MAX_LAYERS = 20;

enum { AUX_NONE = 0, AUX_RESIDUAL = 1, AUX_UNMASKED = 2 };
enum { LOSS_TANH = 0, LOSS_DYNTANH = 1, LOSS_L1 = 2, LOSS_L1_SQRT = 3, LOSS_L1_LOGL1 = 4 };
enum { SCHED_CONSTANT = 0, SCHED_1CYCLEPOLY = 1, SCHED_CIRCLE = 2 };

struct AdamScalars {
  float decay, one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt, eps, step_size;
};

// Device-resident schedule / optimiser state: the training loop never synchronises the host.
struct TrainState {
  int active;          // this step runs (iteration < max_iterations and no NaN)
  int iteration;       // TrainerACE.iteration
  int max_iterations;  // ScheduleACE.max_iterations
  int in_cooldown;
  int warmup_epoch;    // last_epoch of the warm-up LinearLR / of OneCycleLR
  int cooldown_epoch;  // last_epoch of the cool-down LinearLR
  int nan_flag;
  int opt_steps;       // AdamW state['step']
  int crit_count;      // entries of the cool-down criterion ring in use (<= 100)
  int crit_pos;        // next slot of the ring to overwrite
  int calib_steps;
  float loss_weight;   // soft clamp of this iteration
  float last_loss, last_inliers;
  float crit_buf[100];  // cooldown_criterium_buffer (ace_schedule.py:44,121-125) as a ring: only its minimum is ever used
  double lr;            // param_group['lr']
  double calib_g, calib_m, calib_v;
  double beta1_pow, beta2_pow;  // beta^opt_steps
  AdamScalars adam;
  // pose-refinement network (refine_poses.py): own AdamW
  int pose_enable, pose_opt_steps;
  double pose_b1pow, pose_b2pow;
  AdamScalars pose_adam;
  // fp16 operands: the gradient chain is propagated scaled by grad_scale (a power of two, so that scaling commutes with fp16 rounding
  // wherever nothing under- or overflows) and un-scaled where it meets the fp32 optimiser. Chosen by the schedule wave from the largest
  // |d loss / d fc3 output| of the step before (what torch.cuda.amp.GradScaler does with inf checks, ace_schedule.py:70,107-113). bf16: 1.
  float grad_scale, inv_grad_scale;
  // bit patterns of the largest propagated gradient magnitudes of the running step, scaled units (absmax_publish): 64 words on 64
  // different 128-byte lines, workgroup b folds into word (b & 63) * 32. ONE word would serialise every wavefront's atomic of a launch
  // on one L2 line (11-13 ns each: measured +51 us on the input-gradient chain, +13 us on the loss kernel); readers take the maximum of
  // the 64 (absmax_all). Last member: the host's state read stops before it.
  uint32_t dz_absmax_slots[64 * 32];
};

// Per-row metadata of the gathered batch, written where the batch is gathered and read by the loss kernel: without it the loss kernel
// starts with a chain of three dependent loads (idx -> view_idx -> view_image) in front of its first computation, because vmcnt
// completes in order. {view, image, target u, target v (float bits)} of row r; dst == null: not written.
struct GatherMeta {
  int4* dst;
  const int32_t* view_idx;
  const int32_t* view_image;
  const float* target_px;
  const int* hold;   // null, or the trainer's sticky fault word: while it is set the gather stores nothing (the rows of the faulted step must
                     // survive until the host has finished that step, head_api.hip wgo_recover)
};

struct SchedConfig {
  int schedule, iterations, warmup_iterations, cooldown_iterations;
  int loss_type, circle_schedule, refine_calibration;
  float soft_clamp, soft_clamp_min;
  double lr_min, lr_max, warmup_lr, cooldown_trigger_percent;
  double beta1, beta2, eps, weight_decay, calib_lr;
  int pose_refinement, pose_wait;
  double pose_lr;
  int f16;   // fp16 operands (dynamic gradient scale) instead of bf16
};

struct RowGemmArgs {
  const uint16_t* In;    // [M][K] bf16
  const uint16_t* W;     // [N][K] bf16
  const float* bias;     // [N] or null
  const uint16_t* add;   // [M][N] or null: added before the activation
  // ReLU masks as bits (round 6; the input-gradient layers used to re-read the forward layer's whole 16-bit output tile through LDS only to
  // test `> 0`: 36.7 MB per step, 20 KiB of LDS-DMA per tile and layer). The forward layer and the input-gradient layer that needs its mask
  // run on the same 80 x 128 tiles with the same accumulator layout, so the mask is LANE-PRIVATE: every multiplier lane packs the 40 bits
  // of its own outputs -- fragment f = 2 j + i: bits 9 - f / 25 - f of word x (word y) = the two (next two) of its four outputs are > 0
  // after the 16-bit rounding -- and the backward lane loads the same 8 bytes: [(row tile * 4 + column tile) * 4 + wave][lane] uint2,
  // 2 KiB per tile instead of 20.
  uint2* mask_out;        // forward (bias + ReLU) launches: where the bits go, or null (inference)
  const uint2* mask_in;   // input-gradient launches: out_main is zeroed where the bit is clear; null = not a masked launch
  const uint16_t* res;   // [M][N] residual input for AUX_RESIDUAL
  uint16_t* out_main;
  uint16_t* out_aux;
  float* bias_partials;  // [row tiles * 2][512] column sums of out_main (masked launches) or null
  int M, N, K, relu, aux_mode;
  const TrainState* st;
  uint32_t* absmax;  // fp16 gradient launches: TrainState::dz_absmax_slots (else null)
};

struct WgradArgs {
  const uint16_t* dZ[MAX_LAYERS];
  const uint16_t* In[MAX_LAYERS];
  int64_t w_off[MAX_LAYERS], b_off[MAX_LAYERS];
  float* slabs;
  int64_t slab_stride;
  int M, nslabs, n_layers;
  const TrainState* st;
  const uint16_t* zeros;  // >= 256 bytes of zeros (source of the DMA for rows past the end of a slab)
};

struct LossArgs {
  const uint16_t* act;  // [n][512] output of fc2
  const uint16_t* W3;   // [no][512] bf16
  const float* b3;      // [no] fp32
  int n, no, use_homogeneous;
  float mean[3], max_inv_scale, min_inv_scale, h_beta;
  // training only (idx == null -> inference)
  const int64_t* idx;
  const int4* meta;   // GatherMeta::dst of the batch `idx` (null: the chain idx -> view_idx -> view_image is followed here)
  const float* target_px;
  const float* target_crds;      // [patches][3] ground-truth scene coordinates (zeros = none) or null: use_depth mode
  const int32_t* view_idx;
  const float* view_aug_inv;
  const float* view_K;
  const float* view_Kinv;
  const int32_t* view_image;
  const float* image_pose_inv;   // [images][16] world->cam poses used by this step (refined ones under pose refinement)
  float* row_dT;                 // [n][12] d(loss)/d(pose rows 0..2) per batch row, or null
  int* row_image;                // [n] image of each batch row, or null
  int loss_type, refine_calibration;
  float hard_clamp, depth_min, depth_max, depth_target, inlier_px, inv_batch, focal_init;
  const TrainState* st;
  // outputs
  float* out_xyz;        // [n][3] or null; with planar_hw > 0: [frames][3][planar_hw] maps (row m = frame * planar_hw + pixel)
  int planar_hw, row_offset;   // row_offset: index of this launch's row 0 in the whole batch (chunked inference)
  uint16_t* dZ;          // [n][512] gradient wrt the fc2 pre-activation
  float* fc3_partials;   // [blocks][fc3_stride]
  int64_t fc3_stride;
  float* stat_partials;  // [blocks][4]
  float* bias_partials;  // [blocks][512] column sums of dZ
  uint32_t* absmax;      // fp16 training: TrainState::dz_absmax_slots (else null)
  const int* fault;      // training: the trainer's sticky fault word (null: none). While it is set the launch is a no-op: the buffers of the
                         // faulted step stay as they are until the host's fall-back has finished that step
};

struct GradReduceArgs {
  const float* slabs;
  int64_t slab_stride;
  int nslabs;
  const float* fc3_partials;
  int64_t fc3_stride;
  const float* stat_partials;
  int n_loss_blocks;
  const float* bias_partials;  // [n_layers][bias_layer_stride]
  int64_t bias_layer_stride;
  int bias_count[MAX_LAYERS];  // partial rows per layer
  int n_layers;
  float* grad;
  int64_t n_wide, n_params;
  const TrainState* st;
  int skip_wide;   // fused single-GPU step: the slabs are summed by adamw_kernel itself, only the tail is reduced here
  const int* fault;   // the trainer's rowseq fault word (null: none); written to statistics slot 3
};

struct AdamArgs {
  float* params;
  float* m;
  float* v;
  const float* grad;
  uint16_t* Wb;
  uint16_t* WbT;
  uint16_t* W3b;
  int64_t w_off[MAX_LAYERS], b_off[MAX_LAYERS];
  int64_t fc3_off, n_fc3, n_params;
  int n_layers, no;
  const TrainState* st;
  // fused single-GPU step (acez_train_step): wide-layer gradients are read as the fixed-order sum of the wgrad slabs
  // (the same additions grad_reduce_kernel performs) instead of from `grad`; null in the backward / all-reduce / update flow
  const float* slabs;
  int nslabs;
  int64_t slab_stride;
  GradReduceArgs tail;   // with slabs != null: the partials of the small parameters and statistics (reduced here as well)
  int* fault;            // the trainer's rowseq fault word: a faulted step updates nothing
  int f16;               // the compute copies W / W^T / W3 are fp16 (else bf16)
  int layer_lo, layer_hi;   // wide layers whose WEIGHT tiles this launch updates (sharded data-parallel update: the rank's own
                            // layers); biases, fc3 and the statistics are always handled. 0 .. n_layers = everything
};

// wgrad_opt_kernel (single-GPU fused step): the weight-gradient launch finishes the optimiser step of the wide layers itself. The two
// row slabs of a 128 x 128 gradient tile run on two CUs of ONE XCD; each sends the half of its partial tile the other one owns through
// that XCD's L2 (`xch`) and bumps the owner's counter (`flags`, the hand-off of rowseq_kernel: L2-local atomic, bounded sc1 poll, no
// fence), then applies AdamW to its own half: slab 0 + slab 1 in that order, the additions grad_reduce_kernel / adamw_kernel perform.
// What a loader wave of wgrad_opt_kernel whose exchange poll expired leaves behind, so that the host's fall-back can FINISH the step
// (head_api.hip wgo_recover: wgrad_kernel on the step's untouched buffers, then wgo_recover_kernel on exactly the regions whose wave
// timed out, with the step's own optimiser scalars): after it the parameters are bitwise those of the two-launch flow's step.
struct WgoFaultRec {
  AdamScalars s;          // st->adam of the faulted step (the schedule wave of that launch has already moved the state on)
  float inv_scale;        // st->inv_grad_scale of the faulted step
  int M;                  // its batch rows
  uint32_t epoch;         // WgradOptArgs::epoch of the faulted launch (0: no wgrad_opt fault is pending)
  uint32_t pad;
  const uint16_t* in0;    // WgradArgs::In[0] of the faulted launch (the trainer swaps its two input buffers every step)
};

struct WgradOptArgs {
  AdamArgs ad;           // the optimiser's arguments (slabs unused; tail = the partial buffers of this step: NaN / overflow guards)
  float* xch;            // [n_layers * 16 tiles][2 owners][64][128] fp32
  uint32_t* flags;       // [n_layers * 16 tiles][2 owners][32]: one counter per receiving workgroup on its own 128-byte line
  uint32_t target;       // value of a counter once both sending waves of this launch have stored (2 x launches so far)
  uint32_t spin_limit;   // poll budget, as RowSeqArgs::spin_limit
  int nsmall;            // workgroups 0 .. nsmall - 1 also run one small-parameter block of the optimiser each (adamw_small_columns); 0: none
  int do_post;           // the last workgroup also runs the schedule wave that closes the step (sched_post_wave)
  unsigned long long* trace;   // diagnostics build (ACEZ_WGO_TRACE=1, tools/wgo_trace.py): [256 workgroups][12 waves][8] s_memtime stamps; else null
  uint32_t epoch;        // launches so far, this one included (> 0)
  uint32_t* status;      // [workgroups][8 loader waves]: epoch * 4 + 3 = "this wave's poll expired in launch `epoch`, its rows of the half tile
                         // were NOT updated" (written by timed-out waves only: nothing is stored on the normal path)
  WgoFaultRec* rec;      // written by the timed-out waves of the FIRST faulting launch (later launches see the fault word and skip by guard)
  int fault_mod;         // diagnostics build: workgroups with b % fault_mod == 1 wait for a count that never comes (a partial fault); 0: none
};

// ---- the one-launch chains (head_kernels.hip): a chain's layer table and the launches' arguments
struct SeqLayer {
  const uint16_t *In, *W;
  const float* bias;
  const uint16_t *add, *res;
  uint2* mask_out;          // RowGemmArgs::mask_out / mask_in
  const uint2* mask_in;
  uint16_t *out_main, *out_aux;
  float* bias_partials;
  int aux_mode, pad;
};
constexpr int SEQ_MAX_LAYERS = 8;
struct RowSeqArgs {
  SeqLayer layer[SEQ_MAX_LAYERS];
  int n_layers, M;
  const TrainState* st;
  uint32_t* flags;     // [64 row tiles][32] progress words + [SEQ_FAULT_WORD] the fault word
  uint32_t base[64];   // per row tile: seams completed by earlier launches (a launch only touches the row tiles of ITS batch)
  uint32_t spin_limit; // poll budget of a hand-off (polls of >= ~0.5 us); expired: fault word + st->active = 0
  uint32_t poll_bias;  // 0; tests (seq_account): added to every seam this launch POLLS for, not to what it posts -- a seam that never comes
  uint32_t* xcc_dbg;   // null, or [8 + 256]: words 0..7 |= 1 << XCC_ID of the workgroups with blockIdx & 7 = word (sticky); word
                       // 8 + 4 mt + nt = XCC_ID of the workgroup that owned tile (mt, nt) in the last launch (tests: the four column
                       // tiles of a row tile must report the same XCD)
                       // flags[SEQ_FAULT_WORD] = the sticky fault word (non-zero: a poll of this trainer has expired, every launch returns at
                       // once), flags[SEQ_FAULT_WORD + 1] = a copy of the poll budget (diagnostics)
};

// rowseq_loss_kernel / rowstep_kernel: the loss launch as a stage of the chain's launch (head_kernels.hip, "rowseq_loss")
struct SeqLossArgs {
  LossArgs loss;
  int nblk;                  // loss blocks of the batch (loss_kernel's grid)
  const uint16_t* feat;      // the next batch: gather_rows' arguments (n_next = 0: none)
  const int64_t* idx_next;
  uint16_t* out_next;
  int n_next;
  GatherMeta meta;
};

// rowstep_kernel: both chains and the loss stage of a fused step in one launch (head_kernels.hip, "rowstep")
struct RowStepArgs {
  SeqLayer fwd[SEQ_MAX_LAYERS], bwd[SEQ_MAX_LAYERS];
  int n_fwd, n_bwd, M;
  const TrainState* st;
  uint32_t* flags;       // as RowSeqArgs: flags, base, spin_limit, xcc_dbg -- once for both chains
  uint32_t base[64];
  uint32_t spin_limit;
  uint32_t poll_bias;
  uint32_t* xcc_dbg;
  SeqLossArgs x;
};
static_assert(sizeof(RowStepArgs) <= 4096, "kernel-argument segment");

// ---- the schedule wave's arguments in the launches that carry it (step_begin_kernel, adamw_next_kernel, wgrad_opt_kernel, step_begin_pose_kernel)
struct PostArgs {
  const TrainState* src;   // the slot the closing step's kernels read
  TrainState* st;          // the slot the bookkeeping writes (the other one; == src: in place)
  SchedConfig c;
  const float* grad_stats;
  float inv_global_batch;
  float* log_loss;
  float* log_inl;
  int log_cap;
  const int* fault;
  const float* stat_partials;   // the loss kernel's per-workgroup statistics of the step being closed (slot 3: largest |ds|) and their count
  int n_loss_blocks;
};

// ---- grids and workgroup shapes the host and the kernels agree on
constexpr int WGRAD_RING = 4;                       // slots of the [dZ | In] stage ring, 32 KiB each (RING - 1 stages in flight per CU)
constexpr int WGRAD_LOADERS = 8;                    // loader waves per workgroup (beside the 4 multiplier waves)
constexpr int WGRAD_THREADS = 256 + 64 * WGRAD_LOADERS;
// Workgroups of the optimiser's part of a launch: the first adamw_small_blocks() handle the small parameters (biases, fc3) and, in
// the fused step, the statistics; then one workgroup per 64 x 64 weight tile. (Small first: each of them is a chain of dependent
// round trips -- partials -> butterfly -> p, m, v -> store -- that should run under the streaming tile blocks, not after them.)
__host__ __device__ inline int adamw_small_blocks(int n_layers, int64_t n_fc3, bool fused) {
  const int64_t n_small = (int64_t)n_layers * 512 + n_fc3;
  return fused ? (int)((n_small + 4 + 63) / 64)   // fused: 64 outputs per workgroup, four lanes each (adamw_small_columns)
               : (int)((n_small + 255) / 256);
}
// small-parameter workgroups of a fused optimiser launch (wgrad_opt_kernel: one per 32 outputs, in the multiplier waves of the first ones)
__host__ __device__ inline int small_cols_blocks(int n_layers, int64_t n_fc3, int lanes_per_output) {
  const int64_t per = 256 / lanes_per_output;
  return (int)(((int64_t)n_layers * 512 + n_fc3 + 4 + per - 1) / per);
}
constexpr int GR_TAIL_LANES = 8;   // lanes per output of grad_reduce_kernel's tail (4: 97 workgroups with 80 loads per lane in flight; 8: 193 with 40)
__host__ __device__ inline int grad_reduce_tail_blocks(int n_layers, int64_t n_fc3) { return small_cols_blocks(n_layers, n_fc3, GR_TAIL_LANES); }

// ---- whole-frame inference (head_maps.hip)
struct HeadMapsArgs {
  const uint16_t* In;       // [n][512] feature rows
  const uint16_t* Wf;       // fragment-ordered weights of the L wide layers
  const float* params;      // the flat fp32 parameter vector (bias of layer l at l * 262656 + 262144)
  uint16_t* R[8];           // R[b], b = 1 .. nb: [n][512] scratch of the residual stream after block b - 1 (unused entries null)
  uint16_t* Out;            // [n][512]: the output of the last wide layer (fc2), what loss_kernel's fc3 reads -- or null with `fc3` below
  int n, nb;
  // fc3 + de-homogenisation on the finished tile (ace_network.py:135-149): the arithmetic of loss_body's phases A / B (same per-lane FMA
  // chains, the same DPP wave sum, the same expressions: the same function of the activations as loss_kernel's); the
  // [n][512] activation map is then neither written nor read (315 MB each way per 64 frames) and the separate launch (117 us) is gone.
  int fc3;                  // 1: write scene coordinates to out_xyz instead of activations to Out
  const uint16_t* W3;       // [no][512] 16-bit
  const float* b3;          // [no]
  int no, use_homogeneous;
  float mean[3], max_inv_scale, min_inv_scale, h_beta;
  float* out_xyz;           // [n][3], or with planar_hw > 0 [frames][3][planar_hw] (row m = frame * planar_hw + pixel), rows offset by row_offset
  int planar_hw, row_offset;
};

// ---- pose refinement (pose_kernels.hip, pose_small.hip, pose_fused.hip)
struct PoseNetArgs {
  const float* P;          // flat parameters
  const float* Wt;         // [4][128][128] transposed copies of conv2, conv3, fc1, fc2 (pose_transpose_kernel), forward only
  const float* T0;         // [I][16] original world->cam poses
  int I;
  float w;                 // update weight (refine_poses.py:165)
  float *a1, *a2, *a3, *r, *f1, *f2;   // [I][128] activations
  float* delta;            // [I][12]
  float* pose_cur;         // [I][16] refined poses (forward) 
  const float* dT;         // [I][12] gradient wrt the refined pose (backward)
  float *ddelta, *dz2, *dz1, *dr, *dzc3, *dzc2, *dzc1;   // backward: gradients wrt each layer's pre-activation output
  const int* active;
  int ortho;               // 0 gram-schmidt, 1 procrustes (--refinement_ortho)
  unsigned long long* trace;   // diagnostics build (ACEZ_POSE_TRACE=1, tools/pose_trace.py): [tiles][16] s_memtime stamps of thread 0; else null
};
constexpr int64_t PN_SKIP_W = 0, PN_SKIP_B = 1536, PN_C1_W = 1664, PN_C1_B = 3200, PN_C2_W = 3328, PN_C2_B = 19712, PN_C3_W = 19840,
                  PN_C3_B = 36224, PN_F1_W = 36352, PN_F1_B = 52736, PN_F2_W = 52864, PN_F2_B = 69248, PN_F3_W = 69376, PN_F3_B = 70912;
constexpr int PN_IMG = 16;     // images per workgroup
struct PoseWgradArgs {
  const float* dY[7]; const float* X[7];
  int O[7], K[7], xpitch[7];
  int64_t offW[7], offB[7];
  int I;
  float* grad;            // pose gradient vector (d_grad + n_params + 4)
  const int* active;
  int job_start[8];       // prefix sums of ceil(O / 16) * ceil(K / 16) over the layers
  // Fused optimiser (single-GPU step: the tile's gradient is final inside this workgroup, so AdamW -- adamw_small_kernel's arithmetic --
  // is applied on the spot and the transposed forward copies Wt[wt_slot] of the four 128 x 128 layers are refreshed): fuse = 0 in
  // the backward / all-reduce / update flow, where adamw_small_kernel and pose_transpose_kernel do this after the all-reduce.
  int fuse;
  float *p, *m, *v, *Wt;
  int wt_slot[7];         // index into Wt[4][128][128] of the layer, -1: none
  const AdamScalars* sc;
  const int* enable;      // st->pose_enable (ace_trainer.py:634-636)
  const int* fault;       // rowseq fault word: an abandoned step updates nothing
  unsigned long long* trace;   // diagnostics build (ACEZ_POSE_TRACE=1): [jobs][16] s_memtime stamps of thread 0; else null
};
// W = waves of the workgroup (template parameter of pose_small.hip's bodies): W / 2 reduction slices, 64 W threads. The forward (S3) runs with
// 8 waves, the reduce + backward chain (S1) with 4: its launch is shared with the optimiser's 256-thread workgroups (twice the waves to
// dispatch cost more than the shorter layers gave back), and its gradients keep the two-slice summation order.
constexpr int PN4_W_FWD = 8, PN4_W_BWD = 4;
// T = images per pose workgroup: 16 = the v_mfma_f32_16x16x4_f32 bodies of pose_kernels.hip (256 threads), 4 = the small tiles of
// pose_small.hip (a quarter of the matrix time per layer, four times as many CUs, 512 threads; the default). A launch's workgroups
// all have pose_threads<T>() threads: in the launches shared with the optimiser its workgroups use the first 256 (the other waves
// return at once), the gather's rows are spread over the waves there are.
template <int T>
constexpr int pose_threads() { return 256; }              // the launches that hold S1 (PN4_W_BWD = 4 waves)
template <int T>
constexpr int pose_fwd_threads() { return T == 16 ? 256 : 64 * PN4_W_FWD; }

// ---------------------------------------------------------------------------------------------------
// Every kernel the host launches (head_api.hip, head_group.hip), declared with the launch bounds of its definition. Templates: the product's
// instantiations, once -- ACEZ_*_KERNELS(extern template __global__, E) here, ACEZ_*_KERNELS(template __global__, E) in the defining unit.
// ---------------------------------------------------------------------------------------------------
// head_kernels.hip (the chain unit)
template <bool BIAS_RELU, bool HAS_ADD, bool HAS_MASK, int AUX, class E>
__global__ __launch_bounds__(512) void rowgemm80_kernel(RowGemmArgs a);
template <bool BWD, class E>
__global__ __launch_bounds__(512) void rowseq_kernel(RowSeqArgs a);
__global__ __launch_bounds__(512) void seq_probe_kernel(uint32_t* rec /*[256]*/, int mtiles);
template <class E, int LR>
__global__ __launch_bounds__(256) void loss_kernel(LossArgs a);
template <class E, int LR>
__global__ __launch_bounds__(256) void loss_gather_kernel(LossArgs a, int nblk, const uint16_t* __restrict__ feat, const int64_t* __restrict__ idx_next,
                                                          uint16_t* __restrict__ out, int n_next, GatherMeta meta);
template <class E>
__global__ __launch_bounds__(512) void rowseq_loss_kernel(RowSeqArgs a, SeqLossArgs x);
template <class E>
__global__ __launch_bounds__(512) void rowstep_kernel(RowStepArgs a);
#define ACEZ_CHAIN_KERNELS(X, E)                                                                                                       \
  X void rowgemm80_kernel<true, false, false, AUX_NONE, E>(RowGemmArgs);                                                               \
  X void rowgemm80_kernel<true, false, false, AUX_RESIDUAL, E>(RowGemmArgs);                                                           \
  X void rowgemm80_kernel<false, false, true, AUX_NONE, E>(RowGemmArgs);                                                               \
  X void rowgemm80_kernel<false, false, true, AUX_UNMASKED, E>(RowGemmArgs);                                                           \
  X void rowgemm80_kernel<false, true, true, AUX_UNMASKED, E>(RowGemmArgs);                                                            \
  X void rowgemm80_kernel<false, true, true, AUX_NONE, E>(RowGemmArgs);                                                                \
  X void rowseq_kernel<false, E>(RowSeqArgs);                                                                                          \
  X void rowseq_kernel<true, E>(RowSeqArgs);                                                                                           \
  X void rowseq_loss_kernel<E>(RowSeqArgs, SeqLossArgs);                                                                               \
  X void rowstep_kernel<E>(RowStepArgs);                                                                                               \
  X void loss_kernel<E, 4>(LossArgs);                                                                                                  \
  X void loss_gather_kernel<E, 4>(LossArgs, int, const uint16_t*, const int64_t*, uint16_t*, int, GatherMeta);
ACEZ_CHAIN_KERNELS(extern template __global__, EltBf16)
ACEZ_CHAIN_KERNELS(extern template __global__, EltF16)

// head_optim.hip (the optimiser unit)
__global__ __launch_bounds__(256) void gather_kernel(const uint16_t* __restrict__ feat, const int64_t* __restrict__ idx, uint16_t* __restrict__ out, int n,
                                                     const TrainState* st, GatherMeta meta);
__global__ __launch_bounds__(256) void step_begin_kernel(const uint16_t* __restrict__ feat, const int64_t* __restrict__ idx, uint16_t* __restrict__ out, int n,
                                                         PostArgs p, GatherMeta meta);
template <class E>
__global__ __launch_bounds__(WGRAD_THREADS) void wgrad_kernel(WgradArgs a);
template <class E>
__global__ __launch_bounds__(WGRAD_THREADS) void wgrad_opt_kernel(WgradArgs a, WgradOptArgs o, PostArgs post);
template <class E>
__global__ __launch_bounds__(512) void wgo_recover_kernel(AdamArgs ad, const float* __restrict__ slabs, int64_t slab_stride, const uint32_t* __restrict__ status,
                                                          const WgoFaultRec* __restrict__ rec, int n_layers);
__global__ __launch_bounds__(256) void grad_reduce_kernel(GradReduceArgs a);
__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a);
__global__ __launch_bounds__(256, 4) void adamw_next_kernel(AdamArgs a, int n_adam, const uint16_t* __restrict__ feat, const int64_t* __restrict__ idx_next,
                                                            uint16_t* __restrict__ out, int n_next, PostArgs p, GatherMeta meta);
__global__ __launch_bounds__(256) void transpose16_kernel(const uint16_t* __restrict__ Wb, uint16_t* __restrict__ WbT, int layer_lo);
__global__ __launch_bounds__(256) void import16_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ Wb, uint16_t* __restrict__ WbT, int own_lo,
                                                       int own_hi);
__global__ __launch_bounds__(256) void recast_kernel(AdamArgs a);
__global__ void sched_reactivate_kernel(TrainState* st);
__global__ void sched_init_kernel(TrainState* st, SchedConfig c);
__global__ __launch_bounds__(64) void sched_post_kernel(const TrainState* src, TrainState* st, SchedConfig c, const float* grad_stats, float inv_global_batch,
                                                        float* log_loss, float* log_inl, int log_cap, const int* fault, const float* stat_partials,
                                                        int n_loss_blocks);
#define ACEZ_OPTIM_KERNELS(X, E)                                                                                                       \
  X void wgrad_kernel<E>(WgradArgs);                                                                                                   \
  X void wgrad_opt_kernel<E>(WgradArgs, WgradOptArgs, PostArgs);                                                                       \
  X void wgo_recover_kernel<E>(AdamArgs, const float*, int64_t, const uint32_t*, const WgoFaultRec*, int);
ACEZ_OPTIM_KERNELS(extern template __global__, EltBf16)
ACEZ_OPTIM_KERNELS(extern template __global__, EltF16)

// ... and the pose chain it includes (pose_kernels.hip -> pose_small.hip -> pose_fused.hip)
__global__ __launch_bounds__(256) void pose_compose_kernel(const float* T0 /*[I][16]*/, const float* delta /*[I][12]*/, float w, float* out /*[I][16]*/,
                                                           int n_images, const int* active, int ortho);
__global__ __launch_bounds__(256) void pose_compose_bwd_kernel(const float* T0, const float* delta, float w, const float* dT /*[I][12]*/,
                                                               float* ddelta /*[I][12]*/, int n_images, const int* active, int ortho);
__global__ __launch_bounds__(256) void pose_mlp_fwd_kernel(PoseNetArgs a);
__global__ __launch_bounds__(256) void pose_transpose_kernel(const float* P, float* Wt, const int* active);
__global__ __launch_bounds__(256) void pose_mlp_bwd_kernel(PoseNetArgs a);
template <int PW_BATCH, int PW_WAVES>
__global__ __launch_bounds__(64 * PW_WAVES, PW_BATCH <= 32 ? PW_WAVES / 2 : 2) void pose_mlp_wgrad_kernel(PoseWgradArgs a);
__global__ __launch_bounds__(256) void pose_grad_reduce2_kernel(const float* row_dT /*[n][12]*/, const int* row_image /*[n]*/, int n, float* dT /*[I][12]*/,
                                                                int n_images, const int* active);
template <int T>
__global__ __launch_bounds__(pose_fwd_threads<T>(), T == 16 ? 2 : 1) void step_begin_pose_kernel(const uint16_t* __restrict__ feat, const int64_t* __restrict__ idx,
                                                                 uint16_t* __restrict__ out, int n, PostArgs p, int do_post, PoseNetArgs a, int np,
                                                                 GatherMeta meta);
template <int T>
__global__ __launch_bounds__(pose_fwd_threads<T>()) void pose_fwd_t_kernel(PoseNetArgs a);
template <int T>
__global__ __launch_bounds__(256, 3) void adamw_pose_kernel(AdamArgs a, PoseNetArgs pn, const float* row_dT, const int* row_image, int n, int np);
template <int T>
__global__ __launch_bounds__(256, 3) void grad_reduce_pose_kernel(GradReduceArgs a, PoseNetArgs pn, const float* row_dT, const int* row_image, int n, int np);
__global__ __launch_bounds__(256, 4) void adamw_split_pose_kernel(AdamArgs a, int npb, float* p, float* m, float* v, const float* g, int64_t n,
                                                                  const AdamScalars* sc, const int* enable, const int* active, const int* fault,
                                                                  const float* reduced_fault, float* Wt, int n_adam, const uint16_t* __restrict__ feat,
                                                                  const int64_t* __restrict__ idx_next, uint16_t* __restrict__ out, int n_next, GatherMeta meta);
#define ACEZ_POSE_KERNELS(X, T)                                                                                                        \
  X void step_begin_pose_kernel<T>(const uint16_t*, const int64_t*, uint16_t*, int, PostArgs, int, PoseNetArgs, int, GatherMeta);       \
  X void adamw_pose_kernel<T>(AdamArgs, PoseNetArgs, const float*, const int*, int, int);                                              \
  X void grad_reduce_pose_kernel<T>(GradReduceArgs, PoseNetArgs, const float*, const int*, int, int);
ACEZ_POSE_KERNELS(extern template __global__, 4)
ACEZ_POSE_KERNELS(extern template __global__, 16)
extern template __global__ void pose_fwd_t_kernel<4>(PoseNetArgs);
extern template __global__ void pose_mlp_wgrad_kernel<16, 8>(PoseWgradArgs);

// head_maps.hip
__global__ __launch_bounds__(256) void wfrag_pack_kernel(const uint16_t* __restrict__ Wb, uint16_t* __restrict__ Wf, int n_frags);
template <class E>
__global__ __launch_bounds__(512) void head_maps_kernel(HeadMapsArgs a);
extern template __global__ void head_maps_kernel<EltBf16>(HeadMapsArgs);
extern template __global__ void head_maps_kernel<EltF16>(HeadMapsArgs);

}  // namespace acez

// ---- the head group's chain launch (rowseq_group_kernel, head_kernels.hip; host: head_group.hip). These three names live in the global
// namespace, where the group's file has always declared them: the kernel's symbol is part of the stored profiles.
constexpr int GROUP_MAX = 8;

// one member's chain layer tables (device memory, written once by acez_train_group_create)
struct GroupHead {
  acez::SeqLayer fwd[2][acez::MAX_LAYERS];   // [which of the trainer's two input buffers is R[0] this step][layer] (acez_train_step_next swaps them)
  acez::SeqLayer bwd[acez::MAX_LAYERS];
  uint32_t* flags;               // the trainer's progress words + sticky fault word (RowSeqArgs::flags)
  uint32_t spin_limit;
  int pad;
};

// per-step arguments (kernel argument block: no host-to-device copy per step)
struct RowSeqGroupArgs {
  const GroupHead* heads;
  const acez::TrainState* st[GROUP_MAX];
  int M[GROUP_MAX];
  int variant[GROUP_MAX];              // GroupHead::fwd index
  uint32_t base[GROUP_MAX][64];        // per member and row tile: seams completed by earlier launches (RowSeqArgs::base)
  uint32_t poll_bias[GROUP_MAX];       // RowSeqArgs::poll_bias
  int H, layer0, n_layers, mtiles;     // layers [layer0, layer0 + n_layers) of every member's table; mtiles = the largest member's
};
template <bool BWD, class E>
__global__ __launch_bounds__(512) void rowseq_group_kernel(RowSeqGroupArgs a);
#define ACEZ_GROUP_KERNELS(X, E) \
  X void rowseq_group_kernel<false, E>(RowSeqGroupArgs); \
  X void rowseq_group_kernel<true, E>(RowSeqGroupArgs);
ACEZ_GROUP_KERNELS(extern template __global__, acez::EltBf16)
ACEZ_GROUP_KERNELS(extern template __global__, acez::EltF16)
