// head_sched.h -- the schedule: learning-rate recurrences, the hot copy of TrainState and the wave that closes a step, shared by the sched_*
// kernels and every launch that carries the wave (head_optim.hip, pose_fused.hip).
#pragma once
#include "head_opt.h"

namespace acez {

// ---------------------------------------------------------------------------------------------------
// schedule (one thread): ace_schedule.py:72-101 before the step, :115-126 after it. The learning rate is
// advanced with the same chainable recurrences torch.optim.lr_scheduler uses, in double.
// ---------------------------------------------------------------------------------------------------
// cos(pi x) for x in [0,1] with basic operations only (Taylor around the nearest multiple of 1/2).
__device__ double det_cos_pi(double x) {
  const double PI = 3.14159265358979323846;
  // reduce: cos(pi x) = -sin(pi (x - 1/2))
  const double y = (x - 0.5) * PI;  // in [-pi/2, pi/2]
  const double y2 = y * y;
  // sin(y), Taylor to y^21 (|y| <= pi/2: remainder < 1e-17)
  double term = y, sum = y;
  for (int k = 1; k <= 11; ++k) {
    term = -term * y2 / (double)((2 * k) * (2 * k + 1));
    sum += term;
  }
  return -sum;
}

__device__ double onecycle_lr(const SchedConfig& c, int step_num) {
  // torch OneCycleLR(max_lr, total_steps, pct_start=0.3, anneal='cos', div_factor=25, final_div_factor=1e4,
  //                  three_phase=False, cycle_momentum=False)
  const double initial_lr = c.lr_max / 25.0;
  const double min_lr = initial_lr / 1e4;
  const double end1 = 0.3 * (double)c.iterations - 1.0;
  const double end2 = (double)c.iterations - 1.0;
  double start, end, pct;
  if ((double)step_num <= end1 || c.iterations <= 1) {
    start = initial_lr; end = c.lr_max;
    pct = (end1 > 0) ? (double)step_num / end1 : 1.0;
  } else {
    start = c.lr_max; end = min_lr;
    pct = ((double)step_num - end1) / (end2 - end1);
  }
  const double cos_out = det_cos_pi(pct) + 1.0;
  return end + (start - end) / 2.0 * cos_out;
}

// The scalar part of TrainState (everything but the criterion ring) as a struct of named locals: the schedule code runs on such a
// copy, loaded with ONE batch of loads and written back once. Operating on `st->field` directly made every access its own global
// round trip (no alias information: ~25 dependent L2 accesses, 5.5 us for one wavefront -- as long as the whole batch gather it
// shares a launch with).
struct SchedHot {
  int active, iteration, max_iterations, in_cooldown, warmup_epoch, cooldown_epoch, nan_flag, opt_steps, crit_count, crit_pos, calib_steps;
  float loss_weight, last_loss, last_inliers;
  double lr, calib_g, calib_m, calib_v, beta1_pow, beta2_pow;
  AdamScalars adam;
  int pose_enable, pose_opt_steps;
  double pose_b1pow, pose_b2pow;
  AdamScalars pose_adam;
  float grad_scale, inv_grad_scale;
};
__device__ __forceinline__ SchedHot load_hot(const TrainState* st) {
  SchedHot h;
  h.active = st->active; h.iteration = st->iteration; h.max_iterations = st->max_iterations; h.in_cooldown = st->in_cooldown;
  h.warmup_epoch = st->warmup_epoch; h.cooldown_epoch = st->cooldown_epoch; h.nan_flag = st->nan_flag; h.opt_steps = st->opt_steps;
  h.crit_count = st->crit_count; h.crit_pos = st->crit_pos; h.calib_steps = st->calib_steps;
  h.loss_weight = st->loss_weight; h.last_loss = st->last_loss; h.last_inliers = st->last_inliers;
  h.lr = st->lr; h.calib_g = st->calib_g; h.calib_m = st->calib_m; h.calib_v = st->calib_v; h.beta1_pow = st->beta1_pow; h.beta2_pow = st->beta2_pow;
  h.adam = st->adam;
  h.pose_enable = st->pose_enable; h.pose_opt_steps = st->pose_opt_steps; h.pose_b1pow = st->pose_b1pow; h.pose_b2pow = st->pose_b2pow;
  h.pose_adam = st->pose_adam;
  h.grad_scale = st->grad_scale; h.inv_grad_scale = st->inv_grad_scale;
  return h;
}
__device__ __forceinline__ void store_hot(TrainState* st, const SchedHot& h) {
  st->active = h.active; st->iteration = h.iteration; st->max_iterations = h.max_iterations; st->in_cooldown = h.in_cooldown;
  st->warmup_epoch = h.warmup_epoch; st->cooldown_epoch = h.cooldown_epoch; st->nan_flag = h.nan_flag; st->opt_steps = h.opt_steps;
  st->crit_count = h.crit_count; st->crit_pos = h.crit_pos; st->calib_steps = h.calib_steps;
  st->loss_weight = h.loss_weight; st->last_loss = h.last_loss; st->last_inliers = h.last_inliers;
  st->lr = h.lr; st->calib_g = h.calib_g; st->calib_m = h.calib_m; st->calib_v = h.calib_v; st->beta1_pow = h.beta1_pow; st->beta2_pow = h.beta2_pow;
  st->adam = h.adam;
  st->pose_enable = h.pose_enable; st->pose_opt_steps = h.pose_opt_steps; st->pose_b1pow = h.pose_b1pow; st->pose_b2pow = h.pose_b2pow;
  st->pose_adam = h.pose_adam;
  st->grad_scale = h.grad_scale; st->inv_grad_scale = h.inv_grad_scale;
}

__device__ __forceinline__ void sched_prepare_hot(SchedHot& h, const SchedConfig& c, float crit_min) {
  // everything the kernels of iteration `h.iteration` need: cool-down decision, active flag, loss weight, AdamW scalars
  const int it = h.iteration;
  // check_and_set_cooldown(iteration)   ace_schedule.py:72-101
  if (c.schedule == SCHED_1CYCLEPOLY && !h.in_cooldown && it >= c.warmup_iterations) {
    const bool by_duration = it >= (h.max_iterations - c.cooldown_iterations);
    const int cnt = h.crit_count;
    const bool dynamic = (cnt > 0) && ((double)crit_min > c.cooldown_trigger_percent);   // min(buffer) > trigger, ace_schedule.py:86-90
    if (by_duration || dynamic) {
      h.in_cooldown = 1;
      h.cooldown_epoch = 0;
      h.max_iterations = it + c.cooldown_iterations;
    }
  }
  h.active = (it < h.max_iterations && !h.nan_flag) ? 1 : 0;   // ace_trainer.py:509-510
  // loss weight of this iteration (ace_loss.py:55-69)
  float wgt = c.soft_clamp;
  if (c.loss_type == LOSS_DYNTANH) {
    double sw = (double)it / (double)c.iterations;
    if (c.circle_schedule) sw = 1.0 - sqrt(1.0 - sw * sw);
    wgt = (float)((1.0 - sw) * (double)c.soft_clamp + (double)c.soft_clamp_min);
  }
  h.loss_weight = wgt;
  // scalars of torch.optim.AdamW for this step (double like the Python side, then cast like the fp32 kernels);
  // beta^step is kept as a running product (one multiply per step, same value as pow to ~1e-16 relative)
  {
    const double lr = h.lr;
    const double b1p = h.beta1_pow * c.beta1, b2p = h.beta2_pow * c.beta2;  // beta^(opt_steps + 1)
    const double bc1 = 1.0 - b1p;
    const double bc2 = 1.0 - b2p;
    AdamScalars s;
    s.decay = (float)(1.0 - lr * c.weight_decay);
    s.one_minus_beta1 = (float)(1.0 - c.beta1);
    s.beta2 = (float)c.beta2;
    s.one_minus_beta2 = (float)(1.0 - c.beta2);
    s.bc2_sqrt = (float)sqrt(bc2);
    s.eps = (float)c.eps;
    s.step_size = (float)(lr / bc1);
    h.adam = s;
  }
  if (c.pose_refinement) {
    h.pose_enable = (it > c.pose_wait) ? 1 : 0;   // ace_trainer.py:634
    const double b1p = h.pose_b1pow * c.beta1, b2p = h.pose_b2pow * c.beta2;
    AdamScalars s;
    s.decay = (float)(1.0 - c.pose_lr * c.weight_decay);
    s.one_minus_beta1 = (float)(1.0 - c.beta1);
    s.beta2 = (float)c.beta2;
    s.one_minus_beta2 = (float)(1.0 - c.beta2);
    s.bc2_sqrt = (float)sqrt(1.0 - b2p);
    s.eps = (float)c.eps;
    s.step_size = (float)(c.pose_lr / (1.0 - b1p));
    h.pose_adam = s;
  }
}

__device__ void sched_prepare(TrainState* st, const SchedConfig& c, float crit_min) {
  SchedHot h = load_hot(st);
  sched_prepare_hot(h, c, crit_min);
  store_hot(st, h);
}

// Executed by ONE full wavefront (all 64 lanes must call it): the lanes cooperate on the minimum of the cool-down
// criterion ring, lane 0 does the scalar bookkeeping.
// The schedule state lives in TWO slots (acez_trainer::st_slot): the kernels of a step read the slot the host passes them, the
// bookkeeping that closes the step reads that slot (`src`) and writes the OTHER one (`st`), which the host hands to every later
// launch. So the bookkeeping may run beside kernels that still read the old slot -- the optimiser's own launch (adamw_next_kernel) --
// without any ordering between them. Every path through this function leaves `st` a complete state (src == st: in place).
__device__ void sched_post_wave(const TrainState* src, TrainState* st, const SchedConfig& c, const float* grad_stats, float inv_global_batch,
                                float* log_loss, float* log_inl, int log_cap, const int* fault, const float* stat_partials, int n_loss_blocks,
                                const GradReduceArgs* tail = nullptr) {
  const int lane = threadIdx.x & 63;
  const uint32_t my_stripe = __builtin_nontemporal_load(&src->dz_absmax_slots[lane * 32]);
  uint32_t amax_bits = my_stripe;   // fp16: largest propagated gradient of the step (scaled units), over the 64 stripes
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) amax_bits = max(amax_bits, (uint32_t)__shfl_xor((int)amax_bits, off));
  // every load of the wave first: the scalar state (used by lane 0), the statistics, this lane's two ring entries
  SchedHot h = load_hot(src);
  const float ring0 = src->crit_buf[lane], ring1 = (lane + 64 < 100) ? src->crit_buf[lane + 64] : 0.f;
  // tail mode: the loss kernel's partials are requested with the state above, before anything is looked at (they sat behind the branch
  // below: a second dependent round trip of the wave that closes every step)
  float g0 = 0.f, g1 = 0.f, g2 = 0.f;
  if (tail) {   // inside the optimiser's own launch (adamw_next_kernel / wgrad_opt_kernel): the reduced statistics are being written by sibling
                // workgroups of this launch, so the wave reduces the loss kernel's partials itself -- tail_output's arithmetic: the same bits
    int64_t d;
    const int64_t k0 = (int64_t)tail->n_layers * 512 + (tail->n_params - tail->n_wide);
    g0 = tail_output(*tail, k0, lane, d); g1 = tail_output(*tail, k0 + 1, lane, d); g2 = tail_output(*tail, k0 + 2, lane, d);
  }
  // (split flow: a rank's fault arrives all-reduced in statistics slot 3, and adamw_body raises the local fault word from it -- in
  // adamw_next_kernel inside the SAME launch as this wave, so the word itself would be a race here; the statistic is not)
  const bool fault_reduced = !tail && fmodf(grad_stats[3], 1024.f) != 0.f;
  if ((fault && *fault) || fault_reduced || !h.active) {
    // the step was abandoned (rowseq fault: no iteration is counted, nothing is logged) or the schedule has ended (state frozen,
    // ace_trainer.py:509-510): the other slot becomes a copy
    if (src != st) {
      st->crit_buf[lane] = ring0;
      if (lane + 64 < 100) st->crit_buf[lane + 64] = ring1;
      st->dz_absmax_slots[lane * 32] = my_stripe;
      if (lane == 0) store_hot(st, h);
    }
    return;
  }
  if (!tail) { g0 = grad_stats[0]; g1 = grad_stats[1]; g2 = grad_stats[2]; }
  const float loss = g0 * inv_global_batch;
  const float inl = g1 * inv_global_batch;
  // minimum of the ring as it will be after this step's push: the entries that stay, and the new value
  float crit_min = inl;
  {
    const int cnt = h.crit_count, pos = h.crit_pos;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = lane + 64 * k;
      const bool keep = i < cnt && !(cnt == 100 && i == pos);
      if (keep) crit_min = fminf(crit_min, k == 0 ? ring0 : ring1);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) crit_min = fminf(crit_min, __shfl_xor(crit_min, off));
  }
  {   // the ring as it is after this step's push (1cyclepoly: the new value replaces entry crit_pos), written by all lanes
    const bool push = c.schedule == SCHED_1CYCLEPOLY;
    const int pos = h.crit_pos;
    st->crit_buf[lane] = (push && lane == pos) ? inl : ring0;
    if (lane + 64 < 100) st->crit_buf[lane + 64] = (push && lane + 64 == pos) ? inl : ring1;
  }
  st->dz_absmax_slots[lane * 32] = 0u;   // the stripes of the state the NEXT step's kernels fold into
  if (lane != 0) return;
  h.last_loss = loss;
  h.last_inliers = inl;
  if (loss != loss) h.nan_flag = 1;   // ace_trainer.py:615-617
  const int it = h.iteration;
  if (it < log_cap) { log_loss[it] = loss; log_inl[it] = inl; }
  // fp16: an overflowing step's head update was skipped by adamw_body / wgrad_opt_kernel (the same test on the same words; split flow: the
  // all-reduced flag in statistics slot 3), as GradScaler.step skips optimizer.step(): AdamW's step count does not advance either
  // (ace_schedule.py:112-113). The pose / calibration optimisers are stepped outside the scaler (ace_trainer.py:634-640): they advance.
  const bool head_skipped = c.f16 && (f16_overflow(amax_bits) || (!tail && grad_stats[3] >= 1024.f));
  if (!head_skipped) {
    h.opt_steps += 1;
    h.beta1_pow *= c.beta1;
    h.beta2_pow *= c.beta2;
  }
  if (c.pose_refinement && h.pose_enable) {
    h.pose_opt_steps += 1;
    h.pose_b1pow *= c.beta1;
    h.pose_b2pow *= c.beta2;
  }
  // calibration refiner: its own AdamW on the scalar g (refine_calibration.py:21-26,58-59)
  if (c.refine_calibration) {
    const double g = (double)g2;
    const double lr = c.calib_lr;
    h.calib_steps += 1;
    double p = h.calib_g;
    p = p * (1.0 - lr * c.weight_decay);
    h.calib_m = h.calib_m + (g - h.calib_m) * (1.0 - c.beta1);
    h.calib_v = h.calib_v * c.beta2 + (1.0 - c.beta2) * g * g;
    const double bc1 = 1.0 - pow(c.beta1, (double)h.calib_steps);
    const double bc2 = 1.0 - pow(c.beta2, (double)h.calib_steps);
    const double denom = sqrt(h.calib_v) / sqrt(bc2) + c.eps;
    p = p - (lr / bc1) * (h.calib_m / denom);
    // fp32 parameter in the reference
    h.calib_g = (double)(float)p;
    h.calib_m = (double)(float)h.calib_m;
    h.calib_v = (double)(float)h.calib_v;
  }
  // scheduler.step()   ace_schedule.py:115-126
  if (c.schedule == SCHED_1CYCLEPOLY) {
    if (h.in_cooldown) {
      // LinearLR(start=1, end=lr_min/lr_max, total_iters=cooldown_iterations), chainable form
      const int e = ++h.cooldown_epoch;
      const double sf = 1.0, ef = c.lr_min / c.lr_max;
      if (e <= c.cooldown_iterations)
        h.lr = h.lr * (1.0 + (ef - sf) / ((double)c.cooldown_iterations * sf + (double)(e - 1) * (ef - sf)));
    } else {
      const int e = ++h.warmup_epoch;
      const double sf = c.warmup_lr / c.lr_max, ef = 1.0;
      if (e <= c.warmup_iterations)
        h.lr = h.lr * (1.0 + (ef - sf) / ((double)c.warmup_iterations * sf + (double)(e - 1) * (ef - sf)));
    }
    // rolling buffer of the last 100 batch_inliers (the entry itself was written above)
    const int pos = h.crit_pos;
    h.crit_pos = (pos + 1 == 100) ? 0 : pos + 1;
    if (h.crit_count < 100) h.crit_count += 1;
  } else if (c.schedule == SCHED_CIRCLE) {
    const int e = ++h.warmup_epoch;
    h.lr = onecycle_lr(c, e);
  }
  if (c.f16) {
    // Gradient scale of the NEXT step (the role of torch.cuda.amp.GradScaler.update, ace_schedule.py:107-113): the power of two that
    // would have put this step's largest propagated gradient near 4096 -- fp16 tops out at 65504: a factor of 16 for the change from
    // one step to the next. After an overflow (an inf was stored: this step's update was skipped by adamw_body, as GradScaler.step
    // skips it) the scale drops by 2^8. Powers of two only: scaling then commutes with fp16 rounding for every value in range.
    int e = ilogbf(h.grad_scale);
    if (f16_overflow(amax_bits)) e -= 8;
    else if (amax_bits != 0u) e = ilogbf(4096.f / (__uint_as_float(amax_bits) * h.inv_grad_scale));
    e = min(16, max(-8, e));
    h.grad_scale = ldexpf(1.f, e);
    h.inv_grad_scale = ldexpf(1.f, -e);
  }
  h.iteration = it + 1;   // ace_trainer.py:495
  sched_prepare_hot(h, c, crit_min);   // bookkeeping of the NEXT iteration, so that a step needs a single schedule launch
  store_hot(st, h);
}

}  // namespace acez
