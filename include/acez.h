/*
 * acez.h -- C ABI of libacez.so, the MI355X (gfx950) implementation of ACE Zero's hot path.
 *
 * Two groups of entry points, one per hot-path row group of SURVEY.md section 8:
 *
 *   (R) DSAC* RANSAC-PnP registration     replaces  dsacstar/dsacstar.cpp:66-186 (dsacstar_rgb_forward),
 *                                                   bound at dsacstar/dsacstar.cpp:898-899 as
 *                                                   dsacstar.forward_rgb and called from
 *                                                   register_mapping.py:229-242.
 *   (T) scene-coordinate head training    replaces  ace_trainer.py:454-497 (run_epoch gathers) and
 *                                                   ace_trainer.py:499-679 (training_step), i.e.
 *                                                   ace_network.py:120-149 (Head.forward),
 *                                                   ace_loss.py:39-91 (ReproLoss.compute),
 *                                                   ace_schedule.py:72-126 (ScheduleACE).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / pybind types cross this boundary.
 *   - every "d_" pointer is a DEVICE pointer (HBM), every "h_" pointer a host pointer.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream). All device work is enqueued on it;
 *     functions documented as asynchronous return before the work completes.
 *   - return value: ACEZ_OK (0) or a negative error code; nothing throws across the boundary.
 *     "PnP failed" is NOT an error (dsacstar_util.h:104-117,185-196): the call succeeds with a zero pose.
 *   - the library owns only its contexts and their workspaces; all in/out buffers are caller-owned.
 */
#ifndef ACEZ_H
#define ACEZ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACEZ_OK 0
#define ACEZ_ERR_INVALID (-1)   /* bad argument (null pointer, bad shape, unsupported option)          */
#define ACEZ_ERR_HIP (-2)       /* a HIP runtime call failed; acez_last_error() has the message         */
#define ACEZ_ERR_NODEVICE (-3)  /* no gfx950 device visible                                              */
#define ACEZ_ERR_NAN (-4)       /* NaN loss detected (ace_trainer.py:615-617 aborts here)                */

/* Message of the last error on this thread (never NULL). */
const char* acez_last_error(void);
/* Library version string, e.g. "acez 0.1 (gfx950)". */
const char* acez_version(void);
/* Number of visible HIP devices (0 when there is none; never fails). */
int acez_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * (R) DSAC* registration
 * ---------------------------------------------------------------------------------------------- */

/* Arguments of dsacstar.forward_rgb (dsacstar.cpp:66-78) that are shared by all frames of a batch. */
typedef struct acez_ransac_params {
  int32_t hypotheses;        /* ransacHypotheses    (register_mapping.py:64, 64; ace_zero.py:140, 32)   */
  int32_t max_tries;         /* max_hypotheses_tries (register_mapping.py:67 1e6; ace_zero.py:233, 16)  */
  float inlier_threshold;    /* inlierThreshold, px (register_mapping.py:70, 10)                        */
  float inlier_alpha;        /* inlierAlpha         (register_mapping.py:73, 100)                       */
  float max_reproj;          /* maxReproj, px       (register_mapping.py:76, 100)                       */
  int32_t subsampling;       /* subSampling = network.OUTPUT_SUBSAMPLE = 8 (ace_network.py:159)         */
  int32_t max_ref_steps;     /* MAX_REF_STEPS = 100 (dsacstar.cpp:47); <=0 selects 100                  */
  int32_t reserved;
} acez_ransac_params;

/* Per-frame pinhole intrinsics: focalLength, ppointX, ppointY of dsacstar.cpp:70-72. */
typedef struct acez_intrinsics {
  float focal, ppx, ppy;
} acez_intrinsics;

typedef struct acez_ransac acez_ransac; /* opaque context: stream-ordered workspaces for up to max_frames */

/* Create a registration context able to process batches of up to `max_frames` frames of at most
 * `max_h` x `max_w` scene coordinates (60x80 for 480x640 input). device < 0 selects the current device. */
int acez_ransac_create(acez_ransac** out, int max_frames, int max_h, int max_w, int device);
void acez_ransac_destroy(acez_ransac* ctx);

/* Batched device variant -- scene coordinates never leave HBM.
 *   d_scene_coords  float32 [n_frames][3][h][w], the layout Regressor.forward produces (ace_network.py:265-270)
 *   h_intrinsics    n_frames entries (host)
 *   seed            randomSeed of dsacstar.cpp:77
 *   h_frame_ids     n_frames entries (host) or NULL (= 0..n-1). The random stream is keyed by
 *                   (seed, frame_id, hypothesis, try, draw), see DESIGN.md "RNG"; this replaces the
 *                   call-order dependent ThreadRand (thread_rand.cpp:13-42).
 *   d_out_poses     float32 [n_frames][4][4] row-major cam->world pose (dsacstar.cpp:177-182)
 *   d_out_inliers   int32   [n_frames] return value of forward_rgb (dsacstar.cpp:185)
 *   d_out_masks     uint8   [n_frames][h][w] inlier map that produced the pose, or NULL
 * Asynchronous on `stream`. */
int acez_register_rgb_device(acez_ransac* ctx, const float* d_scene_coords, int n_frames, int h, int w,
                             const acez_ransac_params* params, const acez_intrinsics* h_intrinsics,
                             uint64_t seed, const uint64_t* h_frame_ids, float* d_out_poses,
                             int32_t* d_out_inliers, uint8_t* d_out_masks, void* stream);

/* Host-buffer variant with the exact argument meaning of dsacstar.forward_rgb for ONE frame
 * (what the reference's pybind wrapper would call). Strides are in elements, as an ATen accessor
 * reads them (dsacstar.cpp:83-84). Synchronous. Returns ACEZ_OK and writes *out_inliers. */
int acez_register_rgb_host(acez_ransac* ctx, const float* h_scene_coords, int64_t stride_c,
                           int64_t stride_h, int64_t stride_w, int h, int w,
                           const acez_ransac_params* params, const acez_intrinsics* intr, uint64_t seed,
                           uint64_t frame_id, float* h_out_pose16, int32_t* out_inliers,
                           uint8_t* h_out_mask /* nullable, h*w */);

/* Diagnostics for the parity tests: copies the per-hypothesis results of the LAST device call.
 *   h_hyp_poses  float64 [n_frames][hypotheses][6]  (rvec, tvec) after sampling
 *   h_scores     float64 [n_frames][hypotheses]     soft inlier scores
 *   h_best       int32   [n_frames]                 selected hypothesis
 *   h_refined    float64 [n_frames][6]              (rvec, tvec) after refinement
 * Any pointer may be NULL. Synchronous. */
int acez_ransac_debug_fetch(acez_ransac* ctx, int n_frames, int hypotheses, double* h_hyp_poses,
                            double* h_scores, int32_t* h_best, double* h_refined);

/* RGB backward: the reference's commented-out dsacstar.backward_rgb (dsacstar.cpp:208-490). Samples and scores exactly as
 * acez_register_rgb_device does for the same (seed, frame id), turns the scores into soft-max probabilities, refines every
 * hypothesis with probability >= 0.001 and returns the expected pose loss per frame with its gradient with respect to the scene
 * coordinates: the hypothesis path through the refinement's normal equations, -(J^T J)^+ J^T over the final inliers' reprojection
 * errors (zero for a hypothesis if an entry exceeds 10), and the score path through every pixel's error and, by central
 * differences of P3P (eps 0.001), the hypothesis' minimal set.
 *   d_scene_coords, params, h_intrinsics, seed, h_frame_ids   as in acez_register_rgb_device
 *   d_gt_poses, w_loss_rot, w_loss_trans, soft_clamp, d_out_grad, d_out_loss   as in acez_register_rgbd_backward_device
 * Deterministic. Asynchronous on `stream`. Calls on one context share its workspaces: serialise them (one stream at a time). */
int acez_register_rgb_backward_device(acez_ransac* ctx, const float* d_scene_coords, const float* d_gt_poses, int n_frames, int h,
                                      int w, const acez_ransac_params* params, const acez_intrinsics* h_intrinsics,
                                      float w_loss_rot, float w_loss_trans, float soft_clamp, uint64_t seed,
                                      const uint64_t* h_frame_ids, float* d_out_grad, double* d_out_loss, void* stream);

/* Host-buffer variant for ONE frame: strides in elements; the gradient is added to h_grad with its own strides. Synchronous. */
int acez_register_rgb_backward_host(acez_ransac* ctx, const float* h_scene_coords, int64_t stride_c, int64_t stride_h,
                                    int64_t stride_w, const float* h_gt_pose16, int h, int w, const acez_ransac_params* params,
                                    const acez_intrinsics* intr, float w_loss_rot, float w_loss_trans, float soft_clamp,
                                    uint64_t seed, uint64_t frame_id, float* h_grad, int64_t g_stride_c, int64_t g_stride_h,
                                    int64_t g_stride_w, double* out_loss);

/* Diagnostics of the LAST acez_register_rgb_backward_* call, as acez_ransac_rgbd_backward_debug_fetch except:
 *   h_samples    int32  [n_frames][hypotheses][4]  scan indices x*h+y of the kept minimal set
 *   h_mask_words uint64 [n_frames][hypotheses][ceil(h*w / 256) * 4]  final inliers over ALL cells in scan order (x-outer, y-inner) */
int acez_ransac_rgb_backward_debug_fetch(acez_ransac* ctx, int n_frames, int hypotheses, int h, int w, int32_t* h_samples,
                                         double* h_hyp_poses, double* h_scores, double* h_probs, double* h_losses,
                                         double* h_ref_poses, uint64_t* h_mask_words, double* h_entropy);

/* RGB-D registration: the reference's commented-out dsacstar.forward_rgbd (dsacstar.cpp:493-640). A pose from 3D-3D
 * correspondences (Kabsch on three cells per hypothesis, 3D distance scores, Kabsch refinement on the inliers), no PnP.
 * Same context as the RGB calls; acez_ransac_params keeps its fields with these meanings here:
 *   hypotheses, max_tries, max_ref_steps   as above
 *   inlier_threshold   inlierThreshold in CENTIMETRES (3D distance)
 *   inlier_alpha       inlierAlpha
 *   max_reproj         maxDistError in CENTIMETRES (distance errors are clamped to it)
 *   subsampling        unused
 *   d_scene_coords   float32 [n_frames][3][h][w] scene coordinates, metres (the layout acez_register_rgb_device takes)
 *   d_camera_coords  float32 [n_frames][3][h][w] camera coordinates back-projected from measured depth, metres; a cell is
 *                    valid when its coordinate is finite with z != 0
 *   seed, h_frame_ids  key the random stream as in acez_register_rgb_device
 *   d_out_poses      float32 [n_frames][4][4] row-major cam->world pose (pose2trans)
 *   d_out_inliers    int32   [n_frames] inliers of the last accepted refinement step (0 if none was accepted)
 *   d_out_masks      uint8   [n_frames][h][w] that step's inlier map, or NULL
 * A frame with fewer than 3 valid cells gives the identity pose and 0 inliers. Asynchronous on `stream`. */
int acez_register_rgbd_device(acez_ransac* ctx, const float* d_scene_coords, const float* d_camera_coords, int n_frames,
                              int h, int w, const acez_ransac_params* params, uint64_t seed,
                              const uint64_t* h_frame_ids, float* d_out_poses, int32_t* d_out_inliers,
                              uint8_t* d_out_masks, void* stream);

/* Camera coordinates for acez_register_rgbd_device from measured depth, in ONE launch for all frames: the back-projection of the
 * feature-map cell centres (stride * x + stride / 2, stride * y + stride / 2).
 *   d_depth        float32 [n_frames][h][w] camera z at the cell centres, metres; 0 = no depth
 *   d_focal        float32 [n_frames] each frame's focal length, pixels (device memory)
 *   ppx, ppy       principal point shared by the frames, pixels
 *   d_out_coords   float32 [n_frames][3][h][w]: ((px - ppx) / f * d, (py - ppy) / f * d, d), evaluated in float32 in exactly this
 *                  order (the mapping buffer's formula, so mapping targets and registration agree bit for bit); +0 in all three
 *                  channels where d == 0
 * Asynchronous on `stream`. */
int acez_camera_coordinates(const float* d_depth, const float* d_focal, float ppx, float ppy, int n_frames, int h, int w,
                            int stride, float* d_out_coords, void* stream);

/* Host-buffer variant of dsacstar.forward_rgbd for ONE frame; strides in elements for each tensor. Synchronous. */
int acez_register_rgbd_host(acez_ransac* ctx, const float* h_scene_coords, int64_t sc_stride_c, int64_t sc_stride_h,
                            int64_t sc_stride_w, const float* h_camera_coords, int64_t cc_stride_c,
                            int64_t cc_stride_h, int64_t cc_stride_w, int h, int w,
                            const acez_ransac_params* params, uint64_t seed, uint64_t frame_id,
                            float* h_out_pose16, int32_t* out_inliers, uint8_t* h_out_mask /* nullable, h*w */);

/* Diagnostics of the LAST acez_register_rgbd_* call:
 *   h_samples    int32   [n_frames][hypotheses][3]  map indices y*w+x of the triple each hypothesis was fitted to (-1: none)
 *   h_hyp_poses  float64 [n_frames][hypotheses][6]  (rvec, tvec) after sampling
 *   h_scores     float64 [n_frames][hypotheses]     soft inlier scores
 *   h_best       int32   [n_frames]                 selected hypothesis (the first maximum)
 *   h_refined    float64 [n_frames][6]              (rvec, tvec) after refinement
 * Any pointer may be NULL. Synchronous. */
int acez_ransac_rgbd_debug_fetch(acez_ransac* ctx, int n_frames, int hypotheses, int32_t* h_samples,
                                 double* h_hyp_poses, double* h_scores, int32_t* h_best, double* h_refined);

/* RGB-D backward: the reference's commented-out dsacstar.backward_rgbd (dsacstar.cpp:642-895). Samples and scores exactly as
 * acez_register_rgbd_device does for the same (seed, frame id), turns the scores into soft-max probabilities, refines every
 * hypothesis with probability >= 0.001, and returns the expected pose loss E = sum_h p_h loss_h per frame with its gradient with
 * respect to the scene coordinates (the hypothesis path through the refinement's Kabsch fit plus the score path).
 *   d_scene_coords, d_camera_coords, params, seed, h_frame_ids   as in acez_register_rgbd_device
 *   d_gt_poses       float32 [n_frames][4][4] row-major cam->world ground truth
 *   w_loss_rot, w_loss_trans, soft_clamp   loss = w_rot * angle (degrees) + w_trans * |camera centre error|, softly clamped
 *                    (sqrt(soft_clamp * loss)) above soft_clamp, at most 1e7
 *   d_out_grad       float32 [n_frames][3][h][w]: the gradient is ADDED to it (the reference's +=)
 *   d_out_loss       float64 [n_frames] expected loss
 * Deterministic: the same inputs give the same bits. Asynchronous on `stream`. Calls on one context share its workspaces (the
 * fp64 gradient accumulator among them): serialise them, one stream at a time. */
int acez_register_rgbd_backward_device(acez_ransac* ctx, const float* d_scene_coords, const float* d_camera_coords,
                                       const float* d_gt_poses, int n_frames, int h, int w, const acez_ransac_params* params,
                                       float w_loss_rot, float w_loss_trans, float soft_clamp, uint64_t seed,
                                       const uint64_t* h_frame_ids, float* d_out_grad, double* d_out_loss, void* stream);

/* Host-buffer variant for ONE frame: strides in elements; the gradient is added to h_grad with its own strides. Synchronous. */
int acez_register_rgbd_backward_host(acez_ransac* ctx, const float* h_scene_coords, int64_t sc_stride_c, int64_t sc_stride_h,
                                     int64_t sc_stride_w, const float* h_camera_coords, int64_t cc_stride_c,
                                     int64_t cc_stride_h, int64_t cc_stride_w, const float* h_gt_pose16, int h, int w,
                                     const acez_ransac_params* params, float w_loss_rot, float w_loss_trans, float soft_clamp,
                                     uint64_t seed, uint64_t frame_id, float* h_grad, int64_t g_stride_c, int64_t g_stride_h,
                                     int64_t g_stride_w, double* out_loss);

/* Diagnostics of the LAST acez_register_rgbd_backward_* call (h, w: its frame size):
 *   h_samples, h_hyp_poses, h_scores   as acez_ransac_rgbd_debug_fetch
 *   h_probs      float64 [n_frames][hypotheses]     soft-max probabilities
 *   h_losses     float64 [n_frames][hypotheses]     loss of each (refined) hypothesis
 *   h_ref_poses  float64 [n_frames][hypotheses][6]  (rvec, tvec) after refinement (the sampled pose if p < 0.001)
 *   h_mask_words uint64  [n_frames][hypotheses][ceil(h*w / 512) * 8]  final inlier set over the valid cells in scan order
 *                (x-outer, y-inner): bit j % 64 of word j / 64 is valid cell j; zero if not refined or no step was accepted
 *   h_entropy    float64 [n_frames]                 entropy (bits) of the probabilities
 * Any pointer may be NULL. Synchronous. */
int acez_ransac_rgbd_backward_debug_fetch(acez_ransac* ctx, int n_frames, int hypotheses, int h, int w, int32_t* h_samples,
                                          double* h_hyp_poses, double* h_scores, double* h_probs, double* h_losses,
                                          double* h_ref_poses, uint64_t* h_mask_words, double* h_entropy);

/* ------------------------------------------------------------------------------------------------
 * (T) head training / inference
 * ---------------------------------------------------------------------------------------------- */

#define ACEZ_HEAD_CHANNELS 512 /* ace_network.py:82, hard-coded in the reference too */

/* learning-rate schedules of ace_schedule.py:17-67 */
#define ACEZ_SCHED_CONSTANT 0
#define ACEZ_SCHED_1CYCLEPOLY 1
#define ACEZ_SCHED_CIRCLE 2
/* loss types of ace_loss.py:39-91 */
#define ACEZ_LOSS_TANH 0
#define ACEZ_LOSS_DYNTANH 1
#define ACEZ_LOSS_L1 2
#define ACEZ_LOSS_L1_SQRT 3
#define ACEZ_LOSS_L1_LOGL1 4

typedef struct acez_head_desc {
  int32_t num_head_blocks;   /* train_ace.py:83, default 1 -> 8 layers of 512x512 + fc3                */
  int32_t use_homogeneous;   /* train_ace.py:89, default 1 -> fc3 has 4 outputs                         */
  float mean[3];             /* Head.mean (ace_network.py:118)                                          */
  float max_inv_scale;       /* 1/homogeneous_max_scale = 0.25 (ace_network.py:112)                     */
  float min_inv_scale;       /* 1/homogeneous_min_scale = 100  (ace_network.py:114)                     */
  float h_beta;              /* ln2/(1-max_inv_scale)          (ace_network.py:113)                     */
} acez_head_desc;

typedef struct acez_train_config {
  acez_head_desc head;
  int32_t max_batch;           /* upper bound of rows per step on this rank (train_ace.py:137, 5120)     */
  int32_t global_batch;        /* loss normaliser B (ace_trainer.py:613); = max_batch on one GPU         */
  /* loss (ace_trainer.py:158-166, ace_loss.py) */
  int32_t loss_type;
  float soft_clamp;            /* repro_loss_soft_clamp 50                                               */
  float soft_clamp_min;        /* repro_loss_soft_clamp_min 1                                            */
  int32_t circle_schedule;     /* ace_loss.py:62                                                         */
  float hard_clamp;            /* repro_loss_hard_clamp 1000                                             */
  float depth_min, depth_max, depth_target; /* 0.1, 1000, 10 (train_ace.py:166-176)                      */
  float inlier_px_threshold;   /* learning_rate_cooldown_trigger_px_threshold 10                         */
  /* optimiser + schedule (ace_schedule.py) */
  int32_t schedule;
  int32_t iterations;          /* options.iterations                                                     */
  double lr_min, lr_max;
  int32_t warmup_iterations;   /* 1cyclepoly                                                             */
  double warmup_lr;
  int32_t cooldown_iterations;
  double cooldown_trigger_percent; /* 0.7                                                                */
  double beta1, beta2, eps, weight_decay; /* AdamW defaults 0.9 0.999 1e-8 1e-2                          */
  /* calibration refinement (refine_calibration.py): 0 = off */
  int32_t refine_calibration;
  float focal_init;            /* CalibrationRefiner.focal_length_init                                   */
  double calib_lr;
  /* pose refinement (refine_poses.py): 0 = none, 1 = naive (the 3x4 poses are the parameters, :224-234),
   * 2 = mlp (PoseNetwork(0,128), :152-176) */
  int32_t pose_refinement;
  int32_t pose_refinement_wait;   /* train_ace.py:220                                                     */
  double pose_refinement_lr;      /* train_ace.py:223, 1e-3                                               */
  float pose_refinement_weight;   /* train_ace.py:216, 0.1                                                */
  int32_t pose_refinement_ortho;  /* --refinement_ortho (train_ace.py:226): 0 = gram-schmidt, 1 = procrustes */
  /* 16-bit operand format of the head's GEMMs (features, activations, propagated gradients, weight copies; fp32 accumulation,
   * fp32 geometry / loss / optimiser either way). The reference runs the head under fp16 autocast (train_ace.py --use_half True,
   * ace_trainer.py:330,517-518): ACEZ_DTYPE_FP16 mirrors that (the gradient chain carries a power-of-two scale that the device-side
   * schedule adapts every step, the role torch.cuda.amp.GradScaler plays in ace_schedule.py:70,107-113); ACEZ_DTYPE_BF16 is BASELINE.json's north_star and the default. --use_half False (fp32) is
   * rejected, never silently replaced. d_features of acez_train_buffer / acez_head_forward are in this format. */
  int32_t compute_dtype;
  /* 1: a context for acez_head_forward / acez_head_forward_maps only (Regressor at registration time, register_mapping.py:201-242): no
   * gradient, weight-gradient, partial-sum or second input buffers are allocated (they are 60 % of a whole-frame context's memory) and
   * the training entry points return ACEZ_ERR_INVALID. 0: a trainer (which can also run inference). */
  int32_t inference_only;
} acez_train_config;
#define ACEZ_DTYPE_BF16 0
#define ACEZ_DTYPE_FP16 1
#define ACEZ_DTYPE_FP32 2

/* Caller-owned parameter storage, so the host side can expose the same state_dict keys as
 * ace_network.Head (ace_trainer.py:690-693) as views of one flat tensor.
 * Flat order = Head.named_parameters(): for each 512x512 layer {weight[out][in], bias[out]},
 * then fc3.weight[no][512], fc3.bias[no]  (2 103 300 floats for the default head). */
typedef struct acez_param_buffers {
  float* d_params;  /* fp32 master weights                                   */
  float* d_adam_m;  /* AdamW exp_avg                                         */
  float* d_adam_v;  /* AdamW exp_avg_sq                                      */
  float* d_grad;    /* flat fp32 gradient + 4 trailing stats floats {loss_sum, inlier_count, focal_grad, nan_flag};
                       this is the bucket a data-parallel host all-reduces between
                       acez_train_backward and acez_train_update */
  int64_t n_params; /* must equal acez_head_num_params(head)                 */
  /* pose-refinement network, flat in PoseNetwork.named_parameters() order (head_skip, conv1..3, fc1..3; 70 924
   * floats); only read when cfg.pose_refinement == 2. Its gradient is appended to d_grad after the 4 statistics,
   * so d_grad holds n_params + 4 + n_pose_params floats and one all-reduce still covers everything. */
  float* d_pose_params;
  float* d_pose_m;
  float* d_pose_v;
  int64_t n_pose_params; /* mlp: ACEZ_POSE_MLP_PARAMS; naive: 12 * n_images (d_pose_params = the [n_images][3][4] poses); none: 0 */
} acez_param_buffers;
#define ACEZ_POSE_MLP_PARAMS 70924

/* The training buffer of ace_trainer.py:330-340, with the per-image data stored once per view
 * (image x augmentation pass) instead of once per patch. */
typedef struct acez_train_buffer {
  const void* d_features;      /* bf16 (fp16 with ACEZ_DTYPE_FP16) [n_patches][512]                    */
  const float* d_target_px;    /* f32  [n_patches][2]                                                  */
  const int32_t* d_view_idx;   /* i32  [n_patches]  -> view                                            */
  int64_t n_patches;
  const float* d_view_aug_inv; /* f32 [n_views][3][4]   aug_poses_inv (ace_trainer.py:331)             */
  const float* d_view_K;       /* f32 [n_views][3][3]   intrinsics                                     */
  const float* d_view_Kinv;    /* f32 [n_views][3][3]   intrinsics_inv                                 */
  const int32_t* d_view_image; /* i32 [n_views]  -> image (pose_idx of ace_trainer.py:339)             */
  int32_t n_views;
  const float* d_image_pose_inv; /* f32 [n_images][4][4] world->cam poses_inv (ace_trainer.py:332)      */
  int32_t n_images;
  const float* d_target_crds;  /* f32 [n_patches][3] ground-truth scene coordinates from depth, zeros where none
                                  (ace_trainer.py:338); non-NULL selects the use_depth variant of the step
                                  (ace_trainer.py:567-574,601-609), NULL the constant-depth proxy target */
} acez_train_buffer;

typedef struct acez_train_state {
  int32_t iteration;        /* TrainerACE.iteration                                                    */
  int32_t max_iterations;   /* ScheduleACE.max_iterations (rewritten by the cool-down trigger)         */
  int32_t in_cooldown;
  int32_t nan_flag;
  double lr;                /* lr the NEXT optimiser step will use                                     */
  float last_loss;          /* loss of the last completed step (already / global_batch)                */
  float last_batch_inliers; /* fraction, ace_trainer.py:586                                            */
  double focal_scale;       /* 1 + global_f (refine_calibration.py:28-32)                              */
  float grad_scale;         /* fp16: the power of two on the propagated gradients of the NEXT step (GradScaler's scale); bf16: 1 */
  int32_t opt_steps;        /* AdamW steps applied so far (< iteration when fp16 overflows skipped updates, as GradScaler.step does) */
} acez_train_state;

typedef struct acez_trainer acez_trainer;

int64_t acez_head_num_params(const acez_head_desc* head);
int acez_trainer_create(acez_trainer** out, const acez_train_config* cfg, const acez_param_buffers* params,
                        int device);
void acez_trainer_destroy(acez_trainer* tr);
int acez_trainer_set_buffer(acez_trainer* tr, const acez_train_buffer* buf);
/* Re-derive the bf16 compute copies (W and W^T) from the fp32 master weights; call after loading weights. */
int acez_trainer_sync_weights(acez_trainer* tr, void* stream);

/* One iteration of ace_trainer.py:499-679 on `n` buffer rows selected by d_indices (int64, device),
 * split in two so that a data-parallel host can all-reduce d_grad in between:
 *   backward: schedule bookkeeping, gather, head forward, loss, head backward -> d_grad
 *   update  : AdamW on the fp32 masters, bf16 recast, scheduler step
 * Both are asynchronous and never synchronise the host. A step issued after the schedule has ended
 * (iteration >= max_iterations, ace_trainer.py:509-510) is a device-side no-op. */
int acez_train_backward(acez_trainer* tr, const int64_t* d_indices, int n, void* stream);
int acez_train_update(acez_trainer* tr, void* stream);
/* acez_train_update with the NEXT acez_train_backward's indices announced (a data-parallel rank knows its rows of the next batch: every
 * rank draws the same epoch permutation, ace_trainer.py:466-494): the next batch is gathered, and this step's schedule bookkeeping
 * closed, inside the optimiser's launch, so the next acez_train_backward called with the same device pointer and count starts with the
 * forward chain instead of a gather launch. Same contract for the announced indices as acez_train_step_next; any other next call is
 * still correct. Bitwise the same parameters and state as acez_train_update. With the pose network (--pose_refinement mlp) the rows are
 * gathered in the optimiser's launch as well and the next backward's first launch keeps the pose forward and the schedule wave. With
 * d_indices_next == NULL or n_next == 0 (a rank whose shard holds no row of the next batch): exactly acez_train_update. */
int acez_train_update_next(acez_trainer* tr, const int64_t* d_indices_next, int n_next, void* stream);
/* Sharded data-parallel update (reduce-scatter of the weight gradients, each rank updates its own layers, all-gather
 * of the 16-bit compute copies; no reference counterpart -- the reference is single-GPU):
 *   acez_train_update_layers        AdamW on the weight matrices of wide layers [layer_lo, layer_hi) only (d_grad holds their reduced
 *                                   gradients) and on ALL small parameters (biases, fc3: their gradients are all-reduced, the update is
 *                                   replicated); closes the step's schedule bookkeeping like acez_train_update
 *   acez_trainer_export_weights16   16-bit W[out][in] of layers [layer_lo, layer_hi) -> d_dst  ((hi - lo) x 512 x 512 elements)
 *   acez_trainer_import_weights16   d_src -> the 16-bit W of those layers, and rebuilds their transposed copies
 *   acez_trainer_import_weights16_all  the receiving side of the all-gather in ONE launch: d_src_all = [L][512][512] 16-bit (every rank's
 *                                   layers); all layers OUTSIDE [own_lo, own_hi) are taken over (W and W^T), the rank's own stay as its
 *                                   optimiser wrote them
 * The fp32 masters / moments of layers a rank does not own go stale on it; the host copies the owners' values in before it reads them. */
int acez_train_update_layers(acez_trainer* tr, int layer_lo, int layer_hi, void* stream);
int acez_trainer_export_weights16(acez_trainer* tr, int layer_lo, int layer_hi, void* d_dst, void* stream);
int acez_trainer_import_weights16(acez_trainer* tr, int layer_lo, int layer_hi, const void* d_src, void* stream);
int acez_trainer_import_weights16_all(acez_trainer* tr, int own_lo, int own_hi, const void* d_src_all, void* stream);

/* Single-GPU step = backward + update, with the wide-layer weight gradients handed straight to the optimiser: bitwise the same
 * parameters as the two calls above; afterwards d_grad holds the bias / fc3 gradients and the statistics only (its wide-layer weight
 * part is not written). Without pose refinement, and while the one-launch chains are enabled (acez_trainer_seq_status), the weight-gradient
 * launch applies the whole optimiser step itself (wgrad_opt_kernel: the split-K halves of a tile are exchanged inside one XCD's L2 and
 * never reach memory) and closes the step's schedule; otherwise the slabs go through memory to a separate optimiser launch. That step is
 * two launches: the forward chain, the loss and the input-gradient chain as one (rowstep_kernel), then wgrad_opt_kernel.
 * acez_trainer_set_step_chain(tr, 0) (the Python HeadTrainer calls it at creation when ACEZ_STEP_CHAIN=0 is set), profiling
 * (acez_trainer_set_profiling) and a head whose chains are longer than eight layers keep the two chains in a launch each, the loss inside the second (three launches; ACEZ_LOSS_IN_CHAIN=0: four) -- bitwise the same step, so the flows
 * may alternate. Use backward / all-reduce / update when ranks exchange d_grad. */
int acez_train_step(acez_trainer* tr, const int64_t* d_indices, int n, void* stream);
/* acez_train_step with the NEXT step's indices announced (run_epoch walks consecutive slices of one permutation, ace_trainer.py:466-494,
 * so the caller knows them): the next batch is gathered inside this step's launches (beside the loss kernel, into the second of the
 * trainer's two input buffers; with pose refinement: inside the optimiser launch, with the schedule bookkeeping). The next call must pass the same device pointer and count to profit; a different pointer or count is still correct (the batch
 * is then gathered again). The rows gathered ahead are recognised by (pointer, count) only: the n_next indices at d_indices_next must
 * not be rewritten, nor their memory freed and reused, between this call and the next step call -- acez_trainer_set_buffer and
 * acez_trainer_sync_weights drop the rows gathered ahead. NULL = acez_train_step. */
int acez_train_step_next(acez_trainer* tr, const int64_t* d_indices, int n, const int64_t* d_indices_next, int n_next, void* stream);

/* Training group: h (1..8) independent trainers stepped together (ace_zero.py --seed_parallel_workers: the seed trials side by side).
 * One acez_train_group_step advances every member by exactly one step, bitwise what acez_train_step (or acez_train_step_next with the
 * same announcement) on each member, one after the other, produces; single steps and group steps may be mixed in any order. The two
 * dependent GEMM chains of all members run as one launch each (rowseq_group_kernel: layer l of every member before layer l + 1); every
 * other launch is the member's own. Each member keeps its weights, optimiser and schedule state, buffer and loss settings; state, log and
 * diagnostics are read from the members as before. Members must outlive the group.
 * acez_train_group_create returns ACEZ_ERR_INVALID (and creates nothing) for: h outside [1, 8], a member listed twice, members on
 * different devices or with different compute_dtype / num_head_blocks / use_homogeneous, a member with pose_refinement,
 * refine_calibration or inference_only.
 * acez_train_group_step: d_indices[i] / n[i] as acez_train_step for member i; d_next[i] / n_next[i] as acez_train_step_next (d_next ==
 * NULL or d_next[i] == NULL: no announcement for that member). Arguments are checked before anything is launched. */
typedef struct acez_train_group acez_train_group;
int acez_train_group_create(acez_train_group** out, acez_trainer* const* members, int h);
void acez_train_group_destroy(acez_train_group* g);
int acez_train_group_step(acez_train_group* g, const int64_t* const* d_indices, const int32_t* n, const int64_t* const* d_next,
                          const int32_t* n_next, void* stream);

/* Synchronises `stream` and copies the schedule state. */
int acez_trainer_get_state(acez_trainer* tr, acez_train_state* h_out, void* stream);
/* Per-iteration log kept on the device: loss and batch_inliers of iterations [first, first+count). */
int acez_trainer_get_log(acez_trainer* tr, int first, int count, float* h_loss, float* h_inliers, void* stream);
/* Scene coordinates predicted in the last backward call: f32 [n][3] (diagnostics / tests). */
int acez_trainer_last_scene_coords(acez_trainer* tr, float* h_xyz, int n, void* stream);

/* Diagnostics for the roofline measurement (bench.py): bracket every kernel launch of the following steps with HIP
 * events on the launch stream; get_profile synchronises and returns summed milliseconds and launch counts for the
 * 8 kernel classes {sched, gather, gemm_fwd, loss, gemm_dgrad, wgrad, grad_reduce, adamw}, then clears the record. */
int acez_trainer_set_profiling(acez_trainer* tr, int enable);
int acez_trainer_get_profile(acez_trainer* tr, float* h_ms8, int32_t* h_counts8);

/* Status of the one-launch GEMM chains (rowseq_kernel): *enabled = 1 while the trainer uses them, *probe = result
 * of the placement probe run by acez_trainer_create (1 passed, 0 failed -> per-layer launches from the start, -1 not run), *faults =
 * number of times a bounded hand-off poll expired and the trainer fell back to per-layer launches (acez_trainer_get_state performs the
 * fall-back; the abandoned iterations are device-side no-ops and are not counted in acez_train_state.iteration). No reference
 * counterpart. Any pointer may be NULL.
 * A step is atomic under either kind of fault (ace_trainer.py:620-640): a poll that expires inside one of the GEMM chains abandons the
 * step before anything of it is applied (state = the step before); a poll that expires in the fused weight-gradient / optimiser launch
 * (wgrad_opt_kernel) is FINISHED by the same fall-back -- the launches issued after it were no-ops, the step's operands are intact, the
 * rows that were not updated are updated with that step's optimiser scalars -- so that the state is exactly the step after, bit for bit
 * what acez_train_backward + acez_train_update would have produced. */
int acez_trainer_seq_status(acez_trainer* tr, int* enabled, int* probe, int* faults);
/* The merged chain launch of the plain fused step (acez_train_step): *enabled = 1 while such a step would take it (profiling off),
 * *steps = steps that have run through it. Any pointer may be NULL. */
int acez_trainer_step_chain_status(acez_trainer* tr, int* enabled, long long* steps);
int acez_trainer_set_step_chain(acez_trainer* tr, int enable);   /* default 1; may be changed between any two steps */

/* Diagnostics for the tests: copy one intermediate device buffer of the last backward call to the host (synchronous).
 * kind 0: post-ReLU output of wide layer `index`, bf16 [n][512];  1: dZ of layer `index`, bf16 [n][512];
 * 2: residual stream `index` (0 = the gathered batch), bf16 [n][512];  3: weight-gradient slab `index`, f32 [n_wide];
 * 4: bias-gradient partial rows of layer `index`, f32 [max_batch/32][512];  5: s_memtime stamps of the chain kernel
 * (ACEZ_CHAIN_TRACE=1), u64 [2][256];  6: XCD placement record of the one-launch GEMM chains (ACEZ_SEQ_XCC=1), u32 [8 + 256]:
 * words 0..7 = OR of 1 << XCC_ID over the workgroups with blockIdx & 7 = word, word 8 + 4 mt + nt = XCC_ID that ran tile
 * (mt, nt) in the last launch;  10: the hand-off state of the one-launch chains, u32 [64][32] progress words (word 8 nt + w of row
 * tile mt's line: the last seam wave w of column tile nt has completed) + [32] the line of the sticky fault word (word 0) + [64] the
 * host's seam bases per row tile; `bytes` must be exactly (64 * 32 + 32 + 64) * 4;  11: the loss kernel's fc3 partials, f32
 * [16-row blocks][(513 no + 3) & ~3] (per block: no weight rows of 512, then no bias sums);  12: its statistics partials, f32
 * [16-row blocks][4] (loss, inliers, focal gradient, unused);  13: the 16-bit compute copy of the fc3 weights, [no][512];  with pose
 * refinement, 14: the loss kernel's per-row pose gradients, f32 [n][12];  15: the image of each row, i32 [n];  16: the refined poses
 * the loss read, f32 [n_images][16]  (`index` must be 0 for 11 - 16).  No reference counterpart (autograd internals). */
int acez_trainer_debug_read(acez_trainer* tr, int kind, int index, void* h_out, int64_t bytes, void* stream);

/* Current refined world->cam poses of all images, f32 [n_images][3][4] (PoseRefiner.get_all_current_poses,
 * refine_poses.py:184-210); the original poses when pose refinement is off. Synchronous. */
int acez_trainer_get_poses(acez_trainer* tr, float* h_poses34, void* stream);

/* Head inference (Regressor.get_scene_coordinates, ace_network.py:262-263) on n feature rows:
 *   d_features bf16 [n][512]  ->  d_out_xyz f32 [n][3].
 * Asynchronous for passes of more than 5120 rows per max_batch chunk. A pass small enough for the one-launch chains (<= 5120 rows) ends
 * with a read of the trainer's fault word, i.e. it SYNCHRONISES `stream` before it returns: an expired hand-off poll would have left
 * garbage in d_out_xyz, and the call repeats the pass on per-layer launches in that case (it also performs a pending training
 * fall-back, see acez_trainer_seq_status). */
int acez_head_forward(acez_trainer* tr, const void* d_features, int n, float* d_out_xyz, void* stream);

/* Head.forward for whole frames, written as Regressor.forward's [B,3,H,W] maps (ace_network.py:265-270): the input of
 * acez_register_rgb_device, so that scene coordinates go encoder -> head -> RANSAC without leaving HBM
 * (register_mapping.py:209-213 copies them to the CPU instead).
 *   d_features  16-bit [n_frames * h * w][512] in the trainer's compute_dtype (bfloat16 or float16), rows in (frame, y, x) order
 *               (acez_encoder_forward's output for an encoder of the same compute_dtype)
 *   d_out_maps  float32  [n_frames][3][h][w] */
int acez_head_forward_maps(acez_trainer* tr, const void* d_features, int n_frames, int h, int w, float* d_out_maps,
                           void* stream);

/* =====================================================================================================
 * E. Feature encoder: ace_network.py:14-59 Encoder.forward
 *    11 convolutions, two residual blocks, output stride 8 (Regressor.OUTPUT_SUBSAMPLE, ace_network.py:159).
 * ===================================================================================================== */
#define ACEZ_ENCODER_LAYERS 11
/* Layer order of the weight/bias pointer arrays == Encoder.__init__ (ace_network.py:26-40):
 *   conv1 conv2 conv3 conv4 res1_conv1 res1_conv2 res1_conv3 res2_conv1 res2_conv2 res2_conv3 res2_skip */

typedef struct acez_encoder acez_encoder; /* opaque: 16-bit weight matrices + activation workspaces for max_frames frames */

/* h_weights[i]  float32 host pointer, torch Conv2d layout [c_out][c_in][k][k] (state_dict "<name>.weight")
 * h_biases[i]   float32 host pointer [c_out]                                   (state_dict "<name>.bias")
 * out_channels  Encoder(out_channels): c_out of res2_conv3 and res2_skip (512 in every shipped encoder)
 * max_frames / max_h / max_w   capacity of one internal pass; acez_encoder_forward chunks larger batches.
 * compute_dtype ACEZ_DTYPE_BF16 or ACEZ_DTYPE_FP16: the 16-bit format of the weights, of every activation and of the feature rows.
 *               The reference runs this network under fp16 autocast (ace_trainer.py:366-367 buffer creation, register_mapping.py:209-210
 *               registration; ace_network.py:41-59): ACEZ_DTYPE_FP16 is that arithmetic (fp16 operands, fp32 accumulation, one rounding
 *               per layer output). Must equal the compute_dtype of the head that consumes the rows. */
int acez_encoder_create(acez_encoder** out, const float* const* h_weights, const float* const* h_biases,
                        int out_channels, int max_frames, int max_h, int max_w, int compute_dtype, int device);
void acez_encoder_destroy(acez_encoder* enc);

/* Spatial size of the feature map for an h x w input: three stride-2, pad-1, 3x3 convolutions. */
int acez_encoder_output_size(int h, int w, int* out_h, int* out_w);

/* Encoder.forward (ace_network.py:42-59) for n_frames grayscale frames.
 *   d_images    float32 [n_frames][1][h][w], normalised as dataset.py:150-153 does
 *   d_features  16-bit (the context's compute_dtype) [n_frames * out_h * out_w][out_channels]: one row per feature-map pixel in
 *               (frame, y, x) order -- the row layout of acez_train_buffer.d_features and of acez_head_forward's input
 * 16-bit operands, fp32 accumulation (the reference runs this network under fp16 autocast, register_mapping.py:209).
 * Asynchronous on `stream`. */
int acez_encoder_forward(acez_encoder* enc, const float* d_images, int n_frames, int h, int w, void* d_features,
                         void* stream);

/* Training-buffer sampling for a batch of views whose features were just computed (ace_trainer.py:404-431): per view,
 * `samples_per_view` rows are drawn uniformly with replacement among the pixels whose mask byte is non-zero
 * (torch.multinomial(mask, n, replacement=True), ace_trainer.py:419-422) and written, view after view, to the output
 * arrays -- which are slices of acez_train_buffer's d_features / d_target_px / d_view_idx at the current fill offset.
 *   d_view_features  16-bit [n_views * map_h * map_w][channels]   (acez_encoder_forward's output; rows are copied, not interpreted)
 *   d_masks          uint8 [n_views][map_h][map_w] validity at feature resolution (the nearest-neighbour resize of
 *                    ace_trainer.py:373-374), or NULL = every pixel valid. Every view must have a valid pixel
 *                    (the reference skips empty views, ace_trainer.py:377-378; so must the caller).
 *   seed, first_view_id   the draw of sample s of view v is a counter-based stream keyed by (seed, first_view_id + v, s)
 *   view_index_base  value written to d_out_view_idx for view 0 (index into the caller's per-view tables)
 *   d_out_features   16-bit [n_views * samples_per_view][channels]
 *   d_out_target_px  float32  [n_views * samples_per_view][2] = 8 * (x + 0.5, y + 0.5)   (ace_util.py:7-13)
 *   d_out_view_idx   int32    [n_views * samples_per_view]
 *   d_out_pixel      int32    [n_views * samples_per_view] chosen feature-map pixel y * map_w + x, or NULL (diagnostics)
 * Asynchronous on `stream`. */
int acez_buffer_sample_views(const void* d_view_features, const uint8_t* d_masks, int n_views, int map_h, int map_w,
                             int channels, int samples_per_view, uint64_t seed, uint64_t first_view_id,
                             int32_t view_index_base, void* d_out_features, float* d_out_target_px,
                             int32_t* d_out_view_idx, int32_t* d_out_pixel, void* stream);

/* acez_buffer_sample_views for views of any sizes in ONE launch, read in place from a resident feature store (no gathered copy of
 * the mapped frames' feature maps). For each view the draws, rows and outputs equal those of acez_buffer_sample_views with the same
 * seed, first_view_id and view index, bit for bit.
 *   d_features       16-bit [n_feature_rows][channels]: the store (e.g. every resident frame's map, one after the other)
 *   d_masks          uint8 validity bytes of the views (layout as in acez_buffer_sample_views, per view), or NULL
 *   mask_bytes       size of d_masks in bytes (ignored without masks)
 *   d_view_table     int64 [n_views][4] on the device: (first feature row, map_h, map_w, byte offset of the mask in d_masks or -1 = every
 *                    pixel valid). Every view must fit max_hw, the store and the masks; one that does not is skipped (its output rows are
 *                    left as they were) rather than read out of bounds.
 *   max_hw           largest map_h * map_w in the table, at most 24576 (checked here, without reading the table)
 *   other arguments  as acez_buffer_sample_views; view v's samples go to output rows v * samples_per_view + s.
 * Asynchronous on `stream`; no host synchronisation. */
int acez_buffer_sample_views_table(const void* d_features, int64_t n_feature_rows, const uint8_t* d_masks, int64_t mask_bytes,
                                   const int64_t* d_view_table, int n_views, int max_hw, int channels, int samples_per_view,
                                   uint64_t seed, uint64_t first_view_id, int32_t view_index_base, void* d_out_features,
                                   float* d_out_target_px, int32_t* d_out_view_idx, int32_t* d_out_pixel, void* stream);

/* Augmented training views of resident frames (dataset.py:283-343: resize by a common factor, rotate about the centre, ColorJitter
 * brightness / contrast on the grey values, a validity mask that goes through the same warp with zero padding), the step in front of the
 * encoder when ace_trainer.py:293-452 fills the buffer with --use_aug True. Up to three launches per batch of views of one canvas size
 * (the warp; + a per-view reduction when jitter is on; + the mask when one is asked for) instead of a dozen framework kernels and a 157 MB sampling grid per 64 views.
 *   d_images      float32 [n_images][H][W] normalised grey frames, resident on the device
 *   d_image_index int32 [n_views]: the frame each view is taken from
 *   d_theta       float32 [n_views][6]: the affine map of torch.nn.functional.affine_grid(align_corners=False) -- normalised output
 *                 coordinates (x_n, y_n, 1) -> normalised source coordinates -- row-major 2 x 3
 *   d_jitter      float32 [n_views][2] = (brightness, contrast) factors applied as torchvision's ColorJitter does on (v * 0.25 + 0.4)
 *                 clamped to [0, 1] (dataset.py:148), or NULL
 *   d_out_views   float32 [n_views][hs][ws]: bilinear, reflection padding (F.grid_sample(..., padding_mode="reflection", align_corners=False))
 *   d_out_mask    uint8 [n_views][map_h][map_w] or NULL: the zero-padded bilinear warp of an all-ones image, > 0, taken at the pixels the
 *                 nearest-neighbour resize to feature resolution reads (ace_trainer.py:373-374): what acez_buffer_sample_views expects
 *   d_scratch     float32 [n_views] (the per-view mean of the brightness-adjusted frame; used only with d_jitter)
 * Asynchronous on `stream`. */
int acez_buffer_warp_views(const float* d_images, int n_images, int H, int W, const int32_t* d_image_index, const float* d_theta,
                           const float* d_jitter, int n_views, int hs, int ws, float* d_out_views, uint8_t* d_out_mask, int map_h,
                           int map_w, float* d_scratch, void* stream);

/* =====================================================================================================
 * F. Point-cloud extraction
 * =====================================================================================================
 * Replaces the per-frame body of ace_vis_util.get_point_cloud_from_network (ace_vis_util.py:430-591; callers
 * export_point_cloud.py:87-94, ace_zero.py:379-400) from the point where the scene-coordinate maps of a batch of frames
 * exist on the device (acez_head_forward_maps' output): reprojection error against the pixel grid (:481-499),
 * scene-coordinate gradient with reflect padding (:501-510), the escalating gradient thresholds 0.1 / 0.5 / 1 / inf
 * (:443,512-516), depth filter and "keep all if nothing survives" (:518-526), reprojection threshold of 1 px (:451,528-530)
 * with the relaxed k-th-error branch (:535-544) and the random sub-sampling branch (:545-551), and the merge into one
 * point list in frame order with the OpenCV -> OpenGL flip (:574-587).  `torch.randperm`'s stream is replaced by a
 * counter-based draw keyed by (seed, first_frame_id + frame, rank of the surviving point); everything else is bit-exact
 * against the restatement in oracle/cloud_oracle.py, which is pinned on the reference function's own output.
 *   d_scene_coords        float32 [n_frames][3][map_h][map_w]
 *   d_poses_inv           float32 [n_frames][12]: rows of the 3x4 world -> camera transform (gt_inv_pose[:, :3], :479)
 *   d_intrinsics          float32 [n_frames][9]: row-major K
 *   filter_depth          metres (export_point_cloud.py:94 passes 100); dense_cloud as ace_vis_util.py:453-456
 *   points_per_image_min  int(100000 / len(data_loader)), points_per_image_max  int(1000000 / len(data_loader)) (:458-459)
 *   opengl_convention     non-zero: y and z negated as the reference returns them
 *   d_keep                uint8 [n_frames][map_h * map_w]   out: 1 = the pixel's point is part of the cloud
 *   d_counts              int32 [n_frames]                  out: points kept per frame
 *   d_offsets             int32 [n_frames + 1]              out: exclusive prefix of d_counts; [n_frames] = total N
 *   d_out_xyz             float32 [n_frames * map_h * map_w][3], first N rows written, frame after frame, pixel order
 *   d_out_source          int32 [same], frame * map_h * map_w + pixel of every point (colour lookup), or NULL
 * Asynchronous on `stream`. */
int acez_point_cloud_filter(const float* d_scene_coords, const float* d_poses_inv, const float* d_intrinsics, int n_frames,
                            int map_h, int map_w, float filter_depth, int dense_cloud, int points_per_image_min,
                            int points_per_image_max, uint64_t seed, uint64_t first_frame_id, int opengl_convention,
                            uint8_t* d_keep, int32_t* d_counts, int32_t* d_offsets, float* d_out_xyz, int32_t* d_out_source,
                            void* stream);

/* =====================================================================================================
 * G. Pose evaluation against ground truth (eval_poses.py, eval_poses_util.py of the reference)
 * =====================================================================================================
 * estimate_alignment (eval_poses_util.py:70-180) and the per-frame errors of eval_poses.py:140-170 in fp64 on the device:
 * RANSAC over similarity transforms fitted to three camera centres (Kabsch, eval_poses_util.py:20-45), the inlier test of
 * get_inliers (translation in the aligned frame AND rotation angle), stable top-k shortlist, refinement on the inlier sets,
 * then t_err = |(T G).t - E.t| / scale and r_err = angle(R_est (T G)_R^T) in degrees for every frame.  Host pointers in and
 * out; one synchronisation per call.  DESIGN.md section 4d lists the declared deviations from the reference.
 * Without a device acez_align_create returns ACEZ_ERR_NODEVICE; there is no CPU path. */
typedef struct acez_align acez_align;

typedef struct {
  double threshold_t;              /* metres: inlier test and accuracy (--pose_error_thresh_t, 0.05)            */
  double threshold_r;              /* degrees: inlier test and accuracy (--pose_error_thresh_r, 5)             */
  double confidence_threshold;     /* frames with confidence strictly above it (and finite GT) take part        */
  int32_t estimate_alignment;      /* 0: T = I, scale = 1 (--estimate_alignment False)                         */
  int32_t estimate_scale;          /* similarity (1) or rigid (0) Kabsch                                        */
  int32_t min_confident_estimates; /* fewer confident frames: status "failed" (10)                             */
  int32_t ransac_iterations;       /* hypotheses H, <= max_hyp (10000)                                          */
  int32_t refinement_max_hyp;      /* shortlist length, 1..64 (12)                                              */
  int32_t refinement_max_it;       /* refinement iterations per shortlisted hypothesis (8)                     */
  uint64_t seed;                   /* key of the counter-based sample stream (unused with a sample table)       */
} acez_align_params;

int acez_align_create(acez_align** out, int max_frames, int max_hyp, int device);
void acez_align_destroy(acez_align* ctx);

/* gt_c2w, est_c2w  double [n_frames][4][4] cam -> world; confidence double [n_frames]
 * samples          int32 [ransac_iterations][3] indices into the confident frames (in frame order), or NULL: own stream
 * out_T            double [16] row-major alignment (zeros if failed); out_scale (1 if failed); out_status 0 ok, 1 failed
 * out_scores       int32 [ransac_iterations] inlier count per hypothesis, out_valid int32 [same] 1 if its sample passed
 *                  the sample test; both optional (NULL), all zero when RANSAC did not run
 * out_t_err        double [n_frames] metres; out_r_err double [n_frames] degrees (inf if failed, NaN for non-finite GT)
 * out_accurate     frames with r_err < threshold_r and t_err < threshold_t */
int acez_align_evaluate(acez_align* ctx, const double* gt_c2w, const double* est_c2w, const double* confidence, int n_frames,
                        const acez_align_params* params, const int32_t* samples, double* out_T, double* out_scale,
                        int32_t* out_status, int32_t* out_scores, int32_t* out_valid, double* out_t_err, double* out_r_err,
                        int32_t* out_accurate);

/* =====================================================================================================
 * H. Rendering the reconstruction video (ace_visualizer.py's pyrender passes, headless)
 * =====================================================================================================
 * One frame of two layers on `stream`, written to a device uint8 image:
 *   points     d_xyz float32 [n_points][3] (world, OpenGL convention), d_rgb uint8 [n_points][3]; each point is a 2 x 2 px square
 *              (the reference's point_size = 2: the 2 x 2 pixels whose centres are nearest to the projection) with a depth test;
 *              nearest wins, equal depths go to the lower index. Points with depth outside [znear, zfar] are dropped. Background black.
 *   triangles  d_tri_xyz float32 [n_tris][3 vertices][3], d_tri_rgba uint8 [n_tris][4]; flat colour, both windings, a depth test
 *              among themselves only (no test against the points), top-left fill rule on vertices snapped to 1/256 px. Triangles
 *              that cross the near plane are CLIPPED against it in camera space (the clipped quad is drawn as a fan of two);
 *              per pixel, depths beyond zfar are dropped; a triangle with a projected vertex 2^21 px or more off the centre is dropped.
 *              The covered pixels are blended on top of the points as ace_visualizer._blend_images does it: in double,
 *              rgb * (a / 255) + background * (1 - a / 255), truncated to uint8.
 *   camera     cam_to_world double [16] row-major, rigid, OpenGL convention (looks down -z); pinhole with yfov = pi/3, square
 *              pixels, principal point at the frame centre (pyrender.PerspectiveCamera(yfov=pi/3, aspectRatio=W/H)).
 *   width, height   render size (1280 x 720 by default); flipped_portrait != 0: the render (e.g. 720 x 1280) is rotated by -90 degrees,
 *              so d_frame is [width][height][3] instead of [height][width][3].
 *   d_work     uint64 [2 * width * height] scratch (the two per-pixel key planes), owned by the caller.
 * Asynchronous on `stream`; nothing is allocated. */
int acez_render_frame(const float* d_xyz, const uint8_t* d_rgb, int64_t n_points, const float* d_tri_xyz, const uint8_t* d_tri_rgba,
                      int64_t n_tris, const double* cam_to_world, float znear, float zfar, int width, int height, int flipped_portrait,
                      unsigned long long* d_work, uint8_t* d_frame, void* stream);
/* Textured triangles (the image thumbnails inside the registration frustums, ace_vis_util.get_image_box). A texture is a uint8
 * [h][w][3] RGB image (row 0 at the top) followed by its mip chain in one device block built by acez_render_texture_build: level
 * k + 1 is max(1, w_k / 2) x max(1, h_k / 2) (integer halving), level k starts right after level k - 1, and each texel of level k + 1
 * is (a + b + c + d + 2) >> 2 per channel over the 2 x 2 block at (2x, 2y) of level k, the block's second column / row clamped to the
 * level's last one (only a level 1 texel wide or high needs it). */
#define ACEZ_RENDER_MAX_TEX_TRIANGLES 32
#define ACEZ_RENDER_MAX_TEXTURES 16
typedef struct acez_tex_triangle {
  float xyz[3][3];        /* world vertices (OpenGL convention), like a row of d_tri_xyz */
  float uv[3][2];         /* per-vertex (u, v): u across the image's columns (0 = left edge, 1 = right edge), v down its rows (0 = top) */
  int32_t texture;        /* index into the texture table */
  int32_t reserved;       /* 0 */
} acez_tex_triangle;
typedef struct acez_texture {
  int64_t offset;         /* byte offset of level 0 in d_texels */
  int32_t width, height;  /* level 0 size */
} acez_texture;
/* Levels and bytes of the chain of a width x height texture (host only): levels = 1 + floor(log2(max(width, height))). */
int acez_render_texture_size(int width, int height, int* out_levels, int64_t* out_bytes);
/* The chain of a device uint8 [height][width][3] image into d_chain (chain_bytes >= acez_render_texture_size's bytes): level 0 is a
 * copy of the image, then one launch per level. Asynchronous on `stream`. */
int acez_render_texture_build(const uint8_t* d_image, int width, int height, uint8_t* d_chain, int64_t chain_bytes, void* stream);
/* acez_render_frame with up to ACEZ_RENDER_MAX_TEX_TRIANGLES textured triangles (host array; they travel to the kernels as launch
 * arguments, so every index is checked here before anything is launched) over up to ACEZ_RENDER_MAX_TEXTURES textures (host table,
 * each chain wholly inside d_texels[0, texel_bytes)). Textured triangle t takes triangle id n_tris + t in the SAME key plane as the
 * flat ones: it is clipped, snapped and filled by the same rules and depth-tests against them. A pixel it wins takes the texel colour
 * (opaque: alpha 255) instead of the point colour:
 *   uv        perspective-correct at the pixel centre: the pixel's ray meets the triangle's plane in camera space; barycentrics from
 *             the three triple products with the unclipped vertices (independent of near-plane clipping);
 *   lod       rho^2 = max(|d(s,t)/dx|^2, |d(s,t)/dy|^2) from the analytic screen-space derivatives of (s, t) = (u w, v h) in level-0
 *             texels; lambda = log2(rho^2) / 2 with log2(m 2^e) ~ e + (m - 1) for m in [1, 2) (exact in float: the exponent and the
 *             mantissa bits). lambda <= 0 (rho^2 <= 1): level 0; otherwise levels floor(lambda) and floor(lambda) + 1 mixed by the
 *             fraction (GL's LINEAR_MIPMAP_LINEAR), the last level alone from there on, and for a rho^2 that is not finite;
 *   filter    bilinear per level about texel centres (s - 1/2, t - 1/2), clamp to edge; the mixed float colour + 1/2 truncated.
 * Every float operation is the one tests/render_texture_oracle.py restates. n_tex_tris == 0 gives acez_render_frame's frame. */
int acez_render_frame_tex(const float* d_xyz, const uint8_t* d_rgb, int64_t n_points, const float* d_tri_xyz, const uint8_t* d_tri_rgba,
                          int64_t n_tris, const acez_tex_triangle* tex_tris, int n_tex_tris, const acez_texture* textures, int n_textures,
                          const uint8_t* d_texels, int64_t texel_bytes, const double* cam_to_world, float znear, float zfar, int width,
                          int height, int flipped_portrait, unsigned long long* d_work, uint8_t* d_frame, void* stream);
/* Exported for the CPU tests (tests/test_render_cpu.py checks the camera set-up against tests/render_oracle.py without a GPU); the
 * product calls it only through acez_render_frame. The camera acez_render_frame projects with (host only, no device needed): out_w2c12 float32 [3][4] = [R^T | -R^T t] of the rigid
 * cam_to_world, computed in double and rounded once; out_focal = (height / 2) * sqrt(3) in pixels. Same argument checks. */
int acez_render_camera(const double* cam_to_world, float znear, float zfar, int width, int height, float* out_w2c12, float* out_focal);

/* =====================================================================================================
 * I. Image ingest (the reference's per-frame image path, dataset.py:189-195,227-237,146-160,293)
 * =====================================================================================================
 * Decoded uint8 RGB frames -> what Pillow's 8-bit resize(BILINEAR), convert("L") and the host's normalisation give, bit for bit:
 *   resize      separable, horizontal pass first, its result kept as uint8. For output index xx of an axis of `in` -> `out` samples:
 *               scale = in / out, fs = max(scale, 1), support = fs, center = (xx + 0.5) * scale, xmin = max(int(center - support
 *               + 0.5), 0), xmax = min(int(center + support + 0.5), in); the tap at source index xmin + x is tri((x + xmin - center
 *               + 0.5) / fs) with tri(v) = max(0, 1 - |v|); the taps are summed in order in double, each divided by the sum and fixed
 *               to int(0.5 + k * 2^22); a pass computes (2^21 + sum pixel * k) >> 22 clipped to 0 .. 255;
 *   grey        L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16;
 *   normalise   d_norm[L]: a float32 table of 256 entries the caller builds (the host path's own expression applied to 0 .. 255), so
 *               the device does no float arithmetic.
 * acez_ingest_coeffs: the table of one axis (host only, no device needed; the CPU tests check it against a restatement, and callers
 * size d_tables with its ksize). out_ksize = ceil(support) * 2 + 1; out_bounds int32 [out][2] = (xmin, tap count); out_taps int32
 * [out][ksize], zero past the tap count. out_bounds / out_taps may be NULL (ksize only). Tables are cached per (in, out) pair. */
int acez_ingest_coeffs(int in_size, int out_size, int* out_ksize, int32_t* out_bounds, int32_t* out_taps);
/* n frames of one source size in two launches on `stream` (horizontal: d_src -> d_tmp; vertical + grey + table: -> outputs), after
 * the two axes' tables have been copied into d_tables on the same stream. Asynchronous; nothing is allocated; every pointer is owned
 * by the caller:
 *   d_src       uint8 [n][H][W][3]
 *   d_tmp       uint8 [n][H][nw][3] scratch
 *   d_tables    int32 scratch of table_bytes >= 4 * (nw * (2 + ksize_x) + nh * (2 + ksize_y)) bytes, ksize_x / ksize_y from
 *               acez_ingest_coeffs(W, nw) / (H, nh). Calls that share it must share the stream.
 *   d_norm      float32 [256]
 *   d_out_rgb   uint8 [n][nh][nw][3], or NULL
 *   d_out_grey  float32 [n][1][nh][nw]
 * ACEZ_ERR_INVALID, before anything is launched, for: a null pointer (other than d_out_rgb), n outside 1 .. 65535, a side outside
 * 1 .. 32768, a resized frame of more than 16384 scene coordinates (what the registration kernel takes), a table block too small. */
int acez_ingest_frames(const uint8_t* d_src, int n, int H, int W, int nh, int nw, uint8_t* d_tmp, int32_t* d_tables, int64_t table_bytes,
                       const float* d_norm, uint8_t* d_out_rgb, float* d_out_grey, void* stream);

/* =====================================================================================================
 * J. Reprojection score of held-out views (benchmark_poses.py --method reproject)
 * =====================================================================================================
 * M coloured points seen from T views on a grid of oh x ow cells (a cell = an 8 x 8 px block of the network's input frame):
 *   d_xyz      float32 [n_points][3] world coordinates (OpenCV convention), d_rgb uint8 [n_points][3]; n_points <= 2^24
 *   d_views    float32 [n_views][15]: the 3 x 4 world -> camera rows (OpenCV camera: looks down +z), focal, cx, cy in CELL units
 *              (pixels / 8)
 *   d_targets  uint8 [n_views][oh][ow][3]: the held-out frames' cell means (the function below)
 *   projection xc = m0 x + m1 y + m2 z + m3 (left to right; yc, zc alike), dropped unless zc >= 0.1; iz = 1 / zc;
 *              u = cx + (f xc) iz, v = cy + (f yc) iz, dropped unless 0 <= u < ow and 0 <= v < oh; cell (floor v, floor u). All fp32,
 *              round to nearest, no contraction
 *   nearest    per cell the smallest (bits of zc << 32 | point index): the nearest point, at equal depth the lower index
 *   accumulate a point adds its R, G, B and 1 to its cell's 32-bit sums if zc <= zmin * b, b = float(1.0 + double(depth_band))
 *   score      per cell with count > 0: colour = (sum + count / 2) / count (integers); d_out_sse[view] += the three squared
 *              differences to the target, d_out_covered[view] += 1; d_out_image uint8 [n_views][oh][ow][3] (0 where nothing landed)
 *              and d_out_mask uint8 [n_views][oh][ow] (1 = covered) are optional (NULL)
 * The outputs depend on no ordering of the atomics. Asynchronous on `stream`; nothing is allocated: d_scratch (8-byte aligned) holds
 * at least acez_reproject_scratch_size's bytes (host only, no device needed). ACEZ_ERR_INVALID before anything is launched for: a null
 * pointer (other than the two optional ones), n_views outside 1 .. 65535, oh or ow outside 1 .. 4096, n_points outside 0 .. 2^24,
 * depth_band outside 0 .. 1, a scratch block too small. tests/reproject_restated.py restates every operation in numpy. */
int acez_reproject_scratch_size(int n_views, int oh, int ow, int64_t* out_bytes);
int acez_reproject_score(const float* d_xyz, const uint8_t* d_rgb, int64_t n_points, const float* d_views, int n_views, int oh, int ow,
                         const uint8_t* d_targets, float depth_band, void* d_scratch, int64_t scratch_bytes, int64_t* d_out_sse,
                         int32_t* d_out_covered, uint8_t* d_out_image, uint8_t* d_out_mask, void* stream);
/* Cell means: d_frames uint8 [n_frames][H][W][3] -> d_out uint8 [n_frames][ceil(H/8)][ceil(W/8)][3], per channel the mean over the
 * cell's pixels, (sum + count / 2) / count in integers (half up); a cell cut by the frame's edge averages the pixels it has. */
int acez_reproject_cell_means(const uint8_t* d_frames, int n_frames, int H, int W, uint8_t* d_out, void* stream);

/* =====================================================================================================
 * K. TSDF fusion of depth maps along the estimated poses, and the surface as a mesh (fuse_depth.py)
 * =====================================================================================================
 * The volume has nx x ny x nz voxels, x fastest: voxel (i, j, k) is element (k * ny + j) * nx + i of
 *   d_tsdf    float32 [nz][ny][nx]     truncated signed distance in units of the truncation, <= 1, positive in free space
 *   d_weight  float32 [nz][ny][nx]     number of observations, capped; 0 = never observed (the tsdf value is then not read by the
 *                                      extraction; the integration reads it, so it must be finite: the caller clears it)
 *   d_colour  float32 [3][nz][ny][nx]  R, G, B planes, 0 .. 255; optional (NULL)
 * `origin` (ox, oy, oz) is the world position of voxel (0, 0, 0)'s centre (OpenCV convention, metres), v = voxel_size, tau = truncation.
 * Every entry point is stateless and allocates nothing; every buffer is the caller's. All float arithmetic below is fp32, round to
 * nearest, one rounding per operation in the order written (the unit is built without contraction), division is IEEE division.
 * tests/tsdf_restated.py restates all of it in numpy.
 *
 * INTEGRATE. One thread per voxel walks the call's frames in table order and keeps the voxel in registers, so the result does not
 * depend on how the caller cuts a sequence into calls. Frame row (acez_tsdf_frame): m[12] = the 3 x 4 world -> camera rows, focal,
 * ppx, ppy in pixels of THIS frame, its size h x w, and `offset`: the element index of its pixel (0, 0) in d_depth (uint16, raw
 * sensor units, row-major h x w) and, times 3, in d_rgb (uint8 RGB, optional). Frames of different sizes may share a call. Per frame:
 *   1. px = ox + float(i) * v                                                (py, pz alike)
 *   2. xc = ((m0 * px + m1 * py) + m2 * pz) + m3                             (yc from m4..m7, zc from m8..m11)
 *   3. skip unless zc > 0
 *   4. u = (focal * xc) / zc + ppx,  w_ = (focal * yc) / zc + ppy            (pixel index and image coordinate are the same number)
 *   5. skip unless u >= -0.5 && u < float(w) - 0.5 && w_ >= -0.5 && w_ < float(h) - 0.5     (tested on the floats: rejects NaN / inf)
 *      ix = min(int(floor(u + 0.5)), w - 1), iy = min(int(floor(w_ + 0.5)), h - 1)          (the min only guards the sum's rounding)
 *   6. raw = d_depth[offset + iy * w + ix]; skip if raw == 0; d = float(raw) * depth_unit; skip if d > max_depth
 *   7. sdf = d - zc; skip if sdf < -tau
 *   8. t = min(1, sdf / tau)
 *   9. w1 = weight + 1; tsdf = (tsdf * weight + t) / w1; with colour, per channel c = (c * weight + float(rgb)) / w1;
 *      weight = min(w1, max_weight)
 * A workgroup is a brick of 32 x 4 x 2 voxels. With frustum_skip != 0, thread f of the brick first tests frame f against the brick's
 * box in double (the eight corners against the five planes zc > 0, u >= -0.5, u < w - 0.5 and the two of w_, each with a slack of
 * 1e-5 of the magnitudes that enter, some twenty times the rounding error of steps 1-4), and the brick's waves pass over a frame whose
 * test says that every voxel fails step 3 or 5. The results are those of frustum_skip == 0, bit for bit.
 * h_frames is a HOST array of n_frames rows, checked here (that is what bounds every index the kernel forms) and copied into d_frames,
 * device scratch of n_frames rows, on `stream`; the copy has completed when the call returns (h_frames may be reused), the kernel is
 * asynchronous. Calls that share d_frames must share the stream. n_frames = 0 does nothing.
 * ACEZ_ERR_INVALID, before anything is launched, for: a null pointer (other than d_colour, d_rgb; d_colour without d_rgb leaves the
 * colour as it is, d_rgb without d_colour is refused), a dimension < 1 or nx * ny * nz >= 2^31, v or tau not > 0 (or not finite),
 * depth_unit, max_depth or max_weight not > 0, n_frames outside 0 .. 256, a row with h or w outside 1 .. 32768, focal not > 0,
 * a non-finite number, offset < 0 or offset + h * w > n_pixels (the length of d_depth in elements). */
#define ACEZ_TSDF_MAX_FRAMES 256
typedef struct {
  float m[12];
  float focal, ppx, ppy;
  int32_t h, w;
  int32_t reserved;
  int64_t offset;
} acez_tsdf_frame;
int acez_tsdf_integrate(float* d_tsdf, float* d_weight, float* d_colour, int nx, int ny, int nz, float ox, float oy, float oz,
                        float voxel_size, float truncation, const uint16_t* d_depth, const uint8_t* d_rgb, int64_t n_pixels,
                        const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames, float depth_unit, float max_depth,
                        float max_weight, int frustum_skip, void* stream);
/* EXTRACT (naive surface nets: one vertex per active cell, one quad per sign-changing voxel edge; no case table).
 * A voxel is KNOWN if weight >= min_weight and INSIDE if tsdf < 0 (-0.0 is outside). Cell (i, j, k), i < nx - 1, j < ny - 1,
 * k < nz - 1, has the corners (i + dx, j + dy, k + dz), corner number dx + 2 dy + 4 dz; it is ACTIVE if all eight are known and not
 * all on one side. A cell's linear index is its corner 0's voxel index. Its vertex: over the 12 edges in the order
 *   x: (0,1) (2,3) (4,5) (6,7)   y: (0,2) (1,3) (4,6) (5,7)   z: (0,4) (1,5) (2,6) (3,7)      (a, b) = corner numbers, a the lower end
 * every edge whose ends differ in side adds its crossing, s = da / (da - db), point = pa + s * (pb - pa) per component with pa, pb the
 * corners' (dx, dy, dz) as floats, to a running sum (three components, in edge order); mean = sum / float(count); the vertex is
 * ox + (float(i) + mean_x) * v, and alike in y and z. Colour: the same running sum and mean of ca + s * (cb - ca) per channel, then
 * min(max(floor(mean + 0.5), 0), 255) as uint8.
 *   acez_tsdf_cells, d_vertex_rank == NULL: d_active uint8 [nz][ny][nx] := 1 for the active cells, 0 elsewhere.
 *   acez_tsdf_cells, d_vertex_rank = the INCLUSIVE prefix sum (int32) of d_active: every active cell writes its vertex, and its colour
 *     if d_colour and d_out_colours are given, to row rank - 1 of d_out_vertices float32 [n_vertices][3] / d_out_colours uint8
 *     [n_vertices][3] (a rank outside 1 .. n_vertices writes nothing). Vertex ids ascend with the cell's linear index.
 * Faces: axis a = x, y, z with (a, b, c) = (x, y, z), (y, z, x), (z, x, y). The edge from voxel p to p + e_a makes a quad if both ends
 * are known, their sides differ and the four cells p - e_b - e_c, p - e_c, p, p - e_b (in this order c0, c1, c2, c3: counter-clockwise
 * seen from +a) are in range and active; it gives the triangles (c0, c1, c2), (c0, c2, c3) if the lower end p is inside, and
 * (c0, c2, c1), (c0, c3, c2) if it is outside: the normals point to positive tsdf (free space).
 *   acez_tsdf_faces, d_edge_rank == NULL: d_edge_flags uint8 [3][nz][ny][nx] (axis-major, the edge at its lower end's voxel index) := 1 / 0.
 *   acez_tsdf_faces, d_edge_rank = the inclusive prefix sum (int32) of d_edge_flags: the edge of rank r writes its triangles to rows
 *     2 (r - 1), 2 (r - 1) + 1 of d_out_faces int32 [n_faces][3] (nothing past n_faces), vertex id = d_vertex_rank[cell] - 1.
 * Faces are therefore axis-major, then ascending in the edge's linear index: the mesh is a deterministic function of the volume.
 * Asynchronous. ACEZ_ERR_INVALID for a null pointer (other than the optional ones named), a dimension < 1, nx * ny * nz >= 2^31 / 3,
 * v not > 0, a negative output count. */
int acez_tsdf_cells(const float* d_tsdf, const float* d_weight, const float* d_colour, int nx, int ny, int nz, float ox, float oy,
                    float oz, float voxel_size, float min_weight, uint8_t* d_active, const int32_t* d_vertex_rank,
                    float* d_out_vertices, uint8_t* d_out_colours, int64_t n_vertices, void* stream);
int acez_tsdf_faces(const float* d_tsdf, const float* d_weight, int nx, int ny, int nz, float min_weight, const uint8_t* d_active,
                    uint8_t* d_edge_flags, const int32_t* d_vertex_rank, const int32_t* d_edge_rank, int32_t* d_out_faces,
                    int64_t n_faces, void* stream);

/* =====================================================================================================
 * K2. The same fusion on a block-sparse volume: scenes whose dense volume does not fit (fuse_depth.py --sparse True)
 * =====================================================================================================
 * The VIRTUAL grid is section K's: origin, nx x ny x nz, v, tau; nothing of its size is ever stored but one byte (mark) and one int32
 * (table) per BLOCK. A block is 8 x 8 x 8 voxels; the block grid has bx = ceil(nx / 8), by, bz blocks, block (bi, bj, bk) has the
 * linear index (bk * by + bj) * bx + bi (x fastest) and holds the voxels 8 bi .. 8 bi + 7 (and alike). A block grid of 2^31 entries
 * or more is refused. Blocks that get storage are numbered by SLOTS 0 .. n_blocks - 1 in ascending block index:
 *   d_block_table  int32 [bz][by][bx]                the block's slot, or -1 (any value outside 0 .. n_blocks - 1 reads as -1)
 *   d_slot_blocks  int32 [n_blocks]                  the slot's block index (a value that is no block index: the slot is passed over,
 *                                                    nothing of it is read or written)
 *   d_tsdf, d_weight  float32 [n_blocks][8][8][8]    voxel (i, j, k) is element (k & 7) * 64 + (j & 7) * 8 + (i & 7) of its block's slot
 *   d_colour       float32 [3][n_blocks][8][8][8]    optional
 * The caller clears the storage as in section K (finite tsdf, weight 0 = never observed). The table lives in device memory, so a bad
 * entry cannot be refused on the host without a synchronisation per call; the kernels bound every index they form from it instead.
 * Voxels of a block beyond nx, ny, nz are never written and read as unknown. A voxel of a block without a slot is UNKNOWN.
 *
 * MARK (acez_tsdf_mark) decides where blocks are needed. One thread per depth pixel (ix, iy) of the call's frames (table and packed
 * buffer as in acez_tsdf_integrate). raw == 0 or d = float(raw) * depth_unit > max_depth (fp32, step 6) marks nothing. Otherwise,
 * everything in DOUBLE, one rounding per operation in the order written (R = the row's 3 x 3 part, t = m3, m7, m11; S = 1e-5):
 *   per frame   C = the transposed cofactors of R, each a difference of two products: C00 = R11 R22 - R12 R21, C01 = R02 R21 - R01 R22,
 *               C02 = R01 R12 - R02 R11, C10 = R12 R20 - R10 R22, C11 = R00 R22 - R02 R20, C12 = R02 R10 - R00 R12,
 *               C20 = R10 R21 - R11 R20, C21 = R01 R20 - R00 R21, C22 = R00 R11 - R01 R10; det = (R00 C00 + R01 C10) + R02 C20;
 *               I = C / det (nine divisions; |det| < 1e-6 is refused on the host)
 *               A_c = max(|o_c|, |o_c + double(n_c - 1) * v|)                 (how far a voxel centre is from 0, per world axis c)
 *               M_r = ((|R_r0| A_0 + |R_r1| A_1) + |R_r2| A_2) + |t_r|,  e_r = S * M_r      (camera axis r)
 *               s_a = (|I_a0| e_0 + |I_a1| e_1) + |I_a2| e_2                               (world axis a)
 *               su = S * ((|ppx| + double(w)) + 1),  sv = S * ((|ppy| + double(h)) + 1)
 *   per pixel   sd = S * (d + tau);  z in { max(d - sd, 0), (d + tau) + sd };  u in { (ix - 0.5) - su, (ix + 0.5) + su };
 *               w_ in { (iy - 0.5) - sv, (iy + 0.5) + sv }
 *               the eight corners: x = ((u - ppx) / focal) * z, y = ((w_ - ppy) / focal) * z,
 *               world_a = (I_a0 (x - t_0) + I_a1 (y - t_1)) + I_a2 (z - t_2);  lo_a, hi_a = their min and max
 *               first_a = max(floor(((lo_a - s_a) - o_a) / v) - 1, 0),  last_a = min(ceil(((hi_a + s_a) - o_a) / v) + 1, n_a - 1)
 *               nothing unless first_a <= last_a on every axis; else d_block_flags[block] := 1 for every block of
 *               first_a >> 3 .. last_a >> 3. Flags are only ever set: the caller clears d_block_flags uint8 [bz][by][bx] once, and
 *               any number of calls in any split of the frames leaves the same bytes. Plain stores of the same value, no atomics.
 * Why this is a SUPERSET of what the dense extraction reads (min_weight > 0). (1) tsdf < 0 with weight > 0 needs a frame whose step 8
 * gave t < 0, that is sdf in [-tau, 0): the mean of values >= 0 is not negative. (2) For that frame the voxel's fp32 triple
 * T = (xc, yc, zc) has floor(u + 0.5) = ix, so (focal xc) / zc + ppx is in [ix - 0.5, ix + 0.5] up to the three roundings of step 4
 * and the one of u + 0.5, each below 2^-23 of |u - ppx| + |u| + 1 <= 2 (|ppx| + w + 1): within su, some forty times that; d - zc is in
 * [-tau, 0) up to one rounding of d + tau: within sd. So T lies in the widened cell, the convex hull of the eight corners (z >= 0).
 * (3) The voxel's exact centre P = o + index * v has the exact camera point Q = R P + t, and |Q_r - T_r| <= e_r: step 1 rounds twice
 * (2^-23 of A), step 2 four times (2^-22 of M_r), against S = 1e-5, the margin section K's frustum skip takes. P = I (Q - t) =
 * I (T - t) + I (Q - T) then lies in the corners' box widened by s_a. (4) first / last widen by one more voxel, so the box holds the
 * voxel and its 26 neighbours. (5) An active cell has an inside corner, and its eight corners are among that corner's neighbours; a
 * quad's edge has an inside end, and the four cells around the edge hold both ends, so all their corners are that end's neighbours.
 * Every voxel the dense extraction reads to make a vertex or a face therefore lies in a marked block, and a cell with a corner in an
 * unmarked block is inactive in the dense volume too (it would need an inside corner, whose neighbours are all marked).
 * ACEZ_ERR_INVALID as in acez_tsdf_integrate (null pointer, dimension < 1, v, tau, depth_unit, max_depth not > 0, the frame table's
 * rows, an offset past the buffer), for the block-grid limit and for a singular pose.
 *
 * INTEGRATE (acez_tsdf_integrate_blocks). One workgroup of 512 threads per slot, thread = voxel of the block, x fastest. Every voxel
 * whose global index (i, j, k) lies inside nx, ny, nz runs section K's steps 1-9 over the call's frames, with the GLOBAL index in
 * step 1; it is the same device function as the dense kernel's. The frustum skip is section K's, on the block's box. The voxels of
 * the allocated blocks therefore hold the dense volume's bits, whatever the split into calls. Arguments and refusals as in
 * acez_tsdf_integrate, plus n_blocks < 0 or > bx by bz and the block-grid limit; n_blocks = 0 does nothing.
 *
 * EXTRACT (acez_tsdf_cells_blocks, acez_tsdf_faces_blocks): section K's cells, vertices, colours, quads and orientation, with
 * "unknown" extended to voxels outside the grid and voxels of blocks without a slot; min_weight must be > 0. One workgroup per slot
 * loads the block and its one-voxel halo through the table. The two modes and the prefix sums between them are section K's, over
 *   d_active, d_vertex_rank   [n_blocks][8][8][8]       d_edge_flags, d_edge_rank   [3][n_blocks][8][8][8]
 * so vertex ids ascend by block index, then by voxel index inside the block, and faces are axis-major, then in that order. A cell's
 * vertex is o + (float(global index) + mean) * v. The mesh is the dense mesh with its rows in another order, if every block the
 * dense extraction reads has a slot (MARK). ACEZ_ERR_INVALID as in acez_tsdf_cells / acez_tsdf_faces, plus min_weight not > 0,
 * n_blocks < 0 or > bx by bz, n_blocks * 512 >= 2^31 / 3 and the block-grid limit. */
int acez_tsdf_mark(uint8_t* d_block_flags, int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, float truncation,
                   const uint16_t* d_depth, int64_t n_pixels, const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames,
                   float depth_unit, float max_depth, void* stream);
int acez_tsdf_integrate_blocks(float* d_tsdf, float* d_weight, float* d_colour, const int32_t* d_slot_blocks, int n_blocks, int nx, int ny,
                               int nz, float ox, float oy, float oz, float voxel_size, float truncation, const uint16_t* d_depth,
                               const uint8_t* d_rgb, int64_t n_pixels, const acez_tsdf_frame* h_frames, int n_frames,
                               acez_tsdf_frame* d_frames, float depth_unit, float max_depth, float max_weight, int frustum_skip,
                               void* stream);
int acez_tsdf_cells_blocks(const float* d_tsdf, const float* d_weight, const float* d_colour, const int32_t* d_block_table,
                           const int32_t* d_slot_blocks, int n_blocks, int nx, int ny, int nz, float ox, float oy, float oz,
                           float voxel_size, float min_weight, uint8_t* d_active, const int32_t* d_vertex_rank, float* d_out_vertices,
                           uint8_t* d_out_colours, int64_t n_vertices, void* stream);
int acez_tsdf_faces_blocks(const float* d_tsdf, const float* d_weight, const int32_t* d_block_table, const int32_t* d_slot_blocks,
                           int n_blocks, int nx, int ny, int nz, float min_weight, const uint8_t* d_active, uint8_t* d_edge_flags,
                           const int32_t* d_vertex_rank, const int32_t* d_edge_rank, int32_t* d_out_faces, int64_t n_faces, void* stream);

/* =====================================================================================================
 * K3. Tracking frames against the volume: frame-to-model pose refinement on the SDF (fuse_depth.py --refine_poses)
 * =====================================================================================================
 * The volume that all frames built is the model; a frame's pose is moved so that its back-projected depth pixels fall on the model's
 * zero level (the tracking half of KinectFusion in the SDF form of Bylow et al.: no ray-cast, no correspondences). Gauss-Newton on
 * the trilinear SDF, the loop resident on the device (acezero_amd.fusion's _Volume.track enqueues
 * max_iterations ACCUMULATE + UPDATE pairs per call and reads the result back once; tests/track_restated.py restates both in numpy).
 * The volume, the packed uint16 depth buffer and the frame table are section K's (K2's for the block-sparse twin). Of a row only
 * focal, ppx, ppy, h, w and offset are used; m must be finite (the rows' checks are section K's) but is ignored: the poses live in
 * the state. Every frame of a call runs its own loop; frames do not interact.
 *
 * STATE. d_state: n_frames records of 45 doubles owned by the caller, frame f at element 45 f. [0..11] the current camera -> world
 * pose, rows 0..2 of the 4 x 4, row-major (R = columns 0..2, t = column 3); [12] status: 0 running, 1 converged, 2 degenerate;
 * [13] the number of records written; [14], [15] count and rms of the previous record; [16..44] the 29 totals of the last UPDATE that
 * ran. A loop starts from the pose, status 0, the rest 0.
 *
 * ACCUMULATE (acez_tsdf_track_accumulate; acez_tsdf_track_accumulate_blocks on section K2's storage). Grid (tiles, n_frames) with
 * tiles = ceil(h w / 256) of the call's LARGEST frame; workgroup (x, f) takes the pixels i = 256 x .. 256 x + 255 of frame f, row-major,
 * ix = i % w, iy = i / w. A workgroup of a frame whose status != 0 returns at once; so does one with 256 x >= h w of its own frame
 * (its row of d_partials is never written and never read). Per pixel:
 *   raw = d_depth[offset + i]. NO SAMPLE if raw == 0 or d32 = float(raw) * depth_unit (fp32, section K step 6) > max_depth.
 *   From here everything is fp64, round to nearest, one rounding per operation in the order written (the unit is built without
 *   contraction); floats (d32, ppx, ppy, focal, origin, v, tau, the voxels' tsdf) enter by exact conversion.
 *   z = d32,  x = ((ix - ppx) * z) / focal,  y = ((iy - ppy) * z) / focal
 *   pw_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a                                          (a = 0, 1, 2: the world point)
 *   g_a = (pw_a - origin_a) / v,  i0_a = floor(g_a),  fr_a = g_a - i0_a
 *   NO SAMPLE unless on every axis g_a is finite and 0 <= i0_a <= n_a - 2 (all eight corners i0 + (dx, dy, dz) are voxels).
 *   NO SAMPLE unless all eight corners have weight >= min_weight (fp32 comparison). Sparse: a corner in a block without a slot (table
 *   entry outside 0 .. n_blocks - 1) has weight 0 and tsdf 1; min_weight must be > 0 there. (d_slot_blocks belongs to the volume's
 *   description as in K2; the look-up goes through the table alone and does not read it.)
 *   NO SAMPLE if every corner's tsdf >= 1 (truncated free space: the interpolant is flat, there is no gradient).
 *   With c_(dx dy dz) the corners' tsdf and (fx, fy, fz) = fr:
 *     along x, the four edges:  e_(dy dz) = c_(1 dy dz) - c_(0 dy dz),   c_(dy dz) = c_(0 dy dz) + fx * e_(dy dz)
 *     along y:                  h_dz = c_(1 dz) - c_(0 dz),               c_dz = c_(0 dz) + fy * h_dz
 *     along z:                  gz = c_1 - c_0,                            value = c_0 + fz * gz
 *     the analytic derivative of that interpolant in the same nesting:
 *       gx_dz = e_(0 dz) + fy * (e_(1 dz) - e_(0 dz)),  gx = gx_0 + fz * (gx_1 - gx_0);     gy = h_0 + fz * (h_1 - h_0);     gz as above
 *   r = tau * value (metres),  n = (tau / v) * (gx, gy, gz)  (the quotient once, then three products)
 *   a = pw - t: the lever about the pivot, the frame's current camera centre
 *   J = [n_x, n_y, n_z, a_y n_z - a_z n_y, a_z n_x - a_x n_z, a_x n_y - a_y n_x]           (each cross term: two products, one difference)
 *   the 29 terms:  [0] 1   [1..21] J_i J_j, i <= j, row-major (the upper triangle of J J^T)   [22..27] J_i r   [28] r r
 *   A pixel without a sample, and a lane past h w, contributes 29 zeros.
 * Reduction, section N's: pixel i is lane i % 64 of wavefront (i / 64) % 4 of tile i / 256. Per term: within a wavefront the xor
 * butterfly v = v + v[lane ^ s] for s = 32, 16, 8, 4, 2, 1, then the tile's four wavefronts added in ascending order,
 * (((w0 + w1) + w2) + w3). d_partials double [n_frames][tiles][29]: one row per tile. No atomics: nothing depends on scheduling.
 * The frame table: h_frames is checked on every call (that is what bounds every index the kernel forms) and sizes the grid; with
 * upload != 0 it is copied into d_frames as in section K (the copy has completed when the call returns), with upload == 0 d_frames
 * must hold these rows from an earlier call on the same stream, and the call is asynchronous: a loop uploads once.
 * The voxel loads are the cost: eight fp32 pairs per sample. A tile is a segment of 256 pixels of one or two image rows, whose points
 * run along a line through the volume, so neighbouring lanes read neighbouring voxels.
 *
 * UPDATE (acez_tsdf_track_update). One workgroup of 256 threads per frame; d_frames as ACCUMULATE left it, `tiles` the row stride of
 * d_partials. If status != 0, or [13] is not in 0 .. max_iterations - 1, it returns at once. Totals: thread t adds the frame's rows
 * t, t + 256, .. (below min(ceil(h w / 256), tiles)) in ascending order from 0.0, per term; the 256 threads' sums are reduced as above.
 * Then, in this order (acezero_amd/csrc/track_solve.h is the text; only +, -, *, / and sqrt occur, so that the device, the host
 * instantiation and numpy give the same bits):
 *   count = total[0], rms = sqrt(total[28] / count), 0 if count is not > 0
 *   record [13] of the frame's history (16 doubles each: pose (12), count, total[28], rms, and the status this update ends with) is
 *   written, [13] += 1, [14], [15] = count, rms, the totals are kept
 *   (a) from the second record on: |rms - previous| < rel_rms -> status 1, pose unchanged
 *   (b) a total that is not finite, or count < min_count -> status 2, pose unchanged
 *   (c) H = the symmetric matrix of [1..21], b = [22..27]; lambda = damping * (((((H00 + H11) + H22) + H33) + H44) + H55) / 6);
 *       H' = H + lambda I. Cholesky H' = L L^T in place, column j = 0 .. 5: d = H'_jj - L_j0^2 - .. - L_j(j-1)^2 (subtracted in this
 *       order); d <= 1e-12 * the largest diagonal entry of H' (or not a number) -> status 2, pose unchanged; L_jj = sqrt(d);
 *       L_ij = (H'_ij - L_i0 L_j0 - .. - L_i(j-1) L_j(j-1)) / L_jj for i > j
 *   (d) y_i = (b_i - L_i0 y_0 - .. - L_i(i-1) y_(i-1)) / L_ii, i = 0 .. 5;  x_i = (y_i - L_(i+1)i x_(i+1) - .. - L_5i x_5) / L_ii,
 *       i = 5 .. 0;  (u, omega) = -x
 *   (e) retraction (Cayley): q = (1, omega / 2) / sqrt(((1 + hx hx) + hy hy) + hz hz) with h = omega / 2, as (qw, qx, qy, qz);
 *       D = [1 - 2 (qy qy + qz qz), 2 (qx qy - qw qz), 2 (qx qz + qw qy);  2 (qx qy + qw qz), 1 - 2 (qx qx + qz qz), 2 (qy qz - qw qx);
 *            2 (qx qz - qw qy), 2 (qy qz + qw qx), 1 - 2 (qx qx + qy qy)]
 *   (f) R <- D R with (D R)_rc = (D_r0 R_0c + D_r1 R_1c) + D_r2 R_2c;  t <- t + u. The pivot is t, so the rotation leaves it in place.
 *       A new pose that is not finite -> status 2, pose unchanged.
 * d_history double [n_frames][max_iterations][16].
 * The damping keeps a direction the frame does not observe (a single wall: sliding in its plane) nearly still; with damping 0 such a
 * frame ends degenerate. Gauss-Newton on a TSDF sees no further than tau: an error beyond it is not recovered.
 *
 * ACCUMULATE without upload and UPDATE are asynchronous on `stream`. ACEZ_ERR_INVALID, before anything is launched, for: what section K
 * (K2) refuses for the same arguments (dimensions, v, tau, depth_unit, max_depth, the frame count and rows, the block grid and count);
 * a null d_state, d_partials, d_history, d_frames or volume (the sparse twin takes null storage with n_blocks = 0: every corner is
 * unknown); min_weight not finite (sparse: not > 0); tiles < 0; max_iterations < 1; rel_rms or damping negative or not finite;
 * min_count < 6. */
int acez_tsdf_track_accumulate(const float* d_tsdf, const float* d_weight, int nx, int ny, int nz, float ox, float oy, float oz,
                               float voxel_size, float truncation, const uint16_t* d_depth, int64_t n_pixels,
                               const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames, int upload, float depth_unit,
                               float max_depth, float min_weight, const double* d_state, double* d_partials, void* stream);
int acez_tsdf_track_accumulate_blocks(const float* d_tsdf, const float* d_weight, const int32_t* d_block_table,
                                      const int32_t* d_slot_blocks, int n_blocks, int nx, int ny, int nz, float ox, float oy, float oz,
                                      float voxel_size, float truncation, const uint16_t* d_depth, int64_t n_pixels,
                                      const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames, int upload,
                                      float depth_unit, float max_depth, float min_weight, const double* d_state, double* d_partials,
                                      void* stream);
int acez_tsdf_track_update(const double* d_partials, int tiles, const acez_tsdf_frame* d_frames, int n_frames, double rel_rms,
                           double damping, int min_count, int max_iterations, double* d_state, double* d_history, void* stream);

/* =====================================================================================================
 * L. Dense depth for RGB reconstructions: plane-sweep multi-view stereo (estimate_depth.py)
 * =====================================================================================================
 * Frames arrive as in section K: packed buffers of n_pixels elements and a HOST table of acez_mvs_frame rows (= acez_tsdf_frame:
 * m[12] the 3 x 4 world -> camera rows, focal, ppx, ppy in pixels of THIS frame, h, w, and `offset`, the element index of the frame's
 * pixel (0, 0) in every packed buffer of the call). Frames of different sizes may share a call. Camera model and pixel convention are
 * section K's: u = (focal * xc) / zc + ppx, pixel index = image coordinate, nearest pixel floor(u + 0.5), so the fuser reads a depth
 * map at the coordinates it was estimated at. Every entry point is stateless, allocates nothing and reads no environment variable;
 * kernels run on `stream`. All float arithmetic is fp32, round to nearest, one rounding per operation in the order written (the unit
 * is built without contraction), division is IEEE division, int(x) truncates. tests/mvs_restated.py restates all of it in numpy.
 *
 * PREFILTER (acez_mvs_prefilter, one launch over all frames). Per pixel (x, y) of a frame, integers only: sum and n = the sum and the
 * number of the frame's pixels in [x - 4, x + 4] x [y - 4, y + 4]; m = (sum + n / 2) / n; g = min(max(I - m + 128, 0), 255).
 * d_grey and d_out are uint8 [n_pixels] and must not overlap. The table is copied into d_frames (device scratch of n_frames rows) on
 * `stream`; the copy has completed when the call returns. n_frames in 1 .. 65535.
 *
 * RELATIVE POSE (acez_mvs_relative; host only, no device needed; the sweep and the check call it). From the rows r (reference) and s
 * (source), in DOUBLE, one rounding per operation, then each of the 12 numbers rounded once to float:
 *   R[i][j] = (s.m[4i] * r.m[4j] + s.m[4i+1] * r.m[4j+1]) + s.m[4i+2] * r.m[4j+2]
 *   t[i]    = s.m[4i+3] - ((R[i][0] * r.m[3] + R[i][1] * r.m[7]) + R[i][2] * r.m[11])
 *   out12   = float of R[0][0], R[0][1], R[0][2], t[0], R[1][0], ...           (a point of r's camera -> s's camera)
 *
 * SWEEP (acez_mvs_sweep, one launch per reference frame r, on the PREFILTERED buffer g). S sources h_sources[0 .. S-1] (rows of the
 * table), D planes fronto-parallel to r and uniform in inverse depth, window radius w, truncation T, `keep`, uniqueness percentage q.
 *   planes    inv_near = 1 / z_near; inv_far = 1 / z_far; step = (inv_near - inv_far) / float(D - 1)      (host, fp32)
 *             inv_k = inv_far + float(k) * step; z_k = 1 / inv_k, k = 0 (far) .. D - 1 (near)
 *   ray       rx = (float(x) - r.ppx) / r.focal, ry = (float(y) - r.ppy) / r.focal of reference pixel p' = (x, y)
 *   raw(p', k, s), with M = the relative pose r -> s, f, cx, cy, hs, ws = s's focal, ppx, ppy, h, w:
 *     1. X = rx * z_k, Y = ry * z_k
 *     2. xc = ((M0 * X + M1 * Y) + M2 * z_k) + M3                              (yc from M4..M7, zc from M8..M11)
 *     3. u = (f * xc) / zc + cx, v = (f * yc) / zc + cy
 *     4. IN VIEW iff zc > 0 && u >= 0 && u <= float(ws - 1) && v >= 0 && v <= float(hs - 1)      (on the floats: NaN fails)
 *     5. x0 = int(floor(u)), x1 = min(x0 + 1, ws - 1), fx = u - float(x0); y0, y1, fy alike     (all four texels inside the frame)
 *     6. a = g_s[y0][x0], b = g_s[y0][x1], c = g_s[y1][x0], d = g_s[y1][x1] as floats;
 *        top = a + fx * (b - a); bot = c + fx * (d - c); val = top + fy * (bot - top); sample = int(val + 0.5)
 *     7. raw = min(|g_r(p') - sample|, T) in view, T out of view; T for a p' outside the reference frame (never in view)
 *   A_s(p, k) = the sum of raw over the (2w + 1)^2 pixels p' around p. C(p, k) = the sum of the `keep` smallest of A_0 .. A_{S-1}.
 *   k* = the first minimum of C over k. N* = the number of sources with p itself in view at k*.
 *   C2 = the smallest C(p, k) over the planes with |k - k*| > 1. UNIQUE iff there is no such plane, or
 *        C2 > 0 && 100 * C(k*) <= (100 - q) * C2                               (integers; 0 against 0 is a tie, not a winner)
 *   delta = 0; if 0 < k* < D - 1: den = C(k*-1) - 2 C(k*) + C(k*+1); if den > 0: delta = float(C(k*-1) - C(k*+1)) / float(2 * den)
 *   depth = 1 / (inv_far + (float(k*) + delta) * step), and 0 if N* < keep, or not UNIQUE, or (D > 2 and k* is 0 or D - 1).
 * Outputs at r's offset, row-major h x w: d_out_depth float32 [n_pixels]; optional (NULL) d_out_cost int32 = C(k*), d_out_plane
 * int32 = k* (both written for every pixel, kept or not). Only r's h x w elements are written.
 * Kernel shape (acezero_amd/csrc/mvs_api.hip): a 256-thread workgroup owns 16 x 16 reference pixels, reads their halo of g_r once
 * (up to three halo pixels per thread, kept in registers), then per plane and source writes the raw costs of the (16 + 2w)^2 halo
 * tile to LDS and sums the windows from there; A_s, the four smallest (C, k) and the costs beside the best stay in registers. No cost volume exists in memory. The relative poses and
 * intrinsics are launch arguments. No atomics, no communication between workgroups, plain loads and stores.
 *
 * CHECK (acez_mvs_check, one launch per reference frame, after every source has a depth map in d_depth float32 [n_pixels]).
 * Per pixel (x, y) of r with d = d_depth[r.offset + y * w + x] > 0, per source s:
 *     1. X = rx * d, Y = ry * d (rx, ry as above); xc, yc, zc as step 2 with z_k = d; skip unless zc > 0; u, v as step 3
 *     2. skip unless u >= -0.5 && u < float(ws) - 0.5 && v >= -0.5 && v < float(hs) - 0.5
 *        ix = min(int(floor(u + 0.5)), ws - 1), iy = min(int(floor(v + 0.5)), hs - 1); ds = d_depth[s.offset + iy * ws + ix]
 *     3. s AGREES iff ds > 0 && |ds - zc| <= tolerance * zc
 * The pixel is kept iff at least min(min_consistent, S) sources agree. d_out uint16 [n_pixels] at r's offset:
 * qd = floor(d / depth_unit + 0.5); qd as uint16 if kept and qd <= 65535, else 0. d_depth is not written.
 *
 * ACEZ_ERR_INVALID, before anything is launched, for: a null pointer (other than the two optional outputs), n_pixels < 0, n_frames
 * < 1, a row with h or w outside 1 .. 32768, focal not > 0, a non-finite number, offset < 0 or offset + h * w > n_pixels, `ref` or a
 * source index outside 0 .. n_frames - 1, n_sources outside 1 .. 8, not 0 < z_near < z_far (or not finite), planes
 * outside 2 .. 1024, radius outside 0 .. 4, truncation outside 1 .. 255, keep outside 1 .. n_sources, uniqueness outside 0 .. 100,
 * tolerance not finite or < 0, min_consistent < 0, depth_unit not > 0. */
#define ACEZ_MVS_MAX_SOURCES 8
typedef acez_tsdf_frame acez_mvs_frame;
int acez_mvs_prefilter(const uint8_t* d_grey, uint8_t* d_out, int64_t n_pixels, const acez_mvs_frame* h_frames, int n_frames,
                       acez_mvs_frame* d_frames, void* stream);
int acez_mvs_relative(const acez_mvs_frame* ref, const acez_mvs_frame* src, float* out12);
int acez_mvs_sweep(const uint8_t* d_filtered, int64_t n_pixels, const acez_mvs_frame* h_frames, int n_frames, int ref,
                   const int32_t* h_sources, int n_sources, float z_near, float z_far, int planes, int radius, int truncation, int keep,
                   int uniqueness, float* d_out_depth, int32_t* d_out_cost, int32_t* d_out_plane, void* stream);
int acez_mvs_check(const float* d_depth, int64_t n_pixels, const acez_mvs_frame* h_frames, int n_frames, int ref,
                   const int32_t* h_sources, int n_sources, float tolerance, int min_consistent, float depth_unit, uint16_t* d_out,
                   void* stream);

/* =====================================================================================================
 * M. Semi-global aggregation of the plane costs (estimate_depth.py --aggregation sgm)
 * =====================================================================================================
 * Section L's sweep takes each pixel's best plane on its own, so a textureless surface, whose costs do not tell the planes apart,
 * comes out empty. Here the costs C(p, k) of a reference frame are written to memory, smoothed along scanlines with a small penalty
 * P1 for moving one plane and a larger one P2 for jumping (semi-global matching, Hirschmueller), and the plane is chosen from the
 * smoothed costs by section L's own rule. Three stateless entry points on one reference frame r of section L's frame table; frames,
 * conventions, arithmetic, stream and validation are section L's. Everything from C on is integer arithmetic.
 * tests/sgm_restated.py restates AGGREGATE and SELECT in numpy; VOLUME's reference is tests/mvs_restated.cost_volume.
 *
 * Storage. The VOLUME of r is uint16 [h][w][D], element ((y * w + x) * D + k): C(p, k) in bits 0 .. 14, V(p, k) in bit 15. S is
 * uint32 [h][w][D], the same indexing. Neither carries r.offset: they are scratch of one frame, reused from frame to frame.
 * n_volume is the number of ELEMENTS the caller has allocated for each of the two; all indices into them are 64-bit.
 *
 * VOLUME (acez_mvs_volume). SWEEP's steps 1 - 7, A_s and C(p, k) exactly as written in section L, for every pixel p of r and every
 * plane k, without the reduction over k. V(p, k) = (the number of sources with p itself IN VIEW at k) >= keep. Writes h * w * D
 * elements of d_volume and nothing else. C <= keep * (2w + 1)^2 * T must fit 15 bits.
 *
 * AGGREGATE (acez_mvs_aggregate). `paths` in {4, 8}, penalties 1 <= P1 <= P2 <= 32767. The directions (dy, dx), in this order:
 *   1 (0,+1)  2 (0,-1)  3 (+1,0)  4 (-1,0)  5 (+1,+1)  6 (+1,-1)  7 (-1,+1)  8 (-1,-1);          four paths are directions 1 - 4.
 * For direction r and pixel p = (y, x) with predecessor q = p - r = (y - dy, x - dx):
 *   q outside the frame:  L_r(p, k) = C(p, k)
 *   otherwise:            m = min_j L_r(q, j)
 *                         L_r(p, k) = C(p, k) + min(L_r(q, k), L_r(q, k-1) + P1, L_r(q, k+1) + P1, m + P2) - m
 *                         (the term with k - 1 < 0 or k + 1 > D - 1 is absent)
 * so C <= L_r <= C + P2. C is bits 0 .. 14 of the volume; bit 15 is ignored. With direction = 0 every element of d_s gains
 * S(p, k) = the sum of L_r(p, k) over the `paths` directions; with direction = r in 1 .. paths it gains L_r(p, k) alone (the tests
 * check each direction by itself). d_s is ADDED to, with integer additions whose order is free: the caller zeroes it before the
 * first call of a frame. S <= paths * (32767 + P2) < 2^19.
 * Frames with h = 1 or w = 1 are allowed: every diagonal predecessor is then outside.
 *
 * SELECT (acez_mvs_select). SWEEP's rule from k* to `depth` verbatim on a cost volume X in place of C, X = S (d_s) or, with d_s
 * NULL, C itself (no aggregation ran): k* = the first minimum of X(p, .); C2 = the smallest X(p, k) with |k - k*| > 1; UNIQUE iff
 * there is no such plane or C2 > 0 && 100 * X(k*) <= (100 - q) * C2; delta from X(k* - 1), X(k*), X(k* + 1) as in SWEEP;
 * depth = 1 / (inv_far + (float(k*) + delta) * step), and 0 if !V(p, k*) (SWEEP's N* < keep), or not UNIQUE, or (D > 2 and k* is 0
 * or D - 1). Outputs as SWEEP's, at r.offset: d_out_depth float32 [n_pixels], optional d_out_cost int32 = X(k*), d_out_plane = k*.
 * Every element of d_s that SELECT reads must be <= 8 * 65534 = 524272, which AGGREGATE into a zeroed buffer guarantees; a buffer that
 * was not zeroed, or that several calls with direction = 0 accumulated into, is outside the definition (the kernel packs X and k into
 * one 32-bit key). VOLUME followed by SELECT with d_s NULL gives acez_mvs_sweep's three outputs bit for bit.
 *
 * Kernel shape (acezero_amd/csrc/mvs_api.hip). VOLUME is the sweep kernel's second instantiation: one plane loop, C and V stored
 * per plane. AGGREGATE: one wavefront per scanline of a direction, its lanes hold the planes (lane l: l, l + 64, ...), L_r(q, .) in
 * registers, k - 1 / k + 1 by wave rotates, m by a wave-wide minimum, S by 32-bit integer atomics without return; all scanlines of
 * all directions of a call are one launch. SELECT: 16 lanes per pixel, two passes over the D values. No communication between
 * workgroups.
 *
 * ACEZ_ERR_INVALID, before anything is launched, for everything section L refuses for the same argument, and: keep * (2w + 1)^2 * T
 * > 32767 (VOLUME), `paths` not 4 or 8, `direction` outside 0 .. paths, penalties outside 1 <= P1 <= P2 <= 32767, h or w outside
 * 1 .. 32768, a null d_volume or (AGGREGATE) d_s, n_volume < h * w * D. */
int acez_mvs_volume(const uint8_t* d_filtered, int64_t n_pixels, const acez_mvs_frame* h_frames, int n_frames, int ref,
                    const int32_t* h_sources, int n_sources, float z_near, float z_far, int planes, int radius, int truncation, int keep,
                    uint16_t* d_volume, int64_t n_volume, void* stream);
int acez_mvs_aggregate(const uint16_t* d_volume, uint32_t* d_s, int64_t n_volume, int h, int w, int planes, int paths, int direction, int p1,
                       int p2, void* stream);
int acez_mvs_select(const uint16_t* d_volume, const uint32_t* d_s, int64_t n_volume, int64_t n_pixels, const acez_mvs_frame* h_frames,
                    int n_frames, int ref, float z_near, float z_far, int planes, int uniqueness, float* d_out_depth, int32_t* d_out_cost,
                    int32_t* d_out_plane, void* stream);

/* =====================================================================================================
 * N. Distances between two point clouds: uniform grid, nearest neighbour within a radius, voxel means (eval_geometry.py)
 * =====================================================================================================
 * Three stateless entry points, and the two of the ICP loop at the end of the section whose only state is a caller-owned device
 * block; none allocates anything, every buffer is the caller's. Points are float32 [count][3]. All float
 * arithmetic below is fp32, round to nearest, one rounding per operation in the order written (the unit is built without
 * contraction), division is IEEE division. tests/geometry_restated.py restates all of it in numpy.
 *
 * GRID. origin (ox, oy, oz), cell edge c, dimensions nx, ny, nz, each 1 .. 1024, nx * ny * nz <= 2^24. A point's cell on an axis is
 * floor((x - ox) / c); its linear cell is (k * ny + j) * nx + i (x fastest).
 *
 * CELLS (acez_geom_cells). d_out_cells int32 [n]: the linear cell of every point, or -1 if a coordinate is not finite or a cell
 * index is outside 0 .. n_axis - 1. The caller sorts by it (stably) and builds `cell_start` int32 [cells + 1], element v = the number
 * of sorted points in cells < v: plumbing, not part of this library.
 *
 * NEAREST (acez_geom_nearest). d_ref: the m reference points SORTED BY CELL (none with cell -1), d_ref_index int32 [m] their original
 * indices, d_cell_start as above; d_query: n points in any order. Per query (qx, qy, qz), over ALL reference points (px, py, pz):
 *   dx = qx - px (dy, dz alike),  d2 = (dx * dx + dy * dy) + dz * dz
 *   d_out_d2 = the smallest d2 with d2 <= radius * radius (the product in fp32), d_out_index = the smallest ORIGINAL index among the
 *   points that attain it; +inf and -1 if there is none. A query with a non-finite coordinate has none.
 * That is the whole contract: the result does not depend on the grid or on the order inside a cell, it is the brute-force scan's.
 * The search visits the 3 x 3 x 3 cells around the query's cell, the query's cell indices clamped to -1 .. n_axis (queries outside
 * the box are legal). It is complete because the call refuses c < radius * (1 + 2^-10) (product in fp32): with that margin and at
 * most 1024 cells per axis, the two roundings of (x - ox) / c cannot put a reference that passes d2 <= radius^2 two cells away
 * (DESIGN.md section 4l has the argument). d_cell_start is device data that cannot be checked here: the kernel clamps every range
 * it forms to [0, m], so a malformed table gives wrong numbers, never a read out of bounds. Queries ordered by their own cell run
 * fastest (a workgroup whose queries lie in one or two cells stages the neighbouring ranges in LDS); any order gives the same bits.
 *
 * VOXEL MEANS (acez_geom_voxel_means). d_points: n points sorted stably by voxel; d_segment_start int32 [segments + 1], ascending:
 * segment v is the points start[v] .. start[v + 1] - 1 (clamped to [0, n]). d_out_means float32 [segments][3]: per component the
 * sequential sum in array order, from 0.0f, divided by float(count).
 *
 * Asynchronous on `stream`. ACEZ_ERR_INVALID, before anything is launched, for: a null pointer (an array whose count is 0 may be
 * null), a negative count or one >= 2^31, a dimension outside 1 .. 1024 or more than 2^24 cells, a non-finite origin, c or radius
 * not finite or not > 0, c < radius * (1 + 2^-10). */
int acez_geom_cells(const float* d_points, int64_t n, float ox, float oy, float oz, float cell, int nx, int ny, int nz,
                    int32_t* d_out_cells, void* stream);
int acez_geom_nearest(const float* d_ref, const int32_t* d_ref_index, const int32_t* d_cell_start, int64_t m, float ox, float oy, float oz,
                      float cell, int nx, int ny, int nz, const float* d_query, int64_t n, float radius, float* d_out_d2,
                      int32_t* d_out_index, void* stream);
int acez_geom_voxel_means(const float* d_points, int64_t n, const int32_t* d_segment_start, int64_t segments, float* d_out_means,
                          void* stream);

/* ICP: refine a similarity between two clouds by iterated closest points, the loop resident on the device (DESIGN.md section 4m;
 * acezero_amd.geometry.icp_stage enqueues max_iterations ACCUMULATE + UPDATE pairs and reads the result back once;
 * tests/icp_restated.py restates both in numpy).
 *
 * STATE. d_state: 34 doubles owned by the caller. [0..11] the current transform T, rows 0..2 of the 4 x 4, row-major; [12] status:
 * 0 running, 1 converged, 2 degenerate; [13] the number of records written; [14], [15] fitness and rmse of the previous record;
 * [16..33] the 18 totals of the last UPDATE that ran. A stage starts from T (the identity, or any similarity), status 0, the rest 0.
 *
 * ACCUMULATE (acez_geom_icp_accumulate). The target grid exactly as NEAREST takes it; d_src: the n source points in their own frame;
 * pivot (px, py, pz): any finite point, the host passes the centre of the target's box (it keeps the moments small). If status != 0
 * the kernel returns at once. Otherwise, per source point (x, y, z), with T from the state:
 *   x' = float(((T00 x + T01 y) + T02 z) + T03) in fp64, rounded to fp32 once (y', z' alike): geometry.apply_similarity's arithmetic
 *   q  = the nearest target of x' within the radius under the NEAREST contract above (same d2, same tie rule), so the
 *        correspondences are those of NEAREST on the transformed cloud, bit for bit; none if x' is not finite
 *   a = (double)x' - (double)pivot, b = (double)q - (double)pivot, and the 18 terms, all fp64:
 *     [0] 1   [1..3] a   [4..6] b   [7 + 3 r + c] b_r * a_c   [16] (ax * ax + ay * ay) + az * az   [17] (double)d2
 *   A source without a correspondence contributes eighteen zeros.
 * Reduction: source i is lane i % 64 of wavefront (i / 64) % 4 of workgroup i / 256 (lanes past n hold zeros). Per term: within a
 * wavefront the xor butterfly v = v + v[lane ^ s] for s = 32, 16, 8, 4, 2, 1 (every lane ends with the same bits), then the
 * workgroup's four wavefronts added in ascending order, (((w0 + w1) + w2) + w3). d_partials double [ceil(n / 256)][18]: one row per
 * workgroup. No atomics: nothing depends on scheduling.
 *
 * UPDATE (acez_geom_icp_update). One workgroup of 256 threads. If status != 0, or [13] is not in 0 .. max_iterations - 1, it returns
 * at once. Totals: thread t adds rows t, t + 256, t + 512, .. in ascending order from 0.0, per term; the 256 threads' sums are reduced
 * as above (butterfly, then wavefronts ascending). Then, in this order (acezero_amd/csrc/icp_solve.h is the text):
 *   count = total[0], fitness = count / n, rmse = sqrt(total[17] / count)
 *   record [13] of d_history (16 doubles each: T (12), count, total[17], fitness, rmse) is written, [13] += 1, the totals are kept
 *   (a) from the second record on: |fitness - previous| < rel_fitness and |rmse - previous| < rel_rmse -> status 1, T unchanged
 *   (b) count < 3, a total that is not finite, or sigma1 <= 1e-12 * sigma0 of the covariance -> status 2, T unchanged
 *   else Umeyama: C = S_ba - S_b S_a^T / count = U diag(sigma) V^T (csrc/svd3.h), R = U diag(1, 1, sign) V^T,
 *     s = (sigma0 + sigma1 + sign * sigma2) / (S_aa - |S_a|^2 / count) with with_scale (a scale that is not positive and finite is
 *     status 2), else 1; Delta(x') = s R (x' - pivot - S_a / count) + S_b / count + pivot; T <- Delta * T in fp64.
 * d_history holds max_iterations records.
 *
 * Asynchronous on `stream`. ACEZ_ERR_INVALID, before anything is launched, for: what NEAREST refuses; n < 1; a null d_src, d_state,
 * d_partials or d_history; a pivot that is not finite; max_iterations < 1; a tolerance that is negative or not finite. */
int acez_geom_icp_accumulate(const float* d_ref, const int32_t* d_ref_index, const int32_t* d_cell_start, int64_t m, float ox, float oy,
                             float oz, float cell, int nx, int ny, int nz, const float* d_src, int64_t n, float radius, float px, float py,
                             float pz, const double* d_state, double* d_partials, void* stream);
int acez_geom_icp_update(const double* d_partials, int64_t n, float px, float py, float pz, int with_scale, double rel_fitness,
                         double rel_rmse, int max_iterations, double* d_state, double* d_history, void* stream);

/* =====================================================================================================
 * O. A mesh scored by its surface: samples of the faces, and the polygon crop (eval_geometry.py --sample_spacing, --crop_file)
 * =====================================================================================================
 * Three stateless entry points; none allocates anything, every buffer is the caller's. d_vertices float32 [m][3], d_faces int32
 * [k][3] (triangles, rows of d_vertices). Everything below is fp64 unless it says otherwise, round to nearest, one rounding per
 * operation in the order written (the unit is built without contraction); the random stream is 64-bit integer arithmetic modulo
 * 2^64 with mix64 of acezero_amd/csrc/ransac_math.h. Nothing depends on scheduling: no atomics and no floating-point sum over
 * faces; every face decides its own number of samples, and the only scan, the exclusive sum of those integers, is the caller's.
 * tests/surface_restated.py restates all of it in numpy.
 *
 * COUNTS (acez_geom_face_counts). Per face t with vertices a, b, c (each component widened to fp64):
 *   e1 = b - a, e2 = c - a
 *   n  = (e1y * e2z - e1z * e2y,  e1z * e2x - e1x * e2z,  e1x * e2y - e1y * e2x)
 *   S  = (nx * nx + ny * ny) + nz * nz,  area = 0.5 * sqrt(S)
 *   The face is INVALID if an index is outside 0 .. m - 1 or area is not finite: d_out_areas[t] = -1.0, d_out_counts[t] = 0.
 *   Otherwise d_out_areas[t] = area and, with `density` in samples per square metre:
 *     x = area * density, f = floor(x)
 *     key_t = mix64(mix64(seed) ^ t),  u0 = (key_t >> 11) * 2^-53
 *     d_out_counts[t] = min(f, 2^30) + (u0 < x - f ? 1 : 0)
 *   so the expected count is x: a face smaller than 1 / density is not lost, it gets a sample with probability x.
 *
 * SAMPLE (acez_geom_sample_faces). d_offsets int64 [k + 1]: the exclusive sums of the counts, d_offsets[0] = 0, d_offsets[k] = n.
 * Per sample j of n:
 *   t = the last face in 0 .. k - 1 with d_offsets[t] <= j (faces without samples are skipped by this rule), i = j - d_offsets[t]
 *   r = mix64(key_t + (i + 1) * 0xD1B54A32D192ED03),  u = (r >> 40) * 2^-24,  v = ((r >> 16) & 0xFFFFFF) * 2^-24
 *   if u + v > 1: u = 1 - u, v = 1 - v        (the fold: uniform over the triangle without a square root)
 *   per axis p = float((a + u * e1) + v * e2), rounded to fp32 once;  d_out_points float32 [n][3], d_out_face int32 [n] = t
 *   with d_colours uint8 [m][3]: d_out_colours uint8 [n][3] = floor((((1 - u) - v) * ca + u * cb) + v * cc + 0.5) per channel,
 *   the sums from left to right. d_colours and d_out_colours are both null or both given.
 * t is clamped to 0 .. k - 1 and every vertex index to 0 .. m - 1 before anything is loaded: d_offsets and d_faces are device data
 * that cannot be checked here, and a wrong table gives wrong numbers, never an access out of bounds.
 *
 * CROP (acez_geom_crop_polygon). The volume of a Tanks and Temples crop file: a polygon swept along a coordinate axis. d_polygon
 * float32 [corners][2]: the corners (U, V) in the plane orthogonal to `axis`; (u, v, w) of a point (x, y, z) is (y, z, x) for axis 0,
 * (x, z, y) for axis 1, (x, y, z) for axis 2. d_out_keep uint8 [n] = 1 iff x, y, z are finite, axis_min <= w <= axis_max (fp32
 * comparisons) and the number of crossings is odd. Edge i -> j = (i + 1) mod corners counts only if (V_i > v) != (V_j > v); then, with
 * everything widened to fp64, lhs = (u - U_i) * (V_j - V_i), rhs = (v - V_i) * (U_j - U_i), and the edge is a crossing if
 * V_j > V_i ? lhs < rhs : lhs > rhs. The half-open rule counts a corner once; an edge along u never counts.
 *
 * Asynchronous on `stream`. ACEZ_ERR_INVALID, before anything is launched, for: a null pointer (an array whose count is 0 may be
 * null), a negative count or one >= 2^31, a density that is not positive and finite, samples (n > 0) of a mesh with m = 0 or k = 0,
 * only one of d_colours / d_out_colours, corners outside 3 .. 1024, an axis outside 0 .. 2, axis bounds that are not finite or
 * axis_min > axis_max. */
int acez_geom_face_counts(const float* d_vertices, int64_t m, const int32_t* d_faces, int64_t k, double density, uint64_t seed,
                          int32_t* d_out_counts, double* d_out_areas, void* stream);
int acez_geom_sample_faces(const float* d_vertices, int64_t m, const int32_t* d_faces, int64_t k, const int64_t* d_offsets, int64_t n,
                           uint64_t seed, const uint8_t* d_colours, float* d_out_points, int32_t* d_out_face, uint8_t* d_out_colours,
                           void* stream);
int acez_geom_crop_polygon(const float* d_points, int64_t n, const float* d_polygon, int corners, int axis, float axis_min,
                           float axis_max, uint8_t* d_out_keep, void* stream);

/* =====================================================================================================
 * P. A mesh without its floating fragments: connected components (clean_mesh.py, fuse_depth.py --min_component_faces ..)
 * =====================================================================================================
 * Four stateless entry points; none allocates anything, every buffer is the caller's. d_faces int32 [k][3] (triangles), m the number
 * of vertices. Everything is integer arithmetic, and the result is a function of the mesh alone: no floating-point sum, nothing that
 * depends on scheduling. Connectivity is by index: two vertices with the same coordinates are two vertices (no welding). Surface area
 * per component is not computed: a sum over a component's faces has no fixed order without a sort. tests/mesh_restated.py restates
 * all of it in numpy.
 *
 * Terms. A face is INVALID if an index lies outside 0 .. m - 1, and DEGENERATE if it is not invalid and two of its indices are
 * equal. Invalid and degenerate faces connect nothing and are never kept; every other face is VALID. Two vertices are connected if a
 * valid face holds both; the components are the transitive closure. label[v] is the SMALLEST vertex id of v's component; a vertex in
 * no valid face is its own label. A face's component is the label of its first vertex. A component EXISTS if it has at least one
 * valid face.
 *
 * COMPONENTS (acez_mesh_components). d_labels int32 [m] = label[]; d_status int32 [1] is cleared, and set to a value other than 0
 * only if one of the bounded loops below ran out, which no input can cause (the caller reads it with the counts and refuses the
 * result). A lock-free union-find in three launches, d_labels serving as parent[]:
 *   init     parent[v] = v
 *   hook     one thread per valid face (a, b, c) unites (a, b) and (b, c): find both roots, compare-and-swap the LARGER root under
 *            the SMALLER (expecting the larger to be a root still), and on failure start again from the new roots. parent[v] <= v
 *            always and only ever decreases (a find also replaces parent[v] by the minimum of itself and v's grandparent), so the
 *            smallest vertex of a component never gets a parent and the one root left is that vertex. Every access to parent[] in
 *            this launch is a relaxed agent-scope atomic: a plain load can be served from another XCD's stale line.
 *   flatten  label[v] = the root of v, in place, plain loads (after the kernel boundary).
 * A walk descends strictly: fewer than m steps. A compare-and-swap fails only because another thread linked that root, which
 * happens once per vertex: at most m failures. Both loops stop after m + 1 trips and set *d_status; no thread waits for another.
 *
 * COUNTS (acez_mesh_component_counts). d_faces_of, d_vertices_of int32 [m], cleared here: faces_of[c] = the number of valid faces
 * whose component is c; vertices_of[c] = the number of vertices with label c if component c exists; 0 everywhere else (so a vertex
 * in no valid face counts nowhere). Integer atomic adds; where a wavefront's active lanes share a label, one lane adds their number.
 *
 * Selection (the caller's, acezero_amd/mesh.py with torch operations on the device; all criteria conjunctive, each off by default):
 * rank the existing components by faces_of descending, ties by the smaller label (a stable descending sort over ascending labels).
 * Component c is kept iff faces_of[c] >= min_faces, and (double)faces_of[c] >= min_ratio * (double)(largest faces_of), one fp64
 * product, and rank[c] < keep_largest.
 *
 * SELECT (acez_mesh_select), flag mode. d_keep_component uint8 [m] (indexed by label). d_face_keep uint8 [k] = 1 iff the face is
 * valid and its component is kept, else 0; d_vertex_used uint8 [m] is cleared here and set to 1 (plain byte stores) for the three
 * vertices of every kept face.
 *
 * COMPACT (acez_mesh_compact), scatter mode. d_face_rank int32 [k] and d_vertex_rank int32 [m] are the inclusive sums of the two flag
 * arrays (the caller's), n_faces and n_vertices their last entries. Kept face t goes to row d_face_rank[t] - 1 of d_out_faces int32
 * [n_faces][3] with every index v renamed to d_vertex_rank[v] - 1; used vertex v goes to row d_vertex_rank[v] - 1 of d_out_vertices
 * float32 [n_vertices][3] (the bits are copied) and, with d_colours uint8 [m][3], of d_out_colours uint8 [n_vertices][3]. So the
 * kept faces and the vertices they use keep their original order, and unreferenced vertices disappear. d_colours and d_out_colours
 * are both null or both given.
 *
 * Every index formed from device data (a face's vertices, a label, a rank) is range-checked before it is used as an address: a row
 * outside the output is not written, an index that cannot be renamed becomes -1; wrong tables give wrong numbers, never an access
 * out of bounds.
 *
 * Asynchronous on `stream`. ACEZ_ERR_INVALID, before anything is launched, for: a null pointer (an array whose count is 0 may be
 * null; d_status never), a negative count or one >= 2^31, n_vertices > m or n_faces > k, only one of d_colours / d_out_colours. */
int acez_mesh_components(const int32_t* d_faces, int64_t k, int64_t m, int32_t* d_labels, int32_t* d_status, void* stream);
int acez_mesh_component_counts(const int32_t* d_faces, int64_t k, const int32_t* d_labels, int64_t m, int32_t* d_faces_of,
                               int32_t* d_vertices_of, void* stream);
int acez_mesh_select(const int32_t* d_faces, int64_t k, const int32_t* d_labels, int64_t m, const uint8_t* d_keep_component,
                     uint8_t* d_face_keep, uint8_t* d_vertex_used, void* stream);
int acez_mesh_compact(const float* d_vertices, const uint8_t* d_colours, int64_t m, const int32_t* d_faces, int64_t k,
                      const uint8_t* d_face_keep, const int32_t* d_face_rank, const uint8_t* d_vertex_used, const int32_t* d_vertex_rank,
                      float* d_out_vertices, uint8_t* d_out_colours, int64_t n_vertices, int32_t* d_out_faces, int64_t n_faces,
                      void* stream);

/* =====================================================================================================
 * Q. A mesh with fewer faces: quadric vertex clustering (simplify_mesh.py, fuse_depth.py --simplify_cell)
 * =====================================================================================================
 * Six stateless entry points; none allocates anything, every buffer is the caller's. The stable sorts, the prefix sums and the
 * segment searches between them are the caller's (acezero_amd/simplify.py, torch on the device), the compaction at the end is section
 * P's acez_mesh_compact. The output is a function of the input alone: every floating-point sum has the fixed order given below.
 * Steps 4 - 6 compute in fp64, one rounding per operation (the unit is compiled with -ffp-contract=off), and every result is rounded
 * to fp32 once, at the end. tests/simplify_restated.py restates all of it in numpy, bit for bit.
 *
 * Input: vertices float32 [m][3], colours uint8 [m][3] or none, faces int32 [k][3], cell > 0 (float32), placement quadric or mean.
 *
 * 1 CELLS. A vertex is FINITE if its three coordinates are. origin = the component-wise minimum of the finite vertices, max their
 *   component-wise maximum (fp32; the caller's). The cell of a finite vertex p is floor((p - origin) / cell) per axis, in fp32, one
 *   rounding per operation; a vertex that is not finite has no cell. An axis may have at most 2^21 - 1 cells (the limits of section N
 *   are too small for a room at 1 cm). The key of a cell is x | y << 21 | z << 42 in an int64; a vertex without a cell has the key
 *   2^63 - 1.
 * 2 CLUSTERS. The occupied cells in ascending key order are the clusters 0 .. K - 1. A cluster's vertices are taken in ascending
 *   vertex id (a stable sort of the keys).
 * 3 FACES THAT COUNT. A face is INVALID if an index lies outside 0 .. m - 1 or, with all indices in range and pairwise different, a
 *   vertex of it has no cell; DEGENERATE if its indices are in range and two are equal; VALID otherwise. Only valid faces enter the
 *   steps below.
 * 4 MEAN. mean = (the fp64 sum of the cluster's vertices, each converted to fp64, added one by one to 0.0 in the order of step 2)
 *   / (double)count. The colour is, per channel, (2 sum + count) / (2 count) in integers.
 * 5 QUADRIC. Every corner of every valid face contributes its face's plane quadric to the cluster of that corner's vertex (a face
 *   with two corners in one cluster contributes to it twice). centre = (double)origin + ((double)index + 0.5) * (double)cell per axis
 *   is the cluster's cell centre. For the face (a, b, c), its vertices converted to fp64 and the centre subtracted:
 *   n = (b - a) x (c - a), each component p * q - r * s, unnormalised (the weight is |n|^2 = 4 area^2); d = -((n0 a0 + n1 a1) + n2 a2);
 *   the nine terms n0 n0, n0 n1, n0 n2, n1 n1, n1 n2, n2 n2 (A, symmetric) and d n0, d n1, d n2 (b) are each added to their running
 *   sum, which starts at 0.0. THE ORDER: let the cluster's corners stand in ascending 3 face + corner (a stable sort of the corners
 *   by cluster) at positions 0, 1, .. of its segment. One wavefront takes the cluster: lane l (0 .. 63) adds the corners at positions
 *   l, l + 64, l + 128, .. one by one to its own nine sums (all 0.0 for a lane without a corner); then, for s = 32, 16, 8, 4, 2, 1,
 *   every lane l replaces each of its sums by itself + the sum of lane l xor s (an addition commutes, so all lanes hold the same
 *   bits); the result is lane 0's. Chosen by measurement over one thread per cluster walking the whole segment serially, which is
 *   two to three times slower on fused rooms (tools/simplify_timing.py).
 * 6 PLACEMENT (acezero_amd/csrc/simplify_solve.h). mean: the vertex is the mean. quadric: with r = mean - centre, decompose A with
 *   svd3 (acezero_amd/csrc/svd3.h: A = U diag(s) V^T, fixed sweep order and cap); g_j = -b_j - ((A_j0 r0 + A_j1 r1) + A_j2 r2);
 *   y = r; for i = 0, 1, 2 with s_i > 1e-3 * s_0: y_j = y_j + v_i[j] * (((v_i[0] g0 + v_i[1] g1) + v_i[2] g2) / s_i) (rank 1 on a
 *   wall, 2 on an edge, 3 at a corner). The vertex is centre + y, unless s_0 > 0 does not hold (A is zero), or a y_j is not finite,
 *   or |y_j| > cell: then it is the mean (a FALLBACK). Either way one rounding to fp32.
 * 7 OUTPUT FACES. A valid face is mapped to the clusters of its vertices. It is COLLAPSED if two of the three are equal, else a
 *   candidate: rotated so that its smallest cluster comes first (the orientation stays; (a, b, c) and (a, c, b) are different
 *   faces). Of the candidates with the same rotated triple only the one with the lowest input index survives, the others are
 *   DUPLICATES. The output faces are the surviving rotated triples in input order.
 * 8 OUTPUT VERTICES. The clusters that no output face uses are dropped, the others keep their order, and the faces are renumbered.
 *
 * KEYS (acez_simplify_keys). d_keys int64 [m] = the keys of step 1. Refused before anything is launched if an axis would have 2^21
 *   or more cells: floor((max - origin) / cell) + 1 >= 2^21, or not finite.
 * CLUSTERS (acez_simplify_clusters). d_order int64 [m]: the stable ascending sort of the keys; d_cluster_sorted int32 [m]: for every
 *   sorted position its cluster (the number of different keys before it), m where the key is 2^63 - 1. d_vertex_cluster int32 [m]
 *   = the cluster of every vertex, -1 without a cell.
 * FACES (acez_simplify_faces). d_face_class uint8 [k]: 0 invalid, 1 degenerate, 2 collapsed, 3 candidate. d_triples int32 [k][3]: a
 *   candidate's rotated triple, (m, m, m) for every other face. d_corner_keys int32 [3 k]: the cluster of corner 3 t + c of a valid
 *   face t, m for the corners of the others, so that a stable sort puts every cluster's corners in the order of step 5.
 * QUADRICS (acez_simplify_quadrics). d_sorted_keys int64 [m] the sorted keys, d_segments int64 [m + 1]: cluster c's vertices stand
 *   at the sorted positions d_segments[c] .. d_segments[c + 1] - 1 (an empty range past the last cluster); d_corner_order int64 [3 k]
 *   the stable ascending sort of the corner keys and d_corner_segments int64 [m + 1] likewise. Row c of d_out_quadrics double [m][9]
 *   = the nine sums of step 5 (A: xx, xy, xz, yy, yz, zz; b: x, y, z) for every cluster c, and no other row is written.
 * PLACE (acez_simplify_place). d_sorted_keys, d_order, d_segments as above; d_quadrics the sums of QUADRICS, or null for the mean
 *   placement. Row c of d_out_vertices float32 [m][3], d_out_colours uint8 [m][3] (null iff d_colours is) and d_out_fallback uint8
 *   [m] (1: a fallback) is written for every cluster c and for no other row.
 * UNIQUE (acez_simplify_unique). d_perm int64 [k]: the faces sorted by their triples (first, second, third), equal triples in input
 *   order (two stable sorts: by the third, then by first * (m + 1) + second). d_face_keep uint8 [k] = 1 for the surviving candidates,
 *   else 0; d_cluster_used uint8 [m] is cleared and set to 1 (plain byte stores) for the clusters of the surviving faces.
 * Then acez_mesh_compact on (d_out_vertices, d_out_colours, m, d_triples, k, d_face_keep, d_cluster_used and their inclusive sums).
 *
 * No kernel waits on anything: no atomics, no loop that is not bounded by a segment length, by m or by svd3's sweep cap. Every index formed
 * from device data is range-checked before it is used as an address: wrong tables give wrong numbers, never an access out of bounds.
 *
 * Asynchronous on `stream`. ACEZ_ERR_INVALID, before anything is launched, for: a null pointer (an array whose count is 0 may be
 * null), a negative count or one >= 2^31, a cell that is not positive and finite, bounds that are not finite or not ordered, the
 * limit of 2^21 cells per axis, only one of d_colours / d_out_colours. */
int acez_simplify_keys(const float* d_vertices, int64_t m, float origin_x, float origin_y, float origin_z, float max_x, float max_y,
                       float max_z, float cell, int64_t* d_keys, void* stream);
int acez_simplify_clusters(const int64_t* d_order, const int32_t* d_cluster_sorted, int64_t m, int32_t* d_vertex_cluster, void* stream);
int acez_simplify_faces(const int32_t* d_faces, int64_t k, const int32_t* d_vertex_cluster, int64_t m, uint8_t* d_face_class,
                        int32_t* d_triples, int32_t* d_corner_keys, void* stream);
int acez_simplify_quadrics(const float* d_vertices, int64_t m, const int32_t* d_faces, int64_t k, const int64_t* d_sorted_keys,
                           const int64_t* d_segments, const int64_t* d_corner_order, const int64_t* d_corner_segments, float origin_x,
                           float origin_y, float origin_z, float cell, double* d_out_quadrics, void* stream);
int acez_simplify_place(const float* d_vertices, const uint8_t* d_colours, int64_t m, const int64_t* d_sorted_keys, const int64_t* d_order,
                        const int64_t* d_segments, const double* d_quadrics, float origin_x, float origin_y, float origin_z, float cell,
                        float* d_out_vertices, uint8_t* d_out_colours, uint8_t* d_out_fallback, void* stream);
int acez_simplify_unique(const int32_t* d_triples, const uint8_t* d_face_class, const int64_t* d_perm, int64_t k, int64_t m,
                         uint8_t* d_face_keep, uint8_t* d_cluster_used, void* stream);

/* =====================================================================================================
 * R. A mesh seen from the frames' cameras: model depth, face ids, normals and colours per pixel (render_mesh.py, fuse_depth.py --model_depth_dir)
 * =====================================================================================================
 * A triangle mesh is rasterised into every frame of a table: d_vertices float32 [n_vertices][3] (world, OpenCV convention), d_faces
 * int32 [n_faces][3], d_colours uint8 [n_vertices][3] (optional), and a HOST table of n_frames acez_tsdf_frame rows as in section K
 * (m[12] = the 3 x 4 world -> camera rows, focal, ppx, ppy in pixels of THIS frame, h, w, and `offset`: the element index of the
 * frame's pixel (0, 0) in every per-pixel buffer of the call). Frames of different sizes share a call. Camera and pixel convention
 * are section K's: the pixel index is the image coordinate, so the sample of pixel (ix, iy) is the point (ix, iy) (not + 1/2), and a
 * map rendered here and integrated by acez_tsdf_integrate under the same row is read, for a point of the surface, at the pixel it was
 * rendered into. Coverage and depth are section H's rules in this camera. All float arithmetic is fp32, round to nearest, one
 * rounding per operation in the order written (the unit is built without contraction), division is IEEE division.
 * tests/meshrender_restated.py restates all of it in numpy.
 *
 * Per frame and face t (its id) with the vertices P0, P1, P2 in the face's order:
 *   1. c_k = (xc, yc, zc):  xc = ((m0 * px + m1 * py) + m2 * pz) + m3      (yc from m4..m7, zc from m8..m11). A c_k with a component
 *      that is not finite drops the triangle.
 *   2. near plane: vertex k is IN if zc >= min_depth. None in: dropped. All in: the triangle (c_0, c_1, c_2). Else Sutherland-Hodgman
 *      over the edges (0,1), (1,2), (2,0): an IN vertex is emitted, and an edge whose ends differ emits, with a the IN end and b the other,
 *      t = (min_depth - a.z) / (b.z - a.z), (a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), min_depth). The 3 or 4 points q_0 .. are
 *      drawn as the triangles (q_0, q_1, q_2) and (q_0, q_2, q_3), both under the id t.
 *   3. per triangle and vertex: a = (focal * x) / z, b = (focal * y) / z; unless |a| < 2^21 and |b| < 2^21 for all three the triangle
 *      is dropped BY THE GUARD. u = a + ppx, v = b + ppy, iz = 1 / z; X = int64(rintf(u * 256)), Y alike (ties to even).
 *   4. area = E(0, 1; 2) with E(a, b; p) = (X_p - X_a) * (Y_b - Y_a) - (Y_p - Y_a) * (X_b - X_a). Zero: dropped. Negative: vertices 1
 *      and 2 change places (X, Y and iz) and area = -area: both windings are drawn.
 *   5. box: x from max(0, ceil(min X / 256)) to min(w - 1, floor(max X / 256)), y alike with h; empty: dropped.
 *   6. per pixel (ix, iy) of the box, S = (256 ix, 256 iy): w0 = E(1, 2; S), w1 = E(2, 0; S), w2 = E(0, 1; S). Covered if none is
 *      negative and every zero one belongs to an OWNED edge (a, b): Y_b - Y_a > 0, or Y_b == Y_a and X_b - X_a < 0 (top-left rule).
 *   7. invd = ((float(w0) * iz_0 + float(w1) * iz_1) + float(w2) * iz_2) / float(area), d = 1 / invd; dropped unless d <= max_depth.
 *   8. key = (bits of d) << 32 | t; the pixel keeps the smallest key: the nearest face, and of equal depths the lower id.
 * The image is a function of the mesh and the table alone: no ordering of the atomics enters it.
 *
 * Outputs, each packed by the rows' offsets, each but d_depth optional (NULL). With the winning key's d and t:
 *   d_depth      float32   d; 0 where no face was hit
 *   d_face       int32     t; -1 where no face was hit
 *   d_depth_u16  uint16    q = rintf(d / depth_unit) if q <= 65535, else 0; 0 where no face was hit (the project's depth PNG)
 *   d_normal     uint8 x 3 with c_0, c_1, c_2 of step 1 (the unclipped face), A = c_1 - c_0, B = c_2 - c_0, n = A x B (each component
 *                two products and one difference: Ay * Bz - Az * By, Az * Bx - Ax * Bz, Ax * By - Ay * Bx), the pixel's ray
 *                r = (float(ix) - ppx, float(iy) - ppy, focal): n is negated if (n.x * r.x + n.y * r.y) + n.z * r.z > 0 (it then faces
 *                the camera); len = float(sqrt(double((n.x * n.x + n.y * n.y) + n.z * n.z))); component c -> 128 + rintf((c / len) * 127),
 *                clamped to 1 .. 255. (128, 128, 128) if len is 0 or infinite; (0, 0, 0) where no face was hit
 *   d_colour     uint8 x 3 C_k = c_(k+1) x c_(k+2) (indices mod 3, components as above), e_k = (r.x * C_k.x + r.y * C_k.y) + r.z * C_k.z,
 *                D = (e_0 + e_1) + e_2; per channel m = ((e_0 * float(col_0) + e_1 * float(col_1)) + e_2 * float(col_2)) / D, then
 *                min(floorf(m + 0.5), 255), 0 if that is negative or not a number. The barycentrics come from the unclipped vertices
 *                (section H's textured path), so near-plane clipping does not change them. (0, 0, 0) where no face was hit
 *   d_status     int32 [1] the triangle-frames dropped by the guard of step 3 (a clipped triangle counts once). Not zero: the image
 *                may have a hole there; callers log a warning. Guard-band clipping against the side planes is not done.
 *
 * Work distribution (acezero_amd/csrc/meshrender_api.hip). One lane per face keeps the face's world vertices in
 * registers over the frames its block walks. Per frame the largest box (step 5) of the face's one or two triangles picks the route:
 * at most ACEZ_MESHRENDER_SMALL samples and not clipped: the lane walks the box itself; at most ACEZ_MESHRENDER_LARGE samples, or
 * clipped: the lane's wavefront walks it with 64 lanes; more: the workgroup walks it with 256 threads. All routes run the same
 * steps 2-8, so the route changes no key.
 *
 * acez_meshrender: d_keys uint64 [n_keys] scratch (one key per pixel of the call), the planes of n_pixels elements (x 3 for normal and
 * colour), d_frames device scratch of n_frames rows: all the caller's; nothing is allocated. The table is checked here and copied into
 * d_frames on `stream`; the copy has completed when the call returns, everything else is asynchronous. n_frames = 0 does nothing;
 * n_faces = 0 clears the planes. A face with an index outside 0 .. n_vertices - 1 is passed over by the kernels, which therefore form
 * no index outside their buffers whatever d_faces holds; since the faces live in device memory, refusing such a mesh is
 * acez_meshrender_check_faces' part, on a host copy of the faces (host only, no device needed): acezero_amd.meshrender calls it, or
 * the same test on the device, before it renders.
 * ACEZ_ERR_INVALID, before anything is launched, for: a null d_keys, d_depth, d_status, frame table or (with faces) d_faces or
 * d_vertices; a colour plane without vertex colours; counts outside 0 .. 2^31 - 1; min_depth, max_depth or depth_unit not positive and
 * finite; n_frames outside 0 .. 256; a row section K refuses, with offset + h * w beyond n_pixels or n_keys; |ppx| or |ppy| > 2^20
 * (with the guard that keeps the int64 edge functions below 2^63). */
#define ACEZ_MESHRENDER_SMALL 16      /* samples in the box up to which a lane walks it alone */
#define ACEZ_MESHRENDER_LARGE 1024    /* samples in the box above which the workgroup walks it */
int acez_meshrender_check_faces(const int32_t* h_faces, int64_t n_faces, int64_t n_vertices);
int acez_meshrender(const float* d_vertices, const uint8_t* d_colours, int64_t n_vertices, const int32_t* d_faces, int64_t n_faces,
                    const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames, float min_depth, float max_depth,
                    float depth_unit, unsigned long long* d_keys, int64_t n_keys, float* d_depth, int32_t* d_face, uint16_t* d_depth_u16,
                    uint8_t* d_normal, uint8_t* d_colour, int64_t n_pixels, int32_t* d_status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACEZ_H */
