/* omnisafe_amd.h -- C ABI of libomnisafe_amd.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE hot path of PKU-Alignment/omnisafe: on-policy rollout ->
 * VectorOnPolicyBuffer (dual reward+cost GAE) -> PPOLag / TRPOLag / CPO update.
 * The reference has no FFI for this path (it is pure Python on torch); each
 * entry point below therefore cites the reference Python function whose arithmetic it replaces
 * (paths relative to the reference repository root).  The Python host side (the omnisafe_amd package) binds
 * these symbols with ctypes and mirrors the reference's classes; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _host; the caller owns all memory;
 *    nothing is allocated or freed inside the library;
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream); all calls are
 *    asynchronous w.r.t. the host and never synchronise;
 *  - return value: 0 = OSA_OK, negative = error (osa_strerror); no exceptions cross the boundary;
 *  - all floating point data is IEEE float32 unless declared double; flags are uint8;
 *  - the (T, N) rollout buffer is TIME-MAJOR: element (t, n) of a per-step scalar lives at [t*N + n],
 *    rows of obs/act at [(t*N + n) * ld].  VectorOnPolicyBuffer.get()'s ENV-MAJOR order
 *    (sample i = n*T + t, omnisafe/common/buffer/vector_onpolicy_buffer.py:125-129) is produced by
 *    osa_buffer_get.
 *  - one host thread per device context (the reference is single-threaded per rank).
 */
#ifndef OMNISAFE_AMD_H
#define OMNISAFE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSA_OK 0
#define OSA_EINVAL (-1)       /* bad argument (null pointer, non-positive size, unsupported dims) */
#define OSA_EHIP (-2)         /* a HIP runtime call / kernel launch failed */
#define OSA_EUNSUPPORTED (-3) /* valid in the reference, not implemented here (yet) */

/* advantage estimators: omnisafe/common/buffer/onpolicy_buffer.py:299-331 */
#define OSA_EST_GAE 0
#define OSA_EST_GAE_RTG 1
#define OSA_EST_PLAIN 2
#define OSA_EST_VTRACE 3 /* onpolicy_buffer.py:312-326 -> _calculate_v_trace :338-405; the reference passes
                            the same probabilities as policy and behaviour, i.e. rho = c = 1 */

const char* osa_strerror(int code);
int osa_version(void);            /* ABI version, currently 1 */
const char* osa_build_arch(void); /* "gfx950" */
/* sha256 (first 32 hex digits) of this header and of the kernel sources the library was built from; the
 * Python binding refuses a library whose digest differs from the sources next to it. */
const char* osa_abi_digest(void);

/* ------------------------------------------------------------------------------------------------
 * Rollout buffer (replaces omnisafe/common/buffer/{onpolicy_buffer,vector_onpolicy_buffer}.py)
 * ---------------------------------------------------------------------------------------------- */

/* VectorOnPolicyBuffer.store (vector_onpolicy_buffer.py:96-99 -> onpolicy_buffer.py:143-146):
 * copies the 7 per-step fields of all N envs into row t of the time-major buffer.  obs/act rows
 * have obs_dim/act_dim valid floats and leading dimensions ld_src (source) / ld_buf (buffer). */
int osa_buffer_store_step(int t, int N, int obs_dim, int act_dim,
                          const float* obs, int ld_obs_src, const float* act, int ld_act_src,
                          const float* reward, const float* cost, const float* value_r,
                          const float* value_c, const float* logp,
                          float* buf_obs, int ld_obs_buf, float* buf_act, int ld_act_buf,
                          float* buf_reward, float* buf_cost, float* buf_value_r, float* buf_value_c,
                          float* buf_logp, void* stream);

/* OnPolicyBuffer.finish_path for every path of every env in ONE backward sweep
 * (onpolicy_buffer.py:170-203, _calculate_adv_and_value_targets :299-331, discount_cumsum
 * omnisafe/utils/math.py:76-82).  path_end[t*N+n] != 0 marks the last step of a path whose bootstrap
 * values boot_r/boot_c[t*N+n] are the arguments finish_path(last_value_r, last_value_c, idx=n)
 * received.  Arithmetic is the reference's exactly: delta in float32 (float32-rounded gamma,
 * separately rounded mul/add/sub), recurrences in float64 with unfused multiply-add, results rounded
 * to float32 on store -> bit-exact.  Outputs are time-major (T, N). */
int osa_gae_scan(const float* reward, const float* cost, const float* value_r, const float* value_c,
                 const uint8_t* path_end, const float* boot_r, const float* boot_c, int T, int N,
                 double gamma, double lam, double lam_c, float penalty_coef, int estimator,
                 float* adv_r, float* adv_c, float* target_value_r, float* target_value_c,
                 float* discounted_ret, void* stream);

/* The same sweep parallel over TIME -- the wavefront backward scan with LDS staging: a workgroup owns 16
 * consecutive envs, walks the time axis backwards in tiles of 64 steps staged in LDS with coalesced row
 * segments, and scans each env's 64 steps across the 64 lanes of a wave (Hillis-Steele scan of the affine
 * maps y_t = x_t + c_t y_{t+1}, carries chained from tile to tile).  For few envs / long horizons (e.g.
 * vector_env_nums = 4, T = 5000) where osa_gae_scan leaves the chip idle; the caller picks by (T, N).
 * Same float32 deltas; the float64 recurrences are associated as a tree instead of a chain, so outputs equal
 * osa_gae_scan's to float64 rounding before the final float32 rounding (tests: rtol 1e-5).  Estimators gae,
 * gae-rtg, plain (v-trace is a float32 chain: OSA_EUNSUPPORTED, use osa_gae_scan).
 * Replaces: the same reference code as osa_gae_scan. */
int osa_gae_scan_tiled(const float* reward, const float* cost, const float* value_r, const float* value_c,
                       const uint8_t* path_end, const float* boot_r, const float* boot_c, int T, int N,
                       double gamma, double lam, double lam_c, float penalty_coef, int estimator,
                       float* adv_r, float* adv_c, float* target_value_r, float* target_value_c,
                       float* discounted_ret, void* stream);
/* The same scan SPLIT OVER TIME across workgroups (csrc/buffer_kernels.hip K5c, round 3): levels of 128 steps, a
 * wave = 64 envs x 16 steps with its inputs in registers, per-env carries chained between levels by a decoupled
 * look-back (8-byte agent-scope words in `ws`; a level that contains a path end publishes its carry at once, so
 * chains end at episode boundaries).  (T / 16) x (N / 64) waves whatever the shape: the large-N / long-T buffers
 * where osa_gae_scan has too few lanes in flight and osa_gae_scan_tiled pays its log-depth scan.  Arithmetic: the
 * sequential kernel's step for step given the incoming carry; the carry is assembled by the affine identity
 * (float64 re-association): same tolerance class as osa_gae_scan_tiled, deterministic (independent of timing).
 * ws: osa_gae_chained_ws_doubles(T, N) doubles; the carries and the ticket are initialised by every call, the LAST
 * double is a sticky time-out word the caller zeroes ONCE after allocation: a lane that gives up waiting for a
 * carry (bounded spin: a device shared with / preempted by another long-running kernel) sets it and its outputs
 * are NaN -- osa_gae_chained_timed_out(ws, T, N, &flag) reads it (synchronous 4-byte copy; 0 = fine), which the
 * caller does at its next host synchronisation.  v-trace: OSA_EUNSUPPORTED. */
size_t osa_gae_chained_ws_doubles(int T, int N);
int osa_gae_chained_timed_out(const double* ws, int T, int N, int* out);
int osa_gae_scan_chained(const float* reward, const float* cost, const float* value_r, const float* value_c,
                         const uint8_t* path_end, const float* boot_r, const float* boot_c, int T, int N,
                         double gamma, double lam, double lam_c, float penalty_coef, int estimator,
                         float* adv_r, float* adv_c, float* target_value_r, float* target_value_c,
                         float* discounted_ret, double* ws, void* stream);

/* Advantage statistics of VectorOnPolicyBuffer.get (vector_onpolicy_buffer.py:131-136 ->
 * omnisafe/utils/distributed.py:382-392), split in two phases so the cross-rank all-reduce (RCCL) can
 * sit between them.  stats is 8 doubles on the device:
 *   [0] sum(adv_r) [1] sum(adv_c) [2] n   -- written by phase 1 (local); all-reduce(SUM) [0..2]
 *   [3] sum((adv_r - mean_r)^2)            -- written by phase 2 (local); all-reduce(SUM) [3]
 *   [4] mean_r [5] mean_c (float32-rounded, as the reference's float32 tensors) -- phase 2
 *   [6] std_r = sqrt([3]/[2]) rounded to float32 -- written by osa_buffer_get
 * ws: workspace of at least osa_reduce_ws_bytes() bytes. */
size_t osa_reduce_ws_bytes(void);
int osa_adv_stats_phase1(const float* adv_r, const float* adv_c, long M, double* ws, double* stats,
                         void* stream);
int osa_adv_stats_phase2(const float* adv_r, long M, double* ws, double* stats, void* stream);

/* VectorOnPolicyBuffer.get (vector_onpolicy_buffer.py:113-138): time-major (T,N) -> env-major (N*T)
 * copy of the 8 returned tensors with adv_r <- (adv_r - mean)/(std + 1e-8) if standardize_r and
 * adv_c <- adv_c - mean_c if standardize_c.  Any source/destination pair may be NULL (skipped). */
int osa_buffer_get(int T, int N, int obs_dim, int act_dim,
                   const float* obs, int ld_obs, const float* act, int ld_act, const float* logp,
                   const float* target_value_r, const float* target_value_c, const float* adv_r,
                   const float* adv_c, const float* discounted_ret, double* stats,
                   int standardize_r, int standardize_c,
                   float* out_obs, int ld_out_obs, float* out_act, int ld_out_act, float* out_logp,
                   float* out_target_value_r, float* out_target_value_c, float* out_adv_r,
                   float* out_adv_c, float* out_discounted_ret, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Actor-critic networks (replaces the torch modules + optimisers of
 * omnisafe/models/actor_critic/{actor_critic,constraint_actor_critic}.py on this path)
 *
 * Three MLPs obs_dim -> H -> H -> {act_dim | 1 | 1} (omnisafe/utils/model.py:73-111).  The `hidden` argument of
 * every entry point carries the width H in its low 16 bits (hidden_sizes [H, H]: 64 = every on-policy YAML
 * default; 32, 128 and 256 on the per-step entry points; anything else: OSA_EUNSUPPORTED) and the hidden
 * activation in bits 16-19 (model_cfgs.*.activation,
 * utils/model.py:47-70): 0 tanh (default: `hidden = 64`), 1 relu, 2 sigmoid, 3 softplus, 4 identity.  The per-step
 * entry points (policy step, minibatch, KL, evaluation, Fisher-vector product) implement all five; the persistent
 * passes (osa_ppo_pass / _wide_ / _split_ / _dp_ / _chunked_) are 64-wide tanh only and report 0 from their *_supported
 * probes for anything else, which routes the update to the per-step entry points.  Each network's parameters, Adam moments and
 * gradients live in one PADDED float32 block of P floats described by osa_mlp_layout:
 *   W1 [H][INP] | b1 [H] | W2 [H][H] | b2 [H] | W3 [OUTP][H] | b3 [OUTP] | log_std [OUTP]
 * (INP/OUTP = obs_dim / max(act_dim,1) rounded up to 16; padding is zero and stays zero).  The three
 * blocks are stored back to back: params[3][P] = actor, reward critic, cost critic.  Conversion to
 * the reference's state_dict tensors / flat-parameter order (omnisafe/utils/tools.py:35-129) is an
 * index map built from osa_mlp_layout on the host.
 * ---------------------------------------------------------------------------------------------- */

/* out12 = {INP, OUTP, oW1, ob1, oW2, ob2, oW3, ob3, oLS, P, H, KB} (offsets in floats). */
int osa_mlp_layout(int obs_dim, int act_dim, int hidden, int* out12);

/* ConstraintActorCritic.step (constraint_actor_critic.py:102-109; GaussianLearningActor.predict /
 * log_prob gaussian_learning_actor.py:81-129; VCritic.forward v_critic.py:89-92) for N observation
 * rows: act = mean + exp(log_std) * eps (or mean if deterministic), logp = sum_d Normal.log_prob,
 * value_r, value_c.  eps: optional external standard-normal noise [N][act_dim] (parity tests);
 * when NULL the kernel draws Philox4x32-10 + Box-Muller normals keyed by (seed, offset + *offset_base, row,
 * dim).  offset_base (device pointer, may be NULL = 0) is the part of the stream position that lives in
 * device memory: a captured hipGraph of a whole rollout replays with frozen by-value offsets 1..T and the
 * caller advances *offset_base by T between replays.
 * nets_mask: bit0 actor, bit1 reward critic, bit2 cost critic (bootstrap calls need critics only).
 * Any output pointer may be NULL.  mean_out optionally receives the distribution mean. */
int osa_policy_step(int obs_dim, int act_dim, int hidden, const float* params, const float* obs,
                    int ld_obs, int N, const float* eps, unsigned long long seed,
                    unsigned long long offset, const unsigned long long* offset_base, int deterministic,
                    int nets_mask, float* act, int ld_act, float* value_r, float* value_c, float* logp,
                    float* mean_out, int ld_mean, void* stream);

/* osa_policy_step with ActionScale.step (omnisafe/envs/wrapper.py:510-514) applied to the sampled action in the same
 * launch: act_env[n][d] = old_min[d] + (old_max[d] - old_min[d]) * (act[n][d] - min_action) / (max_action - min_action)
 * -- the bits of osa_action_scale on the same action.  act_env may be NULL (then exactly osa_policy_step). */
int osa_policy_step_scaled(int obs_dim, int act_dim, int hidden, const float* params, const float* obs,
                           int ld_obs, int N, const float* eps, unsigned long long seed,
                           unsigned long long offset, const unsigned long long* offset_base, int deterministic,
                           int nets_mask, float* act, int ld_act, float* value_r, float* value_c, float* logp,
                           float* mean_out, int ld_mean, float* act_env, int ld_env, const float* old_min,
                           const float* old_max, float min_action, float max_action, void* stream);

/* Hyper-parameters of one optimiser step; field names follow algo_cfgs / model_cfgs of
 * omnisafe/configs/on-policy/PPOLag.yaml. */
typedef struct osa_ppo_hparams {
  float clip;             /* algo_cfgs.clip */
  float entropy_coef;     /* algo_cfgs.entropy_coef */
  float critic_norm_coef; /* algo_cfgs.critic_norm_coef */
  float max_grad_norm;    /* algo_cfgs.max_grad_norm */
  float lr_actor;         /* model_cfgs.actor.lr x LinearLR factor of the current epoch */
  float lr_critic;        /* model_cfgs.critic.lr */
  float beta1, beta2, adam_eps; /* torch.optim.Adam defaults 0.9, 0.999, 1e-8 */
  int use_critic_norm;    /* algo_cfgs.use_critic_norm */
  int use_max_grad_norm;  /* algo_cfgs.use_max_grad_norm */
  int use_cost;           /* algo_cfgs.use_cost */
  const float* lr_device; /* optional: { lr_actor, lr_critic } in DEVICE memory, read at execution time instead of the
                           * two by-value fields -- lets a captured hipGraph of optimiser steps be replayed across
                           * epochs while the LinearLR schedule moves.  Honoured by osa_ppo_minibatch(_ext) and
                           * osa_adam_apply; NULL everywhere else */
} osa_ppo_hparams;

/* One minibatch step of PolicyGradient._update's inner loop for all three networks in one launch:
 * _update_reward_critic / _update_cost_critic (omnisafe/algorithms/on_policy/base/policy_gradient.py:
 * 428-445, 468-485: MSE + critic_norm_coef * sum p^2, clip_grad_norm_, Adam) and _update_actor
 * (:514-524) with PPOLag's surrogate advantage (adv_r - lambda adv_c)/(1 + lambda)
 * (naive_lagrange/ppo_lag.py:101-102) and loss_kind 0 = PPO clipped loss (base/ppo.py:66-78) or
 * 1 = plain ratio * adv (policy_gradient.py:574-578).  Data arrays are the ENV-MAJOR tensors of
 * osa_buffer_get; idx[B] selects the minibatch rows (NULL = rows 0..B-1); *lagrange is a device scalar.
 * mode 0: gradient + local clip + Adam;  1: gradient + local clip (caller all-reduces grads[3][P]
 * and calls osa_adam_apply -- clip-then-average order of policy_gradient.py:437-442);  2: raw grads.
 * B <= 64*max_blocks rows are processed by ceil(B/64) workgroups per network (ws: at least
 * osa_minibatch_ws_floats floats when more than one is used, ZERO-INITIALISED ONCE by the caller: its tail
 * holds the partial norms and the arrival / finish counters of the fused slab-reduce + clip/Adam launch, which
 * every call leaves re-armed at zero; use one ws with ONE value of max_blocks).
 * step_stats[16] receives
 *   [0] mse_r [1] mse_c [2] loss_pi [3] mean ratio [4] entropy [5] sum p^2 (V_r) [6] sum p^2 (V_c)
 *   [7] |g_pi| [8] |g_Vr| [9] |g_Vc|   (logged Loss_*_critic = mse + critic_norm_coef * sum p^2). */
size_t osa_minibatch_ws_floats(int obs_dim, int act_dim, int hidden, int max_blocks);
int osa_ppo_minibatch(int obs_dim, int act_dim, int hidden, float* params, float* adam_m,
                      float* adam_v, int* adam_step, float* grads, const float* obs, int ld_obs,
                      const float* act, int ld_act, const float* logp, const float* target_value_r,
                      const float* target_value_c, const float* adv_r, const float* adv_c,
                      const long* idx, int B, const float* lagrange, const osa_ppo_hparams* hp,
                      int loss_kind, int mode, int nets_mask, int max_blocks, float* ws,
                      float* step_stats, void* stream);

/* Extended actor surrogates for the sibling first-order algorithms; everything else is
 * osa_ppo_minibatch.  Per-sample actor loss
 *     l_i = mbar * ratio_scale * s_i + mask_i * kl_coef * KL(pi_theta(.|s_i) || pi_old(.|s_i)),
 * s_i the loss_kind surrogate, mask_i = 1[KL_i <= kl_mask_eta], mbar = mean_i(mask_i) (kl_mask_eta < 0:
 * mask_i = mbar = 1) -- exactly what focops.py:84-88 differentiates (its (B,1) x (B,) broadcast makes the
 * surrogate term see the minibatch MEAN of the mask) -- plus
 * cost_kappa * relu(mean_i(ratio_i * adv_c_i) + cost_excess) when cost_kappa > 0 (value in step_stats[10]).
 * mbar and the penalty are minibatch-level quantities: with a mask or a penalty B <= 64 is required
 * (one block; OSA_EUNSUPPORTED otherwise).
 *   FOCOPS (first_order/focops.py:83-92): loss_kind 1, kl_coef 1, kl_mask_eta = focops_eta,
 *                                         ratio_scale = 1/focops_lam
 *   CUP second stage (first_order/cup.py:96-103): loss_kind 1 on adv = -lambda*coef*adv_c, kl_coef 1
 *   P3O (penalty_function/p3o.py:62-68,112-114): loss_kind 0 + cost_kappa = kappa, cost_excess = Jc - limit
 * old_mean[rows][ld_old_mean] / old_log_std[act_dim]: the behaviour policy's Gaussian per sample (same row
 * indexing as obs).  ext == NULL: identical to osa_ppo_minibatch. */
typedef struct osa_surrogate_ext {
  const float* old_mean;
  int ld_old_mean;
  const float* old_log_std;
  float kl_coef;
  float kl_mask_eta;
  float ratio_scale;
  float cost_kappa;
  float cost_excess;
} osa_surrogate_ext;
int osa_ppo_minibatch_ext(int obs_dim, int act_dim, int hidden, float* params, float* adam_m,
                          float* adam_v, int* adam_step, float* grads, const float* obs, int ld_obs,
                          const float* act, int ld_act, const float* logp,
                          const float* target_value_r, const float* target_value_c,
                          const float* adv_r, const float* adv_c, const long* idx, int B,
                          const float* lagrange, const osa_ppo_hparams* hp, int loss_kind, int mode,
                          int nets_mask, int max_blocks, float* ws, float* step_stats,
                          const osa_surrogate_ext* ext, void* stream);

/* Persistent form of the same update: ONE launch runs a whole pass of PolicyGradient._update's inner
 * loop (policy_gradient.py:366-382) -- ceil(M/B) dependent minibatch steps over the permutation
 * perm[M] (NULL = identity) -- for all three networks, with the parameters resident in LDS
 * and the Adam moments in registers for the whole pass (see csrc/ppo_pass_kernel.hip).  Same
 * arithmetic per step as osa_ppo_minibatch(mode 0); step_stats[ceil(M/B)][16] as above (columns 10..15
 * additionally receive the three networks' Adam bias-correction factors of the step).  A step with
 * B > 64 rows accumulates ceil(B/64) chunks in the accumulator registers before its clip + Adam.  Single
 * process only (world_size == 1: the data-parallel path needs an all-reduce between gradient and
 * Adam and uses osa_ppo_minibatch).  osa_ppo_pass_supported: 1 if (obs_dim, act_dim, hidden) fit.
 * The observation rows must be 16-byte aligned with ld_obs % 4 == 0 (OSA_EUNSUPPORTED otherwise -- pad
 * the rows; the same holds for osa_ppo_dp_step / osa_ppo_dp_pass). */
int osa_ppo_pass_supported(int obs_dim, int act_dim, int hidden);
int osa_ppo_pass(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                 int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                 const float* logp, const float* target_value_r, const float* target_value_c,
                 const float* adv_r, const float* adv_c, const long* perm, long M, int B,
                 const float* lagrange, const osa_ppo_hparams* hp, int loss_kind, int nets_mask,
                 float* step_stats, void* stream);
/* The same persistent pass for WIDE observations (65 <= obs_dim <= 512; callers prefer osa_ppo_pass where it
 * is supported; e.g. SafetyHumanoidVelocity 376/17;
 * model builder omnisafe/utils/model.py:73-111 takes any sizes): the first layer's weights and Adam moments do
 * not fit one compute unit, so they stay in (L2-resident) global memory -- W1 fragments are streamed by the
 * forward pass, the W1 gradient is accumulated in MFMA accumulator registers and norm + clip + Adam are applied
 * by the lanes that hold it; the other layers live in LDS / registers as in osa_ppo_pass (see
 * csrc/wide_pass_kernel.hip).  B <= 64, loss_kind 0/1, single process; same arguments, statistics and
 * arithmetic per step as osa_ppo_pass / osa_ppo_minibatch(mode 0), plus ws: osa_ppo_wide_pass_ws_floats
 * floats of scratch (a tiled private copy of the first layer, of its Adam moments and of its gradient for the
 * duration of the launch; contents undefined afterwards).  OSA_EUNSUPPORTED otherwise. */
int osa_ppo_wide_pass_supported(int obs_dim, int act_dim, int hidden);
size_t osa_ppo_wide_pass_ws_floats(int obs_dim, int act_dim, int hidden);
int osa_ppo_wide_pass(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                      int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                      const float* logp, const float* target_value_r, const float* target_value_c,
                      const float* adv_r, const float* adv_c, const long* perm, long M, int B,
                      const float* lagrange, const osa_ppo_hparams* hp, int loss_kind, int nets_mask,
                      float* ws, float* step_stats, void* stream);
/* osa_ppo_wide_pass with the first layer SPLIT over cooperating compute units (csrc/wide_split_kernel.hip):
 * a network is 1 + ceil(KB / 6) workgroups of one cooperative launch -- every helper owns <= 96 input columns of
 * W1 (LDS) and their Adam moments (registers) for the whole pass, the leader owns the other layers; three
 * hand-offs per step (partial pre-activations, dz1, squared-norm shares) through `xch`
 * (osa_ppo_split_pass_xch_floats floats, zero-initialised once).  local = 0: the workgroups are spread over the
 * XCCs and xch MUST come from osa_dp_exchange_alloc (uncached device memory; OSA_EINVAL otherwise).  local = 1:
 * the workgroups of a network are placed on ONE XCC (blocks net + 8 role of an 8 (C + 1) grid) and xch MUST be
 * ordinary device memory: the hand-offs are then served by that XCC's L2; the kernel verifies the placement
 * (XCC_ID of every workgroup) BEFORE anything is modified and, if it does not hold, every workgroup returns with
 * parameters, Adam state and step counters untouched and the sticky flag set to 2 (repeat with local = 0).
 * Same arguments, statistics and per-step arithmetic as osa_ppo_wide_pass (float32 re-association of the
 * layer-1 sum only).  OSA_EUNSUPPORTED when the shape is not supported or the device cannot hold the
 * workgroups together: use osa_ppo_wide_pass.  A peer that never arrives raises a sticky flag instead of
 * hanging the device: osa_ppo_split_pass_timed_out(xch, &flag) reads it (synchronous copy; 0 = fine). */
int osa_ppo_split_pass_supported(int obs_dim, int act_dim, int hidden);
size_t osa_ppo_split_pass_xch_floats(int obs_dim, int act_dim, int hidden);
int osa_ppo_split_pass(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                       int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                       const float* logp, const float* target_value_r, const float* target_value_c,
                       const float* adv_r, const float* adv_c, const long* perm, long M, int B,
                       const float* lagrange, const osa_ppo_hparams* hp, int loss_kind, int nets_mask,
                       float* xch, int local, float* step_stats, void* stream);
int osa_ppo_split_pass_timed_out(const float* xch, int* out);
/* Clears the sticky word after a tripped PLACEMENT check (flag 2: nothing was modified, the caller repeats the pass
 * with another placement).  Never clear a time-out (flag 1). */
int osa_ppo_split_pass_clear_flag(float* xch);
/* The DATA-PARALLEL form of osa_ppo_split_pass (world_size > 1 without a per-step cross-GPU collective, as
 * osa_ppo_dp_pass does for narrow observations): the arrays hold the all-gathered rollouts of `world` ranks (rank r:
 * rows r M .. r M + M - 1), perm is [world][M] (row r = rank r's shuffle of its OWN M rows, indices in [0, M)).
 * One cooperative launch of world x 3 x (1 + ceil(KB / 6)) workgroups: every virtual rank is a full set of leader
 * + helpers computing ITS minibatch's gradient and ITS clip factor (avg_grads order of the reference:
 * clip_grad_norm_ locally, then average -- policy_gradient.py:437-442, 478-483, 519-524; utils/distributed.py:167-198);
 * then the `world` owners of the same parameters (helper c of every rank; the leaders) exchange their clipped
 * shares, sum them in rank order, divide by world and apply the SAME Adam step to their own replica: no parameter
 * ever crosses between replicas, they stay bit-identical, rank 0's is written back.  step_stats receive the
 * rank-averaged statistics (what Logger.get_stats averages).  xch: osa_ppo_split_dp_xch_floats(...) floats from
 * osa_dp_exchange_alloc (uncached; OSA_EINVAL otherwise), zero-initialised once; its sticky word (1: a workgroup
 * never arrived, 2: placement) is read with osa_ppo_split_pass_timed_out.
 * place = 0, dpx = NULL: rank-major workgroups spread over the XCCs, every hand-off through xch.
 * place = 1: the `world` owners of the same parameters sit on ONE XCC (owner group g = (network, role) on XCC
 * g mod 8) and average through dpx = osa_ppo_split_dp_dpx_floats(...) floats of ORDINARY device memory (zeroed
 * once; OSA_EINVAL for an uncached buffer) served by that XCC's L2, the intra-rank hand-offs stay in xch; the
 * kernel verifies the placement before it modifies anything and otherwise returns untouched with the sticky word
 * at 2 (repeat with place = 0).  OSA_EUNSUPPORTED when the device cannot hold the workgroups together
 * (world x 3 x (C + 1) > compute units; place = 1: ceil(3 (C + 1) / 8) x world > compute units / 8) or the shape
 * is outside osa_ppo_split_pass_supported: use the per-step path (osa_ppo_minibatch mode 1 + all-reduce +
 * osa_adam_apply). */
size_t osa_ppo_split_dp_xch_floats(int obs_dim, int act_dim, int hidden, int world);
size_t osa_ppo_split_dp_dpx_floats(int obs_dim, int act_dim, int hidden, int world);
int osa_ppo_split_dp_pass(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                          int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                          const float* logp, const float* target_value_r, const float* target_value_c,
                          const float* adv_r, const float* adv_c, const long* perm, long M, int B, int world,
                          const float* lagrange, const osa_ppo_hparams* hp, int loss_kind, int nets_mask,
                          float* xch, float* dpx, int place, float* step_stats, void* stream);
/* osa_ppo_pass with the extended actor surrogates of osa_ppo_minibatch_ext (FOCOPS, CUP's second stage,
 * P3O): B <= 64 (the trust-mask mean and the penalty are minibatch-level quantities of one 64-row block);
 * OSA_EUNSUPPORTED otherwise -- use osa_ppo_minibatch_ext.  ext == NULL: osa_ppo_pass.  With cost_kappa > 0
 * step_stats[10] of every step receives the penalty value. */
int osa_ppo_pass_ext(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                 int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                 const float* logp, const float* target_value_r, const float* target_value_c,
                 const float* adv_r, const float* adv_c, const long* perm, long M, int B,
                 const float* lagrange, const osa_ppo_hparams* hp, int loss_kind, int nets_mask,
                 float* step_stats, const osa_surrogate_ext* ext, void* stream);
/* The passes of n INDEPENDENT agents in one launch.  The reference runs the seeds and variants of an experiment
 * as one training per worker of a process pool (ExperimentGrid.run, omnisafe/common/experiment_grid.py:387-471);
 * here every agent of the group is a member of one process and member s's pass -- exactly the arguments and the
 * arithmetic of osa_ppo_pass_ext (has_ext = 0: ext == NULL) -- is three workgroups of a grid of 24 ceil(n / 8):
 * bit-identical to n calls of osa_ppo_pass_ext, in the time of about one while 3 n compute units are free.  Members
 * share (obs_dim, act_dim, hidden) and may differ in everything else (M, B, hyper-parameters, masks, ...), except
 * that one launch is one kernel instantiation: all members have B <= 64 or all have B > 64, and all or none use an
 * extended surrogate (OSA_EINVAL for a mixed array, nothing is launched; the caller issues one call per class).
 * workspace: osa_ppo_pass_group_ws_bytes(n) bytes of device memory, 16-byte aligned, used by the launches of ONE
 * stream: the members' argument blocks are staged there by copy launches ordered on `stream`, so the call may be
 * repeated with the same workspace, and `members` reused, without waiting for the previous pass.  Any n >= 1 (more
 * than compute units / 3 members: the workgroups queue).  The cooperative forms (osa_ppo_chunked_pass, the split and
 * data-parallel passes) and osa_ppo_wide_pass are not grouped. */
typedef struct osa_pass_member {
  float* params;
  float* adam_m;
  float* adam_v;
  int* adam_step;
  const float* obs;
  int ld_obs;
  const float* act;
  int ld_act;
  const float* logp;
  const float* target_value_r;
  const float* target_value_c;
  const float* adv_r;
  const float* adv_c;
  const long* perm;
  long M;
  int B;
  const float* lagrange;
  osa_ppo_hparams hp;
  int loss_kind;
  int nets_mask;
  float* step_stats;
  int has_ext; /* 0: plain surrogate, `ext` ignored */
  osa_surrogate_ext ext;
} osa_pass_member;
size_t osa_ppo_pass_group_ws_bytes(int n);
int osa_ppo_pass_group(int obs_dim, int act_dim, int hidden, const osa_pass_member* members, int n, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Data-parallel optimiser step WITHOUT a per-step cross-GPU collective ("replicated data").  The data
 * arrays hold the all-gathered env-major rollouts of all `world` ranks ([world * M] rows, rank r at
 * rows r*M ..), perm[world][M] each rank's own permutation (local row indices).  One call performs
 * optimiser step `step_index` of the pass for every virtual rank -- `world` workgroups per network
 * compute the locally clipped gradients of rank r's minibatch perm[r][step*B ..] -- then averages them
 * (distributed.avg_grads, omnisafe/utils/distributed.py:193-198, clip-then-average order of
 * policy_gradient.py:437-442) and applies Adam.  Every rank executes the same arithmetic on the same
 * data, so replicas stay bit-identical without exchanging gradients or parameters.  lr_dev: optional
 * device float[2] {lr_actor, lr_critic} overriding hp (keeps a captured hipGraph valid across epochs).
 * slabs: osa_ppo_dp_ws_floats(...) floats.  step_stats[16]: rank-averaged statistics.  The Adam step
 * count used is adam_step[net] + step_index + 1; call osa_ppo_dp_end_pass once after the last step of
 * a pass to advance adam_step by the number of steps. */
size_t osa_ppo_dp_ws_floats(int obs_dim, int act_dim, int hidden, int world);
int osa_ppo_dp_step(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                    int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                    const float* logp, const float* target_value_r, const float* target_value_c,
                    const float* adv_r, const float* adv_c, const long* perm, long M, int B, int world,
                    int step_index, const float* lagrange, const osa_ppo_hparams* hp,
                    const float* lr_dev, int loss_kind, int nets_mask, float* slabs,
                    float* step_stats, void* stream);
int osa_ppo_dp_end_pass(int* adam_step, int nets_mask, int nsteps, void* stream);
/* The two halves of osa_ppo_dp_step for the PER-STEP ALL-REDUCE mode over real ranks (round 5) -- the reference's own
 * structure, policy_gradient.py:437-443 with distributed.py:167-198: clip_grad_norm_, avg_grads, optimizer.step -- on
 * the persistent pass kernel's gradient-only form instead of the per-step kernels (weights staged in LDS once per
 * launch, gradients from registers: 13 us against 48 per 64-row step).
 *   phase 1: the locally clipped gradients and statistics of THIS rank's minibatch (world = 1, perm = its row indices,
 *            M rows of them, step_index = 0) into slabs[3][P + 16]; nothing else is touched;
 *   [caller: ONE flat all-reduce (average) of the slabs]
 *   phase 2: Adam from the slabs (step count adam_step[net] + step_index + 1: pass the step's index within the pass
 *            and call osa_ppo_dp_end_pass after its last step); only the parameter / moment / slab / hp arguments are used.
 *   phase 0: osa_ppo_dp_step. */
int osa_ppo_dp_step_phase(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                          int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                          const float* logp, const float* target_value_r, const float* target_value_c,
                          const float* adv_r, const float* adv_c, const long* perm, long M, int B, int world,
                          int step_index, const float* lagrange, const osa_ppo_hparams* hp,
                          const float* lr_dev, int loss_kind, int nets_mask, float* slabs,
                          float* step_stats, int phase, void* stream);

/* The same replicated-data optimiser chain as ONE cooperative persistent launch per pass: 3 x world
 * workgroups stay resident for all ceil(M/B) steps; workgroup (net, r) keeps its own LDS/register copy
 * of the network and of the Adam moments, computes rank r's locally clipped gradient, publishes it in
 * `exchange` (osa_ppo_dp_pass_ws_floats floats), meets its `world` peers at an agent-scope arrival
 * counter (sync: int[4]: sync[0..2] arrival counters, reset by every call; sync[3] STICKY time-out flag,
 * never reset by the library -- the caller zeroes all four words once at allocation and reads sync[3]
 * at its next host synchronisation; a peer that never arrives is flagged after a bounded spin instead of
 * hanging the device), then sums the
 * gradients in rank order and applies Adam locally -- every peer does identical arithmetic, rank 0's
 * copy is written back at the end and adam_step advances by the number of steps.  Launched with
 * hipLaunchCooperativeKernel, i.e. the runtime verifies that all 3 * world workgroups are co-resident
 * (OSA_EUNSUPPORTED otherwise: use osa_ppo_dp_step).
 * Replaces: the minibatch loop of PolicyGradient._update under torch.distributed
 * (policy_gradient.py:366-382, 437-442; distributed.py:193-198). */
/* Optional: the exchange buffer of osa_ppo_dp_pass in UNCACHED device memory (hipExtMallocWithFlags,
 * hipDeviceMallocUncached).  The kernel recognises such a buffer and hands the gradients over without
 * the agent-scope L2 write-back / invalidate that ordinary (cached) device memory needs.  The one place
 * where the library allocates: the memory type cannot be requested through torch.  OSA_EUNSUPPORTED if
 * the runtime refuses the flag (use an ordinary buffer then). */
int osa_dp_exchange_alloc(size_t floats, float** out);
int osa_dp_exchange_free(float* p);
size_t osa_ppo_dp_pass_ws_floats(int obs_dim, int act_dim, int hidden, int world);
int osa_ppo_dp_pass(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                    int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                    const float* logp, const float* target_value_r, const float* target_value_c,
                    const float* adv_r, const float* adv_c, const long* perm, long M, int B, int world,
                    const float* lagrange, const osa_ppo_hparams* hp, int loss_kind, int nets_mask,
                    float* exchange, int* sync, float* step_stats, void* stream);
/* osa_ppo_dp_pass with an explicit placement.  local = 0: as osa_ppo_dp_pass (grid 3 x world, spread over the
 * XCCs; `exchange` uncached or ordinary memory).  local = 1: the `world` workgroups of a network are the blocks
 * net + 8 r of an 8 x world grid, i.e. they run on ONE XCC, and `exchange` MUST be ordinary device memory
 * (OSA_EINVAL for an osa_dp_exchange_alloc buffer): the hand-offs are served by that XCC's L2.  sync: int[8]
 * (zeroed once by the caller): sync[4..6] receive the bit masks of the XCCs each network's workgroups ran on,
 * sync[7] counts arrivals.  The placement is verified BEFORE anything is modified: if a network's mask holds
 * more than one bit (or a workgroup never arrives) EVERY workgroup returns with parameters, Adam state and step
 * counters untouched and the sticky flag sync[3] is 2 (1): repeat the call with local = 0.  world <= CUs / 8. */
int osa_ppo_dp_pass_placed(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                    int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                    const float* logp, const float* target_value_r, const float* target_value_c,
                    const float* adv_r, const float* adv_c, const long* perm, long M, int B, int world,
                    const float* lagrange, const osa_ppo_hparams* hp, int loss_kind, int nets_mask,
                    float* exchange, int* sync, int local, float* step_stats, void* stream);

/* ONE-SHOT PEER EXCHANGE (round 6; csrc/p2p_pass_kernel.hip): the data-parallel minibatch loop with REAL ranks and no
 * collective on the step path -- SURVEY.md 8(e) "xGMI mapping" (one-shot all-to-all write of the <= 336 KB clipped
 * gradients + local reduce).  Replaces per optimiser step `clip_grad_norm_` -> `distributed.avg_grads` (19 blocking
 * all-reduces) -> `optimizer.step()`: omnisafe/algorithms/on_policy/base/policy_gradient.py:437-443, 478-483, 519-524;
 * omnisafe/utils/distributed.py:167-198.
 *
 * Every rank (one process per GPU) owns ONE exchange buffer of osa_p2p_exchange_floats(...) floats in UNCACHED device
 * memory: osa_p2p_exchange_alloc allocates it zeroed and returns its 64-byte IPC handle (hipIpcGetMemHandle); the host
 * side exchanges the handles (torch.distributed all_gather: a set-up step, once) and maps every peer's buffer with
 * osa_p2p_exchange_open (hipIpcOpenMemHandle; peers may be other devices of the node or other processes on the same
 * device).  osa_p2p_exchange_release unmaps a peer's buffer / frees an own one.  All ranks must have opened all
 * buffers (a barrier) before the first pass.
 *
 * osa_ppo_p2p_pass = osa_ppo_pass on THIS rank's rows (arrays, perm, M, B as there: 3 workgroups, weights in LDS, Adam
 * moments in registers, all ceil(M / B) steps in one launch), except that after the local clip each network's
 * workgroup writes its gradient slab into the buffer of every rank (peers[q], q = 0 .. world - 1 as mapped into this
 * process; peers[rank] = the own buffer), releases at system scope, stores the step's sequence number into its arrival
 * word in every buffer, waits for the `world` arrival words of its own buffer, adds the slabs IN RANK ORDER, divides
 * by world (clip-then-average) and applies Adam: identical arithmetic on every rank, bit-identical replicas, every
 * rank writes its own parameters / moments back.  step_stats: rank-averaged (what Logger.get_stats averages).
 * seq0: optimiser steps exchanged through these buffers before this call -- the SAME on every rank; the caller adds
 * ceil(M / B) after each call (arrival words only grow: nothing is reset between launches).  timeout_s: how long a
 * workgroup waits for a peer before it sets the sticky word read by osa_p2p_exchange_timed_out (the pass then
 * finishes without waiting: results invalid, the device never hangs).  world <= 16; B <= 2048 (B > 64: the workgroup
 * walks through the minibatch's 64-row chunks); shapes as osa_ppo_pass_supported (OSA_EUNSUPPORTED otherwise). */
size_t osa_p2p_exchange_floats(int obs_dim, int act_dim, int hidden, int world);
int osa_p2p_exchange_alloc(size_t floats, float** out, void* ipc_handle64);
int osa_p2p_exchange_open(const void* ipc_handle64, float** out);
int osa_p2p_exchange_release(float* p);
int osa_p2p_exchange_timed_out(const float* own, int* flag);
int osa_ppo_p2p_pass(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                     int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                     const float* logp, const float* target_value_r, const float* target_value_c,
                     const float* adv_r, const float* adv_c, const long* perm, long M, int B, int world, int rank,
                     float* const* peers, unsigned seq0, double timeout_s, const float* lagrange,
                     const osa_ppo_hparams* hp, int loss_kind, int nets_mask, float* step_stats, void* stream);

/* Single-process persistent pass for minibatches of 64 < B <= 2048 rows (the trust-region family's critic
 * updates: batch_size 128, natural_pg.py:205-223) with the ceil(B / 64) 64-row CHUNKS of a minibatch on cooperating
 * workgroups (one compute unit each, per network) instead of one workgroup walking through them: every workgroup
 * keeps the network and its Adam state, computes the raw gradient of its chunk scaled by 1 / rows of the minibatch,
 * the chunks' gradients are summed (exchange: osa_ppo_dp_pass_ws_floats(.., world = ceil(B / 64)) floats, zeroed
 * once), the SUM is clipped by its norm and everybody applies the same Adam step: the arithmetic of
 * osa_ppo_pass / osa_ppo_minibatch(mode 0) on the same rows (float32 re-association of the sum over chunks only).
 * Arguments as osa_ppo_pass plus exchange / sync / local as in osa_ppo_dp_pass_placed (sync: int[8]; sticky
 * sync[3]).  OSA_EUNSUPPORTED for B <= 64 (use osa_ppo_pass) or when the workgroups cannot be co-resident. */
int osa_ppo_chunked_pass(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                         int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                         const float* logp, const float* target_value_r, const float* target_value_c,
                         const float* adv_r, const float* adv_c, const long* perm, long M, int B,
                         const float* lagrange, const osa_ppo_hparams* hp, int loss_kind, int nets_mask,
                         float* exchange, int* sync, int local, float* step_stats, void* stream);
/* osa_ppo_chunked_pass UNDER DATA PARALLELISM (the critic passes of the trust-region family, batch 128, with
 * world_size > 1 -- BASELINE configs 3 and 5; natural_pg.py:205-223 + distributed.py:167-198): arrays and perm as
 * osa_ppo_dp_pass ([world][M] rows, rank r's shuffle of its own rows), world x ceil(B / 64) workgroups per network
 * in one cooperative launch.  Two hand-offs per optimiser step: inside a rank's chunk group (sum of the chunks'
 * gradients, ITS norm, the rank's clip factor -- the arithmetic of one B-row step of that rank), then across ranks
 * (every chunk workgroup publishes its share of the tiles of the rank's sum; everybody adds the `world` clipped sums
 * in rank order, / world) and the same Adam step in every replica.  exchange: osa_ppo_dp_chunked_pass_ws_floats
 * floats (placement rules as osa_ppo_dp_pass_placed); sync: int[64], zero before the first call ([3] sticky
 * time-out / placement flag as there). */
size_t osa_ppo_dp_chunked_pass_ws_floats(int obs_dim, int act_dim, int hidden, int B, int world);
int osa_ppo_dp_chunked_pass(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                            int* adam_step, const float* obs, int ld_obs, const float* act, int ld_act,
                            const float* logp, const float* target_value_r, const float* target_value_c,
                            const float* adv_r, const float* adv_c, const long* perm, long M, int B, int world,
                            const float* lagrange, const osa_ppo_hparams* hp, int loss_kind, int nets_mask,
                            float* exchange, int* sync, int local, float* step_stats, void* stream);

/* Debugging aid: when set to a device buffer of 48 int64, every osa_ppo_minibatch launch records
 * s_memtime phase timestamps [3 networks][16] (used by tools/phase_clocks.py); NULL disables it. */
int osa_debug_set_clock_buffer(long long* dev_ptr);
/* same for osa_ppo_pass: accumulated cycles per phase over the pass, [3 networks][16]. */
int osa_debug_set_pass_clock_buffer(long long* dev_ptr);
/* Debug: per-workgroup {start, end} clocks of the balanced partial-gradient launch of the large-batch step
 * (long long[16 x workgroups]: 100 MHz constant clock start, shader cycles start, the same two at the end; [4..6] shader
 * cycles after the prologue / the first chunk / the last chunk in the -DOSA_PART_CLOCKS build); NULL = off. */
int osa_debug_set_part_clock_buffer(long long* dev_ptr);

/* ---- General actor-critic MLPs (csrc/general_mlp.hip, round 4): ANY hidden_sizes the reference's model builder
 * accepts (omnisafe/utils/model.py:73-111 build_mlp_network: any depth, any widths; actor and critics configured
 * independently, models/actor_critic/actor_critic.py:60-136), e.g. the 1024 x 1024 networks of the reference's
 * published timing table (docs/source/start/efficiency.rst:15-23).  Layer-wise on one float32-MFMA GEMM kernel
 * (forward / backward-data / backward-weight with fused epilogues); the entry points mirror the per-step family
 * above (osa_policy_step_scaled, osa_ppo_minibatch, osa_adam_apply, osa_actor_kl, osa_actor_eval,
 * osa_actor_fvp_raw) with the network shapes in a descriptor instead of the `hidden` word.
 * Parameter block of one network ([3][P] floats as everywhere): per linear layer l  W_l [out_l][ld_l] (ld_l = in_l
 * rounded up to 4, padding zero) | b_l [out_l rounded up to 4]; the actor's log_std [act_dim] follows its last layer.
 * osa_gmlp_layout fills out[0] = P, out[1] = offset of log_std, then {oW, ob, ld} for network 0..2 x layer
 * 0..OSA_GMLP_MAX_LAYERS-1 (-1 / 0 for absent layers): 2 + 72 ints.
 * ws: osa_gmlp_ws_floats(desc, rows) floats of scratch for a call over `rows` rows (layer outputs, dL/dz, partial
 * gradient slabs); contents irrelevant between calls. */
#define OSA_GMLP_MAX_LAYERS 8
typedef struct osa_gmlp_desc {
  int obs_dim, act_dim;
  int n_layers[3];                    /* linear layers (hidden layers + 1) of actor, reward critic, cost critic */
  int width[3][OSA_GMLP_MAX_LAYERS];  /* output width of every linear layer; the last one = act_dim (actor) / 1 */
  int activation[3];                  /* hidden activation: 0 tanh 1 relu 2 sigmoid 3 softplus 4 identity */
} osa_gmlp_desc;
int osa_gmlp_layout(const osa_gmlp_desc* desc, int* out);
size_t osa_gmlp_ws_floats(const osa_gmlp_desc* desc, long rows);
/* ConstraintActorCritic.step (constraint_actor_critic.py:84-109) + ActionScale: arguments as osa_policy_step_scaled. */
int osa_gmlp_policy_step(const osa_gmlp_desc* desc, const float* params, const float* obs, int ld_obs, long N,
                         const float* eps, unsigned long long seed, unsigned long long offset,
                         const unsigned long long* offset_base, int deterministic, int nets_mask, float* act,
                         int ld_act, float* value_r, float* value_c, float* logp, float* mean_out, int ld_mean,
                         float* act_env, int ld_env, const float* old_min, const float* old_max, float min_action,
                         float max_action, float* ws, size_t ws_floats, void* stream);
/* One optimiser step of PolicyGradient._update's inner loop (policy_gradient.py:428-445, 468-485, 514-524): arguments
 * and modes as osa_ppo_minibatch (mode 0 grad + local clip + Adam, 1 grad + local clip -> grads[3][P], 2 raw grads).
 * loss_kind 2 = the raw Fisher-vector product of the actor along `vec` (padded actor vector; fvp_scale = 1 / (M D_a);
 * natural_pg.py:91-119) into grads[0], as osa_actor_fvp_raw. */
int osa_gmlp_minibatch(const osa_gmlp_desc* desc, float* params, float* adam_m, float* adam_v, int* adam_step,
                       float* grads, const float* obs, int ld_obs, const float* act, int ld_act, const float* logp,
                       const float* target_value_r, const float* target_value_c, const float* adv_r,
                       const float* adv_c, const long* idx, long B, const float* lagrange, const osa_ppo_hparams* hp,
                       int loss_kind, int mode, int nets_mask, const float* vec, float fvp_scale, float* ws,
                       size_t ws_floats, float* step_stats, void* stream);
/* osa_gmlp_minibatch with the extended actor surrogates of osa_ppo_minibatch_ext (FOCOPS first_order/focops.py:83-92,
 * CUP's second stage first_order/cup.py:96-103, P3O penalty_function/p3o.py:62-68,112-114) on general networks -- the
 * reference builds any hidden_sizes for them as for every other algorithm (utils/model.py:73-111).  ext == NULL:
 * osa_gmlp_minibatch.  The trust-mask mean and the penalty are minibatch-level quantities: with kl_mask_eta >= 0 or
 * cost_kappa > 0 at most 256 rows (OSA_EUNSUPPORTED otherwise); step_stats[10] receives the penalty value.
 * Minibatches of at most 64 rows (the YAML batch_size) run on the skinny kernels (weights streamed once per pass,
 * clip + Adam from recomputed gradient tiles; OSA_GMLP_SKINNY=0: the tiled GEMM path). */
int osa_gmlp_minibatch_ext(const osa_gmlp_desc* desc, float* params, float* adam_m, float* adam_v, int* adam_step,
                           float* grads, const float* obs, int ld_obs, const float* act, int ld_act, const float* logp,
                           const float* target_value_r, const float* target_value_c, const float* adv_r,
                           const float* adv_c, const long* idx, long B, const float* lagrange,
                           const osa_ppo_hparams* hp, int loss_kind, int mode, int nets_mask, const float* vec,
                           float fvp_scale, float* ws, size_t ws_floats, float* step_stats,
                           const osa_surrogate_ext* ext, void* stream);
/* The launch plan of osa_gmlp_minibatch_ext for these arguments IN THIS PROCESS (the once-per-process switches
 * OSA_GMLP_DEEP, OSA_GMLP_XCD_ORDER, OSA_GMLP_ROW_SPLIT, OSA_GMLP_TOP_FUSE as the launchers read them): the launchers'
 * own decision functions, walked without a launch.  Host only, no GPU needed.  out[0 .. n) receives
 *   [0] ints of the whole record   [1] 1 skinny step (B <= 64) / 0 tiled   [2] fusedn: clip norm from the Gram matrices
 *   [3..5] per network: top layer's forward pass inside the launch below   [6..8] per network: loss inside the top
 *   layer's backward launch   [9] sk_maxT1: workgroups per network of the skinny weight-gradient launch
 *   [10..33] sk_tk[net][layer]: K tiles per 64-row tile of that launch   [34..57] S[net][layer]: row splits of the tiled
 *   weight-gradient GEMM   [58] launches of the tiled step's GEMM kernel (0 for a skinny step), then per launch, in
 *   launch order, OSA_GMLP_PLAN_LAUNCH ints:
 *   TM, TN, BK, AT, BT (the instantiation of the GEMM kernel), splits (grid.z per problem), row split S (0: the launch
 *   does not slice K through slabs), problems, Si[3] (per problem, under a row split), splits[3] (per problem), and
 *   whether the launch remaps its tiles to the XCDs (OSA_GMLP_XCD_ORDER).
 * OSA_EINVAL with out[0] set when n is too short. */
#define OSA_GMLP_PLAN_HEAD 59
#define OSA_GMLP_PLAN_LAUNCH 15
int osa_gmlp_plan(const osa_gmlp_desc* desc, long B, int loss_kind, int mode, int nets_mask, const osa_ppo_hparams* hp,
                  int* out, int n);
/* osa_adam_apply for general networks; fin8x3: 24 floats of device scratch. */
int osa_gmlp_adam_apply(const osa_gmlp_desc* desc, float* params, float* adam_m, float* adam_v, int* adam_step,
                        float* grads, const osa_ppo_hparams* hp, int nets_mask, float* fin8x3, void* stream);
/* osa_actor_kl (kind 0: old_mean == NULL snapshots the mean into mean_out; otherwise KL(old || new) -> out[0] with
 * reduce_mode as there) and osa_actor_eval (kind 1: out[0..3] = loss_pi, loss_cost, KL, mean ratio) for general
 * networks.  actor_params: the actor's block (network 0 of a [3][P] tensor, or a candidate vector). */
int osa_gmlp_actor_stats(const osa_gmlp_desc* desc, const float* actor_params, const float* obs, int ld_obs, long M,
                         const float* old_mean, int ld_old, const float* old_log_std, int kind, int reduce_mode,
                         const float* act, int ld_act, const float* logp, const float* adv_r, const float* adv_c,
                         const float* lagrange, float* mean_out, int ld_mean, float* ws, size_t ws_floats, float* out,
                         void* stream);

/* Adam step on already clipped (and, for world_size > 1, all-reduce-averaged) gradients. */
int osa_adam_apply(int obs_dim, int act_dim, int hidden, float* params, float* adam_m, float* adam_v,
                   int* adam_step, float* grads, const osa_ppo_hparams* hp, int nets_mask,
                   void* stream);

/* Full-batch actor forward over M env-major rows.  With old_mean == NULL it only snapshots the
 * distribution mean into mean_out (old_distribution = actor(obs), policy_gradient.py:357).  Otherwise
 * it evaluates KL(old || new) of torch.distributions.kl._kl_normal_normal: reduce_mode 0 =
 * .sum(-1).mean() (policy_gradient.py:383-389), 1 = .mean() over all M x act_dim elements
 * (natural_pg.py:95, trpo.py:113, cpo.py:133); the scalar lands in *kl_out (device).
 * ws: at least 1024 doubles. */
int osa_actor_kl(int obs_dim, int act_dim, int hidden, const float* actor_params, const float* obs,
                 int ld_obs, long M, const float* old_mean, int ld_old, const float* old_log_std,
                 int reduce_mode, float* mean_out, int ld_mean, double* ws, float* kl_out,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Rollout step (replaces the wrapper chain and the per-env loop of OnPolicyAdapter.rollout)
 * ---------------------------------------------------------------------------------------------- */

/* Normalizer._push (omnisafe/common/normalizer.py:109-139) with a batch of the rows of x selected by
 * mask (NULL = all N rows; zero selected rows = no-op): Chan/Golub/LeVeque merge of the batch mean and
 * centred sum of squares into the running state, var = sumsq/(count-1), std = max(sqrt(var), 1e-2).
 * State: mean/sumsq/var/std float32[D], count int64[1] (all device).  ws: osa_normalizer_ws_doubles(N, D)
 * doubles, ZERO-INITIALISED ONCE by the caller (its FIRST word is the arrival ticket of the single-launch
 * reduction; every call leaves it at zero again, so one workspace sized for the largest N serves any
 * smaller batch afterwards). */
size_t osa_normalizer_ws_doubles(int N, int D);
int osa_normalizer_push(const float* x, int ld, int N, int D, const uint8_t* mask, float* mean,
                        float* sumsq, float* var, float* std_, long* count, double* ws,
                        void* stream);

/* Normalizer.normalize's output (normalizer.py:102-107): y = clamp((x - mean)/std, -clip, clip) for
 * rows selected by mask (others copied unchanged); x copied unchanged while count <= 1. */
int osa_normalizer_apply(const float* x, int ld_x, float* y, int ld_y, int N, int D,
                         const uint8_t* mask, const float* mean, const float* std_, const long* count,
                         float clip, void* stream);

/* ActionScale.step (omnisafe/envs/wrapper.py:510-514):
 * out = old_min + (old_max - old_min) * (act - min_action) / (max_action - min_action). */
int osa_action_scale(const float* act, int ld_act, float* out, int ld_out, int N, int act_dim,
                     const float* old_min, const float* old_max, float min_action, float max_action,
                     void* stream);

/* The per-env loop of OnPolicyAdapter.rollout (omnisafe/adapter/onpolicy_adapter.py:86-136) for all N
 * envs at one step: episode return/cost/length accumulation (_log_value :155-157), path-end flag and
 * bootstrap selection -- 0 if terminated, V(final_observation) (vfinal_*) if truncated, V(next_obs)
 * (vnext_*) at epoch end (:114-126) -- written into row t of the buffer's path_end/boot_r/boot_c, and
 * the finished episodes' metrics (_log_metrics :159-174) into row t of ep_done/ep_*_out, after which
 * the per-env accumulators reset (:128-134).  vnext_* / vfinal_* may be NULL when not needed.
 * reward_row / cost_row (each may be NULL): row t of the buffer's reward / cost columns, filled with the step's
 * reward / cost (buffer.store, :100-108) in the same launch -- for callers without a reward / cost normaliser or an
 * adapter hook that rewrites the row in between (round 3: two copy launches per vector step less). */
int osa_rollout_post_step(int N, int epoch_end, const float* reward, const float* cost,
                          const uint8_t* terminated, const uint8_t* truncated, const float* vnext_r,
                          const float* vnext_c, const float* vfinal_r, const float* vfinal_c,
                          float* ep_ret, float* ep_cost, float* ep_len, uint8_t* path_end,
                          float* boot_r, float* boot_c, uint8_t* ep_done, float* ep_ret_out,
                          float* ep_cost_out, float* ep_len_out, float* reward_row, float* cost_row,
                          void* stream);

/* End-of-epoch log flush of OnPolicyAdapter.rollout (_log_metrics onpolicy_adapter.py:159-174; logger.store of the
 * value means :88-92) in two launches: the finished episodes (done[i] != 0, i = t N + n over the epoch's M = T N
 * slots) compacted in (step, env) order -- out_idx[k] = i, out_vals[0 M + k] = ep_ret[i], [1 M + k] = ep_cost[i],
 * [2 M + k] = ep_len[i], [3 M + k] = extra[i] (extra may be NULL) -- their number in out_count[0], and out_means =
 * { mean(value_r), mean(value_c) } over the M slots (float64 sums in a fixed order).  out_idx: int[M], out_vals:
 * float[4 M]; ws: osa_episode_flush_ws_doubles(M) doubles, zeroed once (every call leaves its ticket at 0). */
size_t osa_episode_flush_ws_doubles(long M);
int osa_episode_flush(const uint8_t* done, const float* ep_ret, const float* ep_cost, const float* ep_len,
                      const float* extra, long M, const float* value_r, const float* value_c, int* out_count,
                      int* out_idx, float* out_vals, float* out_means, double* ws, void* stream);

/* *out = mean of x[idx[0 .. n)] (idx NULL: of x[0 .. n)), float64 accumulation in a fixed order: the Value/Adv the
 * reference logs from the LAST minibatch of the update (policy_gradient.py:369-377, 402). */
int osa_gather_mean(const float* x, const long* idx, long n, float* out, void* stream);

/* SauteAdapter.step for all N envs (omnisafe/adapter/saute_adapter.py:124-196; SimmerAdapter shares it with
 * reset_value = relative budget): safety_obs <- (safety_obs - cost/budget)/saute_gamma; reward_out =
 * reward if safety_obs > 0 else unsafe_reward; finished envs (terminated | truncated) restart from
 * reset_value; the new safety_obs becomes column `col` of the (already normalised) next-observation rows
 * and, when given, of the final-observation rows; ep_budget accumulates it and a finished episode writes
 * its sum to ep_budget_out (Metrics/EpBudget) and restarts from 0. */
int osa_saute_step(int N, const float* cost, const float* reward, const uint8_t* terminated,
                   const uint8_t* truncated, float* safety_obs, const float* budget, float saute_gamma,
                   float unsafe_reward, const float* reset_value, float* reward_out, float* next_rows,
                   int ld_next, float* final_rows, int ld_final, int col, float* ep_budget,
                   float* ep_budget_out, void* stream);

/* Synthetic fixed-shape vector CMDP for throughput runs (stand-in for Safety-Gymnasium, whose physics
 * is third-party CPU code outside the reference repo; same role as tests/simple_env.py:30-90 of the
 * reference): obs ~ N(0,1)^obs_dim, reward ~ N(0,1), cost ~ Bernoulli(cost_p), never terminates,
 * truncates every `horizon` steps with gymnasium's vector auto-reset convention (the returned obs is
 * the post-reset obs; the pre-reset obs goes to final_obs).  reset_only != 0 draws initial
 * observations and zeroes the step counters.  Random draws are keyed by (seed, step + *step_base, env, k);
 * step_base: device pointer or NULL (same role as osa_policy_step's offset_base: graph replay). */
int osa_synth_env_step(unsigned long long seed, unsigned long long step,
                       const unsigned long long* step_base, int N, int obs_dim,
                       int horizon, float cost_p, int* steps, float* obs, int ld_obs, float* reward,
                       float* cost, uint8_t* terminated, uint8_t* truncated, float* final_obs,
                       int ld_final, int reset_only, void* stream);

/* Learnable synthetic vector CMDP "SynthReach-v0" (obs_dim >= 6, 2 actions; stand-in for a
 * Safety-Gymnasium goal task, which is third-party CPU physics outside the reference repo; plays the
 * role of the reference's tests/simple_env.py:30-90 for learning-curve comparisons): a point moves by
 * 0.1*clip(action,-1,1) inside [-1.5,1.5]^2, reward = decrease of the distance to the goal, +1 and a
 * new goal when within 0.15 of it, cost = 1 inside a disc of radius 0.3 around a hazard; never
 * terminates, truncates every `horizon` steps (gymnasium vector auto-reset convention as above).
 * state: N x 8 floats (p, goal, hazard, 2 pad), owned by the caller, updated in place.
 * obs row = [p, goal-p, hazard-p, 0...].  reset_only != 0 draws fresh states and zeroes `steps`. */
int osa_reach_env_step(unsigned long long seed, unsigned long long step,
                       const unsigned long long* step_base, int N, int obs_dim,
                       int horizon, float* state, int* steps, const float* action, int ld_action,
                       float* obs, int ld_obs, float* reward, float* cost, uint8_t* terminated,
                       uint8_t* truncated, float* final_obs, int ld_final, int reset_only,
                       void* stream);

/* Lidar navigation vector CMDP "SynthNavGoal{0,1,2}-v0" (obs_dim >= 60, 2 actions; stand-in for the Safety-Gymnasium
 * Goal tasks behind omnisafe/envs/safety_gymnasium_env.py:160-210 step / reset and envs/core.py:37-182, whose MuJoCo
 * physics is third-party CPU code outside the reference repo; a specification of this package, not a port): a point
 * robot with a unit heading u and a forward speed f.  Under clip(action,-1,1): f <- 0.9 f + 0.02 a0; u is turned by
 * the rational rotation of parameter t = 0.15 a1 (c = (1 - t^2)/(1 + t^2), s = 2t/(1 + t^2)) and renormalised;
 * p <- clip(p + f u, -2, 2).  reward = decrease of the distance to the goal, +1 and a new goal (the first of four
 * candidates in [-1.5,1.5]^2 that keeps 0.55 from every hazard, else the fourth) when within 0.3 of it; cost = 1
 * inside a hazard disc (radius 0.2) or, on level 2, a vase disc (radius 0.1).  level 0 / 1 / 2: 0 / 8 / 10 hazards,
 * 0 / 1 / 10 vases.  Never terminates, truncates every `horizon` steps (gymnasium vector auto-reset convention as
 * above).  state: N x 64 floats owned by the caller, updated in place: p(2) u(2) f f_prev t 0 goal(2) 0 0
 * hazards(10 x 2) vases(10 x 2) 0(12).  obs row = [f, f - f_prev, t, u, 0 (7), goal lidar (16), hazard lidar (16),
 * vase lidar (16), 0...]: an object at distance r in the egocentric 22.5-degree sector k reads max(0, 1 - r/3) in bin
 * k, a bin keeps the maximum of its class.  float32 without fused multiply-adds, correctly rounded / and sqrt: a numpy
 * twin reproduces every bit.  reset_only != 0 draws fresh states and zeroes `steps`. */
int osa_nav_env_step(unsigned long long seed, unsigned long long step,
                     const unsigned long long* step_base, int N, int obs_dim,
                     int horizon, int level, float* state, int* steps, const float* action, int ld_action,
                     float* obs, int ld_obs, float* reward, float* cost, uint8_t* terminated,
                     uint8_t* truncated, float* final_obs, int ld_final, int reset_only,
                     void* stream);

/* Circle-running vector CMDP "SynthNavCircle{0,1,2}-v0" (obs_dim >= 28, 2 actions; stand-in for the Safety-Gymnasium
 * Circle tasks behind omnisafe/envs/safety_gymnasium_env.py:160-210 step / reset, whose MuJoCo physics is third-party
 * CPU code outside the reference repo; a specification of this package, not a port): the robot of SynthNavGoal -- under
 * a = clip(action,-1,1): f <- 0.9 f + 0.02 a0; u turned by the rational rotation of parameter t = 0.15 a1 and
 * renormalised; m = f u; q = clip(p + m, -2, 2); p <- q -- is paid for running round the origin counter-clockwise:
 * reward = ((m_y q_x - m_x q_y) / |q|) / (1 + ||q| - 1|), 0 where |q| = 0.  cost of the transition that led to q:
 * level 0 none, level 1: 1 if |q_x| > 0.75, level 2: 1 if |q_x| > 0.75 or |q_y| > 0.75 (the walls are not observed).
 * The unit circle leaves either corridor, so the unconstrained optimum is infeasible on levels 1 and 2.  Never
 * terminates, truncates every `horizon` steps (gymnasium vector auto-reset convention as above).  state: N x 8 floats
 * owned by the caller, updated in place: p(2) u(2) f f_prev t 0.  A reset of env n at stream position pos takes
 * uniforms 0 .. 3 in (-1.5, 1.5] of Philox block 1 keyed seed ^ OSA_CIRCLE_KEY (0xE7037ED1A0B428DB; counter as
 * osa_nav_env_step's): p = 0.4 (u0, u1), u = (u2, u3) normalised ((1, 0) if the norm is 0), the rest 0; a truncating
 * step at position pos draws its fresh state at the same pos; transitions draw nothing.  obs row = [f, f - f_prev, t,
 * u, 0 (7), lidar of the origin (16), 0...]: the origin reads max(0, 1 - |p|/3) in the egocentric 22.5-degree sector it
 * falls in (osa_nav_env_step's goal lidar with the goal at (0, 0)); at p = (0, 0) no bin is lit.  float32 without fused
 * multiply-adds, correctly rounded / and sqrt: a numpy twin reproduces every bit.  reset_only != 0 draws fresh states
 * and zeroes `steps`.  Launch: half a wave per env (two envs per 64-lane workgroup). */
int osa_circle_env_step(unsigned long long seed, unsigned long long step,
                        const unsigned long long* step_base, int N, int obs_dim,
                        int horizon, int level, float* state, int* steps, const float* action, int ld_action,
                        float* obs, int ld_obs, float* reward, float* cost, uint8_t* terminated,
                        uint8_t* truncated, float* final_obs, int ld_final, int reset_only,
                        void* stream);

/* The Car on the two tasks above: "SynthNavCarGoal{0,1,2}-v0" (obs_dim >= 72, 2 actions; stand-in for the
 * Safety-Gymnasium CarGoal tasks behind omnisafe/envs/safety_gymnasium_env.py:160-210 step / reset -- SafetyCarGoal1-v0
 * is the env of BASELINE config 3 -- whose MuJoCo physics is third-party CPU code outside the reference repo; a
 * specification of this package, not a port).  The Car has two independently driven wheels: under
 * a = clip(action,-1,1), a0 the left and a1 the right wheel, w_l <- 0.9 w_l + 0.02 a0, w_r <- 0.9 w_r + 0.02 a1,
 * f <- 0.5 (w_l + w_r), t <- 0.375 (w_r - w_l); then osa_nav_env_step's motion with that f and t (u turned by the
 * rational rotation of parameter t and renormalised, p <- clip(p + f u, -2, 2)) and its reward, goal resampling,
 * hazards, vases, costs and levels.  state: N x 64 floats owned by the caller, updated in place: osa_nav_env_step's row
 * with three of its zero slots in use, [7] t_prev, [10] w_l, [11] w_r.  A reset is osa_nav_env_step's, under the SAME
 * Philox key and draw allocation (the arena of seed s equals SynthNavGoal's of seed s, so that robots can be compared
 * on identical layouts), with w_l = w_r = t_prev = 0.  obs row = [f, f - f_prev, t, u, w_l, w_r, t - t_prev, 0 (16),
 * goal lidar (16), hazard lidar (16), vase lidar (16), 0...].  float32 without fused multiply-adds: a numpy twin
 * reproduces every bit.  Launch: one wave per env; lanes 0 - 7 also write columns 64 - 71. */
int osa_car_goal_env_step(unsigned long long seed, unsigned long long step,
                          const unsigned long long* step_base, int N, int obs_dim,
                          int horizon, int level, float* state, int* steps, const float* action, int ld_action,
                          float* obs, int ld_obs, float* reward, float* cost, uint8_t* terminated,
                          uint8_t* truncated, float* final_obs, int ld_final, int reset_only,
                          void* stream);

/* "SynthNavCarCircle{0,1,2}-v0" (obs_dim >= 40, 2 actions; stand-in for the Safety-Gymnasium CarCircle tasks behind
 * omnisafe/envs/safety_gymnasium_env.py:160-210 step / reset; a specification of this package, not a port): the Car of
 * osa_car_goal_env_step with the reward, corridor cost and levels of osa_circle_env_step.  state: N x 12 floats owned
 * by the caller, updated in place: p(2) u(2) f f_prev t t_prev 0 0 w_l w_r (the first twelve of osa_car_goal_env_step's
 * row).  A reset is osa_circle_env_step's under the same Philox key, with w_l = w_r = t_prev = 0.  obs row = [f,
 * f - f_prev, t, u, w_l, w_r, t - t_prev, 0 (16), lidar of the origin (16), 0...].  Launch: half a wave per env (two
 * envs per 64-lane workgroup), the 40 columns in two rounds of the half-wave. */
int osa_car_circle_env_step(unsigned long long seed, unsigned long long step,
                            const unsigned long long* step_base, int N, int obs_dim,
                            int horizon, int level, float* state, int* steps, const float* action, int ld_action,
                            float* obs, int ld_obs, float* reward, float* cost, uint8_t* terminated,
                            uint8_t* truncated, float* final_obs, int ld_final, int reset_only,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Trust-region machinery (NaturalPG / TRPO / TRPOLag / CPO actor update)
 *
 * Flat vectors here are PADDED actor parameter vectors of P floats (osa_mlp_layout; padding entries
 * are zero in every vector, so dot products equal those of the reference's compact flat vectors of
 * omnisafe/utils/tools.py:35-129).  The full-batch policy gradient is osa_ppo_minibatch with idx = NULL,
 * B = M, loss_kind = 1, mode = 2, nets_mask = 1 (raw gradient of -mean(ratio * adv) in grads[0]).
 * ---------------------------------------------------------------------------------------------- */

/* NaturalPG._fvp without damping (omnisafe/algorithms/on_policy/base/natural_pg.py:91-111): the
 * Hessian-vector product of mean KL(pi_old || pi_theta) -- `.mean()` over all M x act_dim elements --
 * at theta = theta_old, restricted to the mean-network parameters: J^T diag(1/sigma^2) J vec / (M D_a),
 * computed as forward-mode JVP followed by the ordinary backward pass (no double backward; exact for
 * a Gaussian policy with state-independent log_std because dKL/dmu = 0 at theta_old).  Result (raw,
 * local to this rank) in grads[0 .. P).  ws: osa_minibatch_ws_floats(.., max_blocks) floats.
 * Hidden width 64 with tanh and observations up to 80 wide run on osa_fvp_kernel (csrc/fvp_kernel.hip: theta and vec
 * resident in LDS, the gradient in registers, one slab per workgroup: 72 us per product at 65 536 rows against 162),
 * everything else on the general gradient kernel; the two produce the same bits (environment OSA_FVP_FAST=0 forces the
 * general kernel). */
int osa_actor_fvp_raw(int obs_dim, int act_dim, int hidden, float* params, float* grads,
                      const float* obs, int ld_obs, long M, const float* vec, int max_blocks,
                      float* ws, float* step_stats, void* stream);

/* out = raw + damping * v  (natural_pg.py:119) plus the analytic log_std block of the Fisher matrix:
 * out[ls_off + d] += ls_coef * v[ls_off + d], ls_coef = 2 / act_dim.  (With world_size > 1 the caller
 * averages `raw` across ranks first: distributed.avg_tensor, natural_pg.py:112.) */
int osa_fvp_finish(int n, const float* raw, const float* v, float damping, int ls_off, int ls_n,
                   float ls_coef, float* out, void* stream);

/* conjugate_gradients (omnisafe/utils/math.py:116-132) split at the Fisher-vector product:
 *   osa_cg_init: x = 0, r = b (F(0) = 0), p = r, scal[0] = r.r, scal[1] = 0 (not converged)
 *   osa_cg_step(z = F p): alpha = r.r/(p.z + eps); x += alpha p; r -= alpha z; if sqrt(r.r) <
 *     residual_tol set scal[1] = 1 (the reference's `break`; later calls are no-ops) else
 *     p = r + (r.r_new/(r.r + eps)) p.   scal: 4 floats on the device. */
int osa_cg_init(int n, const float* b, float* x, float* r, float* p, float* scal, void* stream);
int osa_cg_step(int n, const float* z, float* x, float* r, float* p, float* scal, float residual_tol,
                float eps, void* stream);

/* out = a*x + b*y (y may be NULL) and *out = x.y: step-direction algebra of trpo.py:202-222 and
 * cpo.py:284-337, parameter candidates theta_old + frac * step of the line searches. */
int osa_vec_lincomb(int n, float a, const float* x, float b, const float* y, float* out, void* stream);
int osa_vec_dot(int n, const float* x, const float* y, float* out, void* stream);

/* Full-batch evaluation of a candidate actor for the line searches (TRPO._search_step_size
 * trpo.py:102-138, CPO._cpo_search_step cpo.py:114-171): out4 = { loss_pi = -mean(ratio * adv) with
 * adv = (adv_r - lambda adv_c)/(1 + lambda), loss_cost = mean(ratio * adv_c), KL(old || new).mean(),
 * mean ratio }.  ws: at least 4096 doubles. */
int osa_actor_eval(int obs_dim, int act_dim, int hidden, const float* actor_params, const float* obs,
                   int ld_obs, long M, const float* act, int ld_act, const float* logp,
                   const float* adv_r, const float* adv_c, const float* lagrange,
                   const float* old_mean, int ld_old, const float* old_log_std, double* ws,
                   float* out4, void* stream);

/* The minibatch shuffles of an update: perm[row][0 .. M) = a pseudo-random permutation of 0 .. M-1 per row, one row
 * per pass (the DataLoader(shuffle=True) the reference iterates in every pass of _update:
 * algorithms/on_policy/base/policy_gradient.py:357-377, natural_pg.py:196-223 -- torch's RandomSampler = randperm).
 * No sort: a keyed bijection of [0, 2^k) (24 alternating Feistel steps over the two halves of k = ceil(log2 M) bits,
 * cycle-walked into [0, M)), element i of row r depends on (row_seeds[r], i) only.  row_seeds: device int64[rows]
 * (drawn by the host framework's seeded generator); perm: device int64 [rows][M].  M <= 2^40, rows <= 65535. */
int osa_shuffle_rows(const long long* row_seeds, int rows, long M, long long* perm, void* stream);

/* Deterministic evaluation of a saved policy (omnisafe/evaluator.py:399-490), K episodes in ONE launch: episode k
 * plays env index k of a device env from a fresh reset, at Philox stream positions 0 (reset), 1, 2, ... -- the
 * numbers the per-step env launches of a fresh env seeded `seed` draw for env k.  Every step: the raw observation
 * normalised with FROZEN statistics (norm_*: as osa_normalizer_apply, no push; all three NULL: no normaliser; the
 * reference's evaluator keeps pushing, normalizer.py:103), the Saute / Simmer safety column z appended when saute != 0
 * (evaluator.py:432-433; z = 1 at reset, z <- (z - cost / saute_budget) / saute_gamma in float32 after every step,
 * :456-458), the actor mean (fused family: hidden as for osa_policy_step, act_dim <= 32, policy input obs_dim + saute
 * <= 992 columns), ActionScale (old_min / old_max: act_dim floats, as osa_action_scale), the env transition.  In
 * float64: ep_ret += reward, ep_cost += cost_criteria^len * cost (:460-461), then len += 1; early_terminated != 0
 * ends the episode once ep_cost >= cost_limit (:462-466); an episode ends at its first terminated / truncated step
 * (the env's own `horizon`) or after max_steps steps.
 * env_kind: OSA_EVAL_ENV_SYNTH (osa_synth_env_step; cost_p used), OSA_EVAL_ENV_REACH (osa_reach_env_step: obs_dim
 * >= 6, act_dim >= 2), OSA_EVAL_ENV_NAV0 + level (osa_nav_env_step: obs_dim >= 60, act_dim >= 2, policy input <= 928
 * columns) or OSA_EVAL_ENV_CIRCLE0 + level (osa_circle_env_step: obs_dim >= 28, act_dim >= 2; the state stays in
 * registers), OSA_EVAL_ENV_CARGOAL0 + level (osa_car_goal_env_step: obs_dim >= 72, act_dim >= 2, policy input <= 928
 * columns) or OSA_EVAL_ENV_CARCIRCLE0 + level (osa_car_circle_env_step: obs_dim >= 40, act_dim >= 2; the state stays in
 * registers); anything else OSA_EUNSUPPORTED.  Outputs: ep_ret, ep_cost double[K], ep_len int32[K].
 * trace (NULL in production): float[max_steps][K][osa_eval_trace_floats(...)], zero-initialised by the caller; the
 * record of (step, episode) is written while the episode plays: policy input row, env action, reward, cost, 1.0
 * (alive), and the state before the step (SynthReach: 6 floats, SynthNavGoal: the 64-float row,
 * SynthNavCircle: the 8-float row, SynthNavCarGoal: the 64-float row, SynthNavCarCircle: the 12-float row).  Arguments
 * are checked before any launch. */
#define OSA_EVAL_ENV_SYNTH 0
#define OSA_EVAL_ENV_REACH 1
#define OSA_EVAL_ENV_NAV0 16 /* + level 0 .. 2 */
#define OSA_EVAL_ENV_CIRCLE0 32 /* + level 0 .. 2 */
#define OSA_EVAL_ENV_CARGOAL0 48 /* + level 0 .. 2 */
#define OSA_EVAL_ENV_CARCIRCLE0 64 /* + level 0 .. 2 */
int osa_eval_episodes(int env_kind, int K, int obs_dim, int act_dim, int hidden, const float* params,
                      const float* norm_mean, const float* norm_std, const long* norm_count, float norm_clip,
                      const float* old_min, const float* old_max, float min_action, float max_action,
                      unsigned long long seed, int horizon, float cost_p, int max_steps, int saute,
                      float saute_budget, float saute_gamma, int early_terminated, double cost_limit,
                      double cost_criteria, double* ep_ret, double* ep_cost, int* ep_len, float* trace,
                      void* stream);

/* Floats per trace record of osa_eval_episodes (0 for bad dims). */
int osa_eval_trace_floats(int env_kind, int obs_dim, int act_dim, int saute);

/* Stochastic data collection with a saved policy (omnisafe/common/offline/data_collector.py:145-190), one agent's block
 * of total_rows = S dataset rows in ONE launch.  K lanes; lane k plays env index k of a device env from a fresh reset,
 * at Philox stream positions 0 (reset), 1, 2, ... -- the numbers the per-step env launches of a fresh K-env vector env
 * seeded `seed` draw for env k -- and owns the rows [k Q, min((k + 1) Q, S)) with Q = rows_per_lane, which it fills
 * with consecutive episodes; the last one is cut off where the lane's rows end, and a lane with an empty range plays
 * nothing.  S <= K * Q.  Step t (0-based) of lane k writes row i = k Q + t (data_collector.py:166-189):
 *   obs[i]      the RAW env observation; the policy sees it normalised with FROZEN statistics (norm_*: as
 *               osa_eval_episodes; all three NULL: no normaliser);
 *   action[i]   the actor's sample mean + exp(log_std) * eps BEFORE ActionScale (fused family: hidden as for
 *               osa_policy_step, act_dim <= 32); eps of dimension d is the first Box-Muller output of the Philox block
 *               (noise_seed, t + 1, k * act_dim + d): what osa_policy_step draws for row k on the (t + 1)-th step of a
 *               fresh actor seeded noise_seed.  The env receives the scaled action (old_min / old_max: act_dim floats,
 *               as osa_action_scale);
 *   reward[i], cost[i]   of the transition;
 *   next_obs[i] the raw observation of the post-transition state, whether or not the episode ends;
 *   done[i]     1.0 where the step terminates (a description with terminal()) or is the `horizon`-th of its episode
 *               (the time limit is per lane), else 0.0.  After a done row the lane is reset at the SAME stream position
 *               and obs[i + 1] is the observation of the fresh state; otherwise obs[i + 1] = next_obs[i].
 * obs, next_obs: float [S][ld_obs >= obs_dim], [S][ld_next >= obs_dim]; action: float [S][ld_act >= act_dim]; reward,
 * cost, done: float [S].  Only columns [0, obs_dim) / [0, act_dim) of rows [0, S) are written.  ep_ret_sum,
 * ep_cost_sum: double[K], the sums of reward and cost over the lane's rows in row order; ep_count: int32[K], its done
 * rows (data_collector.py:178-194 per lane).
 * env_kind: as osa_eval_episodes, with its least widths; observations up to 304 columns (288 for the kinds with a 64-
 * float state row) -- wider ones, and what osa_eval_episodes refuses: OSA_EUNSUPPORTED.  Arguments are checked before
 * any launch. */
int osa_collect_episodes(int env_kind, int K, int rows_per_lane, long total_rows, int obs_dim, int act_dim, int hidden,
                         const float* params, const float* norm_mean, const float* norm_std, const long* norm_count,
                         float norm_clip, const float* old_min, const float* old_max, float min_action,
                         float max_action, unsigned long long seed, unsigned long long noise_seed, int horizon,
                         float cost_p, float* obs, int ld_obs, float* action, int ld_act, float* reward, float* cost,
                         float* next_obs, int ld_next, float* done, double* ep_ret_sum, double* ep_cost_sum,
                         int* ep_count, void* stream);

/* Rasterised replay of one episode of a geometric device env: frames first .. first + count - 1 of a top-down picture
 * of its state rows, written to rgb as uint8 [count][height][width][3].  The picture is a specification of this
 * package (the reference renders through MuJoCo, third-party CPU code: omnisafe/evaluator.py:511-629 only collects
 * env.render() frames); tests/render_twin.py restates it in numpy and reproduces every byte.
 * env_kind: as osa_eval_episodes -- OSA_EVAL_ENV_REACH, or OSA_EVAL_ENV_NAV0 / CIRCLE0 / CARGOAL0 / CARCIRCLE0 + level
 * 0 .. 2; OSA_EVAL_ENV_SYNTH (no state to draw) and anything else: OSA_EUNSUPPORTED.
 * state: the state row of record 0; record f at state + f * stride floats (episode k of a trace [T][K][rec]:
 * trace + k * rec + (rec - state floats), stride = K * rec).  Row layouts as the env entry points above: SynthReach p,
 * goal, hazard; SynthNavGoal / SynthNavCarGoal p (0, 1), u (2, 3), goal (8, 9), hazards from 12, vases from 32, their
 * counts per level those of the env (0 / 8 / 10 hazards, 0 / 1 / 10 vases); SynthNavCircle / SynthNavCarCircle p, u.
 * Frame f shows record f and the robot's path through records max(0, f - trail) .. f as segments between consecutive
 * positions; nothing before record 0 is read, and a call for frames first .. gives the bytes that a call from 0 gives
 * for them.  hit: NULL or uint8[first + count]; hit[f] != 0 draws the robot of frame f in the hit colour (the caller
 * sets it when record f - 1 had a positive cost).
 * camera 0 (fixed): centre c = (0, 0), half-width 2.25 (SynthReach 1.75), the whole arena; camera 1 (track): c = p of
 * the frame's record, half-width 1.
 * Sub-sample (a, b), 0 <= a, b < S = supersample, of pixel (row i, column j), all in float32 without fused
 * multiply-adds, W = width, H = height:
 *   h = half / float(min(W, H) * S);  x = c.x + float(2 * (j * S + b) + 1 - W * S) * h;
 *   y = c.y + float(H * S - 2 * (i * S + a) - 1) * h   (y points up; the integers are exact in float32).
 * Tests: a disc of centre o and squared radius r2 holds (x, y) iff dx * dx + dy * dy <= r2 with d = (x, y) - o.  A
 * segment from s with extent e at squared half-width hw2: w = (x, y) - s, L2 = e.x * e.x + e.y * e.y,
 * t = L2 == 0 ? 0 : min(max((w.x * e.x + w.y * e.y) / L2, 0), 1), d = w - t * e, inside iff d.x * d.x + d.y * d.y <=
 * hw2 (a robot that stands still gives L2 == 0: the disc of squared radius hw2 round s).
 * Layers, the later one wins; A = 2 (SynthReach 1.5) the arena's half-width:
 *   1 outside    everywhere                                                     (40, 44, 52)
 *   2 floor      |x| <= A and |y| <= A                                          (236, 236, 228)
 *   3 circle tasks: cost region, on the floor where (level >= 1 and |x| > 0.75)
 *     or (level == 2 and |y| > 0.75)                                            (244, 204, 196)
 *     ring       0.9604 <= x * x + y * y <= 1.0404                              (96, 160, 96)
 *   4 hazards    discs, r2 = 0.04 (SynthReach's one hazard 0.09)                (90, 100, 220)
 *   5 goal       disc, r2 = 0.09 (SynthReach 0.0225); the circle tasks have none (70, 190, 90)
 *   6 vases      discs, r2 = 0.01                                               (80, 200, 210)
 *   7 trail      segments record g -> g + 1, e = p[g + 1] - p[g], hw2 = 0.0004  (250, 160, 40)
 *   8 robot      disc round p, r2 = 0.01 (SynthReach 0.0025): Point             (200, 40, 40)
 *                Car (130, 50, 170), either when hit                            (255, 0, 200)
 *   9 heading    segment from p, e = (p + 0.2 * u) - p, hw2 = 0.0009; not SynthReach (20, 20, 20)
 * with every constant the nearest float32.  A channel of a pixel is (sum over its S * S sub-samples + S * S / 2) /
 * (S * S) in integers.
 * OSA_EINVAL before any launch unless: state and rgb non-NULL, rgb 4-byte aligned, count >= 1, first >= 0, trail >= 0,
 * 4 <= width <= 4096 with width % 4 == 0, 1 <= height <= 4096, 1 <= supersample <= 4, camera 0 or 1.
 * OSA_EUNSUPPORTED when count * ceil(width * height / 1024) exceeds 2^31 - 1 (render fewer frames per call).
 * Launch: 256 lanes per 1024 pixels of one frame, a lane 4 horizontally adjacent pixels and one 12-byte store; the
 * frame's row and trail staged in LDS; workgroups are independent (no atomics, no flags). */
int osa_render_episode(int env_kind, const float* state, long stride, int first, int count, int trail,
                       const uint8_t* hit, int camera, int width, int height, int supersample, uint8_t* rgb,
                       void* stream);

/* ---- offline CRR / CCRR (csrc/crr_kernels.hip) ---------------------------------------------------------------------
 * Critic Regularized Regression and its constrained form trained from a device-resident dataset
 * (omnisafe/algorithms/offline/crr.py, c_crr.py).  Networks: a gaussian_learning actor (obs -> act, log_std behind the
 * layers) and `pairs` pairs of Q critics (obs || act -> 1) with a target copy each; every network is one padded float32
 * block in the layout of osa_gmlp_layout (W_l [out][in rounded to 4], b_l rounded to 4, ...), block strides Pa and Pc.
 * Critic blocks in order: reward critic 0, 1, then (pairs == 2) cost critic 0, 1.  At least one hidden layer. */
#define OSA_CRR_NSTAT 12
/* a step's statistics row: 0 Loss_reward_critic, 1 data_Qr, 2 target_Qr, 3 Loss_cost_critic, 4 data_Qc, 5 target_Qc,
 * 6 Loss_actor, 7 current_Qr, 8 current_Qc, 9 PolicyStd, 10 LagrangeMultiplier, 11 unused; the Q entries are FIRST-ROW
 * values (crr.py:152-153, 187), not batch means. */
typedef struct osa_crr_desc {
  int obs_dim, act_dim;
  int n_layers[2];                    /* linear layers of the actor / of a critic (hidden layers + 1) */
  int width[2][OSA_GMLP_MAX_LAYERS];  /* output widths; the last one = act_dim / 1 */
  int activation[2];                  /* OSA_ACT_* of the hidden layers */
  int batch, samples, pairs;          /* B, sampled_action_num S, 1 (CRR) or 2 (CCRR) */
} osa_crr_desc;
typedef struct osa_crr_hparams {
  float gamma, beta, polyak, one_minus_polyak; /* the two Polyak factors as float32 roundings of tau and 1 - tau */
  float lr_actor, lr_critic;
  double beta1, beta2, adam_eps; /* double: torch rounds 1 - beta to float32 from the double difference */
  float cost_limit, lambda_lr;
  int lagrange_open;    /* c_crr.py:181-185: epoch * steps_per_epoch > lagrange_start_step, constant over a block */
  int reference_wiring; /* CCRR: 1 = c_crr.py as written (the reward pair takes both critic updates and values the
                           sampled rows of the cost advantage); 0 = the cost pair has its own update */
} osa_crr_hparams;
typedef struct osa_crr_state {                /* device memory, 16-byte aligned blocks */
  float *actor, *actor_m, *actor_v;           /* [Pa] */
  float *critic, *critic_m, *critic_v;        /* [2 pairs][Pc] */
  float* target;                              /* [2 pairs][Pc] */
  int* adam_step;                             /* [1 + pairs]: actor, reward pair, cost pair */
  float* lagrange;                            /* [4]: lambda, its Adam m, v and step count (CCRR) */
  long* step;                                 /* [1] steps taken: advanced by every step on the device */
} osa_crr_state;
typedef struct osa_crr_data {                 /* the dataset: N rows of float32, never written */
  const float *obs, *act, *reward, *cost, *next_obs, *done;
  int ld_obs, ld_act, ld_next;
  long n_rows;
} osa_crr_data;
typedef struct osa_crr_draw_buffers {         /* step t reads slot t % nslots */
  const long* idx;                            /* [nslots][B] in [0, N) */
  const float *eps_next, *eps_next_c;         /* [nslots][B][act_dim]; the second draw of c_crr.py:112 (CCRR) */
  const float* eps_samp;                      /* [nslots][B S][act_dim] */
  int nslots;
} osa_crr_draw_buffers;
/* out[0..3] = Pa, Pc, offset of log_std in the actor block, OSA_CRR_NSTAT; then (oW, ob, ld) of layers
 * 0..OSA_GMLP_MAX_LAYERS-1 of the actor and of a critic (-1, -1, 0 for absent layers): 4 + 48 ints.  Host only. */
int osa_crr_layout(const osa_crr_desc* desc, int* out);
/* floats of the step's workspace; 0 for a description osa_crr_layout refuses.  Host only. */
size_t osa_crr_ws_floats(const osa_crr_desc* desc);
/* The draws of steps first_step .. first_step + nsteps - 1 into their slots (dataset.py:237-247's randint and the noise
 * of actor.predict, crr.py:134, 166, c_crr.py:112), one launch per buffer: Philox4x32-10 with key seed ^ K (K: one
 * constant per buffer), counter (step, element); idx = multiply-high of the first 64 bits into [0, n_rows); eps = the
 * first Box-Muller normal, element = row * act_dim + d.  OSA_EINVAL before any launch for a null buffer (eps_next_c may
 * be NULL with pairs == 1), nsteps < 1 or > nslots, n_rows < 1. */
int osa_crr_draws(const osa_crr_desc* desc, unsigned long long seed, long first_step, int nsteps, int nslots,
                  long n_rows, long* idx, float* eps_next, float* eps_next_c, float* eps_samp, void* stream);
/* nsteps train steps enqueued on `stream` (crr.py:114-200 / c_crr.py:91-206 per step): gather by index, reward (and
 * cost) critic update on TD targets from the target pair, actor update on the advantage-weighted log-likelihood with
 * the UPDATED critics, the Lagrange step (when lagrange_open) and the Polyak updates.  No host synchronisation and no
 * allocation; the draws' slot and the row of stats [nslots][OSA_CRR_NSTAT] follow *state->step, so a captured step
 * advances on replay.  ws: osa_crr_ws_floats floats, 16-byte aligned.  Arguments are checked before any launch:
 * OSA_EINVAL for null pointers, a short workspace, misaligned blocks, beta <= 0; OSA_EUNSUPPORTED for shapes
 * osa_crr_layout refuses (no hidden layer, more than OSA_GMLP_MAX_LAYERS linear layers, B (1 + S) > 2^20). */
int osa_crr_step(const osa_crr_desc* desc, const osa_crr_hparams* hp, const osa_crr_state* state,
                 const osa_crr_data* data, const osa_crr_draw_buffers* draws, float* stats, float* ws, size_t ws_floats,
                 int nsteps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OMNISAFE_AMD_H */
