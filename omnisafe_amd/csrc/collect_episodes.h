// The persistent collection kernel as a template over an env description (env_device.h), with its arguments and its
// launch: collect_kernels.hip instantiates it for the built-in families, csrc/custom/custom_env.hip for one description
// that is not in this tree.  It is osa_eval_episodes_kernel (eval_episodes.h) turned into a dataset writer: the policy
// SAMPLES, a lane plays episode after episode with the reset inside the kernel, and every step leaves one row
// (obs, action, reward, cost, next_obs, done) of omnisafe/common/offline/data_collector.py:166-189.
#pragma once
#include "eval_episodes.h"

struct OsaCollectArgs {
  // The actor, the frozen normaliser, the scale bounds and the env (seed, horizon, cost_p, level) as the evaluation
  // kernel takes them.  K: lanes; max_steps: rows per lane Q; ep_ret / ep_cost / ep_len: the per-lane float64 sums of
  // reward and cost over the lane's rows and the episodes it finished.  No saute column, no early termination.
  OsaEvalArgs ev;
  long total_rows;  // S: lane k owns rows [k Q, min((k + 1) Q, S))
  unsigned long long noise_seed;
  float *obs, *action, *reward, *cost, *next_obs, *done;
  int ld_obs, ld_act, ld_next;
};

// The actor's sample of (row, dimension) `idx` at noise-stream position `offset`: policy_rows.h:29-42 in its words, and
// like them outside the `fp contract(off)` region below, so that this kernel and osa_policy_step_kernel round
// mu + eps sigma alike.
__device__ __forceinline__ float osa_collect_sample(float mu, float log_std, unsigned long long seed,
                                                    unsigned long long offset, unsigned long long idx) {
  const float sd = expf(log_std);
  uint32_t w[4];
  osa_philox(seed, offset, idx, w);
  float e, e1;
  osa_box_muller(w[0], w[1], e, e1);
  return mu + e * sd;  // Normal.rsample: loc + eps * scale
}

#pragma clang fp contract(off)
// The RAW env observation of lane k's state into its LDS row, lane group g taking a quarter of the columns.
// after_end: the row follows a reset at the position of an ending step (not the reset at position 0).
template <class E>
__device__ __forceinline__ void osa_collect_obs(const OsaEvalArgs& a, float* __restrict__ rrow, int g,
                                                const typename E::Regs& s, const float* __restrict__ srow,
                                                const OsaEnvAt&, bool) {
  for (int c = g; c < a.obs_dim; c += 4) rrow[c] = E::obs_col(s, srow, a.level, c);
}
// The noise env draws both rows of a position pair-wise: (v0, v1) the observation of the step (and of the reset at
// position 0), (c2, d2) the one after the reset of an ending step (osa_synth_env_kernel).
template <>
__device__ __forceinline__ void osa_collect_obs<OsaSynthEnv>(const OsaEvalArgs& a, float* __restrict__ rrow, int g,
                                                             const OsaSynthEnv::Regs&, const float* __restrict__,
                                                             const OsaEnvAt& at, bool after_end) {
  const int D = a.obs_dim;
  for (int pair = g; 2 * pair < D; pair += 4) {
    float v0, v1, c2, d2;
    osa_synth_obs_pair(at.seed, at.pos, at.n, pair, v0, v1, c2, d2);
    rrow[2 * pair] = after_end ? c2 : v0;
    if (2 * pair + 1 < D) rrow[2 * pair + 1] = after_end ? d2 : v1;
  }
}

// The row-wise store form (OSA_COLLECT_ROW_STORES; measured slower than the column-strided stores of the kernel and
// kept for the comparison).  `width` columns of the 16 LDS rows `src` (row stride ld_src) to the dataset rows
// first_row(slot) + t of `dst`: the wave walks along the columns of one slot's row, then along the next slot's, so that a store instruction covers whole
// contiguous pieces of rows (64 consecutive columns of a wide row, several whole rows of a narrow one) and not one
// 4-byte word in each of 16 rows.  A slot past K or whose rows have ended before step t writes nothing.
// OsaRowWalk: where a lane starts in the 16 x width elements and how 64 elements further on moves it (computed once).
struct OsaRowWalk {
  int width, slot0, c0, dq, dr;
};
__device__ __forceinline__ OsaRowWalk osa_row_walk(int width, int lane) {
  return {width, lane / width, lane % width, 64 / width, 64 % width};
}
__device__ __forceinline__ void osa_collect_put(float* __restrict__ dst, int ld, const OsaRowWalk& w,
                                                const float* __restrict__ src, int ld_src, int t, int Q, int block_k,
                                                int K, long S) {
  int slot = w.slot0, c = w.c0;
  while (slot < 16) {
    const int k = block_k + slot;
    const long row = (long)k * Q + t;
    if (k < K && row < S) dst[row * ld + c] = src[slot * ld_src + c];
    c += w.dr;
    slot += w.dq;
    if (c >= w.width) {
      c -= w.width;
      ++slot;
    }
  }
}

// E: the family's description (env_device.h).  Slot mapping of osa_eval_episodes_kernel: lane k of the dataset is row
// j = k & 15 of the wave of workgroup k / 16, and the four lane groups g = lane >> 4 share the columns of its rows.
// LDS, in floats: 16 policy input rows [INP] | 16 env action rows | 16 sample rows | 2 x 16 raw observation rows
// [INP + 1] (this step's and the next one's, swapping roles every step; the odd stride spreads the column-wise accesses
// of the 16 slots over the banks) | 16 state rows with LDS_ROW.
template <int HT, int OT, class E>
__global__ __launch_bounds__(64) void osa_collect_episodes_kernel(OsaCollectArgs ca) {
  extern __shared__ f32x4 osa_collect_lds[];
  const OsaEvalArgs& a = ca.ev;
  const OsaNet& nd = a.nd;
  const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
  const int block_k = blockIdx.x * 16, k = block_k + j;
  const int Q = a.max_steps, INP = nd.INP, RW = INP + 1;
  // the rows of lane k: [k Q, min((k + 1) Q, S)), none for a lane past K or past the end of the block
  long left = ca.total_rows - (long)k * Q;
  left = left < 0 ? 0 : (left > Q ? Q : left);
  const int rows = k < a.K ? (int)left : 0;
  float* const lds = reinterpret_cast<float*>(osa_collect_lds);
  float* __restrict__ xrow = lds + j * INP;
  float* __restrict__ arow = lds + 16 * INP + j * OSA_EVAL_ACT_LD;
  float* const samples = lds + 16 * (INP + OSA_EVAL_ACT_LD);
  float* __restrict__ urow = samples + j * OSA_EVAL_ACT_LD;
  float* const raw = samples + 16 * OSA_EVAL_ACT_LD;
  float* __restrict__ srow = raw + 2 * 16 * RW + j * E::STATE;
  const bool norm_on = a.mean != nullptr && *a.count > 1;
  // reset (stream position 0), as the evaluation kernel's
  OsaEnvAt at = {a.seed, 0, k, a.level, a.cost_p};
  typename E::Regs s = {};
  if constexpr (E::LDS_ROW) {
    for (int c = OSA_NAV_DYN + g; c < E::STATE; c += 4) srow[c] = rows > 0 ? E::fresh_obj(at, c) : 0.f;
    __syncthreads();
  }
  E::fresh(s, at, srow);
  {
    float* __restrict__ rrow = raw + j * RW;
    if (rows > 0) {
      osa_collect_obs<E>(a, rrow, g, s, srow, at, false);
      for (int c = g; c < a.obs_dim; c += 4) xrow[c] = osa_eval_norm(a, norm_on, rrow[c], c);
    }
  }
  double ret = 0.0, cost = 0.0;
  int count = 0, episodes = 0;  // steps of the running episode; episodes finished
  for (int t = 0; t < Q; ++t) {
    const bool live = t < rows;
    if (__ballot(live) == 0) break;  // (one wave per workgroup: a uniform exit; rows never grows with t)
    float* const cur = raw + (t & 1) * 16 * RW;
    float* const nxt = raw + ((t + 1) & 1) * 16 * RW;
    float* __restrict__ nrow = nxt + j * RW;
    __syncthreads();  // this step's input rows and raw rows are in LDS
    f32x4 h1[HT], h2[HT], out[OT];
    osa_mlp_forward<HT, OT>(nd, a.params, live ? xrow : nullptr, INP, true, h1, h2, out);
#pragma unroll
    for (int o = 0; o < OT; ++o) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 16 * o + 4 * g + r;
        if (d < nd.act_dim) {
          const float u = osa_collect_sample(out[o][r], a.params[nd.oLS + d], ca.noise_seed,
                                             (unsigned long long)t + 1, (unsigned long long)k * nd.act_dim + d);
          urow[d] = u;  // the row's `action`: the sample before ActionScale
          arow[d] = osa_action_scale1(u, a.old_min[d], a.old_max[d], a.min_a, a.max_a);
        }
      }
    }
    __syncthreads();  // the row's env action is in LDS; the forward's reads of the input row are done
    at.pos = (unsigned long long)t + 1;
    float rw, cs;
    osa_env_transition<E>(s, srow, at, arow, rw, cs);
    const bool term = osa_env_terminal<E>(s, srow, at);
    count += 1;
    const bool end = term || count >= a.horizon;  // (termination wins over a time limit reached on the same step)
    // the observation of the post-transition state, whether or not the episode ends: next_obs of this row
    if (live) osa_collect_obs<E>(a, nrow, g, s, srow, at, false);
    if (live) {
      ret = ret + (double)rw;
      cost = cost + (double)cs;
      if (end) episodes += 1;
    }
    __syncthreads();  // every slot's next row is whole; the reads of the state rows are done
#ifndef OSA_COLLECT_ROW_STORES
    // Every lane stores the columns it computed: a store instruction puts 4-byte words into the 16 rows of the wave,
    // each row getting the words of its four lane groups.  The row-wise form below costs more than it saves
    // (profiles/collect_timing.json: 1.20 x the time on SynthReach-v0, 1.13 x on SynthNavGoal1-v0 at K = 4096): the
    // walk adds LDS reads and a divergent loop per step, and the memory system evidently merges the words of a row.
    if (live) {
      const long row = (long)k * Q + t;
      const float* __restrict__ crow = cur + j * RW;
      for (int c = g; c < a.obs_dim; c += 4) {
        ca.obs[row * ca.ld_obs + c] = crow[c];
        ca.next_obs[row * ca.ld_next + c] = nrow[c];
      }
      for (int d = g; d < nd.act_dim; d += 4) ca.action[row * ca.ld_act + d] = urow[d];
    }
#else
    // The row-wise form, built for comparison only (tools/collect_timing.py): osa_collect_put.
    const OsaRowWalk obs_walk = osa_row_walk(a.obs_dim, lane), act_walk = osa_row_walk(nd.act_dim, lane);
    osa_collect_put(ca.obs, ca.ld_obs, obs_walk, cur, RW, t, Q, block_k, a.K, ca.total_rows);
    osa_collect_put(ca.next_obs, ca.ld_next, obs_walk, nxt, RW, t, Q, block_k, a.K, ca.total_rows);
    osa_collect_put(ca.action, ca.ld_act, act_walk, samples, OSA_EVAL_ACT_LD, t, Q, block_k, a.K, ca.total_rows);
#endif
    if (live && g == 0) {
      const long row = (long)k * Q + t;
      ca.reward[row] = rw;
      ca.cost[row] = cs;
      ca.done[row] = end ? 1.f : 0.f;
    }
    // the reset of an ending step, at the step's own stream position: what the per-step kernels do on `trunc`
    // (env_frame.h: osa_custom_env_kernel; rollout_kernels.hip: osa_goal_env_kernel for a row with objects)
    if (end) count = 0;
    if constexpr (E::LDS_ROW) {
      if (end)
        for (int c = OSA_NAV_DYN + g; c < E::STATE; c += 4) srow[c] = live ? E::fresh_obj(at, c) : 0.f;
    }
    __syncthreads();  // the stores have read the next rows; the fresh objects are in LDS
    if (end) {
      E::fresh(s, at, srow);
      if (live) osa_collect_obs<E>(a, nrow, g, s, srow, at, true);  // obs of the following row: the fresh reset
    }
    // (each lane normalises the columns it wrote itself)
    if (live)
      for (int c = g; c < a.obs_dim; c += 4) xrow[c] = osa_eval_norm(a, norm_on, nrow[c], c);
  }
  if (k < a.K && g == 0) {
    a.ep_ret[k] = ret;
    a.ep_cost[k] = cost;
    a.ep_len[k] = episodes;
  }
}
#pragma clang fp contract(fast)

// The argument checks every collection entry point makes before it looks at the env.
static inline int osa_collect_check(int K, int rows_per_lane, long total_rows, int obs_dim, int act_dim,
                                    const float* params, const float* norm_mean, const float* norm_std,
                                    const long* norm_count, const float* old_min, const float* old_max,
                                    float min_action, float max_action, int horizon, const float* obs, int ld_obs,
                                    const float* action, int ld_act, const float* reward, const float* cost,
                                    const float* next_obs, int ld_next, const float* done, const double* ep_ret_sum,
                                    const double* ep_cost_sum, const int* ep_count) {
  OSA_REQUIRE(K >= 1 && rows_per_lane >= 1 && total_rows >= 1 && obs_dim >= 1 && act_dim >= 1 && horizon >= 1);
  OSA_REQUIRE(total_rows <= (long)K * rows_per_lane);  // every row has an owner
  OSA_REQUIRE(params && old_min && old_max && max_action != min_action);
  OSA_REQUIRE((norm_mean == nullptr) == (norm_std == nullptr) && (norm_mean == nullptr) == (norm_count == nullptr));
  OSA_REQUIRE(obs && action && reward && cost && next_obs && done && ep_ret_sum && ep_cost_sum && ep_count);
  OSA_REQUIRE(ld_obs >= obs_dim && ld_next >= obs_dim && ld_act >= act_dim);
  return OSA_OK;
}

// A block of total_rows rows of description E at `level`, after osa_collect_check: the remaining checks, the arguments
// and the launch.
template <class E>
static int osa_collect_launch(int level, int K, int rows_per_lane, long total_rows, int obs_dim, int act_dim,
                              int hidden, const float* params, const float* norm_mean, const float* norm_std,
                              const long* norm_count, float norm_clip, const float* old_min, const float* old_max,
                              float min_action, float max_action, unsigned long long seed,
                              unsigned long long noise_seed, int horizon, float cost_p, float* obs, int ld_obs,
                              float* action, int ld_act, float* reward, float* cost, float* next_obs, int ld_next,
                              float* done, double* ep_ret_sum, double* ep_cost_sum, int* ep_count, void* stream) {
  OSA_REQUIRE(obs_dim >= E::OBS && act_dim >= E::ACT);
  const int rc = osa_check_dims(obs_dim, act_dim, hidden);
  if (rc != OSA_OK) return rc;
  OsaCollectArgs ca;
  OsaEvalArgs& a = ca.ev;
  a.nd = osa_make_net(obs_dim, act_dim, hidden);
  const size_t lds =
      (size_t)16 * (a.nd.INP + 2 * OSA_EVAL_ACT_LD + 2 * (a.nd.INP + 1) + (E::LDS_ROW ? E::STATE : 0)) * sizeof(float);
  if (lds > 65536) return OSA_EUNSUPPORTED;  // observations wider than 304 columns (288 with a 64-float state row)
  a.params = params;
  a.K = K; a.obs_dim = obs_dim; a.max_steps = rows_per_lane; a.horizon = horizon;
  a.mean = norm_mean; a.std_ = norm_std; a.count = norm_count; a.clip = norm_clip;
  a.old_min = old_min; a.old_max = old_max; a.min_a = min_action; a.max_a = max_action;
  a.seed = seed; a.cost_p = cost_p;
  a.saute = 0; a.budget = 0.f; a.saute_gamma = 0.f;
  a.early_terminated = 0; a.cost_limit = 0.0; a.cost_criteria = 1.0;
  a.ep_ret = ep_ret_sum; a.ep_cost = ep_cost_sum; a.ep_len = ep_count; a.trace = nullptr;
  a.rec = 0;
  a.level = level;
  ca.total_rows = total_rows; ca.noise_seed = noise_seed;
  ca.obs = obs; ca.action = action; ca.reward = reward; ca.cost = cost; ca.next_obs = next_obs; ca.done = done;
  ca.ld_obs = ld_obs; ca.ld_act = ld_act; ca.ld_next = ld_next;
  const dim3 grid((unsigned)((K + 15) / 16));
#define OSA_CALL(HT, OT, NSB) \
  hipLaunchKernelGGL((osa_collect_episodes_kernel<HT, OT, E>), grid, dim3(64), lds, osa_stream(stream), ca)
  OSA_DISPATCH_OT(a.nd, OSA_CALL);
#undef OSA_CALL
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}
