// The persistent collection kernel as a template over an env description (env_device.h), with its arguments and its
// launch: collect_kernels.hip instantiates it for the built-in families, csrc/custom/custom_env.hip for one description
// that is not in this tree.  It is osa_eval_episodes_kernel (eval_episodes.h) turned into a dataset writer: the policy
// SAMPLES, a lane plays episode after episode with the reset inside the kernel, and every step leaves one row
// (obs, action, reward, cost, next_obs, done) of omnisafe/common/offline/data_collector.py:166-189.
#pragma once
#include "play_episodes.h"

// K: lanes; max_steps: rows per lane Q; ep_ret / ep_cost / ep_len: the per-lane float64 sums of reward and cost over the
// lane's rows and the episodes it finished.
struct OsaCollectArgs : OsaPlayArgs {
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
// E: the family's description (env_device.h).  Slot mapping of osa_eval_episodes_kernel: lane k of the dataset is row
// j = k & 15 of the wave of workgroup k / 16, and the four lane groups g = lane >> 4 share the columns of its rows.
// LDS, in floats: 16 policy input rows [INP] | 16 env action rows | 16 sample rows | 2 x 16 raw observation rows
// [INP + 1] (this step's and the next one's, swapping roles every step; the odd stride spreads the column-wise accesses
// of the 16 slots over the banks) | 16 state rows with LDS_ROW.
template <int HT, int OT, class E>
__global__ __launch_bounds__(64) void osa_collect_episodes_kernel(OsaCollectArgs a) {
  extern __shared__ f32x4 osa_collect_lds[];
  const OsaNet& nd = a.nd;
  const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
  const int block_k = blockIdx.x * 16, k = block_k + j;
  const int Q = a.max_steps, INP = nd.INP, RW = INP + 1;
  // the rows of lane k: [k Q, min((k + 1) Q, S)), none for a lane past K or past the end of the block
  long left = a.total_rows - (long)k * Q;
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
  osa_play_fresh_objects<E>(srow, g, at, rows > 0);
  if constexpr (E::LDS_ROW) __syncthreads();
  OsaParamRow<E> par;  // the running episode's parameters (a description with PARAMS), redrawn at every reset
  osa_play_params<E>(a, s, at, par);
  E::fresh(s, at, srow);
  // the RAW env observation into the lane's LDS row being written: the reset's, then every step's next one
  float* nrow = raw + j * RW;
  const auto put = [&](int c, float v) { nrow[c] = v; };
  if (rows > 0) {
    osa_play_obs<E>(a, g, s, srow, at, false, put);
    for (int c = g; c < a.obs_dim; c += 4) xrow[c] = osa_play_norm(a, norm_on, nrow[c], c);
  }
  double ret = 0.0, cost = 0.0;
  int count = 0, episodes = 0;  // steps of the running episode; episodes finished
  for (int t = 0; t < Q; ++t) {
    const bool live = t < rows;
    if (__ballot(live) == 0) break;  // (one wave per workgroup: a uniform exit; rows never grows with t)
    float* const cur = raw + (t & 1) * 16 * RW;
    float* const nxt = raw + ((t + 1) & 1) * 16 * RW;
    nrow = nxt + j * RW;
    __syncthreads();  // this step's input rows and raw rows are in LDS
    f32x4 h1[HT], h2[HT], out[OT];
    osa_mlp_forward<HT, OT>(nd, a.params, live ? xrow : nullptr, INP, true, h1, h2, out);
#pragma unroll
    for (int o = 0; o < OT; ++o) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 16 * o + 4 * g + r;
        if (d < nd.act_dim) {
          const float u = osa_collect_sample(out[o][r], a.params[nd.oLS + d], a.noise_seed,
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
    if (live) osa_play_obs<E>(a, g, s, srow, at, false, put);
    if (live) {
      ret = ret + (double)rw;
      cost = cost + (double)cs;
      if (end) episodes += 1;
    }
    __syncthreads();  // every slot's next row is whole; the reads of the state rows are done
    // Every lane stores the columns it computed: a store instruction puts 4-byte words into the 16 rows of the wave,
    // each row getting the words of its four lane groups.  A row-wise form (the wave walking along one slot's row at a
    // time) cost more than it saved (profiles/collect_row_stores.json: 1.20 x the time on SynthReach-v0, 1.13 x on
    // SynthNavGoal1-v0 at K = 4096): the walk adds LDS reads and a divergent loop per step, and the memory system
    // evidently merges the words of a row.
    if (live) {
      const long row = (long)k * Q + t;
      const float* __restrict__ crow = cur + j * RW;
      for (int c = g; c < a.obs_dim; c += 4) {
        a.obs[row * a.ld_obs + c] = crow[c];
        a.next_obs[row * a.ld_next + c] = nrow[c];
      }
      for (int d = g; d < nd.act_dim; d += 4) a.action[row * a.ld_act + d] = urow[d];
    }
    if (live && g == 0) {
      const long row = (long)k * Q + t;
      a.reward[row] = rw;
      a.cost[row] = cs;
      a.done[row] = end ? 1.f : 0.f;
    }
    // the reset of an ending step, at the step's own stream position: what the per-step kernels do on `trunc`
    // (env_frame.h: osa_custom_env_kernel; rollout_kernels.hip: osa_goal_env_kernel for a row with objects)
    if (end) {
      count = 0;
      osa_play_fresh_objects<E>(srow, g, at, live);
    }
    __syncthreads();  // the stores have read the next rows; the fresh objects are in LDS
    if (end) {
      osa_play_params<E>(a, s, at, par);
      E::fresh(s, at, srow);
      if (live) osa_play_obs<E>(a, g, s, srow, at, true, put);  // obs of the following row: the fresh reset
    }
    // (each lane normalises the columns it wrote itself)
    if (live)
      for (int c = g; c < a.obs_dim; c += 4) xrow[c] = osa_play_norm(a, norm_on, nrow[c], c);
  }
  if (k < a.K && g == 0) {
    a.ep_ret[k] = ret;
    a.ep_cost[k] = cost;
    a.ep_len[k] = episodes;
    osa_play_params_out<E>(a, k, par);
  }
}
#pragma clang fp contract(fast)

// The argument checks every collection entry point makes before it looks at the env.
static inline int osa_collect_check(const OsaCollectArgs& a, int act_dim) {
  const int rc = osa_play_check(a, act_dim);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(a.total_rows >= 1 && a.total_rows <= (long)a.K * a.max_steps);  // every row has an owner
  OSA_REQUIRE(a.obs && a.action && a.reward && a.cost && a.next_obs && a.done);
  OSA_REQUIRE(a.ld_obs >= a.obs_dim && a.ld_next >= a.obs_dim && a.ld_act >= act_dim);
  return OSA_OK;
}

// A block of a.total_rows rows of description E at a.level, after osa_collect_check: the remaining checks, the rest of
// the arguments (nd) and the launch.
template <class E>
static int osa_collect_launch(OsaCollectArgs a, int act_dim, int hidden, void* stream) {
  OSA_REQUIRE(a.obs_dim >= E::OBS && act_dim >= E::ACT);
  const int rc = osa_check_dims(a.obs_dim, act_dim, hidden);
  if (rc != OSA_OK) return rc;
  a.nd = osa_make_net(a.obs_dim, act_dim, hidden);
  const size_t lds =
      (size_t)16 * (a.nd.INP + 2 * OSA_EVAL_ACT_LD + 2 * (a.nd.INP + 1) + (E::LDS_ROW ? E::STATE : 0)) * sizeof(float);
  if (lds > 65536) return OSA_EUNSUPPORTED;  // observations wider than 304 columns (288 with a 64-float state row)
  const dim3 grid((unsigned)((a.K + 15) / 16));
#define OSA_CALL(HT, OT, NSB) \
  hipLaunchKernelGGL((osa_collect_episodes_kernel<HT, OT, E>), grid, dim3(64), lds, osa_stream(stream), a)
  OSA_DISPATCH_OT(a.nd, OSA_CALL);
#undef OSA_CALL
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}
