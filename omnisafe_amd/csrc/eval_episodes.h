// The persistent evaluation kernel as a template over an env description (env_device.h), with its arguments and its
// launch: eval_kernels.hip instantiates it for the built-in families, csrc/custom/custom_env.hip for one description
// that is not in this tree.
#pragma once
#include "env_device.h"

struct OsaEvalArgs {
  OsaNet nd;  // actor shape; nd.obs_dim = policy input width = obs_dim + saute
  const float* params;
  int K, obs_dim, max_steps, horizon;
  const float *mean, *std_;
  const long* count;
  float clip;
  const float *old_min, *old_max;
  float min_a, max_a;
  unsigned long long seed;
  float cost_p;
  int saute;
  float budget, saute_gamma;
  int early_terminated;
  double cost_limit, cost_criteria;
  double *ep_ret, *ep_cost;
  int* ep_len;
  float* trace;
  int rec;  // floats per trace record
  int level;  // level of the env (a built-in one: env_kind - its family's OSA_EVAL_ENV_* constant)
};

#define OSA_EVAL_ACT_LD 32  // LDS row of the env actions (act_dim <= 32: osa_check_dims)

#pragma clang fp contract(off)
// normalizer.py:104-107 with frozen statistics (osa_normalize_kernel without the mask)
__device__ __forceinline__ float osa_eval_norm(const OsaEvalArgs& a, bool on, float v, int col) {
  if (on) {
    v = (v - a.mean[col]) / a.std_[col];
    v = v < -a.clip ? -a.clip : v;  // (NaN-preserving, as osa_normalize_kernel)
    v = v > a.clip ? a.clip : v;
  }
  return v;
}

// The env observation of episode k (at) into its LDS input row, lane group g taking a quarter of the columns.
template <class E>
__device__ __forceinline__ void osa_eval_obs(const OsaEvalArgs& a, bool norm_on, float* __restrict__ xrow, int g,
                                             const typename E::Regs& s, const float* __restrict__ srow,
                                             const OsaEnvAt&) {
  for (int c = g; c < a.obs_dim; c += 4) xrow[c] = osa_eval_norm(a, norm_on, E::obs_col(s, srow, a.level, c), c);
}
// The noise env draws its observation pair-wise: the non-truncating draw (v0, v1) of every feature pair.
template <>
__device__ __forceinline__ void osa_eval_obs<OsaSynthEnv>(const OsaEvalArgs& a, bool norm_on, float* __restrict__ xrow,
                                                          int g, const OsaSynthEnv::Regs&, const float* __restrict__,
                                                          const OsaEnvAt& at) {
  const int D = a.obs_dim;
  for (int pair = g; 2 * pair < D; pair += 4) {
    float v0, v1, c2, d2;
    osa_synth_obs_pair(at.seed, at.pos, at.n, pair, v0, v1, c2, d2);
    xrow[2 * pair] = osa_eval_norm(a, norm_on, v0, 2 * pair);
    if (2 * pair + 1 < D) xrow[2 * pair + 1] = osa_eval_norm(a, norm_on, v1, 2 * pair + 1);
  }
}

// E: the family's description (env_device.h).
template <int HT, int OT, class E>
__global__ __launch_bounds__(64) void osa_eval_episodes_kernel(OsaEvalArgs a) {
  extern __shared__ f32x4 osa_eval_lds[];
  const OsaNet& nd = a.nd;
  const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
  const int k = blockIdx.x * 16 + j;
  const bool valid = k < a.K;
  const int in_w = nd.obs_dim, INP = nd.INP;
  float* __restrict__ xrow = reinterpret_cast<float*>(osa_eval_lds) + j * INP;
  float* __restrict__ arow = reinterpret_cast<float*>(osa_eval_lds) + 16 * INP + j * OSA_EVAL_ACT_LD;
  const bool norm_on = a.mean != nullptr && *a.count > 1;
  // reset (stream position 0).  A family with objects keeps the state row of episode k in LDS behind the action rows;
  // what a transition changes is in registers either way.
  OsaEnvAt at = {a.seed, 0, k, a.level, a.cost_p};
  float* __restrict__ srow = reinterpret_cast<float*>(osa_eval_lds) + 16 * (INP + OSA_EVAL_ACT_LD) + j * E::STATE;
  typename E::Regs s = {};
  if constexpr (E::LDS_ROW) {
    for (int c = OSA_NAV_DYN + g; c < E::STATE; c += 4) srow[c] = valid ? E::fresh_obj(at, c) : 0.f;
    __syncthreads();  // the row's hazards are in LDS (the reset places the goal away from them)
  }
  E::fresh(s, at, srow);
  if (valid) osa_eval_obs<E>(a, norm_on, xrow, g, s, srow, at);
  float z = 1.f;  // Saute / Simmer safety budget left (evaluator.py:415)
  if (a.saute && g == 0) xrow[a.obs_dim] = z;
  double ret = 0.0, cost = 0.0;
  int len = 0;
  bool alive = valid;
  for (int t = 0; t < a.max_steps; ++t) {
    if (__ballot(alive) == 0) break;  // (one wave per workgroup: a uniform exit)
    __syncthreads();  // this step's input rows are in LDS
    float* rec = (a.trace != nullptr && alive) ? a.trace + ((long)t * a.K + k) * a.rec : nullptr;
    if (rec)
      for (int c = g; c < in_w; c += 4) rec[c] = xrow[c];
    f32x4 h1[HT], h2[HT], out[OT];
    osa_mlp_forward<HT, OT>(nd, a.params, valid ? xrow : nullptr, INP, true, h1, h2, out);
#pragma unroll
    for (int o = 0; o < OT; ++o) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 16 * o + 4 * g + r;
        if (d < nd.act_dim) {
          const float act = osa_action_scale1(out[o][r], a.old_min[d], a.old_max[d], a.min_a, a.max_a);
          arow[d] = act;
          if (rec) rec[in_w + d] = act;
        }
      }
    }
    __syncthreads();  // the row's env action is in LDS; the forward's reads of the input row are done
    at.pos = (unsigned long long)t + 1;
    const bool trunc = t + 1 >= a.horizon;
    float rw, cs;
    if (rec && E::LDS_ROW)  // the lane groups share the columns of a row in LDS; lane group 0 writes out registers
      for (int q = g; q < E::TRACE; q += 4) rec[in_w + nd.act_dim + 3 + q] = E::state_col(s, srow, q);
    if (rec && !E::LDS_ROW && g == 0) {
#pragma unroll
      for (int q = 0; q < E::TRACE; ++q) rec[in_w + nd.act_dim + 3 + q] = E::state_col(s, srow, q);
    }
    osa_env_transition<E>(s, srow, at, arow, rw, cs);
    // the description's own end of the episode (a compile-time false for one without terminal(): the built-in families)
    const bool env_terminal = osa_env_terminal<E>(s, srow, at);
    if (rec && g == 0) {
      rec[in_w + nd.act_dim + 0] = rw;
      rec[in_w + nd.act_dim + 1] = cs;
      rec[in_w + nd.act_dim + 2] = 1.f;
    }
    if (alive) {  // evaluator.py:455-468, in its order
      if (a.saute) {
        z = z - cs / a.budget;
        z = z / a.saute_gamma;
      }
      ret = ret + (double)rw;
      cost = cost + pow(a.cost_criteria, (double)len) * (double)cs;
      const bool term = a.early_terminated && cost >= a.cost_limit;
      len += 1;
      if (term || trunc || env_terminal) {
        alive = false;
        if (g == 0) {
          a.ep_ret[k] = ret;
          a.ep_cost[k] = cost;
          a.ep_len[k] = len;
        }
      } else {
        osa_eval_obs<E>(a, norm_on, xrow, g, s, srow, at);
        if (a.saute && g == 0) xrow[a.obs_dim] = z;
      }
    }
  }
  if (alive && g == 0) {  // max_steps reached first
    a.ep_ret[k] = ret;
    a.ep_cost[k] = cost;
    a.ep_len[k] = len;
  }
}
#pragma clang fp contract(fast)

// The argument checks every entry point makes before it looks at the env.
static inline int osa_eval_check(int K, int obs_dim, int act_dim, const float* params, const float* norm_mean,
                                 const float* norm_std, const long* norm_count, const float* old_min,
                                 const float* old_max, float min_action, float max_action, int horizon, int max_steps,
                                 int saute, float saute_budget, float saute_gamma, const double* ep_ret,
                                 const double* ep_cost, const int* ep_len) {
  OSA_REQUIRE(K >= 1 && obs_dim >= 1 && act_dim >= 1 && max_steps >= 1 && horizon >= 1);
  OSA_REQUIRE(params && old_min && old_max && max_action != min_action && ep_ret && ep_cost && ep_len);
  OSA_REQUIRE((norm_mean == nullptr) == (norm_std == nullptr) && (norm_mean == nullptr) == (norm_count == nullptr));
  OSA_REQUIRE(!saute || (saute_budget != 0.f && saute_gamma != 0.f));
  return OSA_OK;
}

// K episodes of description E at `level`, after osa_eval_check: the remaining checks, the arguments and the launch.
// A trace record holds obs_dim (+ 1 with saute) + act_dim + 3 + E::TRACE floats.
template <class E>
static int osa_eval_launch(int level, int K, int obs_dim, int act_dim, int hidden, const float* params,
                           const float* norm_mean, const float* norm_std, const long* norm_count, float norm_clip,
                           const float* old_min, const float* old_max, float min_action, float max_action,
                           unsigned long long seed, int horizon, float cost_p, int max_steps, int saute,
                           float saute_budget, float saute_gamma, int early_terminated, double cost_limit,
                           double cost_criteria, double* ep_ret, double* ep_cost, int* ep_len, float* trace,
                           void* stream) {
  OSA_REQUIRE(obs_dim >= E::OBS && act_dim >= E::ACT);
  const int in_w = obs_dim + (saute ? 1 : 0);
  const int rc = osa_check_dims(in_w, act_dim, hidden);
  if (rc != OSA_OK) return rc;
  OsaEvalArgs a;
  a.nd = osa_make_net(in_w, act_dim, hidden);
  const size_t lds = (size_t)16 * (a.nd.INP + OSA_EVAL_ACT_LD + (E::LDS_ROW ? E::STATE : 0)) * sizeof(float);
  if (lds > 65536) return OSA_EUNSUPPORTED;  // policy input wider than 992 columns (928 with a 64-float state row)
  a.params = params;
  a.K = K; a.obs_dim = obs_dim; a.max_steps = max_steps; a.horizon = horizon;
  a.mean = norm_mean; a.std_ = norm_std; a.count = norm_count; a.clip = norm_clip;
  a.old_min = old_min; a.old_max = old_max; a.min_a = min_action; a.max_a = max_action;
  a.seed = seed; a.cost_p = cost_p;
  a.saute = saute ? 1 : 0; a.budget = saute_budget; a.saute_gamma = saute_gamma;
  a.early_terminated = early_terminated ? 1 : 0; a.cost_limit = cost_limit; a.cost_criteria = cost_criteria;
  a.ep_ret = ep_ret; a.ep_cost = ep_cost; a.ep_len = ep_len; a.trace = trace;
  a.rec = in_w + act_dim + 3 + E::TRACE;
  a.level = level;
  const dim3 grid((unsigned)((K + 15) / 16));
#define OSA_CALL(HT, OT, NSB) \
  hipLaunchKernelGGL((osa_eval_episodes_kernel<HT, OT, E>), grid, dim3(64), lds, osa_stream(stream), a)
  OSA_DISPATCH_OT(a.nd, OSA_CALL);
#undef OSA_CALL
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}
