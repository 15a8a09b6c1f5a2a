// The persistent evaluation kernel as a template over an env description (env_device.h), with its arguments and its
// launch: eval_kernels.hip instantiates it for the built-in families, csrc/custom/custom_env.hip for one description
// that is not in this tree.
#pragma once
#include "play_episodes.h"

struct OsaEvalArgs : OsaPlayArgs {  // nd.obs_dim = obs_dim + saute
  int saute;
  float budget, saute_gamma;
  int early_terminated;
  double cost_limit, cost_criteria;
  float* trace;
  int rec;  // floats per trace record
};

#pragma clang fp contract(off)
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
  osa_play_fresh_objects<E>(srow, g, at, valid);
  if constexpr (E::LDS_ROW) __syncthreads();
  OsaParamRow<E> par;  // the episode's parameters (a description with PARAMS): drawn once, an episode keeps them
  osa_play_params<E>(a, s, at, par);
  if (valid && g == 0) osa_play_params_out<E>(a, k, par);
  E::fresh(s, at, srow);
  // the env observation of episode k, normalised, into its LDS input row
  const auto put = [&](int c, float v) { xrow[c] = osa_play_norm(a, norm_on, v, c); };
  if (valid) osa_play_obs<E>(a, g, s, srow, at, false, put);
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
        osa_play_obs<E>(a, g, s, srow, at, false, put);
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
static inline int osa_eval_check(const OsaEvalArgs& a, int act_dim) {
  const int rc = osa_play_check(a, act_dim);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(!a.saute || (a.budget != 0.f && a.saute_gamma != 0.f));
  return OSA_OK;
}

// K episodes of description E at a.level, after osa_eval_check: the remaining checks, the rest of the arguments (nd,
// rec) and the launch.  A trace record holds obs_dim (+ 1 with saute) + act_dim + 3 + E::TRACE floats.
template <class E>
static int osa_eval_launch(OsaEvalArgs a, int act_dim, int hidden, void* stream) {
  OSA_REQUIRE(a.obs_dim >= E::OBS && act_dim >= E::ACT);
  const int in_w = a.obs_dim + a.saute;
  const int rc = osa_check_dims(in_w, act_dim, hidden);
  if (rc != OSA_OK) return rc;
  a.nd = osa_make_net(in_w, act_dim, hidden);
  const size_t lds = (size_t)16 * (a.nd.INP + OSA_EVAL_ACT_LD + (E::LDS_ROW ? E::STATE : 0)) * sizeof(float);
  if (lds > 65536) return OSA_EUNSUPPORTED;  // policy input wider than 992 columns (928 with a 64-float state row)
  a.rec = in_w + act_dim + 3 + E::TRACE;
  const dim3 grid((unsigned)((a.K + 15) / 16));
#define OSA_CALL(HT, OT, NSB) \
  hipLaunchKernelGGL((osa_eval_episodes_kernel<HT, OT, E>), grid, dim3(64), lds, osa_stream(stream), a)
  OSA_DISPATCH_OT(a.nd, OSA_CALL);
#undef OSA_CALL
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}
