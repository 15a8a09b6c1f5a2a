// Persistent deterministic evaluation of a saved policy on a device env (omnisafe/evaluator.py:399-490, episodes in
// parallel lanes): one launch plays K episodes.  Episode k is row j = k & 15 of the wave of workgroup k / 16 (the row
// mapping of osa_policy_step_kernel: the four lane groups g = lane >> 4 of a row share its MFMA fragments).  Each step
// of a row: frozen-statistics normalisation of the env observation (osa_normalize_kernel's expression), Saute /
// Simmer safety column, actor mean (osa_mlp_forward), ActionScale (osa_action_scale1), env transition (env_device.h),
// float64 episode sums, early termination.  A workgroup ends when its 16 rows are done: no atomics, no spins and no
// barrier between workgroups.  The kernel template, its arguments and its launch are in eval_episodes.h.
//
// Random numbers: row k replays env index k of the per-step env launches at stream positions 0 (reset), 1, 2, ...
// so that this kernel and the per-step path (omnisafe_amd/evaluator.py) play the same episodes bit for bit.
#include "eval_episodes.h"
#include "eval_families.h"

extern "C" {

int osa_eval_episodes(int env_kind, int K, int obs_dim, int act_dim, int hidden, const float* params,
                      const float* norm_mean, const float* norm_std, const long* norm_count, float norm_clip,
                      const float* old_min, const float* old_max, float min_action, float max_action,
                      unsigned long long seed, int horizon, float cost_p, int max_steps, int saute,
                      float saute_budget, float saute_gamma, int early_terminated, double cost_limit,
                      double cost_criteria, double* ep_ret, double* ep_cost, int* ep_len, float* trace,
                      void* stream) {
  const int rc = osa_eval_check(K, obs_dim, act_dim, params, norm_mean, norm_std, norm_count, old_min, old_max,
                                min_action, max_action, horizon, max_steps, saute, saute_budget, saute_gamma, ep_ret,
                                ep_cost, ep_len);
  if (rc != OSA_OK) return rc;
  const OsaEvalKind kind = osa_eval_kind(env_kind);
  switch (kind.family) {
#define OSA_LAUNCH(FAMILY, LEVELS, E)                                                                                \
  case FAMILY:                                                                                                       \
    return osa_eval_launch<E>(kind.level, K, obs_dim, act_dim, hidden, params, norm_mean, norm_std, norm_count,      \
                              norm_clip, old_min, old_max, min_action, max_action, seed, horizon, cost_p, max_steps, \
                              saute, saute_budget, saute_gamma, early_terminated, cost_limit, cost_criteria, ep_ret, \
                              ep_cost, ep_len, trace, stream);
    OSA_EVAL_FAMILIES(OSA_LAUNCH)
#undef OSA_LAUNCH
  }
  return OSA_EUNSUPPORTED;
}

int osa_eval_trace_floats(int env_kind, int obs_dim, int act_dim, int saute) {
  if (obs_dim < 1 || act_dim < 1) return 0;
  return obs_dim + (saute ? 1 : 0) + act_dim + 3 + osa_eval_kind(env_kind).state_floats;
}

}  // extern "C"
