// Persistent deterministic evaluation of a saved policy on a device env (omnisafe/evaluator.py:399-490, episodes in
// parallel lanes): one launch plays K episodes.  Episode k is row j = k & 15 of the wave of workgroup k / 16 (the row
// mapping of osa_policy_step_kernel: the four lane groups g = lane >> 4 of a row share its MFMA fragments).  Each step
// of a row: frozen-statistics normalisation of the env observation (osa_normalize_kernel's expression), Saute / Simmer
// safety column, actor mean (osa_mlp_forward), ActionScale, env transition (env_device.h), float64 episode sums,
// early termination.  A workgroup ends when its 16 rows are done: no atomics, no spins and no
// barrier between workgroups.  The kernel template and its launch are in eval_episodes.h; the entry point fills
// OsaEvalArgs, and what the kernel shares with the collection kernel is in play_episodes.h.
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
  const OsaEvalKind kind = osa_eval_kind(env_kind);
  OsaEvalArgs a = {};
  a.params = params;
  a.K = K; a.obs_dim = obs_dim; a.max_steps = max_steps; a.horizon = horizon;
  a.mean = norm_mean; a.std_ = norm_std; a.count = norm_count; a.clip = norm_clip;
  a.old_min = old_min; a.old_max = old_max; a.min_a = min_action; a.max_a = max_action;
  a.seed = seed; a.cost_p = cost_p; a.level = kind.level;
  a.ep_ret = ep_ret; a.ep_cost = ep_cost; a.ep_len = ep_len;
  a.saute = saute ? 1 : 0; a.budget = saute_budget; a.saute_gamma = saute_gamma;
  a.early_terminated = early_terminated ? 1 : 0; a.cost_limit = cost_limit; a.cost_criteria = cost_criteria;
  a.trace = trace;
  const int rc = osa_eval_check(a, act_dim);
  if (rc != OSA_OK) return rc;
  switch (kind.family) {
#define OSA_LAUNCH(FAMILY, LEVELS, E) \
  case FAMILY:                        \
    return osa_eval_launch<E>(a, act_dim, hidden, stream);
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
