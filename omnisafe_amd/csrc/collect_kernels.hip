// Persistent stochastic data collection with a saved policy on a device env (omnisafe/common/offline/data_collector.py:
// 145-190, the rows of one agent in parallel lanes): one launch writes a block of total_rows dataset rows.  Lane k is
// row j = k & 15 of the wave of workgroup k / 16 (the mapping of osa_eval_episodes_kernel) and owns the rows
// [k Q, min((k + 1) Q, S)), which it fills with consecutive episodes: every step samples the actor (policy_rows.h's
// expression and noise stream), scales the action, makes the env transition, keeps the RAW observation before and after
// it, and resets inside the kernel where the episode ends.  Every lane stores the columns it computed; the row-wise
// store form was measured slower (collect_episodes.h, profiles/collect_timing.json).  Every row has one owner: no
// atomics, no spins and no barrier between workgroups.  The kernel template, its arguments and its launch are in
// collect_episodes.h.
//
// Random numbers: lane k replays env index k of the per-step env launches at stream positions 0 (reset), 1, 2, ...
// and row k of the per-step policy launches of a fresh actor seeded noise_seed, so that this kernel and the per-step
// path (omnisafe_amd/offline.py) write the same rows bit for bit.
#include "collect_episodes.h"
#include "eval_families.h"

extern "C" {

int osa_collect_episodes(int env_kind, int K, int rows_per_lane, long total_rows, int obs_dim, int act_dim, int hidden,
                         const float* params, const float* norm_mean, const float* norm_std, const long* norm_count,
                         float norm_clip, const float* old_min, const float* old_max, float min_action,
                         float max_action, unsigned long long seed, unsigned long long noise_seed, int horizon,
                         float cost_p, float* obs, int ld_obs, float* action, int ld_act, float* reward, float* cost,
                         float* next_obs, int ld_next, float* done, double* ep_ret_sum, double* ep_cost_sum,
                         int* ep_count, void* stream) {
  const int rc = osa_collect_check(K, rows_per_lane, total_rows, obs_dim, act_dim, params, norm_mean, norm_std,
                                   norm_count, old_min, old_max, min_action, max_action, horizon, obs, ld_obs, action,
                                   ld_act, reward, cost, next_obs, ld_next, done, ep_ret_sum, ep_cost_sum, ep_count);
  if (rc != OSA_OK) return rc;
  const OsaEvalKind kind = osa_eval_kind(env_kind);
  switch (kind.family) {
#define OSA_LAUNCH(FAMILY, LEVELS, E)                                                                               \
  case FAMILY:                                                                                                      \
    return osa_collect_launch<E>(kind.level, K, rows_per_lane, total_rows, obs_dim, act_dim, hidden, params,        \
                                 norm_mean, norm_std, norm_count, norm_clip, old_min, old_max, min_action,          \
                                 max_action, seed, noise_seed, horizon, cost_p, obs, ld_obs, action, ld_act, reward, \
                                 cost, next_obs, ld_next, done, ep_ret_sum, ep_cost_sum, ep_count, stream);
    OSA_EVAL_FAMILIES(OSA_LAUNCH)
#undef OSA_LAUNCH
  }
  return OSA_EUNSUPPORTED;
}

}  // extern "C"
