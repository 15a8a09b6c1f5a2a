// Persistent stochastic data collection with a saved policy on a device env (omnisafe/common/offline/data_collector.py:
// 145-190, the rows of one agent in parallel lanes): one launch writes a block of total_rows dataset rows.  Lane k is
// row j = k & 15 of the wave of workgroup k / 16 (the mapping of osa_eval_episodes_kernel) and owns the rows
// [k Q, min((k + 1) Q, S)), which it fills with consecutive episodes: every step samples the actor (policy_rows.h's
// expression and noise stream), scales the action, makes the env transition, keeps the RAW observation before and after
// it, and resets inside the kernel where the episode ends.  Every lane stores the columns it computed; a row-wise store
// form was measured slower (collect_episodes.h, profiles/collect_row_stores.json).  Every row has one owner: no atomics,
// no spins and no barrier between workgroups.  The kernel template and its launch are in collect_episodes.h; the entry
// point fills OsaCollectArgs, and what the kernel shares with the evaluation kernel is in play_episodes.h.
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
  const OsaEvalKind kind = osa_eval_kind(env_kind);
  OsaCollectArgs a = {};
  a.params = params;
  a.K = K; a.obs_dim = obs_dim; a.max_steps = rows_per_lane; a.horizon = horizon;
  a.mean = norm_mean; a.std_ = norm_std; a.count = norm_count; a.clip = norm_clip;
  a.old_min = old_min; a.old_max = old_max; a.min_a = min_action; a.max_a = max_action;
  a.seed = seed; a.cost_p = cost_p; a.level = kind.level;
  a.ep_ret = ep_ret_sum; a.ep_cost = ep_cost_sum; a.ep_len = ep_count;
  a.total_rows = total_rows; a.noise_seed = noise_seed;
  a.obs = obs; a.action = action; a.reward = reward; a.cost = cost; a.next_obs = next_obs; a.done = done;
  a.ld_obs = ld_obs; a.ld_act = ld_act; a.ld_next = ld_next;
  const int rc = osa_collect_check(a, act_dim);
  if (rc != OSA_OK) return rc;
  switch (kind.family) {
#define OSA_LAUNCH(FAMILY, LEVELS, E) \
  case FAMILY:                        \
    return osa_collect_launch<E>(a, act_dim, hidden, stream);
    OSA_EVAL_FAMILIES(OSA_LAUNCH)
#undef OSA_LAUNCH
  }
  return OSA_EUNSUPPORTED;
}

}  // extern "C"
