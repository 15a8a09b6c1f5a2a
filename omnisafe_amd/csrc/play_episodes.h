// What the persistent players (eval_episodes.h, collect_episodes.h: 16 lanes per wave play a saved policy on a device
// env from start to finish) share: the arguments, their check, and the device steps both kernels make.
#pragma once
#include <type_traits>

#include "env_device.h"
#include "env_params.h"

// An entry point fills its player's struct from its parameters; the launch completes it (nd, and what it adds itself).
struct OsaPlayArgs {
  OsaNet nd;  // actor shape; nd.obs_dim = policy input width
  const float* params;
  int K, obs_dim, max_steps, horizon;
  const float *mean, *std_;
  const long* count;
  float clip;
  const float *old_min, *old_max;
  float min_a, max_a;
  unsigned long long seed;
  float cost_p;
  double *ep_ret, *ep_cost;  // per lane
  int* ep_len;
  int level;  // level of the env (a built-in one: env_kind - its family's OSA_EVAL_ENV_* constant)
  // a custom description with PARAMS (env_params.h), else unused: the (2, P) ranges, and where a player leaves rows of
  // P floats at stride ld_par (the evaluation: each episode's row; the collection: each lane's last one)
  const float* range;
  float* par;
  int ld_par;
};

#define OSA_EVAL_ACT_LD 32  // LDS row of the env actions (act_dim <= 32: osa_check_dims)

// The argument checks every entry point of a player makes before it looks at the env.
static inline int osa_play_check(const OsaPlayArgs& a, int act_dim) {
  OSA_REQUIRE(a.K >= 1 && a.obs_dim >= 1 && act_dim >= 1 && a.max_steps >= 1 && a.horizon >= 1);
  OSA_REQUIRE(a.params && a.old_min && a.old_max && a.max_a != a.min_a && a.ep_ret && a.ep_cost && a.ep_len);
  OSA_REQUIRE((a.mean == nullptr) == (a.std_ == nullptr) && (a.mean == nullptr) == (a.count == nullptr));
  return OSA_OK;
}

#pragma clang fp contract(off)
// normalizer.py:104-107 with frozen statistics (osa_normalize_kernel without the mask)
__device__ __forceinline__ float osa_play_norm(const OsaPlayArgs& a, bool on, float v, int col) {
  if (on) {
    v = (v - a.mean[col]) / a.std_[col];
    v = v < -a.clip ? -a.clip : v;  // (NaN-preserving, as osa_normalize_kernel)
    v = v > a.clip ? a.clip : v;
  }
  return v;
}

// The env observation of lane k's state (at), lane group g taking a quarter of the columns: put(col, value).
// after_end: the observation follows a reset at the position of an ending step (not the reset at position 0).
template <class E, class Put>
__device__ __forceinline__ void osa_play_obs(const OsaPlayArgs& a, int g, const typename E::Regs& s,
                                             const float* __restrict__ srow, const OsaEnvAt& at, bool after_end,
                                             Put put) {
  if constexpr (std::is_same<E, OsaSynthEnv>::value) {
    // The noise env draws both rows of a position pair-wise: (v0, v1) the observation of the step (and of the reset at
    // position 0), (c2, d2) the one after the reset of an ending step (osa_synth_env_kernel).
    const int D = a.obs_dim;
    for (int pair = g; 2 * pair < D; pair += 4) {
      float v0, v1, c2, d2;
      osa_synth_obs_pair(at.seed, at.pos, at.n, pair, v0, v1, c2, d2);
      put(2 * pair, after_end ? c2 : v0);
      if (2 * pair + 1 < D) put(2 * pair + 1, after_end ? d2 : v1);
    }
  } else {
    for (int c = g; c < a.obs_dim; c += 4) put(c, E::obs_col(s, srow, a.level, c));
  }
}

// The parameter half of a reset at `at` (the reset at position 0, or an in-kernel one at the ending step's position),
// before E::fresh: the episode's row is redrawn into the registers of its lanes -- the same row in the four lane groups
// -- and bound.  Nothing without PARAMS.
template <class E>
__device__ __forceinline__ void osa_play_params(const OsaPlayArgs& a, typename E::Regs& s, const OsaEnvAt& at,
                                                OsaParamRow<E>& row) {
  if constexpr (OsaEnvParams<E>::value > 0) osa_param_reset<E>(s, at, a.range, row);
}
// Lane k's row to a.par (one lane per episode calls it).
template <class E>
__device__ __forceinline__ void osa_play_params_out(const OsaPlayArgs& a, int k, const OsaParamRow<E>& row) {
  if constexpr (OsaEnvParams<E>::value > 0) {
#pragma unroll
    for (int q = 0; q < OsaEnvParams<E>::value; ++q) a.par[(long)k * a.ld_par + q] = row.v[q];
  }
}

// The first half of a reset at `at` for a family with objects (LDS_ROW), which keeps the state row of its lane in LDS:
// the fresh objects into the row (zeros for a lane that plays nothing), lane group g writing a quarter of them: the
// columns [E::DYN, E::STATE), one E::fresh_obj call each.  The caller's barrier and E::fresh follow (the row's hazards
// are in LDS: the reset places the goal away from them).  Columns [0, E::DYN) of the LDS row are never written here:
// they are the Regs.
template <class E>
__device__ __forceinline__ void osa_play_fresh_objects(float* __restrict__ srow, int g, const OsaEnvAt& at, bool on) {
  if constexpr (E::LDS_ROW)
    for (int c = E::DYN + g; c < E::STATE; c += 4) srow[c] = on ? E::fresh_obj(at, c) : 0.f;
}
#pragma clang fp contract(fast)
