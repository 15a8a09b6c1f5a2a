// Per-env transitions of the two device-resident vector envs, shared by their per-step kernels
// (rollout_kernels.hip: osa_synth_env_kernel, osa_reach_env_kernel) and the persistent evaluation kernel
// (eval_kernels.hip).  Every random number is a Philox4x32-10 draw keyed by (seed, stream position `step`, env
// index n), so a caller that replays env n at positions 0, 1, 2, ... sees the same episode as the per-step launches.
#pragma once
#include "mlp_device.h"

// ------------------------------------------------------------------------------------------------
// Synth*-v0: obs ~ N(0,1)^D, reward ~ N(0,1), cost ~ Bernoulli(cost_p), never terminates.
// ------------------------------------------------------------------------------------------------
// Features 2 pair, 2 pair + 1 of env n at position `step`: (a, b) the observation of a step that does not
// truncate (and the final observation of one that does), (c2, d2) the post-reset observation of a truncating step.
__device__ __forceinline__ void osa_synth_obs_pair(unsigned long long seed, unsigned long long step, int n, int pair,
                                                   float& a, float& b, float& c2, float& d2) {
  uint32_t w[4];
  osa_philox(seed, step, ((unsigned long long)n << 20) + pair, w);
  osa_box_muller(w[0], w[1], a, b);
  osa_box_muller(w[2], w[3], c2, d2);  // second pair: the post-reset observation
}

// Reward and cost of env n's transition at position `step`, from the Philox block
// osa_philox(seed ^ OSA_SYNTH_RC_KEY, step, n).
#define OSA_SYNTH_RC_KEY 0x9E3779B97F4A7C15ull
__device__ __forceinline__ float osa_synth_reward(const uint32_t (&w)[4]) {
  float a, b;
  osa_box_muller(w[0], w[1], a, b);
  return a;
}
__device__ __forceinline__ float osa_synth_cost(const uint32_t (&w)[4], float cost_p) {
  return (osa_u01(w[2]) <= cost_p) ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------------
// SynthReach-v0: state p(2) g(2) h(2); dynamics stated in oracle/np_oracle.py:reach_env_step.  float32 without
// fused multiply-adds, so that the CPU twin sees the same arithmetic.
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
__device__ __forceinline__ float osa_reach_dist(float ux, float uy, float vx, float vy) {
  const float dx = ux - vx, dy = uy - vy;
  const float xx = dx * dx, yy = dy * dy;
  return sqrtf(xx + yy);
}

// column k of the observation row of state s: [p, g - p, h - p, 0 ...]
__device__ __forceinline__ float osa_reach_obs_col(const float (&s)[6], int k) {
  float v = 0.f;
  if (k == 0) v = s[0];
  if (k == 1) v = s[1];
  if (k == 2) v = s[2] - s[0];
  if (k == 3) v = s[3] - s[1];
  if (k == 4) v = s[4] - s[0];
  if (k == 5) v = s[5] - s[1];
  return v;
}

__device__ __forceinline__ float osa_reach_uniform(uint32_t w) {  // [-1, 1]
  return 2.f * osa_u01(w) - 1.f;
}

// Random numbers of env n at position `step`: the two Philox blocks
//   osa_philox(seed ^ OSA_REACH_KEY, step, (n << 20) + 1) -> w0,  ... + 2 -> w1;
// w0[0..3], w1[0..1] a fresh state (reset), w1[2..3] a new goal (osa_reach_transition).
#define OSA_REACH_KEY 0xD1B54A32D192ED03ull

// the fresh state of a reset
__device__ __forceinline__ void osa_reach_fresh(const uint32_t (&w0)[4], const uint32_t (&w1)[4], float (&fresh)[6]) {
  fresh[0] = osa_reach_uniform(w0[0]);
  fresh[1] = osa_reach_uniform(w0[1]);
  fresh[2] = osa_reach_uniform(w0[2]);
  fresh[3] = osa_reach_uniform(w0[3]);
  fresh[4] = osa_reach_uniform(w1[0]);
  fresh[5] = osa_reach_uniform(w1[1]);
}

// One transition of state s under the (unclamped) env action (a0, a1); w1 from osa_reach_draw of the same position.
__device__ __forceinline__ void osa_reach_transition(float (&s)[6], float a0_in, float a1_in, const uint32_t (&w1)[4],
                                                     float& r, float& c) {
  const float a0 = fminf(fmaxf(a0_in, -1.f), 1.f);
  const float a1 = fminf(fmaxf(a1_in, -1.f), 1.f);
  const float m0 = 0.1f * a0, m1 = 0.1f * a1;
  const float qx = fminf(fmaxf(s[0] + m0, -1.5f), 1.5f);
  const float qy = fminf(fmaxf(s[1] + m1, -1.5f), 1.5f);
  const float d0 = osa_reach_dist(s[0], s[1], s[2], s[3]);
  const float d1 = osa_reach_dist(qx, qy, s[2], s[3]);
  const bool reached = d1 < 0.15f;
  r = (d0 - d1) + (reached ? 1.f : 0.f);
  c = (osa_reach_dist(qx, qy, s[4], s[5]) < 0.3f) ? 1.f : 0.f;
  s[0] = qx;
  s[1] = qy;
  if (reached) {
    s[2] = osa_reach_uniform(w1[2]);
    s[3] = osa_reach_uniform(w1[3]);
  }
}
#pragma clang fp contract(fast)
