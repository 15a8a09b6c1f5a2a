/* omnisafe_amd_env.h -- a device env of your own: the description contract and the C ABI of the library that
 * omnisafe_amd.build.build_custom_env(header, struct) makes of it (csrc/custom/custom_env.hip).  libomnisafe_amd.so
 * exports none of these symbols; every custom library exports all three.  Error codes are omnisafe_amd.h's.
 *
 * THE DESCRIPTION is a struct of static members in a header of yours.  The header is compiled for gfx950 behind
 * csrc/env_device.h, inside a `#pragma clang fp contract(off)` region: float32, no fused multiply-adds.
 *
 *   struct MyEnv {
 *     static constexpr int STATE = ..;     // floats per row of the (N, STATE) state matrix, 1 .. 64
 *     static constexpr int OBS = ..;       // observation columns, >= 1
 *     static constexpr int DYN = ..;       // leading state floats a transition changes (documentation; <= STATE)
 *     static constexpr int ACT = ..;       // action columns, 1 .. 32
 *     static constexpr int TRACE = ..;     // leading state floats in an evaluator trace record, <= STATE
 *     static constexpr bool LDS_ROW = false;  // must be false: the state of an env is what load() puts into Regs
 *     static constexpr int LEVELS = ..;    // optional: the highest level, 0 .. 2 (default 2)
 *     static constexpr int LANES = ..;     // optional: lanes per env in the per-step kernel, 16 / 32 / 64 (default 32)
 *     struct Regs { ... };                 // an aggregate: the registers that hold a state row
 *     static __device__ void load(Regs&, const float* srow);          // from the env's row of the state matrix
 *     static __device__ void store(const Regs&, float* srow);         // and back (one lane per env calls it)
 *     static __device__ void fresh(Regs&, const OsaEnvAt&, const float* row);   // the state after a reset
 *     static __device__ void transition(Regs&, const float* row, const OsaEnvAt&, float a0, float a1,
 *                                       float& reward, float& cost);  // ACT <= 2: the action columns (ACT = 1:
 *                                                                     // a1 is 0, no second column is read), or
 *     static __device__ void transition(Regs&, const float* row, const OsaEnvAt&, const float* act,
 *                                       float& reward, float& cost);  // any ACT: the env's action row, act[0 .. ACT)
 *     static __device__ float obs_col(const Regs&, const float* row, int level, int col);   // 0 for col >= OBS
 *     static __device__ float state_col(const Regs&, const float* row, int col);            // col < TRACE
 *     static __device__ bool terminal(const Regs&, const float* row, const OsaEnvAt&);      // optional: true ends
 *                                                                     // the episode (see TERMINATION below)
 *   };
 *
 * `row` is never a pointer the description may read (nullptr in the per-step kernel): it exists for the built-in
 * families that keep objects in LDS.  Actions arrive unclamped.  OsaEnvAt {seed, pos, n, level, cost_p} says where
 * the call stands: env index n at position pos of the Philox stream `seed`; draw with
 * osa_philox(seed ^ MY_KEY, pos, ((unsigned long long)n << 20) + block, w) and osa_u01(w[i]) so that the per-step
 * launches (pos = 0 for the reset, then 1, 2, ...) and the evaluation kernel (episode k = env index k) play the same
 * episodes.  fresh() of a truncating step and the transition of the same step see the same pos.  Every lane of an
 * env runs load / transition / terminal / fresh with the same inputs, so they must be deterministic functions of their
 * arguments: no atomics, no cross-lane operations, no memory but the arguments.
 *
 * TERMINATION.  Every env counts the steps of its episode (steps[n]) and truncates when the count reaches `horizon`.
 * A description without terminal() never ends an episode otherwise, so its envs truncate together every `horizon`
 * steps after a common reset.  One with terminal() is asked once per step, after transition(), on the post-transition
 * state and with the OsaEnvAt of that transition; true ends the episode of that env alone:
 *   - the step reports terminated = 1, truncated = 0 and the reward and cost of that transition; termination wins
 *     over a time limit reached on the same step;
 *   - the env is reset by fresh() at the same stream position, exactly as on a truncating step;
 *   - final_obs is NOT written for a terminating env (only truncated paths are bootstrapped from it);
 *   - a step truncates when steps[n] + 1 >= horizon and it is not terminal; steps[n] returns to 0 on either end.
 * The evaluation kernel ends episode k on the same answer, with ep_len the steps played.
 *
 * A static_assert with a message that names the member rejects LDS_ROW == true, STATE outside 1 .. 64, ACT outside
 * 1 .. 32, TRACE > STATE, a missing member, and a member named terminal that cannot be called as stated above (it
 * would silently be an env that never ends).
 */
#ifndef OMNISAFE_AMD_ENV_H
#define OMNISAFE_AMD_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out[0 .. 8) = STATE, OBS, DYN, ACT, TRACE, LEVELS (the highest level), LANES, and 1 where the description has
 * terminal() (else 0).  The Python side reads every dimension from here. */
int osa_custom_env_info(int out[8]);

/* One reset (reset_only != 0) or one step of N envs: the argument list and the semantics of osa_nav_env_step
 * (omnisafe_amd.h).  state is (N, STATE) float32, action (N, >= ACT) with row stride ld_action, obs (N, obs_dim >= OBS)
 * with row stride ld_obs; columns OBS .. obs_dim are written as zeros.  level: 0 .. LEVELS. */
int osa_custom_env_step(unsigned long long seed, unsigned long long step, const unsigned long long* step_base, int N,
                        int obs_dim, int horizon, int level, float* state, int* steps, const float* action,
                        int ld_action, float* obs, int ld_obs, float* reward, float* cost, uint8_t* terminated,
                        uint8_t* truncated, float* final_obs, int ld_final, int reset_only, void* stream);

/* K evaluation episodes in one launch: the argument list and the semantics of osa_eval_episodes (omnisafe_amd.h) with
 * the level in the place of env_kind.  A trace record holds obs_dim (+ 1 with saute) + act_dim + 3 + TRACE floats. */
int osa_custom_eval_episodes(int level, int K, int obs_dim, int act_dim, int hidden, const float* params,
                             const float* norm_mean, const float* norm_std, const long* norm_count, float norm_clip,
                             const float* old_min, const float* old_max, float min_action, float max_action,
                             unsigned long long seed, int horizon, float cost_p, int max_steps, int saute,
                             float saute_budget, float saute_gamma, int early_terminated, double cost_limit,
                             double cost_criteria, double* ep_ret, double* ep_cost, int* ep_len, float* trace,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
