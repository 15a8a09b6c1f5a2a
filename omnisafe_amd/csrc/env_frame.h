// The frame of the per-step kernels of the device envs (env_device.h), the same for every family and written once:
// the arguments, the device-resident part of the Philox stream position, the truncation every `horizon` steps with the
// gymnasium vector auto-reset convention (the returned obs is the post-reset obs, the pre-reset obs is handed back as
// final_observation where the caller asks for it), what an env's first lane writes at the end, and the argument checks
// and the launch of every entry point.  rollout_kernels.hip builds the kernels of the built-in families on it;
// osa_custom_env_kernel below is the kernel of any register-state description and osa_custom_row_env_kernel the one of
// any description with an object row in LDS; csrc/custom/custom_env.hip instantiates one of the two for a description
// that is not in this tree.
#pragma once
#include "env_device.h"
#include "env_params.h"

struct OsaStepArgs {
  unsigned long long seed, step;
  const unsigned long long* step_base;
  int N, D, horizon, level;
  float cost_p;
  float* state;
  int* steps;
  const float* action;
  int ld_a;
  float* obs;
  int ld;
  float *reward, *cost;
  uint8_t *terminated, *truncated;
  float* final_obs;
  int ld_f, reset_only;
};
// The arguments of the per-step kernel of a description with runtime parameters (env_params.h): the (2, P) ranges, read
// through the pointer at every reset, and the (N, ld_par) matrix of the envs' rows.
struct OsaParamStepArgs : OsaStepArgs {
  const float* range;
  float* par;
  int ld_par;
};
template <class E>
using OsaCustomStepArgs = std::conditional_t<(OsaEnvParams<E>::value > 0), OsaParamStepArgs, OsaStepArgs>;

// The stream position of the launch: the host's part and the device-resident one.
__device__ __forceinline__ unsigned long long osa_step_pos(const OsaStepArgs& a) {
  return a.step_base ? a.step + *a.step_base : a.step;
}
// Whether this step of env n truncates (the final observation, then a reset); `count`: the steps of its episode, this
// one included.  (Asked after the transition, whose arithmetic hides the load; asked first, the scalar unit waits for
// it before anything else: profiles/env_frame_timing.json, first_form.)
__device__ __forceinline__ uint8_t osa_step_trunc(const OsaStepArgs& a, int n, int& count) {
  count = a.steps[n] + 1;
  return (count >= a.horizon) ? 1 : 0;
}
// What the first lane of env n writes at the end, besides the state (count, trunc: 0 after a reset alone).  term: the
// description ended the episode itself (osa_env_terminal; never together with trunc); the built-in families have no
// such end and leave it at 0.
__device__ __forceinline__ void osa_step_end(const OsaStepArgs& a, int n, float r, float c, uint8_t trunc, int count,
                                             uint8_t term = 0) {
  if (!a.reset_only) {
    a.reward[n] = r;
    a.cost[n] = c;
    a.terminated[n] = term;
    a.truncated[n] = trunc;
  }
  a.steps[n] = (trunc || term) ? 0 : count;
}

// The argument checks and the launch of every env entry point: `envs` envs per 64-lane workgroup, at least min_obs
// observation columns; has_state: the env has a state matrix and takes actions, at least min_act columns of them (the
// built-in families: two); has_level: it takes a level.
// (Args: OsaStepArgs, or what derives from it for a kernel that takes more.)
template <class Kernel, class Args = OsaStepArgs>
static int osa_env_step(Kernel kernel, int min_obs, int envs, bool has_state, bool has_level, const Args& a,
                        void* stream, int min_act = 2) {
  OSA_REQUIRE(a.N > 0 && a.D >= min_obs && (a.state || !has_state) && a.steps && a.obs && a.ld >= a.D);
  if (has_level) OSA_REQUIRE(a.level >= 0 && a.level <= 2 && (!a.final_obs || a.ld_f >= a.D));
  if (!a.reset_only) {
    OSA_REQUIRE(a.reward && a.cost && a.terminated && a.truncated && a.horizon > 0);
    OSA_REQUIRE(!has_state || (a.action && a.ld_a >= min_act));
  }
  hipLaunchKernelGGL(kernel, dim3((a.N + envs - 1) / envs), dim3(64), 0, osa_stream(stream), a);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

// ------------------------------------------------------------------------------------------------
// The per-step kernel of ANY description that keeps its state in registers (E::LDS_ROW == false): osa_circle_env_kernel
// with the family a template parameter.  LANES lanes per env, 64 / LANES envs per 64-lane workgroup.  Every lane of an
// env computes the whole transition from the state row (redundant, wave-uniform work inside the env's lanes) and the
// strided column loop writes the observation row: lane l the columns l, l + LANES, ..., zeros past E::OBS in a wider
// row; the same loop writes final_obs on a truncating step.  Lane 0 of an env writes the state, reward, cost, flags and
// the step counter.  No LDS, no barrier, no cross-lane operation: the lanes of a missing last env leave at once.
// A description with a terminal() member (osa_env_terminal, env_device.h) ends episodes per env: asked after the
// transition, true gives terminated = 1, truncated = 0, no final_obs row and a reset by fresh() at the same position;
// the time limit is per env as well (steps[n] + 1 >= horizon and not terminal), and steps[n] returns to 0 on either
// end.  The envs that share a wave (4 / 2 / 1 per workgroup at 16 / 32 / 64 lanes) may then diverge at fresh() and at
// the final_obs loop; that is correct as written because no lane waits for another -- the wave runs both sides under
// the exec mask and every lane of an env takes the same side.
// The description gets no row pointer (`row` == nullptr: its state is what load() put into Regs) and the unclamped
// action row of the env in global memory.
// A description with PARAMS (env_params.h) has a row of P floats per env beside the state matrix: loaded and handed to
// bind() after load(), redrawn and bound again before fresh() at every reset -- after final_obs, which therefore shows
// the ended episode under its own parameters -- and written back by lane 0 where it was redrawn.
// LANES: E::LANES where the description declares it (16, 32 or 64), else 32 -- the value measured for the Circle
// kernels (28 and 40 columns: 3.75 us against 4.55 us with 64 lanes, profiles/circle_env_timing.json) and for no other
// shape; profiles/custom_env_timing.json has 16 / 32 / 64 for OsaReachEnv.
// ------------------------------------------------------------------------------------------------
template <class E, class = void>
struct OsaEnvLanes {
  static constexpr int value = 32;
};
template <class E>
struct OsaEnvLanes<E, std::void_t<decltype(E::LANES)>> {
  static constexpr int value = E::LANES;
};
// The highest level a description takes: E::LEVELS where it declares it, else 2 (what osa_env_step lets through).
template <class E, class = void>
struct OsaEnvLevels {
  static constexpr int value = 2;
};
template <class E>
struct OsaEnvLevels<E, std::void_t<decltype(E::LEVELS)>> {
  static constexpr int value = E::LEVELS;
};

#pragma clang fp contract(off)
template <class E, int LANES>
__global__ __launch_bounds__(64) void osa_custom_env_kernel(OsaCustomStepArgs<E> a) {
  static_assert(!E::LDS_ROW, "osa_custom_env_kernel: the description keeps its state row in registers");
  static_assert(LANES == 16 || LANES == 32 || LANES == 64, "osa_custom_env_kernel: 16, 32 or 64 lanes per env");
  const int n = (64 / LANES) * blockIdx.x + threadIdx.x / LANES, lane = threadIdx.x % LANES;
  if (n >= a.N) return;
  const OsaEnvAt at = {a.seed, osa_step_pos(a), n, a.level, 0.f};
  float* __restrict__ srow = a.state + (long)n * E::STATE;
  typename E::Regs s;
  E::load(s, srow);
  constexpr int P = OsaEnvParams<E>::value;
  OsaParamRow<E> par;
  if constexpr (P > 0) {
#pragma unroll
    for (int k = 0; k < P; ++k) par.v[k] = a.par[(long)n * a.ld_par + k];
    E::bind(s, par.v);
  }
  uint8_t trunc = 0, term = 0;
  int count = 0;
  float r = 0.f, c = 0.f;
  if (!a.reset_only) {
    osa_env_transition<E>(s, nullptr, at, a.action + (long)n * a.ld_a, r, c);
    term = osa_env_terminal<E>(s, nullptr, at) ? 1 : 0;  // (a compile-time 0 without E::terminal)
    trunc = osa_step_trunc(a, n, count);
    if (term) trunc = 0;  // termination wins over a time limit reached on the same step
    if (trunc && a.final_obs)
      for (int k = lane; k < a.D; k += LANES)
        a.final_obs[(long)n * a.ld_f + k] = k < E::OBS ? E::obs_col(s, nullptr, a.level, k) : 0.f;
  }
  const bool reset = a.reset_only || trunc || term;
  if (reset) {
    if constexpr (P > 0) osa_param_reset<E>(s, at, a.range, par);
    E::fresh(s, at, nullptr);
  }
  for (int k = lane; k < a.D; k += LANES)
    a.obs[(long)n * a.ld + k] = k < E::OBS ? E::obs_col(s, nullptr, a.level, k) : 0.f;
  if (lane == 0) {
    E::store(s, srow);
    if constexpr (P > 0) {
      if (reset) {
#pragma unroll
        for (int k = 0; k < P; ++k) a.par[(long)n * a.ld_par + k] = par.v[k];
      }
    }
    osa_step_end(a, n, r, c, trunc, count, term);
  }
}
#pragma clang fp contract(fast)

// ------------------------------------------------------------------------------------------------
// The per-step kernel of ANY description with an object row in LDS (E::LDS_ROW == true): what osa_goal_env_kernel
// (rollout_kernels.hip) is for OsaNavEnv<robot, OsaGoal>, with the family a template parameter.  LANES lanes per env,
// 64 / LANES envs per 64-lane workgroup, each env with a slice of E::STATE floats of one __shared__ array:
//   - the env's lanes stage its row from the state matrix (a strided loop), barrier;
//   - load, bind (PARAMS); transition, terminal, the time limit; final_obs on a truncating step (never on a terminating
//     one), by the strided column loop over E::obs_col; barrier (the columns' reads of the objects are done);
//   - on a reset the parameters are redrawn and the env's lanes write E::fresh_obj(at, col) for col = DYN + lane,
//     DYN + lane + LANES, ... into the LDS row and the state matrix; barrier; fresh (which may read the fresh objects);
//   - the observation row by the same column loop, zeros past E::OBS; lane 0 stores the Regs, the redrawn parameter
//     row, reward, cost, flags and the step counter.
// The objects are walked per column through obs_col, as the evaluation kernel walks them, not by a lane-per-object
// pass as in osa_goal_env_kernel: any description fits, at the price of each lane repeating the walk.
// Every barrier stands in workgroup-uniform flow.  The envs of a workgroup may disagree about resetting (terminal(), or
// step counters that differ) and the last workgroup of an odd N has slots without an env: both are predication around
// the stores and the fresh_obj loop, and no lane returns early.  The lanes of a slot without an env shadow env N - 1 --
// they read its rows and compute what its own lanes compute -- and store nothing (`live`).
// `row` is the env's slice: columns [DYN, STATE) are the objects; [0, DYN) hold what was staged and go stale with the
// transition (the state is the Regs).  Arithmetic: float32 without fused multiply-adds, as the description's.
// LANES: OsaEnvLanes<E> as above -- E::LANES, else 32, which is also what was measured fastest here
// (profiles/custom_row_env_timing.json: the Goal rows at 16 / 32 / 64 lanes, fastest at 32 in four of six cases and
// within 5 % of the fastest in the other two; the 150-float Field 25.8 us at 32 lanes against 37 us at 16 and at 64).
// ------------------------------------------------------------------------------------------------
#define OSA_ROW_STATE_MAX 256  // floats of a row in LDS

#pragma clang fp contract(off)
template <class E, int LANES>
__global__ __launch_bounds__(64) void osa_custom_row_env_kernel(OsaCustomStepArgs<E> a) {
  static_assert(E::LDS_ROW, "osa_custom_row_env_kernel: the description keeps an object row in LDS");
  static_assert(LANES == 16 || LANES == 32 || LANES == 64, "osa_custom_row_env_kernel: 16, 32 or 64 lanes per env");
  static_assert(E::STATE >= 1 && E::STATE <= OSA_ROW_STATE_MAX && E::DYN >= 0 && E::DYN <= E::STATE, "row widths");
  constexpr int ENVS = 64 / LANES;
  __shared__ float rows[ENVS * E::STATE];
  const int slot = threadIdx.x / LANES, lane = threadIdx.x % LANES;
  const int n = ENVS * blockIdx.x + slot;
  const bool live = n < a.N;
  const int m = live ? n : a.N - 1;  // (the env whose rows this slot reads)
  float* __restrict__ row = rows + slot * E::STATE;
  float* __restrict__ srow = a.state + (long)m * E::STATE;
  for (int c = lane; c < E::STATE; c += LANES) row[c] = srow[c];
  __syncthreads();
  const OsaEnvAt at = {a.seed, osa_step_pos(a), m, a.level, 0.f};
  typename E::Regs s;
  E::load(s, row);
  constexpr int P = OsaEnvParams<E>::value;
  OsaParamRow<E> par;
  if constexpr (P > 0) {
#pragma unroll
    for (int k = 0; k < P; ++k) par.v[k] = a.par[(long)m * a.ld_par + k];
    E::bind(s, par.v);
  }
  uint8_t trunc = 0, term = 0;
  int count = 0;
  float r = 0.f, c = 0.f;
  if (!a.reset_only) {  // (a kernel argument: uniform)
    osa_env_transition<E>(s, row, at, a.action + (long)m * a.ld_a, r, c);
    term = osa_env_terminal<E>(s, row, at) ? 1 : 0;  // (a compile-time 0 without E::terminal)
    trunc = osa_step_trunc(a, m, count);
    if (term) trunc = 0;  // termination wins over a time limit reached on the same step
    if (live && trunc && a.final_obs)
      for (int k = lane; k < a.D; k += LANES)
        a.final_obs[(long)n * a.ld_f + k] = k < E::OBS ? E::obs_col(s, row, a.level, k) : 0.f;
  }
  __syncthreads();  // every read of the old objects is done
  const bool reset = a.reset_only || trunc || term;
  if (reset) {  // (per env: predication, no barrier inside)
    if constexpr (P > 0) osa_param_reset<E>(s, at, a.range, par);
    for (int col = E::DYN + lane; col < E::STATE; col += LANES) {
      const float o = E::fresh_obj(at, col);
      row[col] = o;
      if (live) srow[col] = o;
    }
  }
  __syncthreads();  // the fresh objects are in LDS
  if (reset) E::fresh(s, at, row);
  if (live)
    for (int k = lane; k < a.D; k += LANES)
      a.obs[(long)n * a.ld + k] = k < E::OBS ? E::obs_col(s, row, a.level, k) : 0.f;
  if (live && lane == 0) {
    E::store(s, srow);
    if constexpr (P > 0) {
      if (reset) {
#pragma unroll
        for (int k = 0; k < P; ++k) a.par[(long)n * a.ld_par + k] = par.v[k];
      }
    }
    osa_step_end(a, n, r, c, trunc, count, term);
  }
}
#pragma clang fp contract(fast)
