// One env description that is not in this tree, as a library of its own (omnisafe_amd.build.build_custom_env):
//   hipcc ... -DOSA_CUSTOM_ENV_HEADER="<absolute path of the header>" -DOSA_CUSTOM_ENV=<struct> custom_env.hip
// The header is included behind env_device.h and inside a `fp contract(off)` region: its arithmetic is float32 without
// fused multiply-adds, and it may use everything env_device.h has (osa_philox, osa_u01, osa_nav_*, OsaNavEnv<...>).
// The description contract and the six entry points are specified in include/omnisafe_amd_env.h.  This file is in a
// directory of its own because every csrc/*.hip goes into libomnisafe_amd.so.
#include "../env_frame.h"
#include "../eval_episodes.h"
#include "../collect_episodes.h"
#include "../scene_render.h"  // OsaScene, OsaDrawAt and the palette, for a description with draw()
#include "../../../include/omnisafe_amd_env.h"

#if !defined(OSA_CUSTOM_ENV_HEADER) || !defined(OSA_CUSTOM_ENV)
#error "custom_env.hip needs -DOSA_CUSTOM_ENV_HEADER=\"<header>\" and -DOSA_CUSTOM_ENV=<struct>"
#endif

#pragma clang fp contract(off)
#include OSA_CUSTOM_ENV_HEADER
#pragma clang fp contract(fast)

using OsaCustomEnv = OSA_CUSTOM_ENV;

// ---- the contract, checked member by member before anything is instantiated --------------------------------------
#define OSA_HAS_CONSTANT(NAME)                                 \
  template <class E, class = void>                             \
  struct OsaHas_##NAME : std::false_type {};                   \
  template <class E>                                           \
  struct OsaHas_##NAME<E, std::void_t<decltype(E::NAME)>> : std::true_type {}
OSA_HAS_CONSTANT(STATE);
OSA_HAS_CONSTANT(OBS);
OSA_HAS_CONSTANT(DYN);
OSA_HAS_CONSTANT(ACT);
OSA_HAS_CONSTANT(TRACE);
OSA_HAS_CONSTANT(LDS_ROW);
#undef OSA_HAS_CONSTANT
template <class E, class = void>
struct OsaHas_Regs : std::false_type {};
template <class E>
struct OsaHas_Regs<E, std::void_t<typename E::Regs>> : std::true_type {};

static_assert(OsaHas_STATE<OsaCustomEnv>::value, "custom env: the description has no member STATE (floats per state row)");
static_assert(OsaHas_OBS<OsaCustomEnv>::value, "custom env: the description has no member OBS (observation columns)");
static_assert(OsaHas_DYN<OsaCustomEnv>::value, "custom env: the description has no member DYN (state floats a transition changes)");
static_assert(OsaHas_ACT<OsaCustomEnv>::value, "custom env: the description has no member ACT (action columns)");
static_assert(OsaHas_TRACE<OsaCustomEnv>::value, "custom env: the description has no member TRACE (state floats of a trace record)");
static_assert(OsaHas_LDS_ROW<OsaCustomEnv>::value, "custom env: the description has no member LDS_ROW (must be false)");
static_assert(OsaHas_Regs<OsaCustomEnv>::value, "custom env: the description has no member struct Regs");

// The functions, asked for only where what they need is there (one message per missing member, not a cascade).
template <class E, class = void>
struct OsaHasLoad : std::false_type {};
template <class E>
struct OsaHasLoad<E, std::void_t<decltype(E::load(std::declval<typename E::Regs&>(), (const float*)nullptr))>>
    : std::true_type {};
template <class E, class = void>
struct OsaHasStore : std::false_type {};
template <class E>
struct OsaHasStore<E, std::void_t<decltype(E::store(std::declval<const typename E::Regs&>(), (float*)nullptr))>>
    : std::true_type {};
template <class E, class = void>
struct OsaHasFresh : std::false_type {};
template <class E>
struct OsaHasFresh<E, std::void_t<decltype(E::fresh(std::declval<typename E::Regs&>(), std::declval<const OsaEnvAt&>(),
                                                    (const float*)nullptr))>> : std::true_type {};
template <class E, class = void>
struct OsaHasObsCol : std::false_type {};
template <class E>
struct OsaHasObsCol<E, std::void_t<decltype(E::obs_col(std::declval<const typename E::Regs&>(), (const float*)nullptr,
                                                       0, 0))>> : std::true_type {};
template <class E, class = void>
struct OsaHasStateCol : std::false_type {};
template <class E>
struct OsaHasStateCol<E, std::void_t<decltype(E::state_col(std::declval<const typename E::Regs&>(),
                                                           (const float*)nullptr, 0))>> : std::true_type {};
template <class E, class = void>
struct OsaHasTransition2 : std::false_type {};
template <class E>
struct OsaHasTransition2<
    E, std::void_t<decltype(E::transition(std::declval<typename E::Regs&>(), (const float*)nullptr,
                                          std::declval<const OsaEnvAt&>(), 0.f, 0.f, std::declval<float&>(),
                                          std::declval<float&>()))>> : std::true_type {};

// terminal() is optional (OsaHasTerminal, env_device.h: whether it can be called), so a member of that NAME which cannot
// be called that way must not pass for "no termination".  The name alone: a lookup of `terminal` in a class derived
// from E and from a class that has one is ambiguous exactly when E has a member of that name, whatever its kind.
struct OsaTerminalName {
  int terminal;
};
template <class E>
struct OsaTerminalProbe : E, OsaTerminalName {};
template <class E, class = void>
struct OsaNamesTerminal : std::true_type {};
template <class E>
struct OsaNamesTerminal<E, std::void_t<decltype(&OsaTerminalProbe<E>::terminal)>> : std::false_type {};

// draw() is optional in the same way (OsaHasDraw, scene_render.h), and a member of that name which cannot be called as
// stated must not pass for "does not draw".
struct OsaDrawName {
  int draw;
};
template <class E>
struct OsaDrawProbe : E, OsaDrawName {};
template <class E, class = void>
struct OsaNamesDraw : std::true_type {};
template <class E>
struct OsaNamesDraw<E, std::void_t<decltype(&OsaDrawProbe<E>::draw)>> : std::false_type {};

// What a drawing description needs besides draw(), each asked for only where what it needs is there.
template <class E, bool = OsaHasDrawView<E>::value>
struct OsaDrawViewOk : std::true_type {};
template <class E>
struct OsaDrawViewOk<E, true> : std::integral_constant<bool, (E::DRAW_VIEW > 0)> {};
template <class E, bool = OsaHas_TRACE<E>::value>
struct OsaDrawTraceOk : std::true_type {};
template <class E>
struct OsaDrawTraceOk<E, true> : std::integral_constant<bool, (E::TRACE >= 1)> {};
template <class E, bool = OsaHasDraw<E>::value>
struct OsaCustomDraw {
  static constexpr bool callable = !OsaNamesDraw<E>::value, position = true, has_view = true, view = true, trace = true,
                        draws = false;
};
template <class E>
struct OsaCustomDraw<E, true> {
  static constexpr bool callable = true, position = OsaHasPosition<E>::value, has_view = OsaHasDrawView<E>::value,
                        view = OsaDrawViewOk<E>::value, trace = OsaDrawTraceOk<E>::value,
                        draws = position && has_view && view && trace && OsaHas_TRACE<E>::value;
};
static_assert(OsaCustomDraw<OsaCustomEnv>::callable,
              "custom env: the description has a member draw that cannot be called as draw(const float* rec, const "
              "OsaDrawAt&, OsaScene&); it would be an env that silently does not draw");
static_assert(OsaCustomDraw<OsaCustomEnv>::position,
              "custom env: a description with draw() needs position(const float* rec, float& x, float& y) (what the "
              "trail and the tracking camera follow)");
static_assert(OsaCustomDraw<OsaCustomEnv>::has_view,
              "custom env: a description with draw() needs DRAW_VIEW (half-width of the fixed camera's view)");
static_assert(OsaCustomDraw<OsaCustomEnv>::view, "custom env: DRAW_VIEW must be greater than 0");
static_assert(OsaCustomDraw<OsaCustomEnv>::trace,
              "custom env: a description with draw() needs TRACE >= 1 (draw() sees the TRACE leading state floats)");

template <class E, bool = OsaHas_Regs<E>::value>
struct OsaCustomFunctions {
  static constexpr bool load = true, store = true, fresh = true, obs_col = true, state_col = true, transition = true,
                        terminal = true, terminates = false;
};
template <class E>
struct OsaCustomFunctions<E, true> {
  static constexpr bool load = OsaHasLoad<E>::value, store = OsaHasStore<E>::value, fresh = OsaHasFresh<E>::value,
                        obs_col = OsaHasObsCol<E>::value, state_col = OsaHasStateCol<E>::value,
                        transition = OsaTakesActionRow<E>::value || OsaHasTransition2<E>::value,
                        terminates = OsaHasTerminal<E>::value,
                        terminal = terminates || !OsaNamesTerminal<E>::value;
};
static_assert(OsaCustomFunctions<OsaCustomEnv>::load, "custom env: the description has no load(Regs&, const float* srow)");
static_assert(OsaCustomFunctions<OsaCustomEnv>::store, "custom env: the description has no store(const Regs&, float* srow)");
static_assert(OsaCustomFunctions<OsaCustomEnv>::fresh,
              "custom env: the description has no fresh(Regs&, const OsaEnvAt&, const float* row)");
static_assert(OsaCustomFunctions<OsaCustomEnv>::obs_col,
              "custom env: the description has no obs_col(const Regs&, const float* row, int level, int col)");
static_assert(OsaCustomFunctions<OsaCustomEnv>::state_col,
              "custom env: the description has no state_col(const Regs&, const float* row, int col)");
static_assert(OsaCustomFunctions<OsaCustomEnv>::transition,
              "custom env: the description has no transition(Regs&, const float* row, const OsaEnvAt&, float a0, float "
              "a1, float& r, float& c) and no transition(..., const float* act, float& r, float& c)");
static_assert(OsaCustomFunctions<OsaCustomEnv>::terminal,
              "custom env: the description has a member terminal that cannot be called as bool terminal(const Regs&, "
              "const float* row, const OsaEnvAt&); it would be an env that never ends");

// The constants' ranges, each asked for only where the constant exists.
template <class E, bool = OsaHas_STATE<E>::value && OsaHas_OBS<E>::value && OsaHas_DYN<E>::value &&
                          OsaHas_ACT<E>::value && OsaHas_TRACE<E>::value && OsaHas_LDS_ROW<E>::value>
struct OsaCustomRanges {
  static constexpr bool registers = true, state = true, obs = true, dyn = true, act = true, trace = true,
                        complete = false;
};
template <class E>
struct OsaCustomRanges<E, true> {
  static constexpr bool registers = !E::LDS_ROW, state = E::STATE >= 1 && E::STATE <= 64, obs = E::OBS >= 1,
                        dyn = E::DYN >= 0 && E::DYN <= E::STATE, act = E::ACT >= 1 && E::ACT <= 32,
                        trace = E::TRACE >= 0 && E::TRACE <= E::STATE, complete = true;
};
static_assert(OsaCustomRanges<OsaCustomEnv>::registers,
              "custom env: LDS_ROW must be false (a description with an object row in LDS needs a kernel of its own, "
              "like osa_goal_env_kernel; out-of-tree descriptions keep their state in registers)");
static_assert(OsaCustomRanges<OsaCustomEnv>::state, "custom env: STATE must be 1 .. 64 floats");
static_assert(OsaCustomRanges<OsaCustomEnv>::obs, "custom env: OBS must be at least 1");
static_assert(OsaCustomRanges<OsaCustomEnv>::dyn, "custom env: DYN must be 0 .. STATE");
static_assert(OsaCustomRanges<OsaCustomEnv>::act, "custom env: ACT must be 1 .. 32 action columns");
static_assert(OsaCustomRanges<OsaCustomEnv>::trace, "custom env: TRACE must not exceed STATE");

constexpr int OSA_CUSTOM_LANES = OsaEnvLanes<OsaCustomEnv>::value;
constexpr int OSA_CUSTOM_LEVELS = OsaEnvLevels<OsaCustomEnv>::value;
static_assert(OSA_CUSTOM_LANES == 16 || OSA_CUSTOM_LANES == 32 || OSA_CUSTOM_LANES == 64,
              "custom env: LANES must be 16, 32 or 64");
static_assert(OSA_CUSTOM_LEVELS >= 0 && OSA_CUSTOM_LEVELS <= 2, "custom env: LEVELS (the highest level) must be 0 .. 2");

// Everything below needs the whole contract; with a part missing the messages above are the only ones.
template <class E, bool = OsaCustomRanges<E>::complete && OsaCustomRanges<E>::registers && OsaCustomRanges<E>::state &&
                          OsaCustomRanges<E>::obs && OsaCustomRanges<E>::act && OsaCustomRanges<E>::trace &&
                          OsaCustomFunctions<E>::load && OsaCustomFunctions<E>::store && OsaCustomFunctions<E>::fresh &&
                          OsaCustomFunctions<E>::obs_col && OsaCustomFunctions<E>::state_col &&
                          OsaCustomFunctions<E>::transition && OsaCustomFunctions<E>::terminal>
struct OsaCustomLib {
  static void info(int*) {}
  static int step(const OsaStepArgs&, void*) { return OSA_EUNSUPPORTED; }
  static int eval(const OsaEvalArgs&, int, int, void*) { return OSA_EUNSUPPORTED; }
  static int collect(const OsaCollectArgs&, int, int, void*) { return OSA_EUNSUPPORTED; }
};
template <class E>
struct OsaCustomLib<E, true> {
  static void info(int* out) {
    const int v[8] = {E::STATE,          E::OBS,           E::DYN, E::ACT, E::TRACE,
                      OSA_CUSTOM_LEVELS, OSA_CUSTOM_LANES, OsaCustomFunctions<E>::terminates ? 1 : 0};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
  }
  static int step(const OsaStepArgs& a, void* stream) {
    OSA_REQUIRE(a.level <= OSA_CUSTOM_LEVELS);
    return osa_env_step(osa_custom_env_kernel<E, OSA_CUSTOM_LANES>, E::OBS, 64 / OSA_CUSTOM_LANES, true, true, a,
                        stream, E::ACT);
  }
  static int eval(const OsaEvalArgs& a, int act_dim, int hidden, void* stream) {
    OSA_REQUIRE(a.level >= 0 && a.level <= OSA_CUSTOM_LEVELS);
    return osa_eval_launch<E>(a, act_dim, hidden, stream);
  }
  static int collect(const OsaCollectArgs& a, int act_dim, int hidden, void* stream) {
    OSA_REQUIRE(a.level >= 0 && a.level <= OSA_CUSTOM_LEVELS);
    return osa_collect_launch<E>(a, act_dim, hidden, stream);
  }
};

// The rasteriser, for a description that draws (and whose contract is whole); every library has both entry points.
template <class E, bool = OsaCustomDraw<E>::draws && OsaCustomDraw<E>::callable && OsaCustomRanges<E>::complete &&
                          OsaCustomRanges<E>::trace>
struct OsaCustomRender {
  static void info(int* out_i, float* out_f) {
    out_i[0] = 0;
    out_f[0] = out_f[1] = 0.f;
  }
  template <class... A>
  static int render(A...) {
    return OSA_EUNSUPPORTED;
  }
};
template <class E>
struct OsaCustomRender<E, true> {
  static void info(int* out_i, float* out_f) {
    out_i[0] = 1;
    out_f[0] = E::DRAW_VIEW;
    out_f[1] = OsaDrawTrack<E>::value;
  }
  template <class... A>
  static int render(A... args) {
    return osa_scene_render_launch<E>(args...);
  }
};
template <class E, bool = OsaHas_TRACE<E>::value>
struct OsaCustomTrace : std::integral_constant<int, 0> {};
template <class E>
struct OsaCustomTrace<E, true> : std::integral_constant<int, E::TRACE> {};

extern "C" {

int osa_custom_render_info(int* out_i, float* out_f) {
  OSA_REQUIRE(out_i && out_f);
  OsaCustomRender<OsaCustomEnv>::info(out_i, out_f);
  out_i[1] = OSA_DRAW_MAX;
  out_i[2] = OsaCustomTrace<OsaCustomEnv>::value;
  out_i[3] = 0;
  return OSA_OK;
}

int osa_custom_render_episode(int level, const float* state, long stride, int first, int count, int trail,
                              const uint8_t* hit, int camera, int width, int height, int supersample, uint8_t* rgb,
                              void* stream) {
  const int rc = osa_render_check(state, rgb, first, count, trail, camera, width, height, supersample);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(level >= 0 && level <= OSA_CUSTOM_LEVELS);
  return OsaCustomRender<OsaCustomEnv>::render(level, state, stride, first, count, trail, hit, camera, width, height,
                                               supersample, rgb, stream);
}

int osa_custom_env_info(int* out) {
  OSA_REQUIRE(out);
  OsaCustomLib<OsaCustomEnv>::info(out);
  return OSA_OK;
}

int osa_custom_env_step(unsigned long long seed, unsigned long long step, const unsigned long long* step_base, int N,
                        int obs_dim, int horizon, int level, float* state, int* steps, const float* action,
                        int ld_action, float* obs, int ld_obs, float* reward, float* cost, uint8_t* terminated,
                        uint8_t* truncated, float* final_obs, int ld_final, int reset_only, void* stream) {
  return OsaCustomLib<OsaCustomEnv>::step(
      {seed, step, step_base, N, obs_dim, horizon, level, 0.f, state, steps, action, ld_action, obs, ld_obs, reward,
       cost, terminated, truncated, final_obs, ld_final, reset_only},
      stream);
}

int osa_custom_eval_episodes(int level, int K, int obs_dim, int act_dim, int hidden, const float* params,
                             const float* norm_mean, const float* norm_std, const long* norm_count, float norm_clip,
                             const float* old_min, const float* old_max, float min_action, float max_action,
                             unsigned long long seed, int horizon, float cost_p, int max_steps, int saute,
                             float saute_budget, float saute_gamma, int early_terminated, double cost_limit,
                             double cost_criteria, double* ep_ret, double* ep_cost, int* ep_len, float* trace,
                             void* stream) {
  OsaEvalArgs a = {};
  a.params = params;
  a.K = K; a.obs_dim = obs_dim; a.max_steps = max_steps; a.horizon = horizon;
  a.mean = norm_mean; a.std_ = norm_std; a.count = norm_count; a.clip = norm_clip;
  a.old_min = old_min; a.old_max = old_max; a.min_a = min_action; a.max_a = max_action;
  a.seed = seed; a.cost_p = cost_p; a.level = level;
  a.ep_ret = ep_ret; a.ep_cost = ep_cost; a.ep_len = ep_len;
  a.saute = saute ? 1 : 0; a.budget = saute_budget; a.saute_gamma = saute_gamma;
  a.early_terminated = early_terminated ? 1 : 0; a.cost_limit = cost_limit; a.cost_criteria = cost_criteria;
  a.trace = trace;
  const int rc = osa_eval_check(a, act_dim);
  return rc != OSA_OK ? rc : OsaCustomLib<OsaCustomEnv>::eval(a, act_dim, hidden, stream);
}

int osa_custom_collect_episodes(int level, int K, int rows_per_lane, long total_rows, int obs_dim, int act_dim,
                                int hidden, const float* params, const float* norm_mean, const float* norm_std,
                                const long* norm_count, float norm_clip, const float* old_min, const float* old_max,
                                float min_action, float max_action, unsigned long long seed,
                                unsigned long long noise_seed, int horizon, float cost_p, float* obs, int ld_obs,
                                float* action, int ld_act, float* reward, float* cost, float* next_obs, int ld_next,
                                float* done, double* ep_ret_sum, double* ep_cost_sum, int* ep_count, void* stream) {
  OsaCollectArgs a = {};
  a.params = params;
  a.K = K; a.obs_dim = obs_dim; a.max_steps = rows_per_lane; a.horizon = horizon;
  a.mean = norm_mean; a.std_ = norm_std; a.count = norm_count; a.clip = norm_clip;
  a.old_min = old_min; a.old_max = old_max; a.min_a = min_action; a.max_a = max_action;
  a.seed = seed; a.cost_p = cost_p; a.level = level;
  a.ep_ret = ep_ret_sum; a.ep_cost = ep_cost_sum; a.ep_len = ep_count;
  a.total_rows = total_rows; a.noise_seed = noise_seed;
  a.obs = obs; a.action = action; a.reward = reward; a.cost = cost; a.next_obs = next_obs; a.done = done;
  a.ld_obs = ld_obs; a.ld_act = ld_act; a.ld_next = ld_next;
  const int rc = osa_collect_check(a, act_dim);
  return rc != OSA_OK ? rc : OsaCustomLib<OsaCustomEnv>::collect(a, act_dim, hidden, stream);
}

}  // extern "C"
