// One env description that is not in this tree, as a library of its own (omnisafe_amd.build.build_custom_env):
//   hipcc ... -DOSA_CUSTOM_ENV_HEADER="<absolute path of the header>" -DOSA_CUSTOM_ENV=<struct> custom_env.hip
// The header is included behind env_device.h and inside a `fp contract(off)` region: its arithmetic is float32 without
// fused multiply-adds, and it may use everything env_device.h has (osa_philox, osa_u01, osa_nav_*, OsaNavEnv<...>).
// The description contract and the entry points are specified in include/omnisafe_amd_env.h.  This file is in a
// directory of its own because every csrc/*.hip goes into libomnisafe_amd.so.
#include <string.h>

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
static_assert(OsaHas_LDS_ROW<OsaCustomEnv>::value, "custom env: the description has no member LDS_ROW (false: the state is the Regs; true: an object row in LDS)");
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

// fresh_obj(const OsaEnvAt&, int col) -> float is what a description with LDS_ROW = true writes its object columns with;
// a member of that name which cannot be called that way is told so (the name alone, as for terminal).
template <class E, class = void>
struct OsaHasFreshObj : std::false_type {};
template <class E>
struct OsaHasFreshObj<E, std::void_t<decltype(static_cast<float>(E::fresh_obj(std::declval<const OsaEnvAt&>(), 0)))>>
    : std::true_type {};
struct OsaFreshObjName {
  int fresh_obj;
};
template <class E>
struct OsaFreshObjProbe : E, OsaFreshObjName {};
template <class E, class = void>
struct OsaNamesFreshObj : std::true_type {};
template <class E>
struct OsaNamesFreshObj<E, std::void_t<decltype(&OsaFreshObjProbe<E>::fresh_obj)>> : std::false_type {};

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

// ---- runtime parameters (optional: PARAMS, PARAM_DEFAULT, PARAM_NAMES, bind) --------------------------------------
#define OSA_HAS_CONSTANT(NAME)                                 \
  template <class E, class = void>                             \
  struct OsaHas_##NAME : std::false_type {};                   \
  template <class E>                                           \
  struct OsaHas_##NAME<E, std::void_t<decltype(E::NAME)>> : std::true_type {}
OSA_HAS_CONSTANT(PARAMS);
OSA_HAS_CONSTANT(PARAM_DEFAULT);
OSA_HAS_CONSTANT(PARAM_NAMES);
#undef OSA_HAS_CONSTANT
template <class E, class = void>
struct OsaHasBind : std::false_type {};
template <class E>
struct OsaHasBind<E, std::void_t<decltype(E::bind(std::declval<typename E::Regs&>(), (const float*)nullptr))>>
    : std::true_type {};
// (the name alone, as for terminal and draw: a bind that cannot be called would be parameters that never arrive)
struct OsaBindName {
  int bind;
};
template <class E>
struct OsaBindProbe : E, OsaBindName {};
template <class E, class = void>
struct OsaNamesBind : std::true_type {};
template <class E>
struct OsaNamesBind<E, std::void_t<decltype(&OsaBindProbe<E>::bind)>> : std::false_type {};

constexpr bool osa_name_char(char c, bool first) {
  return c == '_' || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (!first && c >= '0' && c <= '9');
}
constexpr bool osa_name_is(const char* a, const char* b) {
  for (; *a && *a == *b; ++a, ++b) {}
  return *a == *b;
}
// 0: the names are fine; 1: one is no identifier; 2: two are the same; 3: one is `horizon` or `seed`.
template <class E>
constexpr int osa_param_names_fault() {
  for (int k = 0; k < E::PARAMS; ++k) {
    const char* s = E::PARAM_NAMES[k];
    if (s == nullptr || !osa_name_char(s[0], true)) return 1;
    for (int i = 1; s[i]; ++i)
      if (!osa_name_char(s[i], false)) return 1;
  }
  for (int k = 0; k < E::PARAMS; ++k) {
    if (osa_name_is(E::PARAM_NAMES[k], "horizon") || osa_name_is(E::PARAM_NAMES[k], "seed")) return 3;
    for (int j = 0; j < k; ++j)
      if (osa_name_is(E::PARAM_NAMES[k], E::PARAM_NAMES[j])) return 2;
  }
  return 0;
}
template <class E, bool = false>
struct OsaParamNamesFault : std::integral_constant<int, 0> {};
template <class E>
struct OsaParamNamesFault<E, true> : std::integral_constant<int, osa_param_names_fault<E>()> {};
template <class E, bool = false>
struct OsaParamLengths {
  static constexpr bool defaults = true, names = true;
};
template <class E>
struct OsaParamLengths<E, true> {
  static constexpr bool defaults = (int)std::extent<decltype(E::PARAM_DEFAULT)>::value == E::PARAMS,
                        names = (int)std::extent<decltype(E::PARAM_NAMES)>::value == E::PARAMS;
};

template <class E, bool = OsaHas_PARAMS<E>::value>
struct OsaCustomParams {
  static constexpr bool count = true, has_bind = true, has_default = true, has_names = true, default_len = true,
                        names_len = true, callable = true, declared = false, whole = true;
  static constexpr int names_fault = 0;
};
template <class E>
struct OsaCustomParams<E, true> {
  static constexpr bool count = E::PARAMS >= 1 && E::PARAMS <= OSA_PARAM_MAX,
                        binds = OsaHas_Regs<E>::value && OsaHasBind<E>::value,
                        has_bind = binds || OsaNamesBind<E>::value || !OsaHas_Regs<E>::value,  // (named: `callable`)
                        callable = binds || !OsaNamesBind<E>::value || !OsaHas_Regs<E>::value,
                        has_default = OsaHas_PARAM_DEFAULT<E>::value, has_names = OsaHas_PARAM_NAMES<E>::value,
                        arrays = count && has_default && has_names,
                        default_len = OsaParamLengths<E, arrays>::defaults,
                        names_len = OsaParamLengths<E, arrays>::names, declared = true;
  static constexpr int names_fault = OsaParamNamesFault<E, arrays && default_len && names_len>::value;
  static constexpr bool whole = arrays && binds && default_len && names_len && names_fault == 0;
};
using OsaParamsOf = OsaCustomParams<OsaCustomEnv>;
static_assert(OsaParamsOf::count, "custom env: PARAMS must be 1 .. 16 runtime parameters");
static_assert(OsaParamsOf::has_bind,
              "custom env: a description with PARAMS needs bind(Regs&, const float* par) (what copies the parameters "
              "into Regs)");
static_assert(OsaParamsOf::callable,
              "custom env: the description has a member bind that cannot be called as bind(Regs&, const float* par); "
              "its parameters would never arrive");
static_assert(OsaParamsOf::has_default, "custom env: a description with PARAMS needs PARAM_DEFAULT[PARAMS]");
static_assert(OsaParamsOf::has_names, "custom env: a description with PARAMS needs PARAM_NAMES[PARAMS]");
static_assert(OsaParamsOf::default_len, "custom env: PARAM_DEFAULT must have PARAMS elements");
static_assert(OsaParamsOf::names_len, "custom env: PARAM_NAMES must have PARAMS elements");
static_assert(OsaParamsOf::names_fault != 1, "custom env: every name in PARAM_NAMES must be an identifier");
static_assert(OsaParamsOf::names_fault != 2, "custom env: the names in PARAM_NAMES must differ from each other");
static_assert(OsaParamsOf::names_fault != 3,
              "custom env: PARAM_NAMES must not name `horizon` or `seed` (make() takes those itself)");

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
  static constexpr bool registers = true, fresh_obj = true, state = true, row_state = true, obs = true, dyn = true,
                        act = true, trace = true, complete = false;
};
template <class E>
struct OsaCustomRanges<E, true> {
  // A row in LDS needs fresh_obj; a member of that name with another signature gets the message of its own alone.
  static constexpr bool fresh_obj = !E::LDS_ROW || OsaHasFreshObj<E>::value || !OsaNamesFreshObj<E>::value,
                        registers = !E::LDS_ROW || OsaNamesFreshObj<E>::value,
                        state = E::LDS_ROW || (E::STATE >= 1 && E::STATE <= 64),
                        row_state = !E::LDS_ROW || (E::STATE >= 1 && E::STATE <= OSA_ROW_STATE_MAX), obs = E::OBS >= 1,
                        dyn = E::DYN >= 0 && E::DYN <= E::STATE, act = E::ACT >= 1 && E::ACT <= 32,
                        trace = E::TRACE >= 0 && E::TRACE <= E::STATE, complete = true;
};
static_assert(OsaCustomRanges<OsaCustomEnv>::registers,
              "custom env: LDS_ROW must be false for a description without fresh_obj(const OsaEnvAt&, int col) (the "
              "object columns [DYN, STATE) of a row in LDS are written by it at every reset; a description without "
              "objects keeps its state in registers)");
static_assert(OsaCustomRanges<OsaCustomEnv>::fresh_obj,
              "custom env: the description has a member fresh_obj that cannot be called as float fresh_obj(const "
              "OsaEnvAt&, int col); its object columns would never be written");
static_assert(OsaCustomRanges<OsaCustomEnv>::state,
              "custom env: STATE must be 1 .. 64 floats (a description with LDS_ROW = true may have up to 256)");
static_assert(OsaCustomRanges<OsaCustomEnv>::row_state,
              "custom env: with LDS_ROW = true STATE must be 1 .. 256 floats");
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
// `p`: the parameter arguments of a parameter-taking entry point, nullptr from a plain one.  A library with PARAMS takes
// the former alone (the plain forms would run with unbound parameters), one without PARAMS the latter alone.
struct OsaParamArgs {
  const float* range;
  float* par;
  int ld_par;
};
template <class E, bool = OsaCustomRanges<E>::complete && OsaCustomRanges<E>::registers &&
                          OsaCustomRanges<E>::fresh_obj && OsaCustomRanges<E>::state && OsaCustomRanges<E>::row_state &&
                          OsaCustomRanges<E>::dyn && OsaCustomRanges<E>::obs && OsaCustomRanges<E>::act && OsaCustomRanges<E>::trace &&
                          OsaCustomFunctions<E>::load && OsaCustomFunctions<E>::store && OsaCustomFunctions<E>::fresh &&
                          OsaCustomFunctions<E>::obs_col && OsaCustomFunctions<E>::state_col &&
                          OsaCustomFunctions<E>::transition && OsaCustomFunctions<E>::terminal &&
                          OsaCustomParams<E>::whole>
struct OsaCustomLib {
  static constexpr int P = 0;
  static void info(int*) {}
  static constexpr bool lds_row = false;
  static void param_info(float*, const char**) {}
  static int params(const OsaParamArgs*) { return OSA_EUNSUPPORTED; }
  static int step(const OsaStepArgs&, const OsaParamArgs*, void*) { return OSA_EUNSUPPORTED; }
  static int eval(OsaEvalArgs&, const OsaParamArgs*, int, int, void*) { return OSA_EUNSUPPORTED; }
  static int collect(OsaCollectArgs&, const OsaParamArgs*, int, int, void*) { return OSA_EUNSUPPORTED; }
};
template <class E>
struct OsaCustomLib<E, true> {
  static constexpr int P = OsaEnvParams<E>::value;
  static constexpr bool lds_row = E::LDS_ROW;
  static void info(int* out) {
    const int v[8] = {E::STATE,          E::OBS,           E::DYN, E::ACT, E::TRACE,
                      OSA_CUSTOM_LEVELS, OSA_CUSTOM_LANES, OsaCustomFunctions<E>::terminates ? 1 : 0};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
  }
  static void param_info(float* defaults, const char** names) {
    if constexpr (P > 0)
      for (int k = 0; k < P; ++k) {
        defaults[k] = E::PARAM_DEFAULT[k];
        names[k] = E::PARAM_NAMES[k];
      }
  }
  // The check of the parameter arguments, which every entry point makes first.
  static int params(const OsaParamArgs* p) {
    if ((p != nullptr) != (P > 0)) return OSA_EUNSUPPORTED;
    if (p) OSA_REQUIRE(p->range && p->par && p->ld_par >= P);
    return OSA_OK;
  }
  static int step(const OsaStepArgs& a, const OsaParamArgs* p, void* stream) {
    OSA_REQUIRE(a.level <= OSA_CUSTOM_LEVELS);
    OsaCustomStepArgs<E> args;
    static_cast<OsaStepArgs&>(args) = a;
    if constexpr (P > 0) {
      args.range = p->range;
      args.par = p->par;
      args.ld_par = p->ld_par;
    }
    if constexpr (E::LDS_ROW)
      return osa_env_step(osa_custom_row_env_kernel<E, OSA_CUSTOM_LANES>, E::OBS, 64 / OSA_CUSTOM_LANES, true, true,
                          args, stream, E::ACT);
    else
      return osa_env_step(osa_custom_env_kernel<E, OSA_CUSTOM_LANES>, E::OBS, 64 / OSA_CUSTOM_LANES, true, true, args,
                          stream, E::ACT);
  }
  template <class Args>
  static int player(Args& a, const OsaParamArgs* p) {
    OSA_REQUIRE(a.level >= 0 && a.level <= OSA_CUSTOM_LEVELS);
    if (p) {
      a.range = p->range;
      a.par = p->par;
      a.ld_par = p->ld_par;
    }
    return OSA_OK;
  }
  static int eval(OsaEvalArgs& a, const OsaParamArgs* p, int act_dim, int hidden, void* stream) {
    const int rc = player(a, p);
    return rc != OSA_OK ? rc : osa_eval_launch<E>(a, act_dim, hidden, stream);
  }
  static int collect(OsaCollectArgs& a, const OsaParamArgs* p, int act_dim, int hidden, void* stream) {
    const int rc = player(a, p);
    return rc != OSA_OK ? rc : osa_collect_launch<E>(a, act_dim, hidden, stream);
  }
};

// The rasteriser, for a description that draws (and whose contract is whole); every library has both entry points.
template <class E, bool = OsaCustomDraw<E>::draws && OsaCustomDraw<E>::callable && OsaCustomRanges<E>::complete &&
                          OsaCustomRanges<E>::trace && OsaCustomParams<E>::whole>
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

// The entry points, each in a plain form and a parameter-taking one: the bodies, with `p` as OsaCustomLib takes it.
static int osa_custom_render(const float* par, bool takes_par, int level, const float* state, long stride, int first,
                             int count, int trail, const uint8_t* hit, int camera, int width, int height,
                             int supersample, uint8_t* rgb, void* stream) {
  const int rc = osa_render_check(state, rgb, first, count, trail, camera, width, height, supersample);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(level >= 0 && level <= OSA_CUSTOM_LEVELS);
  if (takes_par != (OsaCustomLib<OsaCustomEnv>::P > 0)) return OSA_EUNSUPPORTED;
  OSA_REQUIRE(!takes_par || par);
  return OsaCustomRender<OsaCustomEnv>::render(level, state, stride, first, count, trail, hit, camera, width, height,
                                               supersample, rgb, par, stream);
}

static int osa_custom_step(const OsaParamArgs* p, unsigned long long seed, unsigned long long step,
                           const unsigned long long* step_base, int N, int obs_dim, int horizon, int level,
                           float* state, int* steps, const float* action, int ld_action, float* obs, int ld_obs,
                           float* reward, float* cost, uint8_t* terminated, uint8_t* truncated, float* final_obs,
                           int ld_final, int reset_only, void* stream) {
  const int rc = OsaCustomLib<OsaCustomEnv>::params(p);
  if (rc != OSA_OK) return rc;
  return OsaCustomLib<OsaCustomEnv>::step(
      {seed, step, step_base, N, obs_dim, horizon, level, 0.f, state, steps, action, ld_action, obs, ld_obs, reward,
       cost, terminated, truncated, final_obs, ld_final, reset_only},
      p, stream);
}

static int osa_custom_eval(const OsaParamArgs* p, int level, int K, int obs_dim, int act_dim, int hidden,
                           const float* params, const float* norm_mean, const float* norm_std, const long* norm_count,
                           float norm_clip, const float* old_min, const float* old_max, float min_action,
                           float max_action, unsigned long long seed, int horizon, float cost_p, int max_steps,
                           int saute, float saute_budget, float saute_gamma, int early_terminated, double cost_limit,
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
  int rc = OsaCustomLib<OsaCustomEnv>::params(p);
  if (rc == OSA_OK) rc = osa_eval_check(a, act_dim);
  return rc != OSA_OK ? rc : OsaCustomLib<OsaCustomEnv>::eval(a, p, act_dim, hidden, stream);
}

static int osa_custom_collect(const OsaParamArgs* p, int level, int K, int rows_per_lane, long total_rows, int obs_dim,
                              int act_dim, int hidden, const float* params, const float* norm_mean,
                              const float* norm_std, const long* norm_count, float norm_clip, const float* old_min,
                              const float* old_max, float min_action, float max_action, unsigned long long seed,
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
  int rc = OsaCustomLib<OsaCustomEnv>::params(p);
  if (rc == OSA_OK) rc = osa_collect_check(a, act_dim);
  return rc != OSA_OK ? rc : OsaCustomLib<OsaCustomEnv>::collect(a, p, act_dim, hidden, stream);
}

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
  return osa_custom_render(nullptr, false, level, state, stride, first, count, trail, hit, camera, width, height,
                           supersample, rgb, stream);
}

int osa_custom_render_episode_params(int level, const float* state, long stride, int first, int count, int trail,
                                     const uint8_t* hit, int camera, int width, int height, int supersample,
                                     uint8_t* rgb, const float* par, void* stream) {
  return osa_custom_render(par, true, level, state, stride, first, count, trail, hit, camera, width, height,
                           supersample, rgb, stream);
}

int osa_custom_env_info(int* out) {
  OSA_REQUIRE(out);
  OsaCustomLib<OsaCustomEnv>::info(out);
  return OSA_OK;
}

int osa_custom_row_info(int* out) {
  OSA_REQUIRE(out);
  out[0] = OsaCustomLib<OsaCustomEnv>::lds_row ? 1 : 0;
  out[1] = OsaCustomLib<OsaCustomEnv>::lds_row ? OSA_ROW_STATE_MAX : 64;
  out[2] = out[3] = 0;
  return OSA_OK;
}

int osa_custom_param_info(int* count, float* defaults, char* names, int cap) {
  OSA_REQUIRE(count);
  constexpr int P = OsaCustomLib<OsaCustomEnv>::P;
  *count = P;
  float value[OSA_PARAM_MAX] = {};
  const char* name[OSA_PARAM_MAX] = {};
  OsaCustomLib<OsaCustomEnv>::param_info(value, name);
  if (defaults)
    for (int k = 0; k < P; ++k) defaults[k] = value[k];
  if (names) {  // the names, a space between two of them, and the terminating 0
    int at = 0;
    for (int k = 0; k < P; ++k) {
      const int len = (int)strlen(name[k]);
      OSA_REQUIRE(at + len + 1 < cap);
      memcpy(names + at, name[k], len);
      at += len;
      if (k + 1 < P) names[at++] = ' ';
    }
    OSA_REQUIRE(at < cap);
    names[at] = 0;
  }
  return OSA_OK;
}

int osa_custom_env_step(unsigned long long seed, unsigned long long step, const unsigned long long* step_base, int N,
                        int obs_dim, int horizon, int level, float* state, int* steps, const float* action,
                        int ld_action, float* obs, int ld_obs, float* reward, float* cost, uint8_t* terminated,
                        uint8_t* truncated, float* final_obs, int ld_final, int reset_only, void* stream) {
  return osa_custom_step(nullptr, seed, step, step_base, N, obs_dim, horizon, level, state, steps, action, ld_action,
                         obs, ld_obs, reward, cost, terminated, truncated, final_obs, ld_final, reset_only, stream);
}

int osa_custom_env_step_params(unsigned long long seed, unsigned long long step, const unsigned long long* step_base,
                               int N, int obs_dim, int horizon, int level, float* state, int* steps,
                               const float* action, int ld_action, float* obs, int ld_obs, float* reward, float* cost,
                               uint8_t* terminated, uint8_t* truncated, float* final_obs, int ld_final, int reset_only,
                               const float* range, float* par, int ld_par, void* stream) {
  const OsaParamArgs p = {range, par, ld_par};
  return osa_custom_step(&p, seed, step, step_base, N, obs_dim, horizon, level, state, steps, action, ld_action, obs,
                         ld_obs, reward, cost, terminated, truncated, final_obs, ld_final, reset_only, stream);
}

int osa_custom_eval_episodes(int level, int K, int obs_dim, int act_dim, int hidden, const float* params,
                             const float* norm_mean, const float* norm_std, const long* norm_count, float norm_clip,
                             const float* old_min, const float* old_max, float min_action, float max_action,
                             unsigned long long seed, int horizon, float cost_p, int max_steps, int saute,
                             float saute_budget, float saute_gamma, int early_terminated, double cost_limit,
                             double cost_criteria, double* ep_ret, double* ep_cost, int* ep_len, float* trace,
                             void* stream) {
  return osa_custom_eval(nullptr, level, K, obs_dim, act_dim, hidden, params, norm_mean, norm_std, norm_count,
                         norm_clip, old_min, old_max, min_action, max_action, seed, horizon, cost_p, max_steps, saute,
                         saute_budget, saute_gamma, early_terminated, cost_limit, cost_criteria, ep_ret, ep_cost,
                         ep_len, trace, stream);
}

int osa_custom_eval_episodes_params(int level, int K, int obs_dim, int act_dim, int hidden, const float* params,
                                    const float* norm_mean, const float* norm_std, const long* norm_count,
                                    float norm_clip, const float* old_min, const float* old_max, float min_action,
                                    float max_action, unsigned long long seed, int horizon, float cost_p,
                                    int max_steps, int saute, float saute_budget, float saute_gamma,
                                    int early_terminated, double cost_limit, double cost_criteria, double* ep_ret,
                                    double* ep_cost, int* ep_len, float* trace, const float* range, float* par,
                                    int ld_par, void* stream) {
  const OsaParamArgs p = {range, par, ld_par};
  return osa_custom_eval(&p, level, K, obs_dim, act_dim, hidden, params, norm_mean, norm_std, norm_count, norm_clip,
                         old_min, old_max, min_action, max_action, seed, horizon, cost_p, max_steps, saute,
                         saute_budget, saute_gamma, early_terminated, cost_limit, cost_criteria, ep_ret, ep_cost,
                         ep_len, trace, stream);
}

int osa_custom_collect_episodes(int level, int K, int rows_per_lane, long total_rows, int obs_dim, int act_dim,
                                int hidden, const float* params, const float* norm_mean, const float* norm_std,
                                const long* norm_count, float norm_clip, const float* old_min, const float* old_max,
                                float min_action, float max_action, unsigned long long seed,
                                unsigned long long noise_seed, int horizon, float cost_p, float* obs, int ld_obs,
                                float* action, int ld_act, float* reward, float* cost, float* next_obs, int ld_next,
                                float* done, double* ep_ret_sum, double* ep_cost_sum, int* ep_count, void* stream) {
  return osa_custom_collect(nullptr, level, K, rows_per_lane, total_rows, obs_dim, act_dim, hidden, params, norm_mean,
                            norm_std, norm_count, norm_clip, old_min, old_max, min_action, max_action, seed,
                            noise_seed, horizon, cost_p, obs, ld_obs, action, ld_act, reward, cost, next_obs, ld_next,
                            done, ep_ret_sum, ep_cost_sum, ep_count, stream);
}

int osa_custom_collect_episodes_params(int level, int K, int rows_per_lane, long total_rows, int obs_dim, int act_dim,
                                       int hidden, const float* params, const float* norm_mean, const float* norm_std,
                                       const long* norm_count, float norm_clip, const float* old_min,
                                       const float* old_max, float min_action, float max_action,
                                       unsigned long long seed, unsigned long long noise_seed, int horizon,
                                       float cost_p, float* obs, int ld_obs, float* action, int ld_act, float* reward,
                                       float* cost, float* next_obs, int ld_next, float* done, double* ep_ret_sum,
                                       double* ep_cost_sum, int* ep_count, const float* range, float* par, int ld_par,
                                       void* stream) {
  const OsaParamArgs p = {range, par, ld_par};
  return osa_custom_collect(&p, level, K, rows_per_lane, total_rows, obs_dim, act_dim, hidden, params, norm_mean,
                            norm_std, norm_count, norm_clip, old_min, old_max, min_action, max_action, seed,
                            noise_seed, horizon, cost_p, obs, ld_obs, action, ld_act, reward, cost, next_obs, ld_next,
                            done, ep_ret_sum, ep_cost_sum, ep_count, stream);
}

}  // extern "C"
