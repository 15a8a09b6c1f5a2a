// The built-in families of the persistent kernels (eval_kernels.hip, collect_kernels.hip): one table of env kinds.
#pragma once
#include "env_device.h"

// The families: the OSA_EVAL_ENV_* constant of level 0, the highest level, the description.
#define OSA_EVAL_FAMILIES(X)                 \
  X(OSA_EVAL_ENV_SYNTH, 0, OsaSynthEnv)      \
  X(OSA_EVAL_ENV_REACH, 0, OsaReachEnv)      \
  X(OSA_EVAL_ENV_NAV0, 2, OsaPointGoal)      \
  X(OSA_EVAL_ENV_CIRCLE0, 2, OsaPointCircle) \
  X(OSA_EVAL_ENV_CARGOAL0, 2, OsaCarGoal)    \
  X(OSA_EVAL_ENV_CARCIRCLE0, 2, OsaCarCircle)

// What the host needs to know of an env_kind: one row per family, matched by family <= env_kind <= family + level.
struct OsaEvalKind {
  int family;            // the OSA_EVAL_ENV_* constant of the family; -1: unknown kind
  int level;             // in the table: the highest level; as returned: env_kind - family
  int state_floats;      // state floats of a trace record
};

static OsaEvalKind osa_eval_kind(int env_kind) {
#define OSA_KIND(FAMILY, LEVELS, E) {FAMILY, LEVELS, E::TRACE},
  static const OsaEvalKind kinds[] = {OSA_EVAL_FAMILIES(OSA_KIND)};
#undef OSA_KIND
  for (const OsaEvalKind& k : kinds)
    if (env_kind >= k.family && env_kind <= k.family + k.level)
      return {k.family, env_kind - k.family, k.state_floats};
  return {-1, 0, 0};
}
