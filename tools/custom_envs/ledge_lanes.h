// tools/custom_env_timing.py: the non-terminating half of tests/custom_envs/ledge.h on the other lane counts, so that
// every Ledge row (which asks terminal() once per step) has its LedgeEndless row beside it.  (The library's digest does
// not follow this include: after a change of ledge.h, touch this file as well.)
#pragma once
#include "../../tests/custom_envs/ledge.h"
struct LedgeEndless16 : LedgeEndless {
  static constexpr int LANES = 16;
};
struct LedgeEndless64 : LedgeEndless {
  static constexpr int LANES = 64;
};
