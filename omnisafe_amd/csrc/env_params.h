// Runtime parameters of a custom description (include/omnisafe_amd_env.h, PARAMETERS): how many it declares, and the
// draw of an env's row at a reset.  Everything that uses them sits behind `if constexpr` on OsaEnvParams<E>::value, so
// a description without the member PARAMS compiles to what it compiled to without this file.
#pragma once
#include <type_traits>

#include "env_device.h"

#define OSA_PARAM_KEY 0x8CB92BA72F3D8DD7ull  // the Philox key of the parameter draws is seed ^ OSA_PARAM_KEY
#define OSA_PARAM_MAX 16

// P of a description: E::PARAMS, or 0 without the member.
template <class E, class = void>
struct OsaEnvParams {
  static constexpr int value = 0;
};
template <class E>
struct OsaEnvParams<E, std::void_t<decltype(E::PARAMS)>> {
  static constexpr int value = E::PARAMS;
};
// (an array of P floats that is still an array at P = 0)
template <class E>
struct OsaParamRow {
  float v[OsaEnvParams<E>::value > 0 ? OsaEnvParams<E>::value : 1];
};

#pragma clang fp contract(off)
// The row of env n for the episode that a reset at stream position `pos` starts: parameter k is word k & 3 of the
// Philox block (seed ^ OSA_PARAM_KEY, pos, (n << 20) + (k >> 2)), uniform in its range (lo = range[k], hi =
// range[P + k]).  lo == hi gives exactly lo (span = 0, u finite), and the clamp keeps a rounded-up lo + span * u (u
// reaches 1) inside the range.  `range` is read at every call: it is the caller's device tensor, which may change
// between two launches of a captured graph.
template <int P>
__device__ __forceinline__ void osa_param_draw(unsigned long long seed, unsigned long long pos, int n,
                                               const float* range, float* par) {
#pragma unroll
  for (int b = 0; 4 * b < P; ++b) {
    uint32_t w[4];
    osa_philox(seed ^ OSA_PARAM_KEY, pos, ((unsigned long long)n << 20) + b, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 4 * b + i;
      if (k < P) {
        const float lo = range[k], hi = range[P + k];
        const float span = hi - lo;
        const float add = span * osa_u01(w[i]);
        par[k] = fminf(lo + add, hi);
      }
    }
  }
}

// What every reset does before E::fresh: redraw the row and hand it to the description.
template <class E>
__device__ __forceinline__ void osa_param_reset(typename E::Regs& s, const OsaEnvAt& at, const float* range,
                                                OsaParamRow<E>& row) {
  if constexpr (OsaEnvParams<E>::value > 0) {
    osa_param_draw<OsaEnvParams<E>::value>(at.seed, at.pos, at.n, range, row.v);
    E::bind(s, row.v);
  }
}
#pragma clang fp contract(fast)
