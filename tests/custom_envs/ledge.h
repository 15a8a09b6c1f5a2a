// A device env written against include/omnisafe_amd_env.h, for the tests: one that ends its own episodes.  A point
// walks along a ledge (the strip |p_y| <= 1) in the +x direction under sideways gusts; it falls off either edge or
// arrives behind x = 3, and both end the episode.  Level 1 charges for walking near an edge (|p_y| > 0.5), level 0
// never costs.
// State row, 6 floats:  [0:2] p  [2:4] v  [4] steps of this episode (as a float)  [5] 0
// Observation, 20 columns (two rounds of the column loop at 16 lanes): 0-1 p, 2-3 v, 4 the distance 1 - |p_y| to the
// nearer edge, and for j = col - 5 in 0 .. 14 the product x[j % 5] * (x[j / 5] + (j + 1) / 8) of the five state floats x.
// Random numbers of env n at position pos, all from osa_philox(seed ^ LEDGE_KEY, pos, (n << 20) + block):
//   block 1 the uniform of a reset (p_y), block 2 the uniform of a transition's gust.
// The numpy twin is tests/ledge_twin.py.
#pragma once
#define LEDGE_KEY 0x3C6EF372FE94F82Bull

// Everything but the end: the same walk on an endless plane (what the library reports as "does not terminate").
struct LedgeEndless {
  static constexpr int STATE = 6, OBS = 20, DYN = 5, ACT = 2, TRACE = 5, LEVELS = 1;
  static constexpr bool LDS_ROW = false;
  struct Regs {
    float x[DYN];
  };
  static __device__ __forceinline__ float pick(const Regs& s, int i) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < DYN; ++k)
      if (i == k) v = s.x[k];
    return v;
  }
  static __device__ __forceinline__ float uniform(uint32_t w, float half) { return half * (2.f * osa_u01(w) - 1.f); }
  static __device__ __forceinline__ void load(Regs& s, const float* __restrict__ srow) {
#pragma unroll
    for (int k = 0; k < DYN; ++k) s.x[k] = srow[k];
  }
  static __device__ __forceinline__ void store(const Regs& s, float* __restrict__ srow) {
#pragma unroll
    for (int k = 0; k < DYN; ++k) srow[k] = s.x[k];
    srow[5] = 0.f;  // (the whole row is the env's, whatever the caller's matrix held)
  }
  static __device__ __forceinline__ void fresh(Regs& s, const OsaEnvAt& at, const float*) {
    uint32_t w[4];
    osa_philox(at.seed ^ LEDGE_KEY, at.pos, ((unsigned long long)at.n << 20) + 1, w);
    s.x[0] = 0.f;
    s.x[1] = uniform(w[0], 0.4f);
    s.x[2] = s.x[3] = 0.f;
    s.x[4] = 0.f;
  }
  static __device__ __forceinline__ void transition(Regs& s, const float*, const OsaEnvAt& at, float a0, float a1,
                                                    float& r, float& c) {
    uint32_t w[4];
    osa_philox(at.seed ^ LEDGE_KEY, at.pos, ((unsigned long long)at.n << 20) + 2, w);
    const float a[2] = {fminf(fmaxf(a0, -1.f), 1.f), fminf(fmaxf(a1, -1.f), 1.f)};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float va = 0.9f * s.x[2 + i], vb = 0.05f * a[i];
      s.x[2 + i] = va + vb;
    }
    s.x[3] = s.x[3] + uniform(w[0], 0.04f);  // the gust
    s.x[0] = s.x[0] + s.x[2];
    s.x[1] = s.x[1] + s.x[3];
    s.x[4] = s.x[4] + 1.f;
    r = s.x[2] + (s.x[0] > 3.f ? 1.f : 0.f);
    c = (at.level >= 1 && fabsf(s.x[1]) > 0.5f) ? 1.f : 0.f;
  }
  static __device__ __forceinline__ float obs_col(const Regs& s, const float*, int, int col) {
    if (col >= OBS) return 0.f;
    if (col < 4) return pick(s, col);
    if (col == 4) return 1.f - fabsf(s.x[1]);
    const int j = col - 5;
    return pick(s, j % 5) * (pick(s, j / 5) + 0.125f * (float)(j + 1));
  }
  static __device__ __forceinline__ float state_col(const Regs& s, const float*, int col) { return pick(s, col); }
};

// The ledge: off either edge, or arrived.
struct Ledge : LedgeEndless {
  static __device__ __forceinline__ bool terminal(const Regs& s, const float*, const OsaEnvAt&) {
    return fabsf(s.x[1]) > 1.f || s.x[0] > 3.f;
  }
};

// The same env on the other lane counts of the generic per-step kernel (the default is 32).
struct Ledge16 : Ledge {
  static constexpr int LANES = 16;
};
struct Ledge64 : Ledge {
  static constexpr int LANES = 64;
};
