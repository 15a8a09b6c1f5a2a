// A device env written against include/omnisafe_amd_env.h, for the tests: what no built-in family has.  A point mass in
// a box of half-width 2, pushed along three axes (ACT = 3: the row form of transition), that glides to goals which are
// redrawn when reached; level 1 charges for flying above or below the slab |p_z| <= 1, level 0 never costs.
// State row, 12 floats:  [0:3] p  [3:6] v  [6:9] g  [9] goals reached this episode  [10:12] 0
// Observation, 70 columns (a second round of the column loop at every LANES): 0-2 p, 3-5 v, 6-8 g - p, and for
// j = col - 9 in 0 .. 60 the product x[j % 9] * (x[j / 9] + (j + 1) / 8) of the first nine state floats x.
// Random numbers of env n at position pos, all from osa_philox(seed ^ GLIDER_KEY, pos, (n << 20) + block):
//   blocks 1 and 2 the six uniforms of a reset (p, then g), block 3 the three of a goal redrawn by the transition.
// The numpy twin is tests/custom_env_twin.py.
#pragma once
#define GLIDER_KEY 0x8F1BBCDCCA62C1D6ull

struct Glider {
  static constexpr int STATE = 12, OBS = 70, DYN = 10, ACT = 3, TRACE = 10, LEVELS = 1;
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
  static __device__ __forceinline__ float dist(const float* p, const float* g) {
    const float dx = p[0] - g[0], dy = p[1] - g[1], dz = p[2] - g[2];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return sqrtf((xx + yy) + zz);
  }
  static __device__ __forceinline__ void load(Regs& s, const float* __restrict__ srow) {
#pragma unroll
    for (int k = 0; k < DYN; ++k) s.x[k] = srow[k];
  }
  static __device__ __forceinline__ void store(const Regs& s, float* __restrict__ srow) {
#pragma unroll
    for (int k = 0; k < DYN; ++k) srow[k] = s.x[k];
    srow[10] = srow[11] = 0.f;  // (the whole row is the env's, whatever the caller's matrix held)
  }
  static __device__ __forceinline__ void fresh(Regs& s, const OsaEnvAt& at, const float*) {
    uint32_t w0[4], w1[4];
    osa_philox(at.seed ^ GLIDER_KEY, at.pos, ((unsigned long long)at.n << 20) + 1, w0);
    osa_philox(at.seed ^ GLIDER_KEY, at.pos, ((unsigned long long)at.n << 20) + 2, w1);
    s.x[0] = uniform(w0[0], 1.f);
    s.x[1] = uniform(w0[1], 1.f);
    s.x[2] = uniform(w0[2], 1.f);
    s.x[3] = s.x[4] = s.x[5] = 0.f;
    s.x[6] = uniform(w0[3], 1.5f);
    s.x[7] = uniform(w1[0], 1.5f);
    s.x[8] = uniform(w1[1], 1.5f);
    s.x[9] = 0.f;
  }
  static __device__ __forceinline__ void transition(Regs& s, const float*, const OsaEnvAt& at,
                                                    const float* __restrict__ act, float& r, float& c) {
    const float d0 = dist(s.x, s.x + 6);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float a = fminf(fmaxf(act[i], -1.f), 1.f);
      const float va = 0.9f * s.x[3 + i], vb = 0.05f * a;
      s.x[3 + i] = va + vb;
      s.x[i] = fminf(fmaxf(s.x[i] + s.x[3 + i], -2.f), 2.f);
    }
    const float d1 = dist(s.x, s.x + 6);
    const bool reached = d1 < 0.4f;
    r = (d0 - d1) + (reached ? 1.f : 0.f);
    c = (at.level >= 1 && fabsf(s.x[2]) > 1.f) ? 1.f : 0.f;
    if (reached) {
      uint32_t w[4];
      osa_philox(at.seed ^ GLIDER_KEY, at.pos, ((unsigned long long)at.n << 20) + 3, w);
      s.x[6] = uniform(w[0], 1.5f);
      s.x[7] = uniform(w[1], 1.5f);
      s.x[8] = uniform(w[2], 1.5f);
      s.x[9] = s.x[9] + 1.f;
    }
  }
  static __device__ __forceinline__ float obs_col(const Regs& s, const float*, int, int col) {
    if (col >= OBS) return 0.f;
    if (col < 6) return pick(s, col);
    if (col < 9) return pick(s, col) - pick(s, col - 6);
    const int j = col - 9;
    return pick(s, j % 9) * (pick(s, j / 9) + 0.125f * (float)(j + 1));
  }
  static __device__ __forceinline__ float state_col(const Regs& s, const float*, int col) { return pick(s, col); }
};

// The same env on the other lane counts of the generic per-step kernel (the default is 32).
struct Glider16 : Glider {
  static constexpr int LANES = 16;
};
struct Glider64 : Glider {
  static constexpr int LANES = 64;
};
