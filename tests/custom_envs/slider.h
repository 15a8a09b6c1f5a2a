// The narrowest env the contract allows, for the tests: ONE action column (ACT = 1) in the two-column form of
// transition, whose a1 must then arrive as 0 -- it is added to the velocity, so anything read behind the env's one
// action float would show.  A bead on a wire: v <- 0.9 v + (0.05 clip(a0) + a1), p <- clip(p + v, -2, 2), reward v,
// cost 1 where |p| > 1.  State row, 2 floats: p, v.  Observation, 3 columns: p, v, p * v.  A reset draws p = 2 u - 1
// from word 0 of osa_philox(seed ^ SLIDER_KEY, pos, (n << 20) + 1).  The numpy twin is in tests/custom_env_twin.py.
#pragma once
#define SLIDER_KEY 0x2545F4914F6CDD1Dull

struct Slider {
  static constexpr int STATE = 2, OBS = 3, DYN = 2, ACT = 1, TRACE = 2, LEVELS = 0;
  static constexpr bool LDS_ROW = false;
  struct Regs {
    float p, v;
  };
  static __device__ __forceinline__ void load(Regs& s, const float* __restrict__ srow) {
    s.p = srow[0];
    s.v = srow[1];
  }
  static __device__ __forceinline__ void store(const Regs& s, float* __restrict__ srow) {
    srow[0] = s.p;
    srow[1] = s.v;
  }
  static __device__ __forceinline__ void fresh(Regs& s, const OsaEnvAt& at, const float*) {
    uint32_t w[4];
    osa_philox(at.seed ^ SLIDER_KEY, at.pos, ((unsigned long long)at.n << 20) + 1, w);
    s.p = 2.f * osa_u01(w[0]) - 1.f;
    s.v = 0.f;
  }
  static __device__ __forceinline__ void transition(Regs& s, const float*, const OsaEnvAt&, float a0, float a1,
                                                    float& r, float& c) {
    const float a = fminf(fmaxf(a0, -1.f), 1.f);
    const float keep = 0.9f * s.v, push = 0.05f * a;
    s.v = keep + (push + a1);
    s.p = fminf(fmaxf(s.p + s.v, -2.f), 2.f);
    r = s.v;
    c = fabsf(s.p) > 1.f ? 1.f : 0.f;
  }
  static __device__ __forceinline__ float obs_col(const Regs& s, const float*, int, int col) {
    return col == 0 ? s.p : (col == 1 ? s.v : (col == 2 ? s.p * s.v : 0.f));
  }
  static __device__ __forceinline__ float state_col(const Regs& s, const float*, int col) {
    return col == 0 ? s.p : (col == 1 ? s.v : 0.f);
  }
};
