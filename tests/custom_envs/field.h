// Field: a deliberately awkward description with an object row in LDS.  A point mass among 73 discs, a row of 150
// floats (wider than a wave, and its 146 object columns divide by neither 16, 32 nor 64), sensors and one 16-bin lidar,
// cost inside any disc, and an episode that ends of its own accord when the mass leaves the arena.  The numpy twin is
// tests/button_twin.py (field_*).
//
// State row, 150 floats: [0:2] p  [2:4] v  -- DYN = 4 --  [4:150] discs 73 x 2.
// Random numbers: key seed ^ FIELD_KEY, osa_nav_uniform's allocation: reset uniforms 0, 1 give p = 0.5 (u0, u1),
// v = 0; object column c is uniform c (blocks 1 .. 38).
// Transition under a = clip(action, -1, 1): v <- 0.9 v + 0.05 a, p <- p + v (each product and sum rounded);
// reward = the progress along x; cost = 1 inside a disc (distance < 0.15); terminal when |x| > 2 or |y| > 2.
// Observation, 20 columns: p, v, then the lidar of the discs in the world frame (the mass has no heading).
// FieldParam is the same description with the discs' radius as a runtime parameter (PARAMS with LDS_ROW = true): at its
// default, 0.15, it plays Field's episodes bit for bit.
#pragma once
#define FIELD_KEY 0x94D049BB133111EBull
template <bool RUNTIME_RADIUS>
struct FieldOf {
  static constexpr int STATE = 150, OBS = 20, DYN = 4, ACT = 2, TRACE = 150, LEVELS = 0, DISCS = 73;
  static constexpr bool LDS_ROW = true;
  struct Regs {
    float p[2], v[2];
    float radius;  // of a disc: the constant, or what bind() puts here (load and fresh then leave it alone)
  };
  static __device__ __forceinline__ void load(Regs& s, const float* __restrict__ row) {
    s.p[0] = row[0];
    s.p[1] = row[1];
    s.v[0] = row[2];
    s.v[1] = row[3];
    if constexpr (!RUNTIME_RADIUS) s.radius = 0.15f;
  }
  static __device__ __forceinline__ void store(const Regs& s, float* __restrict__ srow) {
    srow[0] = s.p[0];
    srow[1] = s.p[1];
    srow[2] = s.v[0];
    srow[3] = s.v[1];
  }
  static __device__ __forceinline__ float fresh_obj(const OsaEnvAt& at, int col) {
    return osa_nav_uniform(at.seed ^ FIELD_KEY, at.pos, at.n, 1, col);
  }
  static __device__ __forceinline__ void fresh(Regs& s, const OsaEnvAt& at, const float*) {
    s.p[0] = 0.5f * osa_nav_uniform(at.seed ^ FIELD_KEY, at.pos, at.n, 1, 0);
    s.p[1] = 0.5f * osa_nav_uniform(at.seed ^ FIELD_KEY, at.pos, at.n, 1, 1);
    s.v[0] = s.v[1] = 0.f;
    if constexpr (!RUNTIME_RADIUS) s.radius = 0.15f;
  }
  static __device__ __forceinline__ void transition(Regs& s, const float* __restrict__ row, const OsaEnvAt&, float a0_in,
                                                    float a1_in, float& r, float& c) {
    const float a0 = fminf(fmaxf(a0_in, -1.f), 1.f), a1 = fminf(fmaxf(a1_in, -1.f), 1.f);
    const float xa = 0.9f * s.v[0], xb = 0.05f * a0, ya = 0.9f * s.v[1], yb = 0.05f * a1;
    s.v[0] = xa + xb;
    s.v[1] = ya + yb;
    const float x0 = s.p[0];
    s.p[0] = s.p[0] + s.v[0];
    s.p[1] = s.p[1] + s.v[1];
    r = s.p[0] - x0;
    bool hit = false;
    for (int i = 0; i < DISCS; ++i)
      hit = hit || osa_reach_dist(s.p[0], s.p[1], row[DYN + 2 * i], row[DYN + 2 * i + 1]) < s.radius;
    c = hit ? 1.f : 0.f;
  }
  static __device__ __forceinline__ bool terminal(const Regs& s, const float*, const OsaEnvAt&) {
    return fabsf(s.p[0]) > 2.f || fabsf(s.p[1]) > 2.f;
  }
  static __device__ __forceinline__ float obs_col(const Regs& s, const float* __restrict__ row, int, int col) {
    if (col == 0) return s.p[0];
    if (col == 1) return s.p[1];
    if (col == 2) return s.v[0];
    if (col == 3) return s.v[1];
    if (col >= OBS) return 0.f;
    float out = 0.f;
    for (int i = 0; i < DISCS; ++i) {
      const float bx = row[DYN + 2 * i] - s.p[0], by = row[DYN + 2 * i + 1] - s.p[1];
      const float xx = bx * bx, yy = by * by;
      if (osa_nav_in_bin(col - 4, bx, by)) out = fmaxf(out, osa_nav_reading(sqrtf(xx + yy)));
    }
    return out;
  }
  static __device__ __forceinline__ float state_col(const Regs& s, const float* __restrict__ row, int col) {
    float v = col >= DYN ? row[col] : 0.f;
    if (col == 0) v = s.p[0];
    if (col == 1) v = s.p[1];
    if (col == 2) v = s.v[0];
    if (col == 3) v = s.v[1];
    return v;
  }
};
struct Field : FieldOf<false> {};
struct FieldParam : FieldOf<true> {
  static constexpr int PARAMS = 1;
  static constexpr float PARAM_DEFAULT[PARAMS] = {0.15f};
  static constexpr const char* PARAM_NAMES[PARAMS] = {"radius"};
  static __device__ __forceinline__ void bind(Regs& s, const float* par) { s.radius = par[0]; }
};
struct Field16 : Field {
  static constexpr int LANES = 16;
};
struct Field32 : Field {
  static constexpr int LANES = 32;
};
struct Field64 : Field {
  static constexpr int LANES = 64;
};
