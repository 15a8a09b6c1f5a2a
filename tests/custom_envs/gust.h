// A device env written against include/omnisafe_amd_env.h, for the tests of runtime parameters: a point mass flies to a
// goal disc through a cross-wind, and every member depends on a parameter.
//   wind   how hard the gusts push in +y                          (transition)
//   drag   the share of its velocity the point loses per step      (transition)
//   band   half-width of the cost-free corridor |p_y| <= band      (cost, observation columns 6 and 7, draw)
//   reach  the goal's radius; the goal lies at x = 1 + 2 reach     (fresh, terminal, draw)
// State row, 6 floats:  [0:2] p  [2:4] v  [4:6] goal
// Observation, 8 columns: 0-1 p, 2-3 v, 4-5 goal - p, 6 band, 7 the distance band - |p_y| to the corridor's nearer wall.
// Random numbers of env n at position pos, all from osa_philox(seed ^ GUST_KEY, pos, (n << 20) + block): block 1 the
// two uniforms of a reset (p_y, goal_y), block 2 the uniform of a transition's gust.  The parameter rows are the
// kernels' own draw (OSA_PARAM_KEY).  The numpy twin is tests/gust_twin.py.
#pragma once
#define GUST_KEY 0x5851F42D4C957F2Dull
#define GUST_WIND 0.2f
#define GUST_DRAG 0.25f
#define GUST_BAND 0.6f
#define GUST_REACH 0.2f

// The flight with its four values as compile-time constants: no PARAMS, load() puts the constants into Regs.
struct GustFlight {
  static constexpr int STATE = 6, OBS = 8, DYN = 4, ACT = 2, TRACE = 6, LEVELS = 0;
  static constexpr bool LDS_ROW = false;
  struct Regs {
    float x[STATE];
    float wind, drag, band, reach;
  };
  static __device__ __forceinline__ float uniform(uint32_t w, float half) { return half * (2.f * osa_u01(w) - 1.f); }
  static __device__ __forceinline__ float dist2(const Regs& s) {
    const float dx = s.x[4] - s.x[0], dy = s.x[5] - s.x[1];
    const float xx = dx * dx, yy = dy * dy;
    return xx + yy;
  }
  static __device__ __forceinline__ void load(Regs& s, const float* __restrict__ srow) {
#pragma unroll
    for (int k = 0; k < STATE; ++k) s.x[k] = srow[k];
    s.wind = GUST_WIND;
    s.drag = GUST_DRAG;
    s.band = GUST_BAND;
    s.reach = GUST_REACH;
  }
  static __device__ __forceinline__ void store(const Regs& s, float* __restrict__ srow) {
#pragma unroll
    for (int k = 0; k < STATE; ++k) srow[k] = s.x[k];
  }
  static __device__ __forceinline__ void fresh(Regs& s, const OsaEnvAt& at, const float*) {
    uint32_t w[4];
    osa_philox(at.seed ^ GUST_KEY, at.pos, ((unsigned long long)at.n << 20) + 1, w);
    s.x[0] = 0.f;
    s.x[1] = uniform(w[0], 0.3f);
    s.x[2] = s.x[3] = 0.f;
    const float off = 2.f * s.reach;
    s.x[4] = 1.f + off;
    s.x[5] = uniform(w[1], 0.5f);
  }
  static __device__ __forceinline__ void transition(Regs& s, const float*, const OsaEnvAt& at, float a0, float a1,
                                                    float& r, float& c) {
    uint32_t w[4];
    osa_philox(at.seed ^ GUST_KEY, at.pos, ((unsigned long long)at.n << 20) + 2, w);
    const float a[2] = {fminf(fmaxf(a0, -1.f), 1.f), fminf(fmaxf(a1, -1.f), 1.f)};
    const float keep = 1.f - s.drag;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float va = keep * s.x[2 + i], vb = 0.2f * a[i];
      s.x[2 + i] = va + vb;
    }
    const float gust = 0.05f + uniform(w[0], 0.05f);
    const float push = s.wind * gust;
    s.x[3] = s.x[3] + push;
    const float before = dist2(s);
    s.x[0] = s.x[0] + s.x[2];
    s.x[1] = s.x[1] + s.x[3];
    r = before - dist2(s);
    c = fabsf(s.x[1]) > s.band ? 1.f : 0.f;
  }
  static __device__ __forceinline__ float obs_col(const Regs& s, const float*, int, int col) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (col == k) v = s.x[k];
    if (col == 4) v = s.x[4] - s.x[0];
    if (col == 5) v = s.x[5] - s.x[1];
    if (col == 6) v = s.band;
    if (col == 7) v = s.band - fabsf(s.x[1]);
    return v;
  }
  static __device__ __forceinline__ float state_col(const Regs& s, const float*, int col) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < STATE; ++k)
      if (col == k) v = s.x[k];
    return v;
  }
};

// The four values as runtime parameters, and a picture that shows two of them.  Without an end of its own (the
// collector's per-step path takes no class that terminates).
struct GustEndless : GustFlight {
  static constexpr int PARAMS = 4;
  static constexpr float PARAM_DEFAULT[PARAMS] = {GUST_WIND, GUST_DRAG, GUST_BAND, GUST_REACH};
  static constexpr const char* PARAM_NAMES[PARAMS] = {"wind", "drag", "band", "reach"};
  static __device__ __forceinline__ void bind(Regs& s, const float* par) {
    s.wind = par[0];
    s.drag = par[1];
    s.band = par[2];
    s.reach = par[3];
  }
  static constexpr float DRAW_VIEW = 2.5f, DRAW_TRACK = 1.f;
  static __device__ __forceinline__ void position(const float* rec, float& x, float& y) {
    x = rec[0];
    y = rec[1];
  }
  static __device__ __forceinline__ void draw(const float* rec, const OsaDrawAt& at, OsaScene& scene) {
    const float band = at.par[2], reach = at.par[3];
    scene.box(-0.5f, -2.f, 2.4f, 2.f, OSA_COLOUR_COST);      // where flying costs
    scene.box(-0.5f, -band, 2.4f, band, OSA_COLOUR_FLOOR);   // the corridor: its walls sit at +-band
    scene.disc(rec[4], rec[5], reach * reach, OSA_COLOUR_GOAL);
    scene.trail(0.0009f, OSA_COLOUR_TRAIL);
    scene.disc(rec[0], rec[1], 0.01f, at.hit ? OSA_COLOUR_HIT : OSA_COLOUR_POINT);
  }
};

// The env of the tests: arriving inside the goal's radius ends the episode.
struct Gust : GustEndless {
  static __device__ __forceinline__ bool terminal(const Regs& s, const float*, const OsaEnvAt&) {
    return dist2(s) <= s.reach * s.reach;
  }
};

// The same env with the defaults as compile-time constants, for the timing (tools/custom_param_timing.py).
struct GustFixed : GustFlight {
  static __device__ __forceinline__ bool terminal(const Regs& s, const float*, const OsaEnvAt&) {
    return dist2(s) <= s.reach * s.reach;
  }
};
