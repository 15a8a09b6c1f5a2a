// The device-resident vector envs: their arithmetic as free functions, and at the end of the file one description per
// family (OsaSynthEnv, OsaReachEnv, OsaNavEnv<robot, task>) that binds it together for the per-step kernels
// (rollout_kernels.hip: osa_synth_env_kernel, osa_reach_env_kernel, osa_goal_env_kernel<robot>,
// osa_circle_env_kernel<robot, lanes>) and the persistent evaluation kernel (eval_kernels.hip).  Every random number is
// a Philox4x32-10 draw keyed by (seed, stream position `step`, env index n), so a caller that replays env n at
// positions 0, 1, 2, ... sees the same episode as the per-step launches.
#pragma once
#include <type_traits>
#include <utility>

#include "mlp_device.h"

// ------------------------------------------------------------------------------------------------
// Synth*-v0: obs ~ N(0,1)^D, reward ~ N(0,1), cost ~ Bernoulli(cost_p), never terminates.
// ------------------------------------------------------------------------------------------------
// Features 2 pair, 2 pair + 1 of env n at position `step`: (a, b) the observation of a step that does not
// truncate (and the final observation of one that does), (c2, d2) the post-reset observation of a truncating step.
__device__ __forceinline__ void osa_synth_obs_pair(unsigned long long seed, unsigned long long step, int n, int pair,
                                                   float& a, float& b, float& c2, float& d2) {
  uint32_t w[4];
  osa_philox(seed, step, ((unsigned long long)n << 20) + pair, w);
  osa_box_muller(w[0], w[1], a, b);
  osa_box_muller(w[2], w[3], c2, d2);  // second pair: the post-reset observation
}

// Reward and cost of env n's transition at position `step`, from the Philox block
// osa_philox(seed ^ OSA_SYNTH_RC_KEY, step, n).
#define OSA_SYNTH_RC_KEY 0x9E3779B97F4A7C15ull
__device__ __forceinline__ float osa_synth_reward(const uint32_t (&w)[4]) {
  float a, b;
  osa_box_muller(w[0], w[1], a, b);
  return a;
}
__device__ __forceinline__ float osa_synth_cost(const uint32_t (&w)[4], float cost_p) {
  return (osa_u01(w[2]) <= cost_p) ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------------
// SynthReach-v0: state p(2) g(2) h(2); dynamics stated in oracle/np_oracle.py:reach_env_step.  float32 without
// fused multiply-adds, so that the CPU twin sees the same arithmetic.
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
__device__ __forceinline__ float osa_reach_dist(float ux, float uy, float vx, float vy) {
  const float dx = ux - vx, dy = uy - vy;
  const float xx = dx * dx, yy = dy * dy;
  return sqrtf(xx + yy);
}

// column k of the observation row of state s: [p, g - p, h - p, 0 ...]
__device__ __forceinline__ float osa_reach_obs_col(const float (&s)[6], int k) {
  float v = 0.f;
  if (k == 0) v = s[0];
  if (k == 1) v = s[1];
  if (k == 2) v = s[2] - s[0];
  if (k == 3) v = s[3] - s[1];
  if (k == 4) v = s[4] - s[0];
  if (k == 5) v = s[5] - s[1];
  return v;
}

__device__ __forceinline__ float osa_reach_uniform(uint32_t w) {  // [-1, 1]
  return 2.f * osa_u01(w) - 1.f;
}

// Random numbers of env n at position `step`: the two Philox blocks
//   osa_philox(seed ^ OSA_REACH_KEY, step, (n << 20) + 1) -> w0,  ... + 2 -> w1;
// w0[0..3], w1[0..1] a fresh state (reset), w1[2..3] a new goal (osa_reach_transition).
#define OSA_REACH_KEY 0xD1B54A32D192ED03ull

// the fresh state of a reset
__device__ __forceinline__ void osa_reach_fresh(const uint32_t (&w0)[4], const uint32_t (&w1)[4], float (&fresh)[6]) {
  fresh[0] = osa_reach_uniform(w0[0]);
  fresh[1] = osa_reach_uniform(w0[1]);
  fresh[2] = osa_reach_uniform(w0[2]);
  fresh[3] = osa_reach_uniform(w0[3]);
  fresh[4] = osa_reach_uniform(w1[0]);
  fresh[5] = osa_reach_uniform(w1[1]);
}

// One transition of state s under the (unclamped) env action (a0, a1); w1 from osa_reach_draw of the same position.
__device__ __forceinline__ void osa_reach_transition(float (&s)[6], float a0_in, float a1_in, const uint32_t (&w1)[4],
                                                     float& r, float& c) {
  const float a0 = fminf(fmaxf(a0_in, -1.f), 1.f);
  const float a1 = fminf(fmaxf(a1_in, -1.f), 1.f);
  const float m0 = 0.1f * a0, m1 = 0.1f * a1;
  const float qx = fminf(fmaxf(s[0] + m0, -1.5f), 1.5f);
  const float qy = fminf(fmaxf(s[1] + m1, -1.5f), 1.5f);
  const float d0 = osa_reach_dist(s[0], s[1], s[2], s[3]);
  const float d1 = osa_reach_dist(qx, qy, s[2], s[3]);
  const bool reached = d1 < 0.15f;
  r = (d0 - d1) + (reached ? 1.f : 0.f);
  c = (osa_reach_dist(qx, qy, s[4], s[5]) < 0.3f) ? 1.f : 0.f;
  s[0] = qx;
  s[1] = qy;
  if (reached) {
    s[2] = osa_reach_uniform(w1[2]);
    s[3] = osa_reach_uniform(w1[3]);
  }
}

// ------------------------------------------------------------------------------------------------
// SynthNavGoal{0,1,2}-v0: a point robot with heading and inertia, a resampled goal, static hazards and vases, seen
// through three egocentric 16-bin lidars.  State row of an env, 64 floats:
//   [0:2] p  [2:4] u (unit heading)  [4] f (forward speed)  [5] f_prev  [6] t (last turn parameter)  [7] 0
//   [8:10] g  [10:12] 0  [12:32] hazards 10 x 2  [32:52] vases 10 x 2  [52:64] 0
// The callers keep the row in LDS (`row`: the objects, read-only between resets) and its first ten floats in
// registers (`d`: what a transition changes), the same in every lane that works on the env.  float32 with only
// + - * / sqrt min max and compares, no fused multiply-adds: the numpy twin kept with the tests (tests/nav_twin.py)
// computes the same bits.
// ------------------------------------------------------------------------------------------------
#define OSA_NAV_KEY 0xA0761D6478BD642Full
#define OSA_NAV_STATE 64  // floats per state row
#define OSA_NAV_DYN 10    // leading floats of the row that a transition changes
#define OSA_NAV_HAZ 12    // first hazard column of the row
#define OSA_NAV_VASE 32   // first vase column of the row

__device__ __forceinline__ int osa_nav_hazards(int level) { return level == 0 ? 0 : (level == 1 ? 8 : 10); }
__device__ __forceinline__ int osa_nav_vases(int level) { return level == 0 ? 0 : (level == 1 ? 1 : 10); }

// E[k] = (float32(cos(k pi / 8)), float32(sin(k pi / 8))) rounded from float64; lidar bin k lies between E[k] and
// E[(k + 1) & 15].
static __device__ const float OSA_NAV_EDGE[16][2] = {
    {1.f, 0.f},
    {0.923879504f, 0.382683426f},
    {0.707106769f, 0.707106769f},
    {0.382683426f, 0.923879504f},
    {6.12323426e-17f, 1.f},
    {-0.382683426f, 0.923879504f},
    {-0.707106769f, 0.707106769f},
    {-0.923879504f, 0.382683426f},
    {-1.f, 1.22464685e-16f},
    {-0.923879504f, -0.382683426f},
    {-0.707106769f, -0.707106769f},
    {-0.382683426f, -0.923879504f},
    {-1.83697015e-16f, -1.f},
    {0.382683426f, -0.923879504f},
    {0.707106769f, -0.707106769f},
    {0.923879504f, -0.382683426f},
};

// Uniform i of env n at position `pos`, ARENA (2 u01 - 1): word i % 4 of block first_block + i / 4.  Blocks 1 .. 13
// hold the 52 uniforms of a reset, blocks 14 and 15 the eight of a transition's goal candidates.
__device__ __forceinline__ float osa_nav_uniform(unsigned long long key, unsigned long long pos, int n,
                                                 int first_block, int i) {
  uint32_t w[4];
  osa_philox(key, pos, ((unsigned long long)n << 20) + (unsigned long long)(first_block + (i >> 2)), w);
  const int q = i & 3;
  const uint32_t x = q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
  return 1.5f * (2.f * osa_u01(x) - 1.f);
}

// Of the four candidate points c[0:2] .. c[6:8], the first whose distance to every hazard is >= KEEP; the fourth if
// none is.
__device__ __forceinline__ void osa_nav_pick_goal(const float (&c)[8], const float* __restrict__ row, int level,
                                                  float& gx, float& gy) {
  const int H = osa_nav_hazards(level);
  gx = c[6];
  gy = c[7];
  bool taken = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bool ok = true;
    for (int h = 0; h < H; ++h) {
      const float* __restrict__ o = row + OSA_NAV_HAZ + 2 * h;
      ok = ok && osa_reach_dist(c[2 * j], c[2 * j + 1], o[0], o[1]) >= 0.55f;
    }
    if (ok && !taken) {
      gx = c[2 * j];
      gy = c[2 * j + 1];
    }
    taken = taken || ok;
  }
}

// Column `col` (12 .. 63) of a fresh state row: hazard and vase coordinates are reset uniforms 12 .. 51, slots past
// the level's counts and the padding are 0.
__device__ __forceinline__ float osa_nav_fresh_obj(unsigned long long key, unsigned long long pos, int n, int level,
                                                   int col) {
  const bool haz = col >= OSA_NAV_HAZ && col < OSA_NAV_HAZ + 2 * osa_nav_hazards(level);
  const bool vase = col >= OSA_NAV_VASE && col < OSA_NAV_VASE + 2 * osa_nav_vases(level);
  return (haz || vase) ? osa_nav_uniform(key, pos, n, 1, col) : 0.f;
}

// The first ten floats of a fresh state row (reset uniforms 0 .. 11); `row` already holds the fresh hazards.
__device__ __forceinline__ void osa_nav_fresh(unsigned long long key, unsigned long long pos, int n, int level,
                                              const float* __restrict__ row, float (&d)[OSA_NAV_DYN]) {
  float u[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) u[i] = osa_nav_uniform(key, pos, n, 1, i);
  d[0] = u[0];
  d[1] = u[1];
  const float xx = u[2] * u[2], yy = u[3] * u[3];
  const float nrm = sqrtf(xx + yy);
  d[2] = nrm > 0.f ? u[2] / nrm : 1.f;
  d[3] = nrm > 0.f ? u[3] / nrm : 0.f;
  d[4] = d[5] = d[6] = d[7] = 0.f;
  const float c[8] = {u[4], u[5], u[6], u[7], u[8], u[9], u[10], u[11]};
  osa_nav_pick_goal(c, row, level, d[8], d[9]);
}

// The motion of a transition from `tt = t * t` on, for a robot that has settled its forward speed f2 and its turn
// parameter t: the heading turned by the rational rotation of parameter t and renormalised, p <- clip(p + m, -2, 2)
// with m = f2 u the attempted displacement.  The point robot (osa_nav_move) and the Car (osa_car_move) differ only in how
// they arrive at (f2, t).
__device__ __forceinline__ void osa_nav_turn_and_go(float (&d)[OSA_NAV_DYN], float f2, float t, float& mx, float& my) {
  const float tt = t * t;
  const float den = 1.f + tt;
  const float cs = (1.f - tt) / den;
  const float sn = (2.f * t) / den;
  const float cx = cs * d[2], sy = sn * d[3], sx = sn * d[2], cy = cs * d[3];
  const float ux = cx - sy, uy = sx + cy;
  const float xx = ux * ux, yy = uy * uy;
  const float nrm = sqrtf(xx + yy);
  const float u2x = ux / nrm, u2y = uy / nrm;
  mx = f2 * u2x;
  my = f2 * u2y;
  d[0] = fminf(fmaxf(d[0] + mx, -2.f), 2.f);
  d[1] = fminf(fmaxf(d[1] + my, -2.f), 2.f);
  d[2] = u2x;
  d[3] = u2y;
  d[5] = d[4];
  d[4] = f2;
  d[6] = t;
}

// The motion of a transition under the (unclamped) env action (a0, a1): f <- 0.9 f + 0.02 a0, the heading turned by the
// rational rotation of parameter t = 0.15 a1 and renormalised, p <- clip(p + m, -2, 2) with m = f u the attempted
// displacement.  Shared by SynthNavGoal and SynthNavCircle.
__device__ __forceinline__ void osa_nav_move(float (&d)[OSA_NAV_DYN], float a0_in, float a1_in, float& mx, float& my) {
  const float a0 = fminf(fmaxf(a0_in, -1.f), 1.f);
  const float a1 = fminf(fmaxf(a1_in, -1.f), 1.f);
  const float fa = 0.9f * d[4], fb = 0.02f * a0;
  const float f2 = fa + fb;
  const float t = 0.15f * a1;
  osa_nav_turn_and_go(d, f2, t, mx, my);
}

// The Car's motion under the (unclamped) env action (a0, a1) = (left wheel, right wheel): each wheel speed lags its
// command, w <- 0.9 w + 0.02 a; the forward speed is the wheels' mean, f = 0.5 (w_l + w_r), and the turn parameter
// their difference, t = 0.375 (w_r - w_l); from there on the point robot's motion.  `d` is a SynthNavGoal `d` whose
// slot 7 holds t_prev, `w` the wheel speeds (w_l, w_r).  Shared by SynthNavCarGoal, SynthNavCarCircle and the
// evaluation kernel.
__device__ __forceinline__ void osa_car_move(float (&d)[OSA_NAV_DYN], float (&w)[2], float a0_in, float a1_in,
                                             float& mx, float& my) {
  const float a0 = fminf(fmaxf(a0_in, -1.f), 1.f);
  const float a1 = fminf(fmaxf(a1_in, -1.f), 1.f);
  const float la = 0.9f * w[0], lb = 0.02f * a0;
  const float ra = 0.9f * w[1], rb = 0.02f * a1;
  w[0] = la + lb;
  w[1] = ra + rb;
  const float sum = w[0] + w[1], dif = w[1] - w[0];
  const float f2 = 0.5f * sum;
  const float t = 0.375f * dif;
  d[7] = d[6];
  osa_nav_turn_and_go(d, f2, t, mx, my);
}

// What a SynthNavGoal transition does after the robot has moved: the reward from the distance to the goal before (d0)
// and after, and a new goal when the old one is reached.
__device__ __forceinline__ void osa_nav_arrive(float (&d)[OSA_NAV_DYN], const float* __restrict__ row, int level,
                                               float d0, unsigned long long key, unsigned long long pos, int n,
                                               float& r) {
  const float d1 = osa_reach_dist(d[0], d[1], d[8], d[9]);
  const bool reached = d1 < 0.3f;
  r = (d0 - d1) + (reached ? 1.f : 0.f);
  if (reached) {
    float cand[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) cand[i] = osa_nav_uniform(key, pos, n, 14, i);
    osa_nav_pick_goal(cand, row, level, d[8], d[9]);
  }
}

// An object o seen from the state: body-frame coordinates (bx, by) of r = o - p and |r|.
__device__ __forceinline__ void osa_nav_see(const float (&d)[OSA_NAV_DYN], float ox, float oy, float& bx, float& by,
                                            float& dist) {
  const float rx = ox - d[0], ry = oy - d[1];
  const float b0 = d[2] * rx, b1 = d[3] * ry, b2 = d[2] * ry, b3 = d[3] * rx;
  bx = b0 + b1;
  by = b2 - b3;
  const float xx = rx * rx, yy = ry * ry;
  dist = sqrtf(xx + yy);
}
// Whether the body-frame direction (bx, by) lies in lidar bin k: E[k] x b >= 0 and E[k + 1] x b < 0.
__device__ __forceinline__ bool osa_nav_in_bin(int k, float bx, float by) {
  const float p0 = OSA_NAV_EDGE[k][0] * by, p1 = OSA_NAV_EDGE[k][1] * bx;
  const float p2 = OSA_NAV_EDGE[(k + 1) & 15][0] * by, p3 = OSA_NAV_EDGE[(k + 1) & 15][1] * bx;
  return p0 - p1 >= 0.f && p2 - p3 < 0.f;
}
__device__ __forceinline__ float osa_nav_reading(float dist) { return fmaxf(0.f, 1.f - dist / 3.f); }
// Whether an object of class cls (1 hazard, 2 vase) at distance dist costs: vases on level 2 only.
__device__ __forceinline__ bool osa_nav_hit(int level, int cls, float dist) {
  return (cls == 1 && dist < 0.2f) || (cls == 2 && level == 2 && dist < 0.1f);
}

// Cost of the transition that led to the state: 1 inside a hazard disc or (level 2) a vase disc.
__device__ __forceinline__ float osa_nav_cost(const float (&d)[OSA_NAV_DYN], const float* __restrict__ row, int level) {
  bool hit = false;
  const int H = osa_nav_hazards(level), V = level == 2 ? osa_nav_vases(level) : 0;
  const float *__restrict__ hz = row + OSA_NAV_HAZ, *__restrict__ vs = row + OSA_NAV_VASE;
  for (int h = 0; h < H; ++h) hit = hit || osa_nav_hit(level, 1, osa_reach_dist(d[0], d[1], hz[2 * h], hz[2 * h + 1]));
  for (int v = 0; v < V; ++v) hit = hit || osa_nav_hit(level, 2, osa_reach_dist(d[0], d[1], vs[2 * v], vs[2 * v + 1]));
  return hit ? 1.f : 0.f;
}

// Columns 0 - 11 of the observation row: 0 f, 1 f - f_prev, 2 t, 3 u_x, 4 u_y, 5 - 11 zero.
__device__ __forceinline__ float osa_nav_sensor_col(const float (&d)[OSA_NAV_DYN], int col) {
  float v = 0.f;
  if (col == 0) v = d[4];
  if (col == 1) v = d[4] - d[5];
  if (col == 2) v = d[6];
  if (col == 3) v = d[2];
  if (col == 4) v = d[3];
  return v;
}

// Lidar column b of the observation row, one lane for the whole walk: 0 - 15 goal lidar, 16 - 31 hazard lidar, 32 - 47
// vase lidar.  An object in bin k reads max(0, 1 - |r| / LIDAR_MAX) there; a bin reads the maximum over its class.
__device__ __forceinline__ float osa_nav_lidar_col(const float (&d)[OSA_NAV_DYN], const float* __restrict__ row,
                                                   int level, int b) {
  const int cls = b >> 4, k = b & 15;
  const int cnt = cls == 0 ? 1 : (cls == 1 ? osa_nav_hazards(level) : osa_nav_vases(level));
  const float* __restrict__ objs = row + (cls == 0 ? 8 : (cls == 1 ? OSA_NAV_HAZ : OSA_NAV_VASE));
  float out = 0.f;
  for (int i = 0; i < cnt; ++i) {
    const float ox = cls == 0 ? d[8] : objs[2 * i], oy = cls == 0 ? d[9] : objs[2 * i + 1];
    float bx, by, dist;
    osa_nav_see(d, ox, oy, bx, by, dist);
    if (osa_nav_in_bin(k, bx, by)) out = fmaxf(out, osa_nav_reading(dist));
  }
  return out;
}

// ------------------------------------------------------------------------------------------------
// SynthNavCircle{0,1,2}-v0: the robot of SynthNavGoal (osa_nav_move) is paid for running round the origin on the
// circle of radius 1 and charged for leaving a corridor |x| <= 0.75 (level 1) or the square |x|, |y| <= 0.75 (level 2)
// that the circle does not fit in; level 0 never costs.  State row of an env, 8 floats: the first eight of
// SynthNavGoal's row.  The callers keep it as a SynthNavGoal `d` whose goal d[8:10] is pinned at (0, 0): the 16-bin
// lidar of the circle's centre is then the goal lidar.  No objects, and nothing drawn but the four uniforms of a
// reset.  The numpy twin is tests/circle_twin.py.
// ------------------------------------------------------------------------------------------------
#define OSA_CIRCLE_KEY 0xE7037ED1A0B428DBull

// The fresh state of a reset: p = 0.4 (u0, u1) (inside every wall), heading (u2, u3) normalised, the rest 0; u0 .. u3
// reset uniforms 0 .. 3 (Philox block 1).
__device__ __forceinline__ void osa_circle_fresh(unsigned long long key, unsigned long long pos, int n,
                                                 float (&d)[OSA_NAV_DYN]) {
  float u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = osa_nav_uniform(key, pos, n, 1, i);
  d[0] = 0.4f * u[0];
  d[1] = 0.4f * u[1];
  const float xx = u[2] * u[2], yy = u[3] * u[3];
  const float nrm = sqrtf(xx + yy);
  d[2] = nrm > 0.f ? u[2] / nrm : 1.f;
  d[3] = nrm > 0.f ? u[3] / nrm : 0.f;
  d[4] = d[5] = d[6] = d[7] = d[8] = d[9] = 0.f;
}

// Reward and cost of a transition that attempted the displacement m and led to the state d.  Reward: the tangential
// part of m at the new position q, counter-clockwise positive, (m x q) / |q|, damped by 1 + ||q| - 1|.
__device__ __forceinline__ void osa_circle_pay(const float (&d)[OSA_NAV_DYN], int level, float mx, float my, float& r,
                                               float& c) {
  const float qx = d[0], qy = d[1];
  const float a = my * qx, b = mx * qy;
  const float num = a - b;
  const float xx = qx * qx, yy = qy * qy;
  const float rad = sqrtf(xx + yy);
  const float dev = fabsf(rad - 1.f);
  r = rad > 0.f ? (num / rad) / (1.f + dev) : 0.f;
  const bool out = (level >= 1 && fabsf(qx) > 0.75f) || (level == 2 && fabsf(qy) > 0.75f);
  c = out ? 1.f : 0.f;
}

// Lidar column k of the observation row, the lidar of the origin: bin k reads max(0, 1 - |p| / 3) when the origin lies
// in sector k; at p = (0, 0) no bin does.
__device__ __forceinline__ float osa_circle_lidar_col(const float (&d)[OSA_NAV_DYN], int k) {
  float bx, by, dist;
  osa_nav_see(d, 0.f, 0.f, bx, by, dist);
  return osa_nav_in_bin(k, bx, by) ? osa_nav_reading(dist) : 0.f;
}

// ------------------------------------------------------------------------------------------------
// SynthNavCarGoal{0,1,2}-v0 and SynthNavCarCircle{0,1,2}-v0: the two tasks above driven by the Car, whose two wheels
// are commanded independently (osa_car_move); everything but the motion and the sensor columns is the point task's.
// State row of a CarGoal env, 64 floats: SynthNavGoal's row with three of its zero slots in use,
//   [7] t_prev  [10] w_l  [11] w_r
// and of a CarCircle env, 12 floats: the first twelve of that row (the goal slots [8:10] stay 0: the circle's centre).
// The callers keep a SynthNavGoal `d` (d[7] = t_prev) and the wheel speeds `w`.
// A reset takes the POINT task's Philox key and draw allocation (OSA_NAV_KEY / OSA_CIRCLE_KEY, osa_nav_fresh /
// osa_circle_fresh) and starts the wheels and t_prev at 0: on purpose, so that SynthNavCarGoal<l> with seed s has the
// arena of SynthNavGoal<l> with seed s (robots compared on identical layouts, one reset in the numpy twins).
// Observation: 24 sensor columns (osa_car_sensor_col), then the task's lidars.  The numpy twin is tests/car_twin.py.
// ------------------------------------------------------------------------------------------------
#define OSA_CAR_SENSORS 24  // sensor columns of the Car
#define OSA_CAR_WHEELS 10   // column of w_l in either state row

// Sensor columns: 0 f, 1 f - f_prev, 2 t, 3 u_x, 4 u_y, 5 w_l, 6 w_r, 7 t - t_prev, 0 past them.
__device__ __forceinline__ float osa_car_sensor_col(const float (&d)[OSA_NAV_DYN], const float (&w)[2], int col) {
  float v = osa_nav_sensor_col(d, col);
  if (col == 5) v = w[0];
  if (col == 6) v = w[1];
  if (col == 7) v = d[6] - d[7];
  return v;
}

// ------------------------------------------------------------------------------------------------
// What a family IS: one description each, the only thing the per-step kernels and the evaluation kernel know of an env.
//   STATE   floats per state row                     OBS    native observation columns
//   DYN     leading state floats a transition changes ACT    least action columns
//   TRACE   state floats of an evaluator trace record LDS_ROW  whether the row's objects live in LDS (`row` below)
//   Regs    what the registers hold of a row; load / store move it from and to the row
//   fresh   the state after a reset                  advance   one transition (a Goal task leaves its cost to the
//   obs_col / state_col   one column of either row              caller's walk over the objects), transition: with it
// Everything works on env `n` at position `pos` of the Philox stream `seed` (OsaEnvAt).  The SynthNav families are a
// robot {OsaPoint, OsaCar} x a task {OsaGoal, OsaCircle}; the structs only bind the arithmetic above together.
// A new family is modelled on OsaNavEnv (or, with its state in registers and no robot, on OsaReachEnv), which have every
// member; OsaSynthEnv is the exception and no template.
// ------------------------------------------------------------------------------------------------
struct OsaEnvAt {
  unsigned long long seed, pos;
  int n, level;  // (level: the SynthNav families'; the others pass 0)
  float cost_p;  // the noise env's cost probability, its one parameter; the other families pass 0 and never read it
};

// Synth*-v0: noise, so only half a description.  It has no state (no load / store, an empty Regs and fresh), its
// observation is drawn pair-wise by the callers (osa_synth_obs_pair; no obs_col), it takes no action (transition ignores
// it) and any width will do: OBS and ACT are the least widths the entry points accept, not native ones.
struct OsaSynthEnv {
  static constexpr int STATE = 0, OBS = 1, DYN = 0, ACT = 1, TRACE = 0;
  static constexpr bool LDS_ROW = false;
  struct Regs {};
  static __device__ __forceinline__ void fresh(Regs&, const OsaEnvAt&, const float*) {}
  static __device__ __forceinline__ void transition(Regs&, const float*, const OsaEnvAt& at, float, float, float& r,
                                                    float& c) {
    uint32_t w[4];
    osa_philox(at.seed ^ OSA_SYNTH_RC_KEY, at.pos, (unsigned long long)at.n, w);
    r = osa_synth_reward(w);
    c = osa_synth_cost(w, at.cost_p);
  }
  static __device__ __forceinline__ float state_col(const Regs&, const float*, int) { return 0.f; }
};

// SynthReach-v0: the six state floats in registers (the row pads them to eight).
struct OsaReachEnv {
  static constexpr int STATE = 8, OBS = 6, DYN = 6, ACT = 2, TRACE = 6;
  static constexpr bool LDS_ROW = false;
  struct Regs {
    float s[6];
  };
  static __device__ __forceinline__ void load(Regs& s, const float* __restrict__ srow) {
#pragma unroll
    for (int k = 0; k < DYN; ++k) s.s[k] = srow[k];
  }
  static __device__ __forceinline__ void store(const Regs& s, float* __restrict__ srow) {
#pragma unroll
    for (int k = 0; k < DYN; ++k) srow[k] = s.s[k];
  }
  static __device__ __forceinline__ void fresh(Regs& s, const OsaEnvAt& at, const float*) {
    uint32_t w0[4], w1[4];
    osa_philox(at.seed ^ OSA_REACH_KEY, at.pos, ((unsigned long long)at.n << 20) + 1, w0);
    osa_philox(at.seed ^ OSA_REACH_KEY, at.pos, ((unsigned long long)at.n << 20) + 2, w1);
    osa_reach_fresh(w0, w1, s.s);
  }
  static __device__ __forceinline__ void transition(Regs& s, const float*, const OsaEnvAt& at, float a0, float a1,
                                                    float& r, float& c) {
    uint32_t w1[4];
    osa_philox(at.seed ^ OSA_REACH_KEY, at.pos, ((unsigned long long)at.n << 20) + 2, w1);
    osa_reach_transition(s.s, a0, a1, w1, r, c);
  }
  static __device__ __forceinline__ float obs_col(const Regs& s, const float*, int, int col) {
    return osa_reach_obs_col(s.s, col);
  }
  static __device__ __forceinline__ float state_col(const Regs& s, const float*, int col) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < DYN; ++k)
      if (col == k) v = s.s[k];
    return v;
  }
};

// The robots.  A robot is the registers it adds to the task's `d`: the Point none, the Car its wheel speeds.
struct OsaPoint {
  static constexpr int SENSORS = 12;  // sensor columns in front of the lidars
  static constexpr int ROW = 8;       // leading floats of the state row that are the robot's
  __device__ __forceinline__ void load(const float*) {}
  __device__ __forceinline__ void store(float*) const {}
  __device__ __forceinline__ void rest() {}
  __device__ __forceinline__ void move(float (&d)[OSA_NAV_DYN], float a0, float a1, float& mx, float& my) {
    osa_nav_move(d, a0, a1, mx, my);
  }
  __device__ __forceinline__ float sensor_col(const float (&d)[OSA_NAV_DYN], int col) const {
    return osa_nav_sensor_col(d, col);
  }
  __device__ __forceinline__ float state_col(float v, int) const { return v; }
};
struct OsaCar {
  static constexpr int SENSORS = OSA_CAR_SENSORS, ROW = OSA_CAR_WHEELS + 2;
  float w[2];  // (w_l, w_r)
  __device__ __forceinline__ void load(const float* __restrict__ row) {
    w[0] = row[OSA_CAR_WHEELS];
    w[1] = row[OSA_CAR_WHEELS + 1];
  }
  __device__ __forceinline__ void store(float* __restrict__ row) const {
    row[OSA_CAR_WHEELS] = w[0];
    row[OSA_CAR_WHEELS + 1] = w[1];
  }
  __device__ __forceinline__ void rest() { w[0] = w[1] = 0.f; }
  __device__ __forceinline__ void move(float (&d)[OSA_NAV_DYN], float a0, float a1, float& mx, float& my) {
    osa_car_move(d, w, a0, a1, mx, my);
  }
  __device__ __forceinline__ float sensor_col(const float (&d)[OSA_NAV_DYN], int col) const {
    return osa_car_sensor_col(d, w, col);
  }
  __device__ __forceinline__ float state_col(float v, int col) const {
    if (col == OSA_CAR_WHEELS) v = w[0];
    if (col == OSA_CAR_WHEELS + 1) v = w[1];
    return v;
  }
};

// The tasks.  ROW: the leading floats of the state row that the task reads into `d` (the Circle's goal stays pinned at
// the origin); LIDARS: 16-bin lidars behind the robot's sensor columns.
struct OsaGoal {
  static constexpr unsigned long long KEY = OSA_NAV_KEY;
  static constexpr int ROW = OSA_NAV_DYN, LIDARS = 3;
  static constexpr bool OBJECTS = true;  // hazards and vases in the row: 64 floats, kept in LDS
  static __device__ __forceinline__ void fresh(float (&d)[OSA_NAV_DYN], const float* __restrict__ row,
                                               const OsaEnvAt& at) {
    osa_nav_fresh(at.seed ^ KEY, at.pos, at.n, at.level, row, d);
  }
  template <class Robot>
  static __device__ __forceinline__ void advance(float (&d)[OSA_NAV_DYN], Robot& bot, const float* __restrict__ row,
                                                 const OsaEnvAt& at, float a0, float a1, float& r, float&) {
    const float d0 = osa_reach_dist(d[0], d[1], d[8], d[9]);
    float mx, my;
    bot.move(d, a0, a1, mx, my);
    osa_nav_arrive(d, row, at.level, d0, at.seed ^ KEY, at.pos, at.n, r);
  }
  static __device__ __forceinline__ float lidar_col(const float (&d)[OSA_NAV_DYN], const float* __restrict__ row,
                                                    int level, int b) {
    return osa_nav_lidar_col(d, row, level, b);
  }
};
struct OsaCircle {
  static constexpr unsigned long long KEY = OSA_CIRCLE_KEY;
  static constexpr int ROW = 8, LIDARS = 1;
  static constexpr bool OBJECTS = false;
  static __device__ __forceinline__ void fresh(float (&d)[OSA_NAV_DYN], const float*, const OsaEnvAt& at) {
    osa_circle_fresh(at.seed ^ KEY, at.pos, at.n, d);
  }
  template <class Robot>
  static __device__ __forceinline__ void advance(float (&d)[OSA_NAV_DYN], Robot& bot, const float*,
                                                 const OsaEnvAt& at, float a0, float a1, float& r, float& c) {
    float mx, my;
    bot.move(d, a0, a1, mx, my);
    osa_circle_pay(d, at.level, mx, my, r, c);
  }
  static __device__ __forceinline__ float lidar_col(const float (&d)[OSA_NAV_DYN], const float*, int, int b) {
    return osa_circle_lidar_col(d, b);
  }
};

// SynthNav{,Car}{Goal,Circle}{0,1,2}-v0.  The Car takes the POINT task's key and reset (Task::KEY, Task::fresh) and
// starts its wheels at rest.
template <class Robot, class Task>
struct OsaNavEnv {
  static constexpr int DYN = Robot::ROW > Task::ROW ? Robot::ROW : Task::ROW;
  static constexpr int STATE = Task::OBJECTS ? OSA_NAV_STATE : DYN, TRACE = STATE;
  static constexpr int SENSORS = Robot::SENSORS, OBS = SENSORS + 16 * Task::LIDARS, ACT = 2;
  static constexpr bool LDS_ROW = Task::OBJECTS;
  struct Regs {
    float d[OSA_NAV_DYN];  // a SynthNavGoal `d`, the same in every lane that works on the env
    Robot bot;
  };
  static __device__ __forceinline__ void load(Regs& s, const float* __restrict__ row) {
#pragma unroll
    for (int k = 0; k < OSA_NAV_DYN; ++k) s.d[k] = k < Task::ROW ? row[k] : 0.f;
    s.bot.load(row);
  }
  static __device__ __forceinline__ void store(const Regs& s, float* __restrict__ srow) {
#pragma unroll
    for (int k = 0; k < OSA_NAV_DYN && k < STATE; ++k) srow[k] = s.d[k];
    s.bot.store(srow);
  }
  // Column `col` (>= DYN) of a fresh row with objects; fresh() wants the fresh hazards in `row`.
  static __device__ __forceinline__ float fresh_obj(const OsaEnvAt& at, int col) {
    return osa_nav_fresh_obj(at.seed ^ Task::KEY, at.pos, at.n, at.level, col);
  }
  static __device__ __forceinline__ void fresh(Regs& s, const OsaEnvAt& at, const float* __restrict__ row) {
    Task::fresh(s.d, row, at);
    s.bot.rest();
  }
  static __device__ __forceinline__ void advance(Regs& s, const float* __restrict__ row, const OsaEnvAt& at, float a0,
                                                 float a1, float& r, float& c) {
    Task::advance(s.d, s.bot, row, at, a0, a1, r, c);
  }
  static __device__ __forceinline__ void transition(Regs& s, const float* __restrict__ row, const OsaEnvAt& at,
                                                    float a0, float a1, float& r, float& c) {
    advance(s, row, at, a0, a1, r, c);
    if (Task::OBJECTS) c = osa_nav_cost(s.d, row, at.level);
  }
  // One lane for the whole column: the robot's sensors, then the task's lidars, 0 past them.
  static __device__ __forceinline__ float obs_col(const Regs& s, const float* __restrict__ row, int level, int col) {
    if (col < SENSORS || col >= OBS) return s.bot.sensor_col(s.d, col);
    return Task::lidar_col(s.d, row, level, col - SENSORS);
  }
  static __device__ __forceinline__ float state_col(const Regs& s, const float* __restrict__ row, int col) {
    float v = 0.f;
    if (Task::OBJECTS && col >= OSA_NAV_DYN) v = row[col];
#pragma unroll
    for (int k = 0; k < OSA_NAV_DYN; ++k)
      if (col == k) v = s.d[k];
    return s.bot.state_col(v, col);
  }
};
using OsaPointGoal = OsaNavEnv<OsaPoint, OsaGoal>;
using OsaPointCircle = OsaNavEnv<OsaPoint, OsaCircle>;
using OsaCarGoal = OsaNavEnv<OsaCar, OsaGoal>;
using OsaCarCircle = OsaNavEnv<OsaCar, OsaCircle>;
static_assert(OsaPointGoal::STATE == 64 && OsaPointGoal::OBS == 60 && OsaPointGoal::DYN == 10, "SynthNavGoal");
static_assert(OsaPointCircle::STATE == 8 && OsaPointCircle::OBS == 28 && OsaPointCircle::DYN == 8, "SynthNavCircle");
static_assert(OsaCarGoal::STATE == 64 && OsaCarGoal::OBS == 72 && OsaCarGoal::DYN == 12, "SynthNavCarGoal");
static_assert(OsaCarCircle::STATE == 12 && OsaCarCircle::OBS == 40 && OsaCarCircle::DYN == 12, "SynthNavCarCircle");
#pragma clang fp contract(fast)

// How the kernels call a description's transition.  `act` is the env's unclamped action row (global memory in a
// per-step kernel, the LDS action row in the evaluation kernel).  The descriptions above take its first two columns by
// value; one with ACT > 2 states the row form instead,
//   transition(Regs&, const float* row, const OsaEnvAt&, const float* act, float& r, float& c)
// and reads act[0 .. ACT).  A description with ACT = 1 in the two-column form gets a1 = 0: the row has no second
// column, and for the last env act[1] would lie behind the caller's buffer.
template <class E, class = void>
struct OsaTakesActionRow : std::false_type {};
template <class E>
struct OsaTakesActionRow<
    E, std::void_t<decltype(E::transition(std::declval<typename E::Regs&>(), (const float*)nullptr,
                                          std::declval<const OsaEnvAt&>(), (const float*)nullptr,
                                          std::declval<float&>(), std::declval<float&>()))>> : std::true_type {};
template <class E>
__device__ __forceinline__ void osa_env_transition(typename E::Regs& s, const float* __restrict__ row,
                                                   const OsaEnvAt& at, const float* __restrict__ act, float& r,
                                                   float& c) {
  if constexpr (OsaTakesActionRow<E>::value)
    E::transition(s, row, at, act, r, c);
  else if constexpr (E::ACT >= 2)
    E::transition(s, row, at, act[0], act[1], r, c);
  else
    E::transition(s, row, at, act[0], 0.f, r, c);
}

// Whether the transition just made ends the episode of its own accord.  A description may state
//   terminal(const Regs&, const float* row, const OsaEnvAt&) -> bool
// on the post-transition state with the OsaEnvAt of that transition; one without the member (every built-in family)
// never terminates, and the answer is a compile-time false that leaves its kernels as they were.
template <class E, class = void>
struct OsaHasTerminal : std::false_type {};
template <class E>
struct OsaHasTerminal<
    E, std::void_t<decltype(static_cast<bool>(E::terminal(std::declval<const typename E::Regs&>(),
                                                          (const float*)nullptr, std::declval<const OsaEnvAt&>())))>>
    : std::true_type {};
template <class E>
__device__ __forceinline__ bool osa_env_terminal(const typename E::Regs& s, const float* __restrict__ row,
                                                 const OsaEnvAt& at) {
  if constexpr (OsaHasTerminal<E>::value)
    return E::terminal(s, row, at);
  else
    return false;
}
