// SynthNavButton{0,1,2}-v0 (Point) and SynthNavCarButton{0,1,2}-v0 (Car): an out-of-tree description with an object row
// in LDS (LDS_ROW = true), with the structure of the Safety-Gymnasium Button tasks.  The robot of SynthNavGoal drives
// to the goal button among four buttons (reward = progress, +1 on a press, which makes another button the goal) and is
// charged for pressing a wrong button, for entering a hazard disc and for coming near a "gremlin", an obstacle that
// runs round a 16-gon.  The numpy twin is tests/button_twin.py.
//
// State row of an env, 64 floats, the same for both robots:
//   [0:2] p  [2:4] u (unit heading)  [4] f  [5] f_prev  [6] t  [7] t_prev (Car; Point 0)  [8:10] g (the goal button)
//   [10] w_l  [11] w_r (Car; Point 0)  [12] k (steps of the episode)  [13] goal button index 0 .. 3
//   -- DYN = 14: the above is what a transition changes, and the Regs --
//   [14:16] 0  [16:24] buttons 4 x 2  [24:40] hazards 8 x 2  [40:58] gremlins 6 x (centre x, centre y, phase)
//   [58:64] 0
// Levels 0 / 1 / 2: 4 / 4 / 4 buttons, 0 / 4 / 8 hazards, 0 / 4 / 6 gremlins; slots past the level's counts are 0.
//
// Random numbers: key seed ^ BUTTON_KEY, the block and word allocation of osa_nav_uniform (uniform i of a reset is
// word i & 3 of block 1 + (i >> 2)): 0 .. 3 the robot's position and heading as in osa_nav_fresh, word 0 of block 2
// (& 3) the first goal button; object column c of the row is uniform c, a gremlin's phase the word itself,
// (word >> 8) & (16 S - 1).  A press takes word 0 of block 20 of the transition's position: the new goal is button
// (index + 1 + word % 3) & 3, one of the other three.
//
// A gremlin does not move in the row: with k the episode's step count, q = (phase + k) mod 16 S, e = q / S,
// f = (q mod S) / S (S = 8, exact) it stands at centre + R ((1 - f) E[e] + f E[(e + 1) & 15]), E = OSA_NAV_EDGE, every
// product and sum rounded on its own; the cost, the lidar and draw() compute that from (row, k).
//
// Transition: the robot's move, k <- k + 1, reward = (d0 - d1) + [d1 < PRESS] with d the distance to the goal button;
// cost = 1 when the new position is within PRESS of a button that is not the goal of this step, inside a hazard disc
// (HAZARD) or within GREMLIN of a gremlin at its position of the new k.  After a press the robot still stands on the
// old goal, which costs from the next step on until it has left.
// Observation: the robot's sensor columns, then four 16-bin lidars: goal button, all buttons, hazards, gremlins
// (Point 12 + 64 = 76 columns, Car 24 + 64 = 88).
#pragma once
#define BUTTON_KEY 0xC2B2AE3D27D4EB4Full
#define BUTTON_K 12        // column of the step count
#define BUTTON_GOAL 13     // column of the goal button's index
#define BUTTON_DYN 14
#define BUTTON_BUTTONS 16  // first button column
#define BUTTON_HAZ 24      // first hazard column
#define BUTTON_GREM 40     // first gremlin column
#define BUTTON_END 58      // first column behind the objects
#define BUTTON_S 8         // steps per edge of a gremlin's 16-gon

struct ButtonTask {
  static constexpr float PRESS = 0.3f, HAZARD = 0.2f, GREMLIN = 0.25f, ORBIT = 0.4f;
  static __device__ __forceinline__ int hazards(int level) { return level == 0 ? 0 : (level == 1 ? 4 : 8); }
  static __device__ __forceinline__ int gremlins(int level) { return level == 0 ? 0 : (level == 1 ? 4 : 6); }
  // word i & 3 of block first_block + (i >> 2), as osa_nav_uniform takes it
  static __device__ __forceinline__ uint32_t word(const OsaEnvAt& at, int first_block, int i) {
    uint32_t w[4];
    const unsigned long long block = (unsigned long long)(first_block + (i >> 2));
    osa_philox(at.seed ^ BUTTON_KEY, at.pos, ((unsigned long long)at.n << 20) + block, w);
    const int q = i & 3;
    return q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
  }
  static __device__ __forceinline__ float fresh_obj(const OsaEnvAt& at, int col) {
    const bool button = col >= BUTTON_BUTTONS && col < BUTTON_HAZ;
    const bool hazard = col >= BUTTON_HAZ && col < BUTTON_HAZ + 2 * hazards(at.level);
    const bool gremlin = col >= BUTTON_GREM && col < BUTTON_GREM + 3 * gremlins(at.level);
    if (gremlin && (col - BUTTON_GREM) % 3 == 2) return (float)((word(at, 1, col) >> 8) & (16 * BUTTON_S - 1));
    return (button || hazard || gremlin) ? osa_nav_uniform(at.seed ^ BUTTON_KEY, at.pos, at.n, 1, col) : 0.f;
  }
  // where gremlin i stands at step count k
  static __device__ __forceinline__ void gremlin_at(const float* __restrict__ row, float k, int i, float& x, float& y) {
    const float* __restrict__ o = row + BUTTON_GREM + 3 * i;
    const int q = ((int)o[2] + (int)k) & (16 * BUTTON_S - 1);
    const int e = q / BUTTON_S, e1 = (e + 1) & 15;
    const float f = (float)(q & (BUTTON_S - 1)) * (1.f / BUTTON_S), g = 1.f - f;
    const float ax = g * OSA_NAV_EDGE[e][0], bx = f * OSA_NAV_EDGE[e1][0];
    const float ay = g * OSA_NAV_EDGE[e][1], by = f * OSA_NAV_EDGE[e1][1];
    const float sx = ax + bx, sy = ay + by;
    const float rx = ORBIT * sx, ry = ORBIT * sy;
    x = o[0] + rx;
    y = o[1] + ry;
  }
  static __device__ __forceinline__ float cost(const float (&d)[OSA_NAV_DYN], const float* __restrict__ row, int level,
                                               float k, int goal) {
    bool hit = false;
    for (int b = 0; b < 4; ++b) {
      const float* __restrict__ o = row + BUTTON_BUTTONS + 2 * b;
      hit = hit || (b != goal && osa_reach_dist(d[0], d[1], o[0], o[1]) < PRESS);
    }
    for (int h = 0; h < hazards(level); ++h) {
      const float* __restrict__ o = row + BUTTON_HAZ + 2 * h;
      hit = hit || osa_reach_dist(d[0], d[1], o[0], o[1]) < HAZARD;
    }
    for (int i = 0; i < gremlins(level); ++i) {
      float x, y;
      gremlin_at(row, k, i, x, y);
      hit = hit || osa_reach_dist(d[0], d[1], x, y) < GREMLIN;
    }
    return hit ? 1.f : 0.f;
  }
  // lidar column b: 0 - 15 goal button (the built-in goal lidar), 16 - 31 buttons, 32 - 47 hazards, 48 - 63 gremlins
  static __device__ __forceinline__ float lidar_col(const float (&d)[OSA_NAV_DYN], const float* __restrict__ row,
                                                    int level, float k, int b) {
    const int cls = b >> 4, bin = b & 15;
    if (cls == 0) return osa_nav_lidar_col(d, row, level, b);
    const int cnt = cls == 1 ? 4 : (cls == 2 ? hazards(level) : gremlins(level));
    float out = 0.f;
    for (int i = 0; i < cnt; ++i) {
      float ox, oy;
      if (cls == 3) {
        gremlin_at(row, k, i, ox, oy);
      } else {
        const float* __restrict__ o = row + (cls == 1 ? BUTTON_BUTTONS : BUTTON_HAZ) + 2 * i;
        ox = o[0];
        oy = o[1];
      }
      float bx, by, dist;
      osa_nav_see(d, ox, oy, bx, by, dist);
      if (osa_nav_in_bin(bin, bx, by)) out = fmaxf(out, osa_nav_reading(dist));
    }
    return out;
  }
};

template <class Robot>
struct ButtonEnv {
  static constexpr int STATE = 64, DYN = BUTTON_DYN, TRACE = 64, ACT = 2, LEVELS = 2;
  static constexpr int SENSORS = Robot::SENSORS, OBS = SENSORS + 64;
  static constexpr bool LDS_ROW = true;
  struct Regs {
    float d[OSA_NAV_DYN];  // a SynthNavGoal `d`; d[8:10] is the goal button
    Robot bot;
    float k, goal;  // the episode's step count and the goal button's index, both exact small integers
  };
  static __device__ __forceinline__ void load(Regs& s, const float* __restrict__ row) {
#pragma unroll
    for (int i = 0; i < OSA_NAV_DYN; ++i) s.d[i] = row[i];
    s.bot.load(row);
    s.k = row[BUTTON_K];
    s.goal = row[BUTTON_GOAL];
  }
  static __device__ __forceinline__ void store(const Regs& s, float* __restrict__ srow) {
#pragma unroll
    for (int i = 0; i < OSA_NAV_DYN; ++i) srow[i] = s.d[i];
    srow[10] = srow[11] = 0.f;
    s.bot.store(srow);
    srow[BUTTON_K] = s.k;
    srow[BUTTON_GOAL] = s.goal;
  }
  static __device__ __forceinline__ float fresh_obj(const OsaEnvAt& at, int col) {
    return ButtonTask::fresh_obj(at, col);
  }
  // `row` holds the fresh buttons: the goal's position is read from it
  static __device__ __forceinline__ void fresh(Regs& s, const OsaEnvAt& at, const float* __restrict__ row) {
    float u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = osa_nav_uniform(at.seed ^ BUTTON_KEY, at.pos, at.n, 1, i);
    s.d[0] = u[0];
    s.d[1] = u[1];
    const float xx = u[2] * u[2], yy = u[3] * u[3];
    const float nrm = sqrtf(xx + yy);
    s.d[2] = nrm > 0.f ? u[2] / nrm : 1.f;
    s.d[3] = nrm > 0.f ? u[3] / nrm : 0.f;
    s.d[4] = s.d[5] = s.d[6] = s.d[7] = 0.f;
    const int goal = (int)(ButtonTask::word(at, 2, 0) & 3u);
    s.d[8] = row[BUTTON_BUTTONS + 2 * goal];
    s.d[9] = row[BUTTON_BUTTONS + 2 * goal + 1];
    s.bot.rest();
    s.k = 0.f;
    s.goal = (float)goal;
  }
  static __device__ __forceinline__ void transition(Regs& s, const float* __restrict__ row, const OsaEnvAt& at,
                                                    float a0, float a1, float& r, float& c) {
    const float d0 = osa_reach_dist(s.d[0], s.d[1], s.d[8], s.d[9]);
    float mx, my;
    s.bot.move(s.d, a0, a1, mx, my);
    s.k = s.k + 1.f;
    const float d1 = osa_reach_dist(s.d[0], s.d[1], s.d[8], s.d[9]);
    const bool pressed = d1 < ButtonTask::PRESS;
    r = (d0 - d1) + (pressed ? 1.f : 0.f);
    const int goal = (int)s.goal;
    c = ButtonTask::cost(s.d, row, at.level, s.k, goal);
    if (pressed) {
      const int next = (goal + 1 + (int)(ButtonTask::word(at, 20, 0) % 3u)) & 3;
      s.goal = (float)next;
      s.d[8] = row[BUTTON_BUTTONS + 2 * next];
      s.d[9] = row[BUTTON_BUTTONS + 2 * next + 1];
    }
  }
  static __device__ __forceinline__ float obs_col(const Regs& s, const float* __restrict__ row, int level, int col) {
    if (col < SENSORS || col >= OBS) return s.bot.sensor_col(s.d, col);
    return ButtonTask::lidar_col(s.d, row, level, s.k, col - SENSORS);
  }
  static __device__ __forceinline__ float state_col(const Regs& s, const float* __restrict__ row, int col) {
    float v = col >= DYN ? row[col] : 0.f;
#pragma unroll
    for (int i = 0; i < OSA_NAV_DYN; ++i)
      if (col == i) v = s.d[i];
    v = s.bot.state_col(v, col);
    if (col == BUTTON_K) v = s.k;
    if (col == BUTTON_GOAL) v = s.goal;
    return v;
  }
  // The picture: buttons (the goal in the goal colour), hazards, gremlins where they stand at rec[12], trail, robot.
  static constexpr float DRAW_VIEW = 2.25f;
  static __device__ __forceinline__ void position(const float* rec, float& x, float& y) {
    x = rec[0];
    y = rec[1];
  }
  static __device__ __forceinline__ void draw(const float* rec, const OsaDrawAt& at, OsaScene& scene) {
    const float px = rec[0], py = rec[1];
    scene.box(-2.f, -2.f, 2.f, 2.f, OSA_COLOUR_FLOOR);
    for (int h = 0; h < ButtonTask::hazards(at.level); ++h)
      scene.disc(rec[BUTTON_HAZ + 2 * h], rec[BUTTON_HAZ + 2 * h + 1], 0.04f, OSA_COLOUR_HAZARD);
    for (int b = 0; b < 4; ++b)
      scene.disc(rec[BUTTON_BUTTONS + 2 * b], rec[BUTTON_BUTTONS + 2 * b + 1], 0.01f,
                 b == (int)rec[BUTTON_GOAL] ? OSA_COLOUR_GOAL : OSA_COLOUR_VASE);
    scene.ring(rec[8], rec[9], 0.0784f, 0.09f, OSA_COLOUR_GOAL);
    for (int i = 0; i < ButtonTask::gremlins(at.level); ++i) {
      float x, y;
      ButtonTask::gremlin_at(rec, rec[BUTTON_K], i, x, y);
      scene.disc(x, y, 0.0225f, OSA_COLOUR_COST);
    }
    scene.trail(0.0004f, OSA_COLOUR_TRAIL);
    const unsigned body = Robot::SENSORS == OSA_CAR_SENSORS ? OSA_COLOUR_CAR : OSA_COLOUR_POINT;
    scene.disc(px, py, 0.01f, at.hit ? OSA_COLOUR_HIT : body);
    scene.segment(px, py, px + 0.2f * rec[2], py + 0.2f * rec[3], 0.0009f, OSA_COLOUR_HEADING);
  }
};
struct Button : ButtonEnv<OsaPoint> {};
struct CarButton : ButtonEnv<OsaCar> {};
static_assert(Button::OBS == 76 && CarButton::OBS == 88, "Button");
