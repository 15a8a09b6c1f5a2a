"""Numpy twin of the SynthNavCarGoal{0,1,2}-v0 and SynthNavCarCircle{0,1,2}-v0 device envs (helper module of the
tests, no tests of its own).

The specification, once: float32 everywhere, every intermediate rounded to float32, no fused multiply-adds, only
+ - * / sqrt abs min max and compares, so that this file and omnisafe_amd/csrc/env_device.h compute the same bits.

The Car has two independently driven wheels.  Under a = clip(action, -1, 1), a0 the left and a1 the right wheel:

    w_l <- 0.9 w_l + 0.02 a0,  w_r <- 0.9 w_r + 0.02 a1      (two products, one sum, each rounded)
    f   <- 0.5 (w_l + w_r)                                     (sum first)
    t   <- 0.375 (w_r - w_l)                                   (difference first)

and from there the point robot's motion (tests/nav_twin.py, from ``tt = t * t`` on): the heading turned by the
rational rotation of parameter t and renormalised, p <- clip(p + f u, -2, 2), m = f u the attempted displacement.
Everything else of a task is the point task's: nav_twin's reward, goal resampling, hazards, vases and costs,
circle_twin's reward and corridor cost.

State row, CarGoal (N, 64): SynthNavGoal's row with three of its zero slots in use,
    [0:2] p, [2:4] u, [4] f, [5] f_prev, [6] t, [7] t_prev, [8:10] g, [10] w_l, [11] w_r, [12:32] hazards 10 x 2,
    [32:52] vases 10 x 2, [52:64] 0.
State row, CarCircle (N, 12): the first twelve of that row; [8:10] stay 0 (the circle's centre, the lidar's object).

Reset: the POINT task's, under the point task's Philox key and draw allocation (nav_twin.nav_reset /
circle_twin.circle_reset), with the wheels and t_prev at 0.  Deliberate: SynthNavCarGoal<l> with seed s has the arena
of SynthNavGoal<l> with seed s, so robots can be compared on identical layouts.

Observation: 24 sensor columns -- 0 f, 1 f - f_prev, 2 t, 3:5 u, 5 w_l, 6 w_r, 7 t - t_prev, 8 .. 23 zero -- then the
task's lidars: CarGoal 24:40 goal, 40:56 hazards, 56:72 vases (72 columns); CarCircle 24:40 the origin (40 columns).
"""
import numpy as np

import circle_twin
import nav_twin
from nav_twin import BOUND, HAZ, LEVEL, VASE, dist, draws, lidar, pick_goal

F = np.float32
DECAY, DRIVE, STEER = F(0.9), F(0.02), F(0.375)
GOAL_OBS, CIRCLE_OBS, SENSORS = 72, 40, 24
T_PREV, W_L, W_R = 7, 10, 11


def car_move(s, action):
    """The motion on the leading 12 floats of either state row (in place).  Returns the attempted displacement m."""
    a = np.minimum(np.maximum(np.asarray(action, np.float32), F(-1)), F(1))
    p, u = s[:, 0:2].copy(), s[:, 2:4].copy()
    wl = ((DECAY * s[:, W_L]).astype(np.float32) + (DRIVE * a[:, 0]).astype(np.float32)).astype(np.float32)
    wr = ((DECAY * s[:, W_R]).astype(np.float32) + (DRIVE * a[:, 1]).astype(np.float32)).astype(np.float32)
    f2 = (F(0.5) * (wl + wr).astype(np.float32)).astype(np.float32)
    t = (STEER * (wr - wl).astype(np.float32)).astype(np.float32)
    tt = (t * t).astype(np.float32)
    den = (F(1) + tt).astype(np.float32)
    c = ((F(1) - tt).astype(np.float32) / den).astype(np.float32)
    sn = ((F(2) * t).astype(np.float32) / den).astype(np.float32)
    ux = ((c * u[:, 0]).astype(np.float32) - (sn * u[:, 1]).astype(np.float32)).astype(np.float32)
    uy = ((sn * u[:, 0]).astype(np.float32) + (c * u[:, 1]).astype(np.float32)).astype(np.float32)
    nrm = np.sqrt(((ux * ux).astype(np.float32) + (uy * uy).astype(np.float32)).astype(np.float32), dtype=np.float32)
    u2 = np.stack([ux / nrm, uy / nrm], 1).astype(np.float32)
    m = (f2[:, None] * u2).astype(np.float32)
    q = (p + m).astype(np.float32)
    q = np.minimum(np.maximum(q, -BOUND), BOUND)
    f_prev, t_prev = s[:, 4].copy(), s[:, 6].copy()
    s[:, 0:2], s[:, 2:4], s[:, 4], s[:, 5], s[:, 6], s[:, T_PREV] = q, u2, f2, f_prev, t, t_prev
    s[:, W_L], s[:, W_R] = wl, wr
    return m


def sensors(s, obs_dim):
    o = np.zeros((s.shape[0], obs_dim), np.float32)
    o[:, 0] = s[:, 4]
    o[:, 1] = (s[:, 4] - s[:, 5]).astype(np.float32)
    o[:, 2] = s[:, 6]
    o[:, 3:5] = s[:, 2:4]
    o[:, 5], o[:, 6] = s[:, W_L], s[:, W_R]
    o[:, 7] = (s[:, 6] - s[:, T_PREV]).astype(np.float32)
    return o


# ------------------------------------------------------------------ CarGoal
def car_goal_reset(seed, pos, N, level):
    """The (N, 64) state of a reset at stream position pos: the point task's (same key, same draws), wheels at rest."""
    return nav_twin.nav_reset(seed, pos, N, level)


def car_goal_step(state, action, level, seed, pos):
    """One transition at stream position pos (no truncation handling).  Returns (new state, reward, cost, reached)."""
    H, V, vase_costs = LEVEL[level]
    s = np.asarray(state, np.float32).copy()
    N = s.shape[0]
    p, g = s[:, 0:2].copy(), s[:, 8:10].copy()
    car_move(s, action)
    q = s[:, 0:2]
    d0, d1 = dist(p, g), dist(q, g)
    reached = d1 < nav_twin.GOAL_R
    reward = ((d0 - d1).astype(np.float32) + reached.astype(np.float32)).astype(np.float32)
    hit = np.zeros(N, bool)
    for h in range(H):
        hit |= dist(q, s[:, HAZ + 2 * h:HAZ + 2 * h + 2]) < nav_twin.HAZ_R
    if vase_costs:
        for v in range(V):
            hit |= dist(q, s[:, VASE + 2 * v:VASE + 2 * v + 2]) < nav_twin.VASE_R
    if reached.any():
        cands = draws(seed, pos, N, 14, 8).reshape(N, 4, 2)
        ng = pick_goal(cands, s[:, HAZ:HAZ + 2 * H].reshape(N, H, 2))
        s[:, 8:10] = np.where(reached[:, None], ng, g)
    return s, reward, hit.astype(np.float32), reached


def car_goal_obs(state, level, obs_dim=GOAL_OBS):
    """The (N, obs_dim) observation of a state."""
    H, V, _ = LEVEL[level]
    s = np.asarray(state, np.float32)
    N = s.shape[0]
    o = sensors(s, obs_dim)
    p, u = s[:, 0:2], s[:, 2:4]
    o[:, 24:40] = lidar(p, u, s[:, 8:10].reshape(N, 1, 2))
    o[:, 40:56] = lidar(p, u, s[:, HAZ:HAZ + 2 * H].reshape(N, H, 2))
    o[:, 56:72] = lidar(p, u, s[:, VASE:VASE + 2 * V].reshape(N, V, 2))
    return o


# ------------------------------------------------------------------ CarCircle
def car_circle_reset(seed, pos, N):
    """The (N, 12) state of a reset at stream position pos: the point task's 8 floats, the rest 0."""
    s = np.zeros((N, 12), np.float32)
    s[:, :8] = circle_twin.circle_reset(seed, pos, N)
    return s


def car_circle_step(state, action, level):
    """One transition (no truncation handling).  Returns (new state, reward, cost): circle_twin's reward and cost of
    the attempted displacement m and the new position q."""
    s = np.asarray(state, np.float32).copy()
    m = car_move(s, action)
    q = s[:, 0:2]
    num = ((m[:, 1] * q[:, 0]).astype(np.float32) - (m[:, 0] * q[:, 1]).astype(np.float32)).astype(np.float32)
    rad = np.sqrt(((q[:, 0] * q[:, 0]).astype(np.float32) + (q[:, 1] * q[:, 1]).astype(np.float32))
                  .astype(np.float32), dtype=np.float32)
    dev = np.abs((rad - F(1)).astype(np.float32))
    on = rad > 0
    safe = np.where(on, rad, F(1))
    reward = np.where(on, ((num / safe).astype(np.float32) / (F(1) + dev).astype(np.float32)).astype(np.float32),
                      F(0)).astype(np.float32)
    out_x, out_y = np.abs(q[:, 0]) > circle_twin.WALL, np.abs(q[:, 1]) > circle_twin.WALL
    cost = {0: np.zeros_like(out_x), 1: out_x, 2: out_x | out_y}[level].astype(np.float32)
    return s, reward, cost


def car_circle_obs(state, obs_dim=CIRCLE_OBS):
    """The (N, obs_dim) observation of a state."""
    s = np.asarray(state, np.float32)
    o = sensors(s, obs_dim)
    o[:, 24:40] = lidar(s[:, 0:2], s[:, 2:4], np.zeros((s.shape[0], 1, 2), np.float32))
    return o


# ------------------------------------------------------------------ the vector envs as the device classes play them
class CarGoalTwin:
    """All lanes reset together every `horizon` steps; stream position 0 is the reset, every step takes the next one
    (a truncating step resets at its own position)."""

    def __init__(self, level, N, horizon, seed):
        self.level, self.N, self.horizon, self.seed = level, N, horizon, seed
        self.pos = 0
        self.since = 0
        self.state = None

    def reset(self):
        self.state = car_goal_reset(self.seed, self.pos, self.N, self.level)
        self.pos += 1
        self.since = 0
        return car_goal_obs(self.state, self.level)

    def step(self, action):
        self.state, r, c, reached = car_goal_step(self.state, action, self.level, self.seed, self.pos)
        self.since += 1
        trunc = self.since % self.horizon == 0
        final = None
        if trunc:
            final = car_goal_obs(self.state, self.level)
            self.state = car_goal_reset(self.seed, self.pos, self.N, self.level)
        self.pos += 1
        return car_goal_obs(self.state, self.level), r, c, trunc, final, reached


class CarCircleTwin:
    """As CarGoalTwin."""

    def __init__(self, level, N, horizon, seed):
        self.level, self.N, self.horizon, self.seed = level, N, horizon, seed
        self.pos = 0
        self.since = 0
        self.state = None

    def reset(self):
        self.state = car_circle_reset(self.seed, self.pos, self.N)
        self.pos += 1
        self.since = 0
        return car_circle_obs(self.state)

    def step(self, action):
        self.state, r, c = car_circle_step(self.state, action, self.level)
        self.since += 1
        trunc = self.since % self.horizon == 0
        final = None
        if trunc:
            final = car_circle_obs(self.state)
            self.state = car_circle_reset(self.seed, self.pos, self.N)
        self.pos += 1
        return car_circle_obs(self.state), r, c, trunc, final
