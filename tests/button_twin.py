"""Numpy twins of the two example descriptions with an object row in LDS, tests/custom_envs/button.h (Button, CarButton:
SynthNavButton{0,1,2}-v0 and SynthNavCarButton{0,1,2}-v0) and tests/custom_envs/field.h (Field); helper module of the
tests, no tests of its own.

The twin rule: float32 everywhere, every intermediate rounded to float32, no fused multiply-adds,
only + - * / sqrt abs min max and compares, and every random number through Philox4x32-10 -> u01 as the device draws
it, so that this file and the headers compute the same bits.

Button.  State row (N, 64), the same for both robots:
    [0:2] p, [2:4] u, [4] f, [5] f_prev, [6] t, [7] t_prev (Car), [8:10] g (the goal button), [10] w_l, [11] w_r (Car),
    [12] k (steps of the episode), [13] goal button index, [14:16] 0, [16:24] buttons 4 x 2, [24:40] hazards 8 x 2,
    [40:58] gremlins 6 x (centre x, centre y, phase), [58:64] 0.
Levels 0 / 1 / 2: 4 buttons, 0 / 4 / 8 hazards, 0 / 4 / 6 gremlins.  Key ``seed ^ BUTTON_KEY``; word i of a reset is word
i % 4 of block 1 + i // 4 of the reset's position, uniform i = 1.5 (2 u01(word i) - 1): uniforms 0 .. 3 the robot (as
nav_twin.nav_reset), word 4 & 3 the first goal button, object column c uniform c, a gremlin's phase (word >> 8) & 127.
A press takes word 0 of block 20 of the transition's position: the new goal is button (index + 1 + word % 3) & 3.
Gremlin i at step count k: q = (phase + k) mod 128, e = q // 8, f = (q % 8) / 8, at centre + 0.4 ((1 - f) E[e] +
f E[e + 1]).  The robots move as in nav_twin / car_twin.

Field.  State row (N, 150): [0:2] p, [2:4] v, [4:150] 73 discs.  Key ``seed ^ FIELD_KEY``, the same allocation.
"""
import numpy as np

import car_twin
import nav_twin
from nav_twin import ARENA, BOUND, EDGE, dist, lidar, philox4x32_10, u01

F = np.float32
BUTTON_KEY = 0xC2B2AE3D27D4EB4F
FIELD_KEY = 0x94D049BB133111EB
K_COL, GOAL_COL, BUTTONS, HAZ, GREM = 12, 13, 16, 24, 40
LEVEL = {0: (0, 0), 1: (4, 4), 2: (8, 6)}  # hazards, gremlins
PRESS, HAZ_R, GREM_R, ORBIT = F(0.3), F(0.2), F(0.25), F(0.4)
S, PERIOD = 8, 128
OBS = {False: 76, True: 88}
SENSORS = {False: 12, True: 24}


def words(key, pos, N, first_block, count):
    """Words 0 .. count-1 of every env at position pos: (N, count) uint32."""
    n = np.arange(N, dtype=np.uint64)[:, None]
    j = np.uint64(first_block) + np.arange((count + 3) // 4, dtype=np.uint64)[None, :]
    w = philox4x32_10(key & 0xFFFFFFFFFFFFFFFF, int(pos), (n << np.uint64(20)) + j)
    return w.reshape(N, -1)[:, :count]


def uniform(w):
    return (ARENA * (F(2) * u01(w) - F(1)).astype(F)).astype(F)


def heading(hx, hy):
    nrm = np.sqrt(((hx * hx).astype(F) + (hy * hy).astype(F)).astype(F), dtype=F)
    on = nrm > 0
    safe = np.where(on, nrm, F(1))
    return np.where(on, hx / safe, F(1)).astype(F), np.where(on, hy / safe, F(0)).astype(F)


# ------------------------------------------------------------------ Button
def button_reset(seed, pos, N, level):
    """The (N, 64) state of a reset at stream position pos (either robot: the wheels start at rest)."""
    H, G = LEVEL[level]
    w = words(seed ^ BUTTON_KEY, pos, N, 1, 64)
    u = uniform(w)
    s = np.zeros((N, 64), F)
    s[:, 0:2] = u[:, 0:2]
    s[:, 2], s[:, 3] = heading(u[:, 2], u[:, 3])
    s[:, BUTTONS:HAZ] = u[:, BUTTONS:HAZ]
    s[:, HAZ:HAZ + 2 * H] = u[:, HAZ:HAZ + 2 * H]
    for i in range(G):
        c = GREM + 3 * i
        s[:, c:c + 2] = u[:, c:c + 2]
        s[:, c + 2] = ((w[:, c + 2] >> np.uint32(8)) & np.uint32(PERIOD - 1)).astype(F)
    goal = (w[:, 4] & np.uint32(3)).astype(np.int64)
    s[:, GOAL_COL] = goal.astype(F)
    s[:, 8:10] = button_at(s, goal)
    return s


def button_at(s, index):
    rows = np.arange(s.shape[0])
    return np.stack([s[rows, BUTTONS + 2 * index], s[rows, BUTTONS + 2 * index + 1]], 1)


def gremlin_at(s, k, i):
    """(N, 2): where gremlin i of every env stands at step count k (N,)."""
    c = GREM + 3 * i
    q = (s[:, c + 2].astype(np.int64) + np.asarray(k).astype(np.int64)) & (PERIOD - 1)
    e, e1 = q // S, (q // S + 1) & 15
    f = ((q & (S - 1)).astype(F) * F(1.0 / S)).astype(F)
    g = (F(1) - f).astype(F)
    out = np.empty((s.shape[0], 2), F)
    for axis in range(2):
        a, b = (g * EDGE[e, axis]).astype(F), (f * EDGE[e1, axis]).astype(F)
        out[:, axis] = (s[:, c + axis] + (ORBIT * (a + b).astype(F)).astype(F)).astype(F)
    return out


def gremlins(s, level):
    """(N, G, 2) at the rows' own step counts."""
    G = LEVEL[level][1]
    return np.stack([gremlin_at(s, s[:, K_COL], i) for i in range(G)], 1) if G else np.zeros((s.shape[0], 0, 2), F)


def point_move(s, action):
    """The point robot's motion on the leading 7 floats of a row (in place), as nav_twin.nav_step states it."""
    a = np.minimum(np.maximum(np.asarray(action, F), F(-1)), F(1))
    p, u, f = s[:, 0:2].copy(), s[:, 2:4].copy(), s[:, 4].copy()
    f2 = ((nav_twin.DECAY * f).astype(F) + (nav_twin.DRIVE * a[:, 0]).astype(F)).astype(F)
    t = (nav_twin.TURN * a[:, 1]).astype(F)
    tt = (t * t).astype(F)
    den = (F(1) + tt).astype(F)
    c = ((F(1) - tt).astype(F) / den).astype(F)
    sn = ((F(2) * t).astype(F) / den).astype(F)
    ux = ((c * u[:, 0]).astype(F) - (sn * u[:, 1]).astype(F)).astype(F)
    uy = ((sn * u[:, 0]).astype(F) + (c * u[:, 1]).astype(F)).astype(F)
    nrm = np.sqrt(((ux * ux).astype(F) + (uy * uy).astype(F)).astype(F), dtype=F)
    u2 = np.stack([ux / nrm, uy / nrm], 1).astype(F)
    q = (p + (f2[:, None] * u2).astype(F)).astype(F)
    s[:, 0:2] = np.minimum(np.maximum(q, -BOUND), BOUND)
    s[:, 2:4], s[:, 4], s[:, 5], s[:, 6] = u2, f2, f, t


def button_step(state, action, level, seed, pos, car):
    """One transition at stream position pos (no end-of-episode handling).  Returns (new state, reward, cost, events)
    with events = {'press', 'wrong', 'hazard', 'gremlin'}: bool (N,) each."""
    H, G = LEVEL[level]
    s = np.asarray(state, F).copy()
    N = s.shape[0]
    p, g = s[:, 0:2].copy(), s[:, 8:10].copy()
    goal = s[:, GOAL_COL].astype(np.int64)
    if car:
        car_twin.car_move(s, action)
    else:
        point_move(s, action)
    s[:, K_COL] = (s[:, K_COL] + F(1)).astype(F)
    q = s[:, 0:2]
    d0, d1 = dist(p, g), dist(q, g)
    press = d1 < PRESS
    reward = ((d0 - d1).astype(F) + press.astype(F)).astype(F)
    wrong, hazard, gremlin = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
    for b in range(4):
        wrong |= (goal != b) & (dist(q, s[:, BUTTONS + 2 * b:BUTTONS + 2 * b + 2]) < PRESS)
    for h in range(H):
        hazard |= dist(q, s[:, HAZ + 2 * h:HAZ + 2 * h + 2]) < HAZ_R
    for i in range(G):
        gremlin |= dist(q, gremlin_at(s, s[:, K_COL], i)) < GREM_R
    if press.any():
        w = words(seed ^ BUTTON_KEY, pos, N, 20, 1)[:, 0]
        nxt = (goal + 1 + (w % np.uint32(3)).astype(np.int64)) & 3
        s[:, GOAL_COL] = np.where(press, nxt.astype(F), s[:, GOAL_COL])
        s[:, 8:10] = np.where(press[:, None], button_at(s, nxt), g)
    cost = (wrong | hazard | gremlin).astype(F)
    return s, reward, cost, {'press': press, 'wrong': wrong, 'hazard': hazard, 'gremlin': gremlin}


def button_obs(state, level, car, obs_dim=None):
    """The (N, obs_dim) observation of a state: sensors, then the goal, button, hazard and gremlin lidars."""
    H, _ = LEVEL[level]
    s = np.asarray(state, F)
    N = s.shape[0]
    first = SENSORS[car]
    obs_dim = obs_dim or OBS[car]
    if car:
        o = car_twin.sensors(s, obs_dim)
    else:
        o = np.zeros((N, obs_dim), F)
        o[:, 0], o[:, 1], o[:, 2] = s[:, 4], (s[:, 4] - s[:, 5]).astype(F), s[:, 6]
        o[:, 3:5] = s[:, 2:4]
    p, u = s[:, 0:2], s[:, 2:4]
    o[:, first:first + 16] = lidar(p, u, s[:, 8:10].reshape(N, 1, 2))
    o[:, first + 16:first + 32] = lidar(p, u, s[:, BUTTONS:HAZ].reshape(N, 4, 2))
    o[:, first + 32:first + 48] = lidar(p, u, s[:, HAZ:HAZ + 2 * H].reshape(N, H, 2))
    o[:, first + 48:first + 64] = lidar(p, u, gremlins(s, level))
    return o


def button_controller(state, car):
    """The scripted controller: steer to the goal button.  (N, 2) float32 actions from the (N, 64) state -- forward /
    turn for the Point, left / right wheel for the Car.  (Plain float arithmetic: the actions are inputs, no twin.)"""
    s = np.asarray(state, np.float64)
    r = s[:, 8:10] - s[:, 0:2]
    bx = s[:, 2] * r[:, 0] + s[:, 3] * r[:, 1]
    by = s[:, 2] * r[:, 1] - s[:, 3] * r[:, 0]
    turn = np.clip(3.0 * by, -1.0, 1.0)
    turn = np.where((bx < 0) & (np.abs(by) < 1e-3), 1.0, turn)
    fwd = np.where(bx > 0, 1.0, 0.1)
    a = np.stack([fwd - turn, fwd + turn], 1) if car else np.stack([fwd, turn], 1)
    return a.astype(F)


BUTTON_VIEW = 2.25  # DRAW_VIEW


def button_draw(car):
    """draw() of button.h restated for tests/scene_twin.py: ``draw(rec, level, hit) -> [primitives]``."""
    def draw(rec, level, hit):
        import scene_twin as T

        C = T.COLOUR
        H, G = LEVEL[level]
        rec = np.asarray(rec, F)
        px, py = rec[0], rec[1]
        prims = [('box', -2, -2, 2, 2, C['FLOOR'])]
        prims += [('disc', rec[HAZ + 2 * h], rec[HAZ + 2 * h + 1], 0.04, C['HAZARD']) for h in range(H)]
        prims += [('disc', rec[BUTTONS + 2 * b], rec[BUTTONS + 2 * b + 1], 0.01,
                   C['GOAL'] if b == int(rec[GOAL_COL]) else C['VASE']) for b in range(4)]
        prims.append(('ring', rec[8], rec[9], 0.0784, 0.09, C['GOAL']))
        for i in range(G):
            x, y = gremlin_at(rec[None, :], rec[None, K_COL], i)[0]
            prims.append(('disc', x, y, 0.0225, C['COST']))
        tip = T.add(px, T.mul(F(0.2), rec[2])), T.add(py, T.mul(F(0.2), rec[3]))
        body = C['CAR'] if car else C['POINT']
        return prims + [('trail', 0.0004, C['TRAIL']), ('disc', px, py, 0.01, C['HIT'] if hit else body),
                        ('segment', px, py, tip[0], tip[1], 0.0009, C['HEADING'])]
    return draw


def button_position(rec):
    return rec[0], rec[1]


# ------------------------------------------------------------------ Field
FIELD_STATE, FIELD_OBS, FIELD_DISCS = 150, 20, 73
FIELD_R, FIELD_WALL = F(0.15), F(2.0)


def field_reset(seed, pos, N, level=0):
    u = uniform(words(seed ^ FIELD_KEY, pos, N, 1, FIELD_STATE))
    s = np.zeros((N, FIELD_STATE), F)
    s[:, 0:2] = (F(0.5) * u[:, 0:2]).astype(F)
    s[:, 4:] = u[:, 4:]
    return s


def field_step(state, action):
    """One transition (no end-of-episode handling).  Returns (new state, reward, cost, terminal)."""
    s = np.asarray(state, F).copy()
    a = np.minimum(np.maximum(np.asarray(action, F), F(-1)), F(1))
    v = ((F(0.9) * s[:, 2:4]).astype(F) + (F(0.05) * a[:, 0:2]).astype(F)).astype(F)
    x0 = s[:, 0].copy()
    s[:, 2:4] = v
    s[:, 0:2] = (s[:, 0:2] + v).astype(F)
    reward = (s[:, 0] - x0).astype(F)
    hit = np.zeros(s.shape[0], bool)
    for i in range(FIELD_DISCS):
        hit |= dist(s[:, 0:2], s[:, 4 + 2 * i:6 + 2 * i]) < FIELD_R
    terminal = (np.abs(s[:, 0]) > FIELD_WALL) | (np.abs(s[:, 1]) > FIELD_WALL)
    return s, reward, hit.astype(F), terminal


def field_obs(state, level=0, obs_dim=FIELD_OBS):
    s = np.asarray(state, F)
    N = s.shape[0]
    o = np.zeros((N, obs_dim), F)
    o[:, 0:4] = s[:, 0:4]
    east = np.tile(np.array([[1, 0]], F), (N, 1))  # (no heading: the world frame is the body frame)
    o[:, 4:20] = lidar(s[:, 0:2], east, s[:, 4:].reshape(N, FIELD_DISCS, 2))
    return o


def field_controller(N, t):
    """The scripted actions of step t: env n pushes along the direction n, every third env only weakly (it truncates
    before it leaves the arena), the others hard enough to terminate on different steps."""
    n = np.arange(N)
    amp = np.where(n % 3 == 2, 0.05, 0.4 + 0.6 * ((n * 7 + 3) % 5) / 4.0)
    return np.stack([amp * np.cos(n + 0.1 * t), amp * np.sin(n + 0.1 * t)], 1).astype(F)


# ------------------------------------------------------------------ the vector envs as the device classes play them
class RowTwin:
    """N envs under the per-env protocol of the per-step kernels: stream position 0 is the reset, every step takes the
    next one; an env that terminates or reaches `horizon` steps is reset at the step's own position (termination wins
    over the time limit; final_obs only for a truncating env)."""

    def __init__(self, kind, level, N, horizon, seed):
        """kind: 'point' | 'car' (Button) | 'field'."""
        self.kind, self.level, self.N, self.horizon, self.seed = kind, level, N, horizon, seed
        self.pos = 0
        self.steps = np.zeros(N, np.int64)
        self.state = None
        self.events = None

    def _reset(self, pos):
        if self.kind == 'field':
            return field_reset(self.seed, pos, self.N)
        return button_reset(self.seed, pos, self.N, self.level)

    def obs(self, state=None):
        state = self.state if state is None else state
        if self.kind == 'field':
            return field_obs(state)
        return button_obs(state, self.level, self.kind == 'car')

    def controller(self, t):
        if self.kind == 'field':
            return field_controller(self.N, t)
        return button_controller(self.state, self.kind == 'car')

    def reset(self):
        self.state = self._reset(self.pos)
        self.pos += 1
        self.steps[:] = 0
        return self.obs()

    def step(self, action):
        """Returns (obs, reward, cost, terminated, truncated, final_obs): final_obs (N, OBS) with the rows of the
        truncating envs filled (the others zero)."""
        if self.kind == 'field':
            self.state, r, c, term = field_step(self.state, action)
            self.events = {'terminal': term}
        else:
            self.state, r, c, self.events = button_step(self.state, action, self.level, self.seed, self.pos,
                                                        self.kind == 'car')
            term = np.zeros(self.N, bool)
        self.steps += 1
        trunc = (self.steps >= self.horizon) & ~term
        final = np.where(trunc[:, None], self.obs(), F(0)).astype(F)
        end = term | trunc
        if end.any():
            self.state = np.where(end[:, None], self._reset(self.pos), self.state)
            self.steps[end] = 0
        self.pos += 1
        return self.obs(), r, c, term, trunc, final


# What the scripted runs must show (tests/test_button_twin.py asserts it on the twin alone; the GPU tests replay the same
# runs): seed, envs, horizon and steps per robot and level, chosen so that every event of the level happens.
SCRIPT_SEED, SCRIPT_N, SCRIPT_HORIZON, SCRIPT_STEPS = 11, 130, 40, 90
FIELD_SEED, FIELD_N, FIELD_HORIZON, FIELD_STEPS = 5, 5, 12, 40
