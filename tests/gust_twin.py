"""Numpy twin of tests/custom_envs/gust.h (helper module of the tests, no tests of its own), under the twin rule of
custom_env_twin.py: float32 everywhere, every intermediate rounded to float32, no fused multiply-adds; random numbers
are Philox4x32-10 blocks keyed by ``(seed ^ KEY, pos, (n << 20) + block)``.  It restates the kernels' parameter draw as
well (include/omnisafe_amd_env.h, PARAMETERS): ``param_draw``.

State row (N, 6): [0:2] p, [2:4] v, [4:6] goal.  Parameter row (N, 4): wind, drag, band, reach.
Block 1 of a position holds the two uniforms of a reset (p_y, goal_y), block 2 the uniform of a transition's gust.
"""
import numpy as np

from nav_twin import philox4x32_10, u01
from scene_twin import COLOUR

F = np.float32
KEY = 0x5851F42D4C957F2D
PARAM_KEY = 0x8CB92BA72F3D8DD7  # OSA_PARAM_KEY
STATE, OBS, ACT, DYN, TRACE, P = 6, 8, 2, 4, 6, 4
NAMES = ('wind', 'drag', 'band', 'reach')
DEFAULT = np.array([0.2, 0.25, 0.6, 0.2], np.float32)
VIEW, TRACK = 2.5, 1.0
MASK = 0xFFFFFFFFFFFFFFFF


def ranges(**cfgs):
    """The (2, P) ranges of ``make(..., **cfgs)``: a number fixes, a pair is (lo, hi), an absent key is the default."""
    out = np.stack([DEFAULT, DEFAULT]).copy()
    for name, v in cfgs.items():
        out[:, NAMES.index(name)] = v if isinstance(v, (tuple, list)) else (v, v)
    return out.astype(np.float32)


def param_draw(rng, seed, pos, n):
    """The rows of the envs ``n`` for the episodes that a reset at position ``pos`` starts: parameter k is word k & 3
    of block k >> 2 under the key seed ^ PARAM_KEY, and v = min(lo + (hi - lo) * u, hi)."""
    rng = np.asarray(rng, np.float32)
    n = np.asarray(n, dtype=np.uint64)
    count = rng.shape[1]
    out = np.empty((len(n), count), np.float32)
    for b in range((count + 3) // 4):
        w = philox4x32_10((seed ^ PARAM_KEY) & MASK, int(pos), (n << np.uint64(20)) + np.uint64(b))
        for i in range(4):
            k = 4 * b + i
            if k < count:
                lo, hi = rng[0, k], rng[1, k]
                span = F(hi - lo)
                add = (span * u01(w[:, i])).astype(np.float32)
                out[:, k] = np.minimum((lo + add).astype(np.float32), hi)
    return out


def _uniform(w, half):
    return (F(half) * (F(2) * u01(w) - F(1)).astype(np.float32)).astype(np.float32)


def _block(seed, pos, n, block):
    n = np.asarray(n, dtype=np.uint64)
    return philox4x32_10((seed ^ KEY) & MASK, int(pos), (n << np.uint64(20)) + np.uint64(block))


def dist2(s):
    dx, dy = (s[:, 4] - s[:, 0]).astype(np.float32), (s[:, 5] - s[:, 1]).astype(np.float32)
    return ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)


def gust_reset(par, seed, pos, n):
    """Fresh rows of the envs ``n`` at position ``pos`` under their parameter rows ``par``."""
    n = np.asarray(n)
    w = _block(seed, pos, n, 1)
    s = np.zeros((len(n), STATE), np.float32)
    s[:, 1] = _uniform(w[:, 0], 0.3)
    s[:, 4] = (F(1) + (F(2) * par[:, 3]).astype(np.float32)).astype(np.float32)
    s[:, 5] = _uniform(w[:, 1], 0.5)
    return s


def gust_step(state, par, action, seed, pos, n=None):
    """One transition under the unclamped (N, >= 2) action; returns (state', reward, cost)."""
    s = state.copy()
    n = np.arange(s.shape[0]) if n is None else np.asarray(n)
    a = np.minimum(np.maximum(np.asarray(action, np.float32)[:, :ACT], F(-1)), F(1))
    keep = (F(1) - par[:, 1]).astype(np.float32)
    va, vb = (keep[:, None] * s[:, 2:4]).astype(np.float32), (F(0.2) * a).astype(np.float32)
    s[:, 2:4] = (va + vb).astype(np.float32)
    gust = (F(0.05) + _uniform(_block(seed, pos, n, 2)[:, 0], 0.05)).astype(np.float32)
    push = (par[:, 0] * gust).astype(np.float32)
    s[:, 3] = (s[:, 3] + push).astype(np.float32)
    before = dist2(s)
    s[:, 0:2] = (s[:, 0:2] + s[:, 2:4]).astype(np.float32)
    r = (before - dist2(s)).astype(np.float32)
    c = (np.abs(s[:, 1]) > par[:, 2]).astype(np.float32)
    return s, r, c


def gust_terminal(state, par):
    return dist2(state) <= (par[:, 3] * par[:, 3]).astype(np.float32)


def gust_obs(state, par, obs_dim=OBS):
    """(N, obs_dim) observation rows; columns past OBS are zeros."""
    s = state
    o = np.zeros((s.shape[0], max(obs_dim, OBS)), np.float32)
    o[:, 0:4] = s[:, 0:4]
    o[:, 4:6] = (s[:, 4:6] - s[:, 0:2]).astype(np.float32)
    o[:, 6] = par[:, 2]
    o[:, 7] = (par[:, 2] - np.abs(s[:, 1])).astype(np.float32)
    return o[:, :obs_dim] if obs_dim <= OBS else o


def steer(state, noise):
    """Actions that fly at the goal (so that episodes end by arriving), plus the caller's noise: a function of the
    twin's state, handed to the device as it is."""
    return (F(3) * (state[:, 4:6] - state[:, 0:2]) - state[:, 2:4] + noise).astype(np.float32)


class GustTwin:
    """The vector env as the device plays it: every env counts its own steps, terminates where gust_terminal says so
    (``terminates=False`` is GustEndless), truncates at `horizon` otherwise, and either end -- like the common reset at
    position 0 -- redraws the env's parameter row from ``ranges`` at that position and then resets the env under the
    new row.  ``rng`` may be rewritten between steps (set_param)."""

    def __init__(self, rng, N, horizon, seed, terminates=True):
        self.rng, self.N, self.horizon, self.seed = np.array(rng, np.float32), N, horizon, seed
        self.terminates = terminates
        self.pos = 0
        self.steps = np.zeros(N, np.int32)
        self.state = self.par = None

    def reset(self):
        n = np.arange(self.N)
        self.par = param_draw(self.rng, self.seed, self.pos, n)
        self.state = gust_reset(self.par, self.seed, self.pos, n)
        self.pos += 1
        self.steps[:] = 0
        return gust_obs(self.state, self.par)

    def step(self, action):
        """Returns (obs, reward, cost, terminated, truncated, final): `final` holds the pre-reset observation -- under
        the ended episode's parameters -- in the rows of the truncating envs and NaN elsewhere."""
        n = np.arange(self.N)
        self.state, r, c = gust_step(self.state, self.par, action, self.seed, self.pos)
        count = self.steps + 1
        term = gust_terminal(self.state, self.par) if self.terminates else np.zeros(self.N, bool)
        trunc = ~term & (count >= self.horizon)
        final = np.full((self.N, OBS), np.nan, np.float32)
        final[trunc] = gust_obs(self.state, self.par)[trunc]
        ended = term | trunc
        self.par[ended] = param_draw(self.rng, self.seed, self.pos, n)[ended]
        self.state[ended] = gust_reset(self.par, self.seed, self.pos, n)[ended]
        self.steps = np.where(ended, 0, count).astype(np.int32)
        self.pos += 1
        return gust_obs(self.state, self.par), r, c, term, trunc, final


def position(rec):
    return rec[0], rec[1]


def gust_draw(par):
    """draw() of gust.h for an episode with the parameter row ``par``, as scene_twin.render takes it."""
    band, reach = F(par[2]), F(par[3])

    def draw(rec, level, hit):
        C = COLOUR
        return [('box', -0.5, -2, 2.4, 2, C['COST']), ('box', -0.5, -band, 2.4, band, C['FLOOR']),
                ('disc', rec[4], rec[5], (reach * reach).astype(np.float32), C['GOAL']), ('trail', 0.0009, C['TRAIL']),
                ('disc', rec[0], rec[1], 0.01, C['HIT'] if hit else C['POINT'])]
    return draw
