"""Numpy twin of tests/custom_envs/glider.h (helper module of the tests, no tests of its own).

The twin rule of a custom device env, once: float32 everywhere, every intermediate rounded to float32, no fused
multiply-adds, only + - * / sqrt min max and compares; random numbers are Philox4x32-10 blocks keyed by
``(seed ^ KEY, pos, (n << 20) + block)``.  Then this file and the header compute the same bits.

State row (N, 12): [0:3] p, [3:6] v, [6:9] g, [9] goals reached this episode, [10:12] 0.
Blocks 1 and 2 of a position hold the six uniforms of a reset (p0 p1 p2 g0 | g1 g2), block 3 the three of a goal that
a transition redraws.
"""
import numpy as np

from nav_twin import philox4x32_10, u01

F = np.float32
KEY = 0x8F1BBCDCCA62C1D6
STATE, OBS, ACT, DYN, TRACE = 12, 70, 3, 10, 10


def _uniform(w, half):
    return (F(half) * (F(2) * u01(w) - F(1)).astype(np.float32)).astype(np.float32)


def _block(seed, pos, N, block):
    n = np.arange(N, dtype=np.uint64)
    return philox4x32_10((seed ^ KEY) & 0xFFFFFFFFFFFFFFFF, int(pos), (n << np.uint64(20)) + np.uint64(block))


def _dist(p, g):
    d = (p - g).astype(np.float32)
    xx, yy, zz = ((d[:, i] * d[:, i]).astype(np.float32) for i in range(3))
    return np.sqrt(((xx + yy).astype(np.float32) + zz).astype(np.float32), dtype=np.float32)


def glider_reset(seed, pos, N):
    w0, w1 = _block(seed, pos, N, 1), _block(seed, pos, N, 2)
    s = np.zeros((N, STATE), np.float32)
    s[:, 0:3] = _uniform(w0[:, 0:3], 1.0)
    s[:, 6] = _uniform(w0[:, 3], 1.5)
    s[:, 7:9] = _uniform(w1[:, 0:2], 1.5)
    return s


def glider_step(state, action, level, seed, pos):
    """One transition under the unclamped (N, >= 3) action; returns (state', reward, cost)."""
    s = state.copy()
    N = s.shape[0]
    d0 = _dist(s[:, 0:3], s[:, 6:9])
    a = np.minimum(np.maximum(np.asarray(action, np.float32)[:, :ACT], F(-1)), F(1))
    va, vb = (F(0.9) * s[:, 3:6]).astype(np.float32), (F(0.05) * a).astype(np.float32)
    s[:, 3:6] = (va + vb).astype(np.float32)
    s[:, 0:3] = np.minimum(np.maximum((s[:, 0:3] + s[:, 3:6]).astype(np.float32), F(-2)), F(2))
    d1 = _dist(s[:, 0:3], s[:, 6:9])
    reached = d1 < F(0.4)
    r = ((d0 - d1).astype(np.float32) + reached.astype(np.float32)).astype(np.float32)
    c = ((level >= 1) & (np.abs(s[:, 2]) > F(1))).astype(np.float32)
    g = _uniform(_block(seed, pos, N, 3)[:, 0:3], 1.5)
    s[:, 6:9] = np.where(reached[:, None], g, s[:, 6:9])
    s[:, 9] = np.where(reached, (s[:, 9] + F(1)).astype(np.float32), s[:, 9])
    return s, r, c


def glider_obs(state, obs_dim=OBS):
    """(N, obs_dim) observation rows; columns past OBS are zeros."""
    s = state
    o = np.zeros((s.shape[0], max(obs_dim, OBS)), np.float32)
    o[:, 0:6] = s[:, 0:6]
    o[:, 6:9] = (s[:, 6:9] - s[:, 0:3]).astype(np.float32)
    for col in range(9, OBS):
        j = col - 9
        k = F(0.125) * F(j + 1)
        o[:, col] = (s[:, j % 9] * (s[:, j // 9] + k).astype(np.float32)).astype(np.float32)
    return o[:, :obs_dim] if obs_dim <= OBS else o


# tests/custom_envs/slider.h: state (N, 2) = p, v; one action column; observation p, v, p * v
SLIDER_KEY = 0x2545F4914F6CDD1D


def slider_reset(seed, pos, N):
    n = np.arange(N, dtype=np.uint64)
    w = philox4x32_10((seed ^ SLIDER_KEY) & 0xFFFFFFFFFFFFFFFF, int(pos), (n << np.uint64(20)) + np.uint64(1))
    s = np.zeros((N, 2), np.float32)
    s[:, 0] = (F(2) * u01(w[:, 0]) - F(1)).astype(np.float32)
    return s


def slider_step(state, action):
    """One transition under the unclamped (N, 1) action; returns (state', reward, cost)."""
    s = state.copy()
    a = np.minimum(np.maximum(np.asarray(action, np.float32)[:, 0], F(-1)), F(1))
    keep, push = (F(0.9) * s[:, 1]).astype(np.float32), (F(0.05) * a).astype(np.float32)
    s[:, 1] = (keep + push).astype(np.float32)
    s[:, 0] = np.minimum(np.maximum((s[:, 0] + s[:, 1]).astype(np.float32), F(-2)), F(2))
    return s, s[:, 1].copy(), (np.abs(s[:, 0]) > F(1)).astype(np.float32)


def slider_obs(state):
    return np.stack([state[:, 0], state[:, 1], (state[:, 0] * state[:, 1]).astype(np.float32)], 1)


class GliderTwin:
    """The vector env as the device class plays it: all lanes reset together every `horizon` steps; stream position
    0 is the reset, every step takes the next one (a truncating step resets at its own position)."""

    def __init__(self, level, N, horizon, seed):
        self.level, self.N, self.horizon, self.seed = level, N, horizon, seed
        self.pos = 0
        self.since = 0
        self.state = None

    def reset(self):
        self.state = glider_reset(self.seed, self.pos, self.N)
        self.pos += 1
        self.since = 0
        return glider_obs(self.state)

    def step(self, action):
        self.state, r, c = glider_step(self.state, action, self.level, self.seed, self.pos)
        self.since += 1
        trunc = self.since % self.horizon == 0
        final = None
        if trunc:
            final = glider_obs(self.state)
            self.state = glider_reset(self.seed, self.pos, self.N)
        self.pos += 1
        return glider_obs(self.state), r, c, trunc, final
