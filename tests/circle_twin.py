"""Numpy twin of the SynthNavCircle{0,1,2}-v0 device envs (helper module of the tests, no tests of its own).

The specification, once: float32 everywhere, every intermediate rounded to float32, no fused multiply-adds, only
+ - * / sqrt abs min max and compares, so that this file and omnisafe_amd/csrc/env_device.h compute the same bits.

State row (N, 8): [0:2] p, [2:4] u (unit heading), [4] f (forward speed), [5] f_prev, [6] t (last turn parameter),
[7] 0.  The motion is SynthNavGoal's (tests/nav_twin.py, restated here on the 8-float row).

Random numbers: Philox4x32-10, key ``seed ^ CIRCLE_KEY``; block j of env n at stream position pos has the counter
(lo = (n << 20) + j, hi = pos).  A reset takes uniforms 0 .. 3 (block 1); transitions draw nothing.
"""
import numpy as np

from nav_twin import ARENA, BOUND, DECAY, DRIVE, TURN, lidar, philox4x32_10, u01

F = np.float32
CIRCLE_KEY = 0xE7037ED1A0B428DB
SPAWN, WALL = F(0.4), F(0.75)
OBS = 28


def draws(seed, pos, N, first_block, count):
    """nav_twin.draws under this env's key: uniforms 0 .. count-1 of every env at position pos, (N, count) float32."""
    n = np.arange(N, dtype=np.uint64)[:, None]
    j = np.uint64(first_block) + np.arange((count + 3) // 4, dtype=np.uint64)[None, :]
    w = philox4x32_10((seed ^ CIRCLE_KEY) & 0xFFFFFFFFFFFFFFFF, int(pos), (n << np.uint64(20)) + j)
    u = u01(w.reshape(N, -1)[:, :count])
    return (ARENA * (F(2) * u - F(1)).astype(np.float32)).astype(np.float32)


def circle_reset(seed, pos, N):
    """The (N, 8) state of a reset at stream position pos (the same on every level)."""
    u = draws(seed, pos, N, 1, 4)
    s = np.zeros((N, 8), np.float32)
    s[:, 0:2] = (SPAWN * u[:, 0:2]).astype(np.float32)
    hx, hy = u[:, 2], u[:, 3]
    nrm = np.sqrt(((hx * hx).astype(np.float32) + (hy * hy).astype(np.float32)).astype(np.float32), dtype=np.float32)
    pos_n = nrm > 0
    safe = np.where(pos_n, nrm, F(1))
    s[:, 2] = np.where(pos_n, hx / safe, F(1))
    s[:, 3] = np.where(pos_n, hy / safe, F(0))
    return s


def circle_step(state, action, level):
    """One transition (no truncation handling: the caller resets with circle_reset).  Returns (new state, reward,
    cost)."""
    s = np.asarray(state, np.float32).copy()
    a = np.minimum(np.maximum(np.asarray(action, np.float32), F(-1)), F(1))
    p, u, f = s[:, 0:2], s[:, 2:4], s[:, 4]
    f2 = ((DECAY * f).astype(np.float32) + (DRIVE * a[:, 0]).astype(np.float32)).astype(np.float32)
    t = (TURN * a[:, 1]).astype(np.float32)
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
    num = ((m[:, 1] * q[:, 0]).astype(np.float32) - (m[:, 0] * q[:, 1]).astype(np.float32)).astype(np.float32)
    rad = np.sqrt(((q[:, 0] * q[:, 0]).astype(np.float32) + (q[:, 1] * q[:, 1]).astype(np.float32))
                  .astype(np.float32), dtype=np.float32)
    dev = np.abs((rad - F(1)).astype(np.float32))
    on = rad > 0
    safe = np.where(on, rad, F(1))
    reward = np.where(on, ((num / safe).astype(np.float32) / (F(1) + dev).astype(np.float32)).astype(np.float32),
                      F(0)).astype(np.float32)
    out_x, out_y = np.abs(q[:, 0]) > WALL, np.abs(q[:, 1]) > WALL
    cost = {0: np.zeros_like(out_x), 1: out_x, 2: out_x | out_y}[level].astype(np.float32)
    out = s.copy()
    out[:, 0:2], out[:, 2:4], out[:, 4], out[:, 5], out[:, 6] = q, u2, f2, f, t
    return out, reward, cost


def circle_obs(state, obs_dim=OBS):
    """The (N, obs_dim) observation of a state: sensor columns, the 16-bin lidar of the origin, zeros."""
    s = np.asarray(state, np.float32)
    N = s.shape[0]
    o = np.zeros((N, obs_dim), np.float32)
    o[:, 0] = s[:, 4]
    o[:, 1] = (s[:, 4] - s[:, 5]).astype(np.float32)
    o[:, 2] = s[:, 6]
    o[:, 3:5] = s[:, 2:4]
    o[:, 12:28] = lidar(s[:, 0:2], s[:, 2:4], np.zeros((N, 1, 2), np.float32))
    return o


class CircleTwin:
    """The vector env as the device class plays it: all lanes reset together every `horizon` steps; stream position
    0 is the reset, every step takes the next one (a truncating step resets at its own position)."""

    def __init__(self, level, N, horizon, seed):
        self.level, self.N, self.horizon, self.seed = level, N, horizon, seed
        self.pos = 0
        self.since = 0
        self.state = None

    def reset(self):
        self.state = circle_reset(self.seed, self.pos, self.N)
        self.pos += 1
        self.since = 0
        return circle_obs(self.state)

    def step(self, action):
        self.state, r, c = circle_step(self.state, action, self.level)
        self.since += 1
        trunc = self.since % self.horizon == 0
        final = None
        if trunc:
            final = circle_obs(self.state)
            self.state = circle_reset(self.seed, self.pos, self.N)
        self.pos += 1
        return circle_obs(self.state), r, c, trunc, final
