"""Numpy twin of tests/custom_envs/ledge.h (helper module of the tests, no tests of its own), under the twin rule of
custom_env_twin.py: float32 everywhere, every intermediate rounded to float32, no fused multiply-adds; random numbers
are Philox4x32-10 blocks keyed by ``(seed ^ KEY, pos, (n << 20) + block)``.

State row (N, 6): [0:2] p, [2:4] v, [4] steps of this episode (as a float), [5] 0.
Block 1 of a position holds the uniform of a reset (p_y), block 2 the uniform of a transition's gust.
"""
import numpy as np

from nav_twin import philox4x32_10, u01

F = np.float32
KEY = 0x3C6EF372FE94F82B
STATE, OBS, ACT, DYN, TRACE = 6, 20, 2, 5, 5


def _uniform(w, half):
    return (F(half) * (F(2) * u01(w) - F(1)).astype(np.float32)).astype(np.float32)


def _block(seed, pos, n, block):
    n = np.asarray(n, dtype=np.uint64)
    return philox4x32_10((seed ^ KEY) & 0xFFFFFFFFFFFFFFFF, int(pos), (n << np.uint64(20)) + np.uint64(block))


def ledge_reset(seed, pos, N, n=None):
    """Fresh rows of the envs ``n`` (default 0 .. N - 1) at position ``pos``."""
    n = np.arange(N) if n is None else np.asarray(n)
    s = np.zeros((len(n), STATE), np.float32)
    s[:, 1] = _uniform(_block(seed, pos, n, 1)[:, 0], 0.4)
    return s


def ledge_step(state, action, level, seed, pos, n=None):
    """One transition under the unclamped (N, >= 2) action; returns (state', reward, cost).  ``n``: the env indices of
    the rows (default 0 .. N - 1)."""
    s = state.copy()
    n = np.arange(s.shape[0]) if n is None else np.asarray(n)
    a = np.minimum(np.maximum(np.asarray(action, np.float32)[:, :ACT], F(-1)), F(1))
    va, vb = (F(0.9) * s[:, 2:4]).astype(np.float32), (F(0.05) * a).astype(np.float32)
    s[:, 2:4] = (va + vb).astype(np.float32)
    s[:, 3] = (s[:, 3] + _uniform(_block(seed, pos, n, 2)[:, 0], 0.04)).astype(np.float32)
    s[:, 0:2] = (s[:, 0:2] + s[:, 2:4]).astype(np.float32)
    s[:, 4] = (s[:, 4] + F(1)).astype(np.float32)
    r = (s[:, 2] + (s[:, 0] > F(3)).astype(np.float32)).astype(np.float32)
    c = ((level >= 1) & (np.abs(s[:, 1]) > F(0.5))).astype(np.float32)
    return s, r, c


def ledge_terminal(state):
    return (np.abs(state[:, 1]) > F(1)) | (state[:, 0] > F(3))


def ledge_obs(state, obs_dim=OBS):
    """(N, obs_dim) observation rows; columns past OBS are zeros."""
    s = state
    o = np.zeros((s.shape[0], max(obs_dim, OBS)), np.float32)
    o[:, 0:4] = s[:, 0:4]
    o[:, 4] = (F(1) - np.abs(s[:, 1])).astype(np.float32)
    for col in range(5, OBS):
        j = col - 5
        k = F(0.125) * F(j + 1)
        o[:, col] = (s[:, j % 5] * (s[:, j // 5] + k).astype(np.float32)).astype(np.float32)
    return o[:, :obs_dim] if obs_dim <= OBS else o


# The trace the GPU test plays (test_custom_env_termination_gpu.py) and whose mix of episode ends test_ledge_twin.py
# establishes from the twin alone: this seed, horizon 12, 48 steps, actions uniform in [-1.5, 1.5].
TRACE_SEED, TRACE_HORIZON, TRACE_STEPS = 5, 12, 48


def trace_actions(N, steps=TRACE_STEPS):
    """(steps, N, 2) float32 actions, uniform in [-1.5, 1.5]: a third of the components is clipped at either bound."""
    return np.random.default_rng(N).uniform(-1.5, 1.5, (steps, N, ACT)).astype(np.float32)


def mixed_groups(term, trunc, group):
    """How many groups of `group` consecutive envs (the envs of one workgroup of the per-step kernel at 64 / group
    lanes) end differently on this step: a terminating, a truncating and (group 4 only) a continuing env."""
    n = 0
    for g in range(0, len(term), group):
        te, tr = term[g:g + group], trunc[g:g + group]
        n += bool(te.any() and tr.any() and (group < 4 or (~(te | tr)).any()))
    return n


class LedgeTwin:
    """The vector env as the device plays it.  Every env counts its own steps: it terminates where ledge_terminal says
    so (never truncating on the same step), truncates when its count reaches `horizon` otherwise, and either end
    resets it at the position of that step.  Stream position 0 is the common reset, every step takes the next one.
    ``terminates=False`` is LedgeEndless."""

    def __init__(self, level, N, horizon, seed, terminates=True):
        self.level, self.N, self.horizon, self.seed, self.terminates = level, N, horizon, seed, terminates
        self.pos = 0
        self.steps = np.zeros(N, np.int32)
        self.state = None

    def reset(self):
        self.state = ledge_reset(self.seed, self.pos, self.N)
        self.pos += 1
        self.steps[:] = 0
        return ledge_obs(self.state)

    def step(self, action):
        """Returns (obs, reward, cost, terminated, truncated, final): `final` holds the pre-reset observation in the
        rows of the truncating envs and NaN elsewhere (rows the device does not write)."""
        self.state, r, c = ledge_step(self.state, action, self.level, self.seed, self.pos)
        count = self.steps + 1
        term = ledge_terminal(self.state) if self.terminates else np.zeros(self.N, bool)
        trunc = ~term & (count >= self.horizon)
        final = np.full((self.N, OBS), np.nan, np.float32)
        final[trunc] = ledge_obs(self.state)[trunc]
        ended = term | trunc
        self.state[ended] = ledge_reset(self.seed, self.pos, self.N)[ended]
        self.steps = np.where(ended, 0, count).astype(np.int32)
        self.pos += 1
        return ledge_obs(self.state), r, c, term, trunc, final
