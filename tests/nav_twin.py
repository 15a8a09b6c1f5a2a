"""Numpy twin of the SynthNavGoal{0,1,2}-v0 device envs (helper module of the tests, no tests of its own).

The specification, once: float32 everywhere, every intermediate rounded to float32, no fused multiply-adds, only
+ - * / sqrt min max and compares, so that this file and omnisafe_amd/csrc/env_device.h compute the same bits.

State row (N, 64): [0:2] p, [2:4] u (unit heading), [4] f (forward speed), [5] f_prev, [6] t (last turn parameter),
[7] 0, [8:10] g, [10:12] 0, [12:32] hazards 10 x 2, [32:52] vases 10 x 2, [52:64] 0.

Random numbers: Philox4x32-10, key ``seed ^ NAV_KEY``; block j of env n at stream position pos has the counter
(lo = (n << 20) + j, hi = pos).  Reset uniform i is word i % 4 of block 1 + i // 4; the eight goal-candidate uniforms
of a transition are the words of blocks 14 and 15 of the transition's position.
"""
import numpy as np

F = np.float32
NAV_KEY = 0xA0761D6478BD642F
LEVEL = {0: (0, 0, False), 1: (8, 1, False), 2: (10, 10, True)}  # hazards, vases, vase contact costs
GOAL_R, HAZ_R, VASE_R, KEEP = F(0.3), F(0.2), F(0.1), F(0.55)
ARENA, BOUND, LIDAR_MAX = F(1.5), F(2.0), F(3.0)
DECAY, DRIVE, TURN = F(0.9), F(0.02), F(0.15)
EDGE = np.stack([np.cos(np.arange(17) * np.pi / 8), np.sin(np.arange(17) * np.pi / 8)], 1).astype(np.float32)
EDGE[16] = EDGE[0]
HAZ, VASE = 12, 32  # first hazard / vase column of the state row
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(key, ctr_hi, ctr_lo):
    """Philox4x32-10.  key, ctr_hi: python ints (64 bit); ctr_lo: uint64 array.  Returns uint32 (..., 4)."""
    ctr_lo = np.asarray(ctr_lo, dtype=np.uint64)
    c = [ctr_lo & M32, ctr_lo >> np.uint64(32),
         np.full(ctr_lo.shape, ctr_hi & 0xFFFFFFFF, np.uint64), np.full(ctr_lo.shape, (ctr_hi >> 32) & 0xFFFFFFFF,
                                                                        np.uint64)]
    k0, k1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & M32]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def u01(x):
    """(0, 1] from 32-bit words, as osa_u01."""
    return ((x >> np.uint32(8)).astype(np.float32) + F(1)) * F(1.0 / 16777216.0)


def draws(seed, pos, N, first_block, count):
    """Uniforms 0 .. count-1 of every env at position pos, ARENA (2 u01 - 1): (N, count) float32."""
    n = np.arange(N, dtype=np.uint64)[:, None]
    j = np.uint64(first_block) + np.arange((count + 3) // 4, dtype=np.uint64)[None, :]
    w = philox4x32_10((seed ^ NAV_KEY) & 0xFFFFFFFFFFFFFFFF, int(pos), (n << np.uint64(20)) + j)
    u = u01(w.reshape(N, -1)[:, :count])
    return (ARENA * (F(2) * u - F(1)).astype(np.float32)).astype(np.float32)


def dist(a, b):
    d = (a - b).astype(np.float32)
    xx, yy = (d[..., 0] * d[..., 0]).astype(np.float32), (d[..., 1] * d[..., 1]).astype(np.float32)
    return np.sqrt((xx + yy).astype(np.float32), dtype=np.float32)


def pick_goal(cands, haz):
    """cands (N, 4, 2), haz (N, H, 2): the first candidate at >= KEEP from every hazard, else the fourth."""
    N = cands.shape[0]
    out = cands[:, 3].copy()
    taken = np.zeros(N, bool)
    for j in range(4):
        ok = np.ones(N, bool)
        for h in range(haz.shape[1]):
            ok &= dist(cands[:, j], haz[:, h]) >= KEEP
        sel = ok & ~taken
        out[sel] = cands[sel, j]
        taken |= ok
    return out


def nav_reset(seed, pos, N, level):
    """The (N, 64) state of a reset at stream position pos."""
    H, V, _ = LEVEL[level]
    u = draws(seed, pos, N, 1, 52)
    s = np.zeros((N, 64), np.float32)
    s[:, 0:2] = u[:, 0:2]
    hx, hy = u[:, 2], u[:, 3]
    nrm = np.sqrt(((hx * hx).astype(np.float32) + (hy * hy).astype(np.float32)).astype(np.float32), dtype=np.float32)
    pos_n = nrm > 0
    safe = np.where(pos_n, nrm, F(1))
    s[:, 2] = np.where(pos_n, hx / safe, F(1))
    s[:, 3] = np.where(pos_n, hy / safe, F(0))
    s[:, HAZ:HAZ + 2 * H] = u[:, 12:12 + 2 * H]
    s[:, VASE:VASE + 2 * V] = u[:, 32:32 + 2 * V]
    s[:, 8:10] = pick_goal(u[:, 4:12].reshape(N, 4, 2), s[:, HAZ:HAZ + 2 * H].reshape(N, H, 2))
    return s


def nav_step(state, action, level, seed, pos):
    """One transition at stream position pos (no truncation handling: the caller resets with nav_reset(seed, pos)).
    Returns (new state, reward, cost, reached)."""
    H, V, vase_costs = LEVEL[level]
    s = state.astype(np.float32).copy()
    N = s.shape[0]
    a = np.minimum(np.maximum(np.asarray(action, np.float32), F(-1)), F(1))
    p, u, f, g = s[:, 0:2], s[:, 2:4], s[:, 4], s[:, 8:10]
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
    q = (p + (f2[:, None] * u2).astype(np.float32)).astype(np.float32)
    q = np.minimum(np.maximum(q, -BOUND), BOUND)
    d0, d1 = dist(p, g), dist(q, g)
    reached = d1 < GOAL_R
    reward = ((d0 - d1).astype(np.float32) + reached.astype(np.float32)).astype(np.float32)
    hit = np.zeros(N, bool)
    for h in range(H):
        hit |= dist(q, s[:, HAZ + 2 * h:HAZ + 2 * h + 2]) < HAZ_R
    if vase_costs:
        for v in range(V):
            hit |= dist(q, s[:, VASE + 2 * v:VASE + 2 * v + 2]) < VASE_R
    out = s.copy()
    out[:, 0:2], out[:, 2:4], out[:, 4], out[:, 5], out[:, 6] = q, u2, f2, f, t
    if reached.any():
        cands = draws(seed, pos, N, 14, 8).reshape(N, 4, 2)
        ng = pick_goal(cands, s[:, HAZ:HAZ + 2 * H].reshape(N, H, 2))
        out[:, 8:10] = np.where(reached[:, None], ng, g)
    return out, reward, hit.astype(np.float32), reached


def lidar(p, u, objs):
    """(N, 16) lidar of objs (N, K, 2) seen from p with heading u."""
    N = p.shape[0]
    out = np.zeros((N, 16), np.float32)
    for h in range(objs.shape[1]):
        r = (objs[:, h] - p).astype(np.float32)
        bx = ((u[:, 0] * r[:, 0]).astype(np.float32) + (u[:, 1] * r[:, 1]).astype(np.float32)).astype(np.float32)
        by = ((u[:, 0] * r[:, 1]).astype(np.float32) - (u[:, 1] * r[:, 0]).astype(np.float32)).astype(np.float32)
        d = np.sqrt(((r[:, 0] * r[:, 0]).astype(np.float32) + (r[:, 1] * r[:, 1]).astype(np.float32))
                    .astype(np.float32), dtype=np.float32)
        val = np.maximum(F(0), (F(1) - (d / LIDAR_MAX).astype(np.float32)).astype(np.float32)).astype(np.float32)
        for k in range(16):
            c0 = ((EDGE[k, 0] * by).astype(np.float32) - (EDGE[k, 1] * bx).astype(np.float32)).astype(np.float32)
            c1 = ((EDGE[k + 1, 0] * by).astype(np.float32) - (EDGE[k + 1, 1] * bx).astype(np.float32)) \
                .astype(np.float32)
            inb = (c0 >= 0) & (c1 < 0)
            out[:, k] = np.where(inb, np.maximum(out[:, k], val), out[:, k])
    return out


def lidar_bins(p, u, objs):
    """(N, K) number of bins that each object falls in (the specification's claim: always 1)."""
    cnt = np.zeros(objs.shape[:2], int)
    for h in range(objs.shape[1]):
        r = (objs[:, h] - p).astype(np.float32)
        bx = ((u[:, 0] * r[:, 0]).astype(np.float32) + (u[:, 1] * r[:, 1]).astype(np.float32)).astype(np.float32)
        by = ((u[:, 0] * r[:, 1]).astype(np.float32) - (u[:, 1] * r[:, 0]).astype(np.float32)).astype(np.float32)
        for k in range(16):
            c0 = ((EDGE[k, 0] * by).astype(np.float32) - (EDGE[k, 1] * bx).astype(np.float32)).astype(np.float32)
            c1 = ((EDGE[k + 1, 0] * by).astype(np.float32) - (EDGE[k + 1, 1] * bx).astype(np.float32)) \
                .astype(np.float32)
            cnt[:, h] += (c0 >= 0) & (c1 < 0)
    return cnt


def nav_obs(state, level):
    """The (N, 60) observation of a state."""
    H, V, _ = LEVEL[level]
    s = np.asarray(state, np.float32)
    N = s.shape[0]
    o = np.zeros((N, 60), np.float32)
    o[:, 0] = s[:, 4]
    o[:, 1] = (s[:, 4] - s[:, 5]).astype(np.float32)
    o[:, 2] = s[:, 6]
    o[:, 3:5] = s[:, 2:4]
    p, u = s[:, 0:2], s[:, 2:4]
    o[:, 12:28] = lidar(p, u, s[:, 8:10].reshape(N, 1, 2))
    o[:, 28:44] = lidar(p, u, s[:, HAZ:HAZ + 2 * H].reshape(N, H, 2))
    o[:, 44:60] = lidar(p, u, s[:, VASE:VASE + 2 * V].reshape(N, V, 2))
    return o


class NavTwin:
    """The vector env as the device class plays it: all lanes reset together every `horizon` steps; stream position
    0 is the reset, every step takes the next one (a truncating step resets at its own position)."""

    def __init__(self, level, N, horizon, seed):
        self.level, self.N, self.horizon, self.seed = level, N, horizon, seed
        self.pos = 0
        self.since = 0
        self.state = None

    def reset(self):
        self.state = nav_reset(self.seed, self.pos, self.N, self.level)
        self.pos += 1
        self.since = 0
        return nav_obs(self.state, self.level)

    def step(self, action):
        self.state, r, c, reached = nav_step(self.state, action, self.level, self.seed, self.pos)
        self.since += 1
        trunc = self.since % self.horizon == 0
        final = None
        if trunc:
            final = nav_obs(self.state, self.level)
            self.state = nav_reset(self.seed, self.pos, self.N, self.level)
        self.pos += 1
        return nav_obs(self.state, self.level), r, c, trunc, final, reached
