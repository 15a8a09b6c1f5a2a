"""Numpy twin of the rollout-side kernels of omnisafe_amd/csrc/rollout_kernels.hip (helper module of the tests, no
tests of its own): osa_rollout_post_step, osa_saute_step, osa_action_scale, osa_normalizer_apply and the float64 truth
that osa_normalizer_push is measured against.

The specification, once, from the contract in include/omnisafe_amd.h:

post_step     one vector step of the per-env loop of the rollout.  The step's reward / cost / 1 are added to the episode
              accumulators (float32).  A path ends where the epoch ends or the env terminated or was truncated.  Its
              bootstrap value is 0 for a terminated env; otherwise V(next observation) at the epoch end and V(final
              observation) for a truncated env -- and the final observation's value WINS where both apply.  A bootstrap
              array that is absent is not applied.  An episode is finished where the env terminated or was truncated
              (the epoch end alone finishes none): its three sums go to the `*_out` rows, which are written nowhere
              else, and the accumulators restart from 0.
saute_step    z <- (z - cost / budget) / saute_gamma; the reward is kept while z > 0 (strictly) and replaced by
              unsafe_reward otherwise; a finished env restarts z from its reset value; the episode's sum of z (taken
              AFTER the restart) goes to ep_budget_out where the env finished and the sum restarts from 0.
action_scale  lo + (hi - lo) (a - min_a) / (max_a - min_a), per action dimension.
normalize_apply   clip((x - mean) / std, -clip, clip) for the selected rows once count > 1; everything else is copied.
              A NaN stays a NaN (the reference clamps with torch.clamp, which propagates it).
RunningMoments    float64 mean and unbiased variance of ALL rows selected so far: the plain truth, no merge formula.

float32 everywhere but RunningMoments, every intermediate rounded to float32, no fused multiply-adds.
"""
import numpy as np

F = np.float32


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def post_step(epoch_end, reward, cost, terminated, truncated, ep_ret, ep_cost, ep_len, vnext_r=None, vnext_c=None,
              vfinal_r=None, vfinal_c=None, fill=np.nan):
    """Returns a dict: ep_ret, ep_cost, ep_len (new accumulators), path_end, boot_r, boot_c, ep_done, and ep_ret_out,
    ep_cost_out, ep_len_out, which hold `fill` wherever no episode finished (the kernel leaves those elements alone)."""
    reward, cost = _f32(reward), _f32(cost)
    N = reward.shape[0]
    assert (vnext_r is None) == (vnext_c is None) and (vfinal_r is None) == (vfinal_c is None)
    o = {k: _f32(v).copy() for k, v in (('ep_ret', ep_ret), ('ep_cost', ep_cost), ('ep_len', ep_len))}
    o['path_end'] = np.zeros(N, np.uint8)
    o['ep_done'] = np.zeros(N, np.uint8)
    o['boot_r'] = np.zeros(N, np.float32)
    o['boot_c'] = np.zeros(N, np.float32)
    for k in ('ep_ret_out', 'ep_cost_out', 'ep_len_out'):
        o[k] = np.full(N, fill, np.float32)
    for n in range(N):
        o['ep_ret'][n] = o['ep_ret'][n] + reward[n]
        o['ep_cost'][n] = o['ep_cost'][n] + cost[n]
        o['ep_len'][n] = o['ep_len'][n] + F(1)
        term, trunc = bool(terminated[n]), bool(truncated[n])
        if not (epoch_end or term or trunc):
            continue
        o['path_end'][n] = 1
        if not term:
            if epoch_end and vnext_r is not None:
                o['boot_r'][n], o['boot_c'][n] = vnext_r[n], vnext_c[n]
            if trunc and vfinal_r is not None:  # after the epoch end's: the final observation's value wins
                o['boot_r'][n], o['boot_c'][n] = vfinal_r[n], vfinal_c[n]
        if term or trunc:
            o['ep_done'][n] = 1
            o['ep_ret_out'][n], o['ep_cost_out'][n], o['ep_len_out'][n] = o['ep_ret'][n], o['ep_cost'][n], o['ep_len'][n]
            o['ep_ret'][n] = o['ep_cost'][n] = o['ep_len'][n] = F(0)
    return o


def saute_step(safety_obs, cost, reward, terminated, truncated, budget, saute_gamma, unsafe_reward, reset_value,
               ep_budget, fill=np.nan):
    """Returns a dict: safety_obs (the new z, also the value of the written observation column), reward_out, ep_budget,
    done, and ep_budget_out holding `fill` wherever the env did not finish."""
    z, cost, reward = _f32(safety_obs), _f32(cost), _f32(reward)
    budget, reset_value, ep_budget = _f32(budget), _f32(reset_value), _f32(ep_budget)
    one = F(1)
    spent = cost / budget
    z = z - spent
    z = z / F(saute_gamma)
    safe = np.where(z > F(0), one, F(0)).astype(np.float32)
    kept = safe * reward
    replaced = (one - safe) * F(unsafe_reward)
    reward_out = kept + replaced
    done = ((np.asarray(terminated) != 0) | (np.asarray(truncated) != 0))
    d = done.astype(np.float32)
    carried = z * (one - d)
    restart = d * reset_value
    z = carried + restart
    total = ep_budget + z
    out = dict(safety_obs=z, reward_out=reward_out, done=done.astype(np.uint8),
               ep_budget=np.where(done, F(0), total).astype(np.float32),
               ep_budget_out=np.where(done, total, F(fill)).astype(np.float32))
    assert all(v.dtype in (np.float32, np.uint8) for v in out.values())
    return out


def action_scale(act, lo, hi, min_a, max_a):
    """act (N, D); lo, hi (D,).  float32, in the order width * offset / range, then + lo."""
    act, lo, hi = _f32(act), _f32(lo), _f32(hi)
    width = hi - lo
    offset = act - F(min_a)
    rng = F(max_a) - F(min_a)
    prod = width[None, :] * offset
    out = lo[None, :] + prod / rng
    assert out.dtype == np.float32
    return out


def normalize_apply(x, mean, std, count, clip, mask=None):
    """x (N, D); mean, std (D,); count int; mask (N,) or None = every row."""
    x = _f32(x)
    y = x.copy()
    if int(count) <= 1:
        return y
    on = np.ones(x.shape[0], bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(invalid='ignore', divide='ignore'):
        v = (x - _f32(mean)[None, :]) / _f32(std)[None, :]
    v = np.where(v < F(-clip), F(-clip), v)  # (comparisons are false for a NaN: it stays)
    v = np.where(v > F(clip), F(clip), v).astype(np.float32)
    y[on] = v[on]
    return y


class RunningMoments:
    """float64 mean and unbiased variance (ddof = 1) per column of the concatenation of all rows pushed so far."""

    def __init__(self, D):
        self.rows = np.zeros((0, D), np.float64)

    def push(self, x, mask=None):
        x = np.asarray(x, np.float64).reshape(-1, self.rows.shape[1])
        if mask is not None:
            x = x[np.asarray(mask) != 0]
        self.rows = np.concatenate([self.rows, x], 0)

    @property
    def count(self):
        return self.rows.shape[0]

    @property
    def mean(self):
        return self.rows.mean(0)

    @property
    def var(self):
        """NaN for fewer than two rows, like the running form's 0 / 0."""
        if self.count < 2:
            return np.full(self.rows.shape[1], np.nan)
        d = self.rows - self.rows.mean(0)
        return (d * d).sum(0) / (self.count - 1)


MOMENT_FACTOR = 4.0  # e_kernel <= MOMENT_FACTOR * max(e_reference, 2**-23): see tests/test_rollout_kernels_gpu.py


def moment_errors(mean, var, truth, skip_var=()):
    """(e_mean, e_var) of float32 running statistics against a RunningMoments: the largest |mean - truth| / (|truth
    mean| + truth std) and |var - truth| / truth var over the columns (variance: not those in skip_var, and 0 while
    fewer than two rows make it undefined)."""
    tm = truth.mean
    tv = truth.var if truth.count > 1 else np.zeros_like(tm)
    scale = np.abs(tm) + np.sqrt(tv)
    assert (scale > 0).all()
    e_mean = float(np.max(np.abs(np.asarray(mean, np.float64) - tm) / scale))
    cols = np.setdiff1d(np.arange(tm.shape[0]), np.asarray(skip_var, int))
    if truth.count < 2 or cols.size == 0:
        return e_mean, 0.0
    assert (tv[cols] > 0).all()
    e_var = float(np.max(np.abs(np.asarray(var, np.float64)[cols] - tv[cols]) / tv[cols]))
    return e_mean, e_var
