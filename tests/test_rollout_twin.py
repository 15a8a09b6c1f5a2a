"""CPU tests: the numpy twin of the rollout-side kernels (tests/rollout_twin.py) against data the unmodified reference
produced -- the Saute / Simmer safety column and shaped rewards, the episode windows and GAE outputs of a PPOLag and of
an early-terminated rollout, the normaliser golden -- and against hand-computed one-line cases of every branch.

Also here: the measurement behind the bound of tests/test_rollout_kernels_gpu.py on the normaliser's statistics.
`KernelStatement` restates osa_norm_push_kernel's arithmetic (float64 shifted batch sums, float32 merge) in numpy;
`e_k / max(e_ref, 2**-23)`, with e_ref the error of the reference's float32 form (np_oracle.Normalizer) against the
float64 truth, is at most 1.10 over the sequences below (mixed batch sizes, 500 single rows, 16 x 4096, offsets 1e3 and
1e4, column scales 1e-3 ... 1e3); the bound is 4.
"""
import numpy as np
import pytest
import torch

import np_oracle as O
import rollout_twin as R
from test_oracle_golden import load_ac

F = np.float32


# ---- Saute / Simmer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['saute', 'simmer'])
def test_saute_step_replays_the_reference_rollout(golden, tag):
    """Column 60 of buffer/obs (the safety state the policy saw at every step), buffer/reward and the Metrics/EpBudget
    window of the reference's PPOSaute / PPOSimmerPID rollout, bit for bit, from the raw env outputs."""
    g = golden(f'{tag}_rollout.npz')
    N, T = int(g['N']), int(g['T'])
    saute_gamma, max_ep_len, safety_budget, unsafe_reward = 0.999, 16, 1.0, -0.5  # oracle/make_golden.py
    scale = (1 - saute_gamma ** max_ep_len) / (1 - saute_gamma) / max_ep_len
    budget = np.full(N, safety_budget * scale, np.float32)
    start = np.ones(N, np.float32)
    if tag == 'simmer':  # the epoch starts from budget / upper budget; the recorded controller steps pin the upper one
        upper = F(2.0 * scale)
        np.testing.assert_array_equal((g['control/budget_rel'][:, 0] / upper).astype(np.float32),
                                      g['control/budget_rel'][:, 1])
        start = (budget / upper).astype(np.float32)
    assert (g['rollout/truncated'][15] & g['rollout/truncated'][31]).all() and g['rollout/truncated'].sum() == 2 * N
    z, ep_budget, episodes = start.copy(), np.zeros(N, np.float32), []
    for t in range(T):
        assert np.array_equal(z, g['buffer/obs'][t, :, 60]), t
        o = R.saute_step(z, g['rollout/cost'][t], g['rollout/reward'][t], g['rollout/terminated'][t],
                         g['rollout/truncated'][t], budget, saute_gamma, unsafe_reward, np.ones(N, np.float32),
                         ep_budget)
        assert np.array_equal(o['reward_out'], g['buffer/reward'][t]), t
        assert np.array_equal(np.isnan(o['ep_budget_out']), o['done'] == 0)
        episodes += [o['ep_budget_out'][n] for n in range(N) if o['done'][n]]
        z, ep_budget = o['safety_obs'], o['ep_budget']
    assert (g['buffer/reward'] == F(unsafe_reward)).sum() > 20  # the unsafe branch is exercised
    assert np.array_equal(np.asarray(episodes, np.float32), g['rollout/ep_budget_window'])


def test_saute_step_z_exactly_zero_is_unsafe():
    """budget 0.5, saute_gamma 1, costs 0.25 and 0.25: z = 1 -> 0.5 -> 0, and 0 is not `> 0`."""
    one = np.ones(1, np.float32)
    args = dict(terminated=[0], truncated=[0], budget=[0.5], saute_gamma=1.0, unsafe_reward=-7.0, reset_value=one)
    a = R.saute_step(one, [0.25], [3.0], ep_budget=[0.0], **args)
    assert a['safety_obs'][0] == F(0.5) and a['reward_out'][0] == F(3.0) and a['ep_budget'][0] == F(0.5)
    b = R.saute_step(a['safety_obs'], [0.25], [3.0], ep_budget=a['ep_budget'], **args)
    assert b['safety_obs'][0] == 0.0 and b['reward_out'][0] == F(-7.0) and b['ep_budget'][0] == F(0.5)
    assert np.isnan(b['ep_budget_out'][0]) and b['done'][0] == 0
    # the same step ending the episode: the reward is decided BEFORE the restart, the sum takes z AFTER it
    c = R.saute_step(a['safety_obs'], [0.25], [3.0], ep_budget=a['ep_budget'], **dict(args, truncated=[1],
                                                                                      reset_value=[0.75]))
    assert c['reward_out'][0] == F(-7.0) and c['safety_obs'][0] == F(0.75) and c['done'][0] == 1
    assert c['ep_budget_out'][0] == F(1.25) and c['ep_budget'][0] == 0.0


# ---- post_step -----------------------------------------------------------------------------------------------------
VN, VF = (F(10), F(20)), (F(30), F(40))


@pytest.mark.parametrize('epoch_end,term,trunc,vnext,vfinal,path_end,boot,done', [
    (0, 0, 0, True, True, 0, (0, 0), 0),      # nothing ends
    (1, 0, 0, True, True, 1, VN, 0),          # epoch end: V(next observation), the episode goes on
    (1, 0, 0, False, True, 1, (0, 0), 0),     # ... no array given: not applied
    (0, 0, 1, True, True, 1, VF, 1),          # truncated: V(final observation)
    (0, 0, 1, True, False, 1, (0, 0), 1),     # ... no array given
    (1, 0, 1, True, True, 1, VF, 1),          # truncated AT the epoch end: the final observation's value wins
    (1, 0, 1, True, False, 1, VN, 1),         # ... and without one the epoch end's stands
    (0, 1, 0, True, True, 1, (0, 0), 1),      # terminated: no bootstrap
    (0, 1, 1, True, True, 1, (0, 0), 1),      # terminated and truncated: terminated decides
    (1, 1, 0, True, True, 1, (0, 0), 1),      # a terminated env at the epoch end
    (1, 1, 1, True, True, 1, (0, 0), 1),
])
def test_post_step_branch_by_hand(epoch_end, term, trunc, vnext, vfinal, path_end, boot, done):
    o = R.post_step(epoch_end, [0.25], [1.0], [term], [trunc], [1.5], [2.0], [6.0],
                    *(([VN[0]], [VN[1]]) if vnext else (None, None)), *(([VF[0]], [VF[1]]) if vfinal else (None, None)),
                    fill=-9.0)
    assert o['path_end'][0] == path_end and o['ep_done'][0] == done
    assert (o['boot_r'][0], o['boot_c'][0]) == (F(boot[0]), F(boot[1]))
    if done:
        assert (o['ep_ret_out'][0], o['ep_cost_out'][0], o['ep_len_out'][0]) == (F(1.75), F(3.0), F(7.0))
        assert (o['ep_ret'][0], o['ep_cost'][0], o['ep_len'][0]) == (0.0, 0.0, 0.0)
    else:
        assert (o['ep_ret_out'][0], o['ep_cost_out'][0], o['ep_len_out'][0]) == (F(-9.0), F(-9.0), F(-9.0))
        assert (o['ep_ret'][0], o['ep_cost'][0], o['ep_len'][0]) == (F(1.75), F(3.0), F(7.0))


def _replay_post_step(g, early):
    """The rollout of the golden `g` with the twin's post_step deciding path ends, bootstraps and episode metrics.  The
    bootstrap VALUES come from the oracle's critics on observations normalised by the oracle's normaliser (both pinned
    to the reference by tests/test_oracle_golden.py), row by row as the reference evaluates them; that the replay feeds
    the right observations is checked against the recorded buffer/obs."""
    torch.set_num_threads(1)
    N, T = int(g['N']), int(g['T'])
    ac, norm = load_ac(g, 'init/'), O.Normalizer((60,), clip=5)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()  # noqa: E731

    def values(rows, which):
        vr, vc = np.zeros(N, np.float32), np.zeros(N, np.float32)
        for n in np.nonzero(which)[0]:
            _, a, b, _ = ac.step(rows[n], deterministic=True)
            vr[n], vc[n] = float(a), float(b)
        return vr, vc

    obs = norm.normalize(t_(g['rollout/resets'][0] if early else g['rollout/reset_obs']))
    ep = {k: np.zeros(N, np.float32) for k in ('ep_ret', 'ep_cost', 'ep_len')}
    rows = {k: np.zeros((T, N), np.float32) for k in ('boot_r', 'boot_c', 'reward')}
    rows['path_end'] = np.zeros((T, N), np.uint8)
    episodes, cost_sum, n_resets = [], F(0), 1
    for t in range(T):
        assert np.array_equal(obs.numpy(), g['buffer/obs'][t]), t
        term, trunc = g['rollout/terminated'][t].copy(), g['rollout/truncated'][t].copy()
        reward, cost = g['rollout/reward'][t].copy(), g['rollout/cost'][t]
        fin = term | trunc
        final = t_(g['rollout/final_obs'][t]).clone()
        if fin.any():  # ObsNormalize: the finished rows of the final observation first, then the next observation
            final[torch.from_numpy(fin)] = norm.normalize(final[torch.from_numpy(fin)])
        obs = norm.normalize(t_(g['rollout/obs'][t]))
        if early:  # the early-termination wrapper: over the cost limit -> zero reward, terminated, a fresh episode
            cost_sum = F(cost_sum + cost[0])
            if cost_sum > g['cost_limit']:
                reward[:], term[:], cost_sum = 0, True, F(0)
                obs = norm.normalize(t_(g['rollout/resets'][n_resets]))
                n_resets += 1
        epoch_end = t == T - 1
        vfinal = values(final, trunc & ~term)
        vnext = values(obs, np.ones(N, bool)) if epoch_end else (None, None)
        o = R.post_step(epoch_end, reward, cost, term, trunc, ep['ep_ret'], ep['ep_cost'], ep['ep_len'], *vnext, *vfinal)
        ep = {k: o[k] for k in ep}
        for k in ('boot_r', 'boot_c', 'path_end'):
            rows[k][t] = o[k]
        rows['reward'][t] = reward
        episodes += [(o['ep_ret_out'][n], o['ep_cost_out'][n], o['ep_len_out'][n]) for n in range(N) if o['ep_done'][n]]
        assert np.array_equal(np.isnan(o['ep_ret_out']), o['ep_done'] == 0)
    assert norm.count == int(g['rollout/norm_count'])
    if early:
        assert n_resets == g['rollout/resets'].shape[0]
    return rows, np.asarray(episodes, np.float32).reshape(-1, 3)


@pytest.mark.parametrize('name', ['ppolag_epoch', 'early_terminated_rollout'])
def test_post_step_replays_the_reference_rollout(golden, name):
    g = golden(f'{name}.npz')
    early = name.startswith('early')
    rows, episodes = _replay_post_step(g, early)
    assert np.array_equal(rows['reward'], g['buffer/reward'])
    assert len(episodes) == (32 if early else 8)
    for k, key in enumerate(('ep_ret', 'ep_cost', 'ep_len')):
        assert np.array_equal(episodes[:, k], g[f'rollout/{key}_window']), key
    gae = O.gae_time_major(g['buffer/reward'], g['buffer/cost'], g['buffer/value_r'], g['buffer/value_c'],
                           rows['path_end'], rows['boot_r'], rows['boot_c'], 0.99, 0.95, 0.95)
    for ok, gk in (('adv_r', 'adv_r'), ('adv_c', 'adv_c'), ('tgt_r', 'target_value_r'), ('tgt_c', 'target_value_c'),
                   ('disc_ret', 'discounted_ret')):
        assert np.array_equal(gae[ok], g[f'buffer/{gk}']), ok
    if early:  # 14 early terminations (no bootstrap) among 18 truncations
        early_steps = (g['buffer/reward'][:, 0] == 0) & (g['rollout/reward'][:, 0] != 0)
        assert early_steps.sum() == 14 and not rows['boot_r'][early_steps].any()
        assert rows['boot_r'][g['rollout/truncated'][:, 0] & ~early_steps].all()


# ---- normaliser ----------------------------------------------------------------------------------------------------
def test_normalize_apply_vs_reference(golden):
    g = golden('normalizer.npz')
    norm, truth = O.Normalizer((7,), clip=5), R.RunningMoments(7)
    for i in range(int(g['n_batches'])):
        x = g[f'in{i}']
        norm.push(torch.from_numpy(x.copy()))
        truth.push(x)
        assert np.array_equal(norm.mean.numpy(), g[f'mean{i}']) and norm.count == int(g[f'count{i}'])
        assert np.array_equal(norm.std.numpy(), g[f'std{i}'], equal_nan=True)
        y = R.normalize_apply(x, g[f'mean{i}'], g[f'std{i}'], g[f'count{i}'], 5.0)
        assert np.array_equal(y, g[f'out{i}']), i
        assert truth.count == int(g[f'count{i}'])
        np.testing.assert_allclose(truth.mean, g[f'mean{i}'], rtol=1e-5, atol=1e-6)
        if truth.count > 1:
            np.testing.assert_allclose(truth.var, g[f'var{i}'], rtol=1e-5)
        else:
            assert np.isnan(truth.var).all() and np.isnan(g[f'var{i}']).all()


def test_normalize_apply_by_hand():
    x = np.array([[0.0, 10.0, -10.0, np.nan], [1.0, 2.0, 3.0, 4.0]], np.float32)
    mean, std = np.array([1, 2, 3, 4], np.float32), np.array([2, 2, 2, 2], np.float32)
    y = R.normalize_apply(x, mean, std, 2, 1.5)
    assert np.array_equal(y, np.array([[-0.5, 1.5, -1.5, np.nan], [0, 0, 0, 0]], np.float32), equal_nan=True)
    for count in (0, 1):  # the statistics are not usable yet: everything passes through
        assert np.array_equal(R.normalize_apply(x, mean, std, count, 1.5), x, equal_nan=True)
    y = R.normalize_apply(x, mean, std, 2, 1.5, mask=[0, 1])
    assert np.array_equal(y[0], x[0], equal_nan=True) and not y[1].any()


def test_action_scale_by_hand():
    y = R.action_scale([[-1.0, 0.0, 1.0, 0.5]], [-2, -2, -2, 3], [4, 4, 4, 3], -1.0, 1.0)
    assert np.array_equal(y, np.array([[-2, 1, 4, 3]], np.float32))


# ---- the bound on the normaliser's statistics -------------------------------------------------------------------------
class KernelStatement:
    """osa_norm_push_kernel's arithmetic: the batch as float64 sums of (x - running mean) and its square, the batch mean
    and centred sum of squares rounded to float32, then the reference's merge in float32."""

    def __init__(self, D):
        self.mean, self.sumsq, self.count = np.zeros(D, np.float32), np.zeros(D, np.float32), 0
        self.var = np.zeros(D, np.float32)

    def push(self, x):
        n = x.shape[0]
        if n == 0:
            return
        c = self.mean.astype(np.float64)
        d = x.astype(np.float64) - c
        s1, s2 = d.sum(0), (d * d).sum(0)
        mean_raw = (c + s1 / n).astype(np.float32)
        sumq_raw = np.maximum(s2 - s1 * s1 / n, 0.0).astype(np.float32)
        new = self.count + n
        if self.count == 0:
            self.mean, self.sumsq = mean_raw, sumq_raw
        else:
            delta = mean_raw - self.mean
            self.mean = self.mean + delta * F(n) / F(new)
            self.sumsq = self.sumsq + (sumq_raw + delta * delta * F(self.count) * F(n) / F(new))
        self.count = new
        with np.errstate(invalid='ignore', divide='ignore'):
            self.var = self.sumsq / F(new - 1)


def _sequences():
    rng = np.random.default_rng(17)
    D = 24
    col = lambda lo, hi: np.linspace(lo, hi, D)  # noqa: E731
    yield 'mixed sizes', [rng.standard_normal((n, D)) * col(0.5, 2) + col(-3, 3) for n in (257, 64, 1, 2000, 33, 4097, 7)]
    yield '500 single rows', [rng.standard_normal((1, D)) * col(0.5, 2) + col(-3, 3) for _ in range(500)]
    yield '16 x 4096', [rng.standard_normal((4096, D)) * col(0.5, 2) + col(-3, 3) for _ in range(16)]
    yield 'offset 1e3', [rng.standard_normal((n, D)) + 1e3 for n in (300, 64, 1, 2000, 33)]
    yield 'offset 1e4', [rng.standard_normal((n, D)) + 1e4 for n in (300, 64, 1, 2000, 33)]
    yield 'column scales', [rng.standard_normal((n, D)) * np.logspace(-3, 3, D) + col(-50, 50) for n in (257, 64, 1, 2000, 33)]


def test_kernel_statement_stays_within_the_bound_of_the_gpu_test(capsys):
    worst = 0.0
    for name, batches in _sequences():
        D = batches[0].shape[1]
        k, ref, truth = KernelStatement(D), O.Normalizer((D,), clip=5), R.RunningMoments(D)
        for x in batches:
            x = x.astype(np.float32)
            k.push(x)
            ref.push(torch.from_numpy(x))
            truth.push(x)
            assert k.count == truth.count
            ek = R.moment_errors(k.mean, k.var, truth)
            er = R.moment_errors(ref.mean.numpy(), ref.var.numpy(), truth)
            for a, b, what in zip(ek, er, ('mean', 'var')):
                ratio = a / max(b, 2.0 ** -23)
                worst = max(worst, ratio)
                assert a <= R.MOMENT_FACTOR * max(b, 2.0 ** -23), (name, what, truth.count, a, b)
    with capsys.disabled():
        print(f'\n[normaliser statistics] worst e_k / max(e_ref, 2^-23) of the numpy statement: {worst:.2f}')


def test_moment_errors_see_a_dropped_or_doubled_row():
    """What the bound is for: one row of 4097 lost, or counted twice, is orders of magnitude outside it."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((4097, 8)) * 2 + 1).astype(np.float32)
    x[-1] += 40  # (a row that matters, as the clamped last row of a block would)
    truth = R.RunningMoments(8)
    truth.push(x)
    for bad in (x[:-1], np.concatenate([x, x[-1:]])):
        k = KernelStatement(8)
        k.push(bad)
        e = R.moment_errors(k.mean, k.var, truth)
        assert min(e) > 1e-3 > 1e3 * R.MOMENT_FACTOR * 2.0 ** -23
