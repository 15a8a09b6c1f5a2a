"""A torch statement of one offline CRR / CCRR train step (crr.py:114-200, c_crr.py:91-206) at a chosen dtype, with
injected draws, and a numpy restatement of the device draws (csrc/crr_kernels.hip).  No import of the product: the
networks are built by hand from state dicts with the reference's names.

    tw = Twin(actor_sd, [reward_pair_sd, cost_pair_sd], actor_act, critic_act, dtype=torch.float64, ...)
    stats = tw.step(batch, eps_next, eps_samp, eps_next_c, lagrange_open)

`wiring='intended'`: the cost pair has its own update; `'reference'`: c_crr.py as written (the reward pair takes the
second critic update too and values the sampled actions of the cost advantage).  The two differ ONLY in the objects
handed to `_critic_update` and `_sample_value`.
"""
import math
import zlib
from collections import OrderedDict

import numpy as np
import torch

from nav_twin import philox4x32_10

ACT = {'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid,
       'softplus': torch.nn.functional.softplus, 'identity': lambda x: x}
KEY_IDX, KEY_NEXT, KEY_NEXTC, KEY_SAMP = 0x43525249445831, 0x4352524E585431, 0x4352524E584332, 0x43525253414D31
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------- draws (numpy)
def draw_idx(seed, step, B, N):
    """idx[b] of a step: the first 64 bits of Philox(seed ^ KEY_IDX, step, b), multiply-high into [0, N)."""
    w = philox4x32_10((seed ^ KEY_IDX) & M64, step, np.arange(B, dtype=np.uint64))
    bits = [int(lo) | (int(hi) << 32) for lo, hi in zip(w[:, 0], w[:, 1])]
    return np.array([(b * N) >> 64 for b in bits], dtype=np.int64)


def draw_eps(seed, key, step, rows, A):
    """eps[row][d] of a step: the first Box-Muller normal of Philox(seed ^ key, step, row A + d), in float64, rounded
    to float32 once."""
    w = philox4x32_10((seed ^ key) & M64, step, np.arange(rows * A, dtype=np.uint64))
    u1 = ((w[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = ((w[:, 1] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.28318530717958647692 * u2)).astype(np.float32).reshape(rows, A)


# ---------------------------------------------------------------------------------------------------- networks
class Mlp:
    def __init__(self, sd, prefix, act, dtype):
        self.act = ACT[act]
        self.layers = []
        j = 0
        while f'{prefix}.{2 * j}.weight' in sd:
            w = torch.as_tensor(sd[f'{prefix}.{2 * j}.weight']).detach().to(dtype).clone().requires_grad_(True)
            b = torch.as_tensor(sd[f'{prefix}.{2 * j}.bias']).detach().to(dtype).clone().requires_grad_(True)
            self.layers.append((w, b))
            j += 1
        self.prefix = prefix

    def __call__(self, x):
        for i, (w, b) in enumerate(self.layers):
            x = torch.nn.functional.linear(x, w, b)  # (nn.Linear's own op: same bits as the reference's modules)
            if i + 1 < len(self.layers):
                x = self.act(x)
        return x

    def named(self):
        out = OrderedDict()
        for j, (w, b) in enumerate(self.layers):
            out[f'{self.prefix}.{2 * j}.weight'], out[f'{self.prefix}.{2 * j}.bias'] = w, b
        return out


class Actor:
    def __init__(self, sd, act, dtype):
        self.log_std = torch.as_tensor(sd['log_std']).detach().to(dtype).clone().requires_grad_(True)
        self.mean = Mlp(sd, 'mean', act, dtype)

    def named(self):
        out = OrderedDict(log_std=self.log_std)
        out.update(self.mean.named())
        return out

    def sample(self, obs, eps):
        return self.mean(obs) + torch.exp(self.log_std) * eps

    def log_prob(self, obs, act):
        return torch.distributions.Normal(self.mean(obs), torch.exp(self.log_std)).log_prob(act).sum(-1)


class Pair:
    def __init__(self, sd, act, dtype):
        self.nets = [Mlp(sd, f'critic_{c}.0', act, dtype) for c in range(2)]

    def named(self):
        out = OrderedDict()
        for n in self.nets:
            out.update(n.named())
        return out

    def __call__(self, obs, act):
        x = torch.cat([obs, act], -1)
        return [n(x).squeeze(-1) for n in self.nets]


class Adam:
    """torch.optim.Adam's default single-tensor step, with state that can be set."""

    def __init__(self, named, lr, dtype, m=None, v=None, t=0):
        self.p = named
        self.lr, self.t = lr, int(t)
        self.m = OrderedDict((k, torch.zeros_like(p) if m is None else torch.as_tensor(m[k]).to(dtype).clone())
                             for k, p in named.items())
        self.v = OrderedDict((k, torch.zeros_like(p) if v is None else torch.as_tensor(v[k]).to(dtype).clone())
                             for k, p in named.items())

    def step(self, b1=0.9, b2=0.999, eps=1e-8):
        self.t += 1
        with torch.no_grad():
            for k, p in self.p.items():
                g = p.grad
                self.m[k].lerp_(g, 1 - b1)
                self.v[k].mul_(b2).addcmul_(g, g, value=1 - b2)
                denom = (self.v[k].sqrt() / math.sqrt(1 - b2 ** self.t)).add_(eps)
                p.addcdiv_(self.m[k], denom, value=-self.lr / (1 - b1 ** self.t))
                p.grad = None


class Twin:  # pylint: disable=too-many-instance-attributes
    def __init__(self, actor_sd, pair_sds, actor_act, critic_act, *, dtype=torch.float64, gamma=0.99, beta=1.0,
                 polyak=0.005, lr_actor=1e-3, lr_critic=1e-3, cost_limit=25.0, lambda_lr=1e-3, lambda_init=1.0,
                 wiring='intended', target_sds=None):
        assert wiring in ('intended', 'reference')
        self.dtype, self.wiring = dtype, wiring
        self.gamma, self.beta, self.polyak = gamma, beta, polyak
        self.actor = Actor(actor_sd, actor_act, dtype)
        self.pairs = [Pair(sd, critic_act, dtype) for sd in pair_sds]
        self.targets = [Pair(sd, critic_act, dtype) for sd in (target_sds or pair_sds)]
        self.opt_actor = Adam(self.actor.named(), lr_actor, dtype)
        self.opt_pairs = [Adam(p.named(), lr_critic, dtype) for p in self.pairs]
        self.ccrr = len(self.pairs) == 2
        self.cost_limit = cost_limit
        self.lam = torch.tensor(max(lambda_init, 0.0), dtype=dtype, requires_grad=True)
        self.opt_lam = Adam(OrderedDict(lam=self.lam), lambda_lr, dtype)
        self.last = {}  # per-row quantities of the last step (tests look at them)

    # one shared critic update: the wirings differ in the objects passed here
    def _critic_update(self, pair, target, opt, signal, obs, act, next_obs, done, eps):
        with torch.no_grad():
            a2 = self.actor.sample(next_obs, eps)
            t1, t2 = target(next_obs, a2)
            y = (signal + (1 - done) * self.gamma * torch.min(t1, t2).unsqueeze(1)).squeeze(1)
        q1, q2 = pair(obs, act)
        loss = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
        loss.backward()
        opt.step()
        return loss.item(), q1[0].item(), y[0].item()

    def _sample_value(self, pair, obs_rep, act_s, S):
        with torch.no_grad():
            q1, q2 = pair(obs_rep, act_s)
            return torch.min(q1, q2).reshape(-1, S).mean(1)

    def step(self, batch, eps_next, eps_samp, eps_next_c=None, lagrange_open=False):
        """One train step; returns the logged scalars by the reference's key."""
        dt = self.dtype
        obs, act, reward, cost, next_obs, done = (torch.as_tensor(x).to(dt) for x in batch)
        eps_next, eps_samp = torch.as_tensor(eps_next).to(dt), torch.as_tensor(eps_samp).to(dt)
        B = obs.shape[0]
        S = eps_samp.shape[0] // B
        out = {}
        ref = self.ccrr and self.wiring == 'reference'
        out['Loss/Loss_reward_critic'], out['Qr/data_Qr'], out['Qr/target_Qr'] = self._critic_update(
            self.pairs[0], self.targets[0], self.opt_pairs[0], reward, obs, act, next_obs, done, eps_next)
        if self.ccrr:
            k = 0 if ref else 1
            out['Loss/Loss_cost_critic'], out['Qc/data_Qc'], out['Qc/target_Qc'] = self._critic_update(
                self.pairs[k], self.targets[k], self.opt_pairs[k], cost, obs, act, next_obs, done,
                torch.as_tensor(eps_next_c).to(dt))
        # ---- actor, with the updated critics
        with torch.no_grad():
            qr_data = torch.min(*self.pairs[0](obs, act))
            obs_rep = obs.unsqueeze(1).repeat(1, S, 1).reshape(B * S, -1)
            act_s = self.actor.sample(obs_rep, eps_samp)
            adv = qr_data - self._sample_value(self.pairs[0], obs_rep, act_s, S)
            if self.ccrr:
                qc_data = torch.min(*self.pairs[1](obs, act))
                mean_qc = self._sample_value(self.pairs[0 if ref else 1], obs_rep, act_s, S)
                arg = (adv - self.lam.detach() * (qc_data - mean_qc)) / self.beta
                w = torch.clamp(torch.exp(arg), 0, 1e10)
            else:
                arg = adv / self.beta
                w = torch.exp(arg)
        self.last = {'arg': arg.clone(), 'w': w.clone(), 'done': done.reshape(-1).clone()}
        loss = (w * -self.actor.log_prob(obs, act)).mean()
        loss.backward()
        self.opt_actor.step()
        out['Loss/Loss_actor'] = loss.item()
        out['Qr/current_Qr'] = qr_data[0].item()
        out['Train/PolicyStd'] = torch.exp(self.actor.log_std).mean().item()
        if self.ccrr:
            if lagrange_open:
                (-self.lam * (mean_qc.mean().item() - self.cost_limit)).backward()
                self.opt_lam.step()
                with torch.no_grad():
                    self.lam.clamp_(min=0.0)
            out['Qc/current_Qc'] = qc_data[0].item()
            out['Metrics/LagrangeMultiplier'] = self.lam.item()
        with torch.no_grad():
            for pair, target in zip(self.pairs, self.targets):
                for tp, p in zip(target.named().values(), pair.named().values()):
                    tp.copy_(self.polyak * p + (1 - self.polyak) * tp)
        return out


def gather(data, idx):
    """dataset.py:237-247 with given indices: the six fields' rows."""
    return tuple(np.asarray(data[k])[np.asarray(idx)] for k in ('obs', 'action', 'reward', 'cost', 'next_obs', 'done'))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a - b))


def random_problem(rng, D, A, actor_hidden, critic_hidden, N, pairs, done_mode='mixed'):
    """State dicts (non-trivial, float32-valued) and a dataset for a case of the table."""
    def mlp(sizes, prefix, sd):
        for j in range(len(sizes) - 1):
            bound = 1.0 / math.sqrt(sizes[j])
            sd[f'{prefix}.{2 * j}.weight'] = torch.from_numpy(
                rng.uniform(-bound, bound, (sizes[j + 1], sizes[j])).astype(np.float32))
            sd[f'{prefix}.{2 * j}.bias'] = torch.from_numpy(rng.uniform(-bound, bound, sizes[j + 1]).astype(np.float32))
    actor = OrderedDict(log_std=torch.from_numpy(rng.uniform(-0.5, 0.2, A).astype(np.float32)))
    mlp([D] + list(actor_hidden) + [A], 'mean', actor)
    pair_sds = []
    for _ in range(pairs):
        sd = OrderedDict()
        for c in range(2):
            mlp([D + A] + list(critic_hidden) + [1], f'critic_{c}.0', sd)
        pair_sds.append(sd)
    done = {'zeros': np.zeros((N, 1)), 'ones': np.ones((N, 1)),
            'mixed': (rng.random((N, 1)) < 0.4).astype(np.float64)}[done_mode]
    if done_mode == 'mixed' and N > 1:
        done[0], done[-1] = 1.0, 0.0
    data = {'obs': rng.standard_normal((N, D)), 'action': rng.uniform(-1, 1, (N, A)),
            'reward': rng.standard_normal((N, 1)), 'cost': (rng.random((N, 1)) < 0.3) * 1.0,
            'next_obs': rng.standard_normal((N, D)), 'done': done}
    return actor, pair_sds, {k: v.astype(np.float32) for k, v in data.items()}


def perturbed(sd, rng, scale):
    """A state dict of the same names with small random float32 values (Adam moments, moved targets)."""
    return OrderedDict((k, torch.from_numpy((rng.standard_normal(tuple(v.shape)) * scale).astype(np.float32)))
                       for k, v in sd.items())


CASES = {  # obs, act, actor hidden, critic hidden, actor activation, critic activation, B, S, N
    'tiny': (7, 3, [24, 40], [24, 40], 'relu', 'relu', 5, 3, 37),
    'one': (33, 1, [96], [96], 'tanh', 'tanh', 1, 1, 1),
    'tile': (60, 2, [64, 64, 64], [64, 64, 64], 'relu', 'relu', 70, 3, 500),
    'yaml': (28, 2, [256, 256, 256], [256, 256, 256], 'relu', 'relu', 256, 10, 4096),
    'mixed': (17, 6, [48, 32], [40], 'tanh', 'relu', 9, 2, 64),
}

ADAM_T0 = 3  # Adam steps every optimiser has behind it at the start of a run
HP = dict(gamma=0.99, beta=1.0, polyak=0.005, lr_actor=1e-3, lr_critic=1e-3)
LAG = dict(cost_limit=0.1, lambda_lr=0.05, lambda_init=0.7)
CLAMP_SEED, CLAMP_Q_SCALE = 15, 20.0  # `tiny`, beta 0.05: the float64 advantage / beta passes 23.03 on a row, 60 on none


def _spec(case, algo, nsteps, done_mode='mixed', seed=0, wiring='intended', open_=True, q_scale=1.0, **hp):
    pairs = 2 if algo == 'CCRR' else 1
    full = dict(HP, **(LAG if pairs == 2 else {}))
    full.update(hp)
    return {'run': dict(case=case, pairs=pairs, nsteps=nsteps, done_mode=done_mode, seed=seed, q_scale=q_scale), 'wiring': wiring,
            'open': open_, 'hp': full}


def run_table():
    """name -> what a compared run is: the table the float32 error file and the GPU tests share."""
    t = {}
    for case in CASES:
        for algo in ('CRR', 'CCRR'):
            for n in (1, 8):
                t[f'{case}/{algo}/{n}'] = _spec(case, algo, n)
    for mode in ('zeros', 'ones'):
        t[f'tiny/CCRR/done-{mode}'] = _spec('tiny', 'CCRR', 2, done_mode=mode)
    t['tiny/CRR/clamp'] = _spec('tiny', 'CRR', 1, seed=CLAMP_SEED, q_scale=CLAMP_Q_SCALE, open_=False, beta=0.05)
    t['tiny/CCRR/clamp'] = _spec('tiny', 'CCRR', 1, seed=CLAMP_SEED, q_scale=CLAMP_Q_SCALE, open_=False, beta=0.05,
                                lambda_init=0.0)
    t['tiny/CCRR/lambda-closed'] = _spec('tiny', 'CCRR', 8, open_=False)
    t['tiny/CCRR/lambda-open'] = _spec('tiny', 'CCRR', 8)
    t['tiny/CCRR/lambda-zero'] = _spec('tiny', 'CCRR', 8, cost_limit=1e3, lambda_lr=0.5, lambda_init=0.3)
    t['tiny/CCRR/reference-wiring'] = _spec('tiny', 'CCRR', 3, wiring='reference')
    return t


def twin_of(spec, dtype, perm=None):
    """`(run, twin after the run, per-step scalars)` of a table entry at a dtype."""
    run = make_run(**spec['run'])
    tw = make_twin(run, dtype, wiring=spec['wiring'], **spec['hp'])
    return run, tw, run_twin(tw, run, lagrange_open=spec['open'], perm=perm)


def make_run(case, pairs, nsteps, done_mode='mixed', seed=0, q_scale=1.0):
    """Everything a run of `nsteps` chained steps of a case starts from, float32-valued: parameters, moved targets,
    non-zero Adam state, the dataset and the injected draws.  `q_scale` multiplies the critics' last layer (wider
    advantages: the clamp case)."""
    D, A, a_h, c_h, a_act, c_act, B, S, N = CASES[case]
    rng = np.random.default_rng([seed, zlib.crc32(case.encode()), pairs, nsteps])
    actor, pair_sds, data = random_problem(rng, D, A, a_h, c_h, N, pairs, done_mode)
    for sd in pair_sds:
        for k in sd:
            if k.endswith(f'.{2 * len(c_h)}.weight'):
                sd[k] = sd[k] * np.float32(q_scale)
    targets = [OrderedDict((k, v + t) for (k, v), t in zip(sd.items(), perturbed(sd, rng, 0.02).values()))
               for sd in pair_sds]
    def moments(sd):
        return perturbed(sd, rng, 0.01), OrderedDict((k, v.abs() * 0.01 + 1e-6) for k, v in perturbed(sd, rng, 0.01).items())
    return {'case': case, 'pairs': pairs, 'nsteps': nsteps, 'actor': actor, 'pair_sds': pair_sds, 'targets': targets,
            'adam_actor': moments(actor), 'adam_pairs': [moments(sd) for sd in pair_sds], 'data': data,
            'idx': rng.integers(0, N, (nsteps, B)), 'eps_next': rng.standard_normal((nsteps, B, A)).astype(np.float32),
            'eps_next_c': rng.standard_normal((nsteps, B, A)).astype(np.float32),
            'eps_samp': rng.standard_normal((nsteps, B * S, A)).astype(np.float32)}


def make_twin(run, dtype, wiring='intended', **hp):
    _, _, _, _, a_act, c_act, _, _, _ = CASES[run['case']]
    tw = Twin(run['actor'], run['pair_sds'], a_act, c_act, dtype=dtype, wiring=wiring, target_sds=run['targets'], **hp)
    tw.opt_actor = Adam(tw.actor.named(), tw.opt_actor.lr, dtype, *run['adam_actor'], t=ADAM_T0)
    tw.opt_pairs = [Adam(p.named(), o.lr, dtype, *mv, t=ADAM_T0)
                    for p, o, mv in zip(tw.pairs, tw.opt_pairs, run['adam_pairs'])]
    return tw


def run_twin(tw, run, lagrange_open=False, perm=None):
    """The run's chained steps on a twin; `perm`: a permutation of the batch rows (row 0 stays: the first-row
    statistics are of that row).  Returns the per-step scalars."""
    B = run['idx'].shape[1]
    S = run['eps_samp'].shape[1] // B
    p = np.arange(B) if perm is None else np.asarray(perm)
    ps = (p[:, None] * S + np.arange(S)[None, :]).reshape(-1)
    return [tw.step(gather(run['data'], run['idx'][k][p]), run['eps_next'][k][p], run['eps_samp'][k][ps],
                    run['eps_next_c'][k][p], lagrange_open) for k in range(run['nsteps'])]


def snapshot(tw):
    """name -> float64 numpy: parameters, targets, Adam moments, the multiplier."""
    out = {}
    def put(prefix, named):
        for k, v in named.items():
            out[f'{prefix}/{k}'] = v.detach().double().numpy().copy()
    put('actor', tw.actor.named())
    put('actor_m', tw.opt_actor.m)
    put('actor_v', tw.opt_actor.v)
    for i, (p, t, o) in enumerate(zip(tw.pairs, tw.targets, tw.opt_pairs)):
        put(f'pair{i}', p.named())
        put(f'target{i}', t.named())
        put(f'pair{i}_m', o.m)
        put(f'pair{i}_v', o.v)
    if tw.ccrr:
        out['lagrange/lambda'] = np.array([tw.lam.item()])
    return out


def error_table(snap, stats, snap64, stats64):
    """quantity -> error against the float64 twin: relative L2 per tensor, relative per scalar (worst step)."""
    err = {k: rel_l2(snap[k], snap64[k]) for k in snap64}
    for key in stats64[0]:
        err[f'scalar/{key}'] = max(abs(a[key] - b[key]) / abs(b[key]) if b[key] != 0 else abs(a[key])
                                   for a, b in zip(stats, stats64))
    return err


def pack_errors(err):
    """quantity -> error as the error file keeps it: group (the part before the first '/') -> the values of its
    quantities in sorted order, three digits."""
    out = {}
    for q in sorted(err):
        out.setdefault(q.split('/', 1)[0], []).append(float(f'{err[q]:.3g}'))
    return out


def unpack_errors(packed, quantities):
    """The inverse for a known set of quantity names; a KeyError / AssertionError where file and names disagree."""
    groups = {}
    for q in sorted(quantities):
        groups.setdefault(q.split('/', 1)[0], []).append(q)
    assert sorted(groups) == sorted(packed), sorted(set(groups) ^ set(packed))
    out = {}
    for g, names in groups.items():
        assert len(names) == len(packed[g]), g
        out.update(zip(names, packed[g]))
    return out


__all__ = ['pack_errors', 'unpack_errors', 'Twin', 'Adam', 'draw_idx', 'draw_eps', 'gather', 'rel_l2', 'random_problem', 'perturbed', 'CASES',
           'KEY_NEXT', 'KEY_NEXTC', 'KEY_SAMP', 'make_run', 'make_twin', 'run_twin', 'snapshot', 'error_table',
           'ADAM_T0']
