"""A plain torch restatement of ``coptidice.py:162-290`` with ``torch.optim.Adam``: the twin that tests/test_dice_cpu.py
holds to the unmodified reference and tests/test_dice_gpu.py holds the device step to.  Runs in any dtype from the same
weights, dataset and injected row indices."""
import functools

import torch
from test_vae_gpu import mlp

NETS = ('nu', 'chi', 'actor')
FNS = ('kl', 'softchi', 'chisquare')
STEPS, GAMMA, ALPHA, COST_LIMIT, COST_UB_EPS, LAMB0, TAU_INIT = 3, 0.99, 0.5, 0.3, 0.05, 0.7, 0.5
LR = {'nu': 1e-3, 'chi': 2e-3, 'actor': 1.5e-3, 'lamb': 0.035, 'tau': 0.003}
# name: D, A, hidden of nu / chi / actor, activation, B, generator seed (chosen so that every branch is taken: below)
CASES = {'one': (3, 1, [8], [8], [8], 'tanh', 1, 0),
         'ragged': (5, 3, [40, 24], [24], [24, 40], 'relu', 7, 0),
         'tiles': (12, 2, [64, 64, 64], [64, 64, 64], [64, 64, 64], 'relu', 43, 0),
         'edge': (12, 2, [256, 256], [256, 256], [256, 256], 'softplus', 4, 0)}


@functools.lru_cache(maxsize=None)
def make_run(name):
    """Weights of the three networks, a dataset with ``init_obs`` and the row indices of STEPS steps, on the CPU."""
    from omnisafe_amd.crr_step import _init_mlp

    D, A, hn, hc, ha, act, B, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(11)
    run = dict(D=D, A=A, act=act, B=B, hidden={'nu': hn, 'chi': hc, 'actor': ha})
    for net, hid, out, prefix in (('actor', ha, A, 'mean'), ('nu', hn, 1, 'net'), ('chi', hc, 1, 'net')):
        sd = {'log_std': torch.full((A,), -0.3)} if net == 'actor' else {}
        for j, (w, b) in enumerate(_init_mlp([D] + hid + [out], 'kaiming_uniform')):
            sd[f'{prefix}.{2 * j}.weight'], sd[f'{prefix}.{2 * j}.bias'] = w, b
        run[net] = sd
    N = 3 * B + 5
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    run['data'] = {'obs': rn(N, D), 'action': torch.tanh(rn(N, A)), 'reward': rn(N, 1), 'cost': rn(N, 1).abs(),
                   'next_obs': rn(N, D), 'done': (torch.rand(N, 1, generator=g) < 0.3).float(), 'init_obs': rn(N, D)}
    run['idx'] = torch.randint(0, N, (STEPS, B), generator=g)
    return run


def divergence(fn):
    """coptidice.py:296-323."""
    if fn == 'kl':
        return (lambda x: x * torch.log(x + 1e-10)), (lambda x: torch.exp(x - 1))
    if fn == 'softchi':
        return (lambda x: torch.where(x < 1, x * (torch.log(x + 1e-10) - 1) + 1, 0.5 * (x - 1) ** 2),
                lambda x: torch.where(x < 0, torch.exp(torch.min(x, torch.zeros_like(x))), x + 1))
    return (lambda x: 0.5 * (x - 1) ** 2), (lambda x: x + 1)


def chi_gradient(ell, tau):
    """d mean(softmax(ell / tau) B ell) / d ell in closed form: (1 / B) weights_j (1 + (ell_j - sum_i p_i ell_i) / tau)."""
    p = torch.softmax(ell / tau, dim=0)
    return p * (1 + (ell - (p * ell).sum()) / tau)


def twin(run, fn, dtype, lamb0=LAMB0, tau_init=TAU_INIT, cost_limit=COST_LIMIT, eps=COST_UB_EPS):
    """``(tensors, stats [STEPS][10], branches)``: every parameter, both Adam moments, lambda and tau after STEPS steps;
    the statistics rows in dice_step.STAT_KEYS' order; which branches of f, f_inv and the relu the rows took."""
    f, f_inv = divergence(fn)
    p = {n: {k: v.to(dtype).clone().requires_grad_() for k, v in run[n].items()} for n in NETS}
    lamb = torch.tensor(lamb0, dtype=torch.float32).clamp(0, 1e3).to(dtype).requires_grad_()
    tau = (torch.tensor(tau_init, dtype=torch.float32) + 1e-6).to(dtype).requires_grad_()
    opt = {n: torch.optim.Adam(list(p[n].values()), lr=LR[n]) for n in NETS}
    opt.update(lamb=torch.optim.Adam([lamb], lr=LR['lamb']), tau=torch.optim.Adam([tau], lr=LR['tau']))
    L = {n: len(run['hidden'][n]) + 1 for n in NETS}
    net = lambda n, x: mlp(p[n], 'net', L[n], x, run['act']).squeeze(-1)  # noqa: E731
    stats, seen = [], set()
    for s in range(STEPS):
        d = {k: v[run['idx'][s]].to(dtype) for k, v in run['data'].items()}
        obs, nobs, iobs = d['obs'], d['next_obs'], d['init_obs']
        r, c, done, B = d['reward'][:, 0], d['cost'][:, 0], d['done'][:, 0], run['B']
        adv = lambda: r - lamb.item() * c + (1 - done) * GAMMA * net('nu', nobs) - net('nu', obs)  # noqa: E731
        w_of = lambda a: torch.relu(f_inv(a / ALPHA))  # noqa: E731
        a = adv()
        w = w_of(a)
        x = (a / ALPHA).detach()
        seen |= {('x<0', bool(v)) for v in x < 0} | {('w<1', bool(v)) for v in w.detach() < 1}
        seen |= {('relu', bool(v)) for v in f_inv(x) > 0}
        nu_loss = (1 - GAMMA) * net('nu', iobs).mean() - ALPHA * f(w).mean() + (w * a).mean()
        wd = w.detach()
        ell = (1 - GAMMA) * net('chi', iobs) + wd * (c + GAMMA * (1 - done) * net('chi', nobs) - net('chi', obs))
        logit = ell / tau.item()
        weights = torch.softmax(logit, dim=0) * B
        log_weights = torch.log_softmax(logit, dim=0) + torch.log(torch.as_tensor(B)).to(dtype)
        kl = (weights * log_weights - weights + 1).mean()
        cost_ub = (wd * c).mean()
        chi_loss = (weights * ell).mean()
        tau_loss = -tau * (kl.detach() - eps)
        lamb_loss = -(lamb * (cost_ub.detach() - cost_limit)).mean()
        for n, loss in (('nu', nu_loss), ('chi', chi_loss), ('lamb', lamb_loss), ('tau', tau_loss)):
            opt[n].zero_grad()
            loss.backward()
            opt[n].step()
        lamb.data.clamp_(min=0, max=1e3)
        tau.data.clamp_(min=1e-6)
        dist = torch.distributions.Normal(mlp(p['actor'], 'mean', L['actor'], obs, run['act']), p['actor']['log_std'].exp())
        with torch.no_grad():
            w4 = w_of(adv())
        policy_loss = -(w4 * dist.log_prob(d['action']).sum(-1)).mean()
        opt['actor'].zero_grad()
        policy_loss.backward()
        opt['actor'].step()
        stats.append([float(v.detach()) for v in (nu_loss, chi_loss, lamb_loss, tau_loss, cost_ub, kl, tau, lamb, policy_loss,
                                         p['actor']['log_std'].exp().mean())])
    out = {'lambda': lamb.detach().double().reshape(1).numpy(), 'tau': tau.detach().double().reshape(1).numpy()}
    for n in NETS:
        for k, v in p[n].items():
            out[f'p/{n}/{k}'] = v.detach().double().numpy()
            out[f'm/{n}/{k}'] = opt[n].state[v]['exp_avg'].double().numpy()
            out[f'v/{n}/{k}'] = opt[n].state[v]['exp_avg_sq'].double().numpy()
    return out, torch.tensor(stats, dtype=torch.float64).numpy(), seen


def branches_wanted(fn):
    """What a case's rows must reach between them: both sides of softchi's branches, and (chisquare) of the relu."""
    return {'kl': set(), 'softchi': {('x<0', True), ('x<0', False), ('w<1', True), ('w<1', False)},
            'chisquare': {('relu', True), ('relu', False)}}[fn]
