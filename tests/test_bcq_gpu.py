"""GPU: offline BCQ / BCQ-Lag (csrc/bcq_kernels.hip through bcq_step.BcqStep) against a plain torch restatement of
``bcq.py:_train`` / ``bcq_lag.py:_train`` run on the CPU in float64, on both routes of ``OSA_BCQ_CHAIN``: the target
chain and ``predict`` alone, three train steps with injected draws, the draws against their numpy restatement,
determinism, graph replay, and both algorithms end to end through ``omnisafe_amd.Agent``.

Tolerance: error <= K * max(e32, 2^-22) with the project's K = 16 and e32 the error of the same restatement run in
float32 against the float64 run -- relative L2 per tensor, relative per scalar (worst step).  Nothing is excluded.  With
OSA_WRITE_PROFILES=1 the ratios go to profiles/bcq_twin_error.md.
"""
import functools
import os

import numpy as np
import pytest
import torch
from test_vae_gpu import mlp, normal, philox  # the restated layers and the draws' formulas

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K, FLOOR, LR, STEPS = 16.0, 2.0 ** -22, 1e-3, 3
GAMMA, COST_GAMMA, POLYAK, PHI, COST_LIMIT, LAMBDA_LR, LAMBDA0 = 0.99, 0.97, 0.005, 0.05, 0.1, 0.05, 0.7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: D, A, actor hidden, critic hidden, activation, B, S
CASES = {'one': (3, 1, [8], [8], 'tanh', 1, 1),
         'ragged': (5, 3, [40, 24], [24, 40], 'relu', 7, 5),
         'blocks': (12, 2, [64, 64, 64], [64, 64, 64], 'relu', 13, 10),
         'edge': (12, 2, [256, 256], [256, 256], 'softplus', 4, 3),
         'over': (12, 2, [300], [300], 'relu', 4, 3)}
# variant: pairs, gate open, minimum_weighting
VARIANTS = {'bcq': (1, False, 0.75), 'lag-open': (2, True, 0.75), 'lag-closed': (2, False, 0.75), 'w1': (1, False, 1.0)}
_RATIOS = {}


def make_desc(name, pairs=2):
    from omnisafe_amd import bcq_step

    D, A, ah, ch, act, B, S = CASES[name]
    return bcq_step.make_desc(D, A, ah, ch, act, act, B, S, pairs)


@functools.lru_cache(maxsize=None)
def make_run(name):
    """Weights of the actor and of two critic pairs, a dataset and the draws of STEPS steps, all on the CPU."""
    from omnisafe_amd import bcq_step, vae_step

    D, A, ah, ch, act, B, S = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    torch.manual_seed(11)
    desc = make_desc(name)
    actor = {f'vae.{k}': v for k, v in vae_step.initial_state_dict(bcq_step.vae_desc_of(desc)).items()}
    nets = [('perturbation', [D + A] + ah + [A], actor)]
    pairs = [{}, {}]
    nets += [(f'critic_{c}.0', [D + A] + ch + [1], pairs[p]) for p in range(2) for c in range(2)]
    for prefix, sizes, dst in nets:
        for j, (w, b) in enumerate(bcq_step._init_mlp(sizes, 'kaiming_uniform')):
            dst[f'{prefix}.{2 * j}.weight'], dst[f'{prefix}.{2 * j}.bias'] = w, b
    N = 3 * B + 5
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    data = {'obs': rn(N, D), 'action': torch.tanh(rn(N, A)), 'reward': rn(N, 1), 'cost': rn(N, 1).abs(),
            'next_obs': rn(N, D), 'done': (torch.rand(N, 1, generator=g) < 0.3).float()}
    draws = dict(idx=torch.randint(0, N, (STEPS, B), generator=g), z_r=rn(STEPS, B * S, 2 * A),
                 z_c=rn(STEPS, B * S, 2 * A), eps=rn(STEPS, B, 2 * A), z_a=rn(STEPS, B, 2 * A))
    return dict(D=D, A=A, La=len(ah) + 1, Lq=len(ch) + 1, act=act, B=B, S=S, actor=actor, pairs=pairs, data=data, **draws)


def predict(run, p, obs, z):
    """PerturbationActor.predict (perturbation_actor.py:76-90) with the given latent."""
    act = mlp(p, 'vae.decoder', run['La'], torch.cat([obs, z], -1), run['act'])
    return act + PHI * torch.tanh(mlp(p, 'perturbation', run['La'], torch.cat([obs, act], -1), run['act']))


def qpair(run, p, obs, a):
    return [mlp(p, f'critic_{c}.0', run['Lq'], torch.cat([obs, a], -1), run['act']) for c in range(2)]


def chain(run, pa, pt, obs, z, w):
    q1, q2 = qpair(run, pt, obs, predict(run, pa, obs, z))
    return w * torch.min(q1, q2) + (1 - w) * torch.max(q1, q2)


def restatement(run, variant, dtype):
    """bcq.py:122-213 / bcq_lag.py:91-193 with torch.optim.Adam per optimiser and common/lagrange.py's update."""
    npairs, gate, w = VARIANTS[variant]
    leaf = lambda sd: {k: v.to(dtype).clone().requires_grad_() for k, v in sd.items()}  # noqa: E731
    pa, crit = leaf(run['actor']), [leaf(sd) for sd in run['pairs'][:npairs]]
    targ = [{k: v.detach().clone() for k, v in c.items()} for c in crit]
    opt_vae = torch.optim.Adam([v for k, v in pa.items() if k.startswith('vae.')], lr=LR)
    opt_act = torch.optim.Adam([v for k, v in pa.items() if k.startswith('perturbation.')], lr=LR)
    opt_c = [torch.optim.Adam(list(c.values()), lr=LR) for c in crit]
    lam = torch.tensor(LAMBDA0, dtype=dtype, requires_grad=True)
    opt_l = torch.optim.Adam([lam], lr=LAMBDA_LR)
    stats = np.zeros((STEPS, 13))
    for s in range(STEPS):
        b = {k: v[run['idx'][s]].to(dtype) for k, v in run['data'].items()}
        for u in range(npairs):
            with torch.no_grad():
                nobs = torch.repeat_interleave(b['next_obs'], run['S'], dim=0)
                qt = chain(run, pa, targ[u], nobs, run['z_c' if u else 'z_r'][s].to(dtype), w)
                qt = qt.reshape(run['B'], -1).max(dim=1)[0].reshape(-1, 1)
                y = (b['cost' if u else 'reward'] + (1 - b['done']) * (COST_GAMMA if u else GAMMA) * qt).squeeze(1)
            q1, q2 = (q.squeeze(-1) for q in qpair(run, crit[u], b['obs'], b['action']))
            loss = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
            opt_c[u].zero_grad()
            loss.backward()
            opt_c[u].step()
            stats[s, 3 + 3 * u:6 + 3 * u] = loss.item(), q1[0].item(), y[0].item()
        mean, raw = torch.chunk(mlp(pa, 'vae.encoder', run['La'], torch.cat([b['obs'], b['action']], -1), run['act']), 2, -1)
        dist = torch.distributions.Normal(mean, torch.clamp(raw, min=-20, max=2).exp())
        z = dist.mean + run['eps'][s].to(dtype) * dist.stddev
        recon = torch.nn.functional.mse_loss(mlp(pa, 'vae.decoder', run['La'], torch.cat([b['obs'], z], -1), run['act']),
                                             b['action'])
        kl = torch.distributions.kl.kl_divergence(dist, torch.distributions.Normal(0, 1)).mean()
        opt_vae.zero_grad()
        (recon + kl).backward()
        opt_vae.step()
        a = predict(run, pa, b['obs'], run['z_a'][s].to(dtype))
        qr = qpair(run, crit[0], b['obs'], a)[0]
        qc = qpair(run, crit[1], b['obs'], a)[0] if npairs == 2 else torch.zeros_like(qr)
        loss_a = -(qr - (lam.item() if npairs == 2 else 0.0) * qc).mean()
        opt_act.zero_grad()
        loss_a.backward()
        opt_act.step()
        if gate:  # common/lagrange.py:104-117
            opt_l.zero_grad()
            (-lam * (qc.mean().item() - COST_LIMIT)).backward()
            opt_l.step()
            lam.data.clamp_(0.0)
        with torch.no_grad():
            for c, t in zip(crit, targ):
                for k in t:
                    t[k].copy_(POLYAK * c[k] + (1 - POLYAK) * t[k])
        stats[s, :3] = (recon + kl).item(), recon.item(), kl.item()
        stats[s, 9:11] = loss_a.item(), qr[0].item()
        if npairs == 2:
            stats[s, 11:13] = qc[0].item(), lam.item()
    out = {'lambda': np.array([lam.item()])}
    for name, p, opt in [('actor', pa, None)] + [(f'pair{u}', c, opt_c[u]) for u, c in enumerate(crit)]:
        for k, v in p.items():
            o = opt or (opt_vae if k.startswith('vae.') else opt_act)
            out[f'p/{name}/{k}'] = v.detach().double().numpy()
            out[f'm/{name}/{k}'] = o.state[v]['exp_avg'].double().numpy()
            out[f'v/{name}/{k}'] = o.state[v]['exp_avg_sq'].double().numpy()
    for u, t in enumerate(targ):
        out.update({f't/pair{u}/{k}': v.double().numpy() for k, v in t.items()})
    return out, stats


def errors(t, stats, t64, s64):
    err = {q: float(np.linalg.norm(t[q] - t64[q]) / np.linalg.norm(t64[q])) for q in t64}
    for c in np.flatnonzero(np.abs(s64).sum(0)):
        err[f'stat{c}'] = float(np.max(np.abs(stats[:, c] - s64[:, c]) / np.abs(s64[:, c])))
    return err


@functools.lru_cache(maxsize=None)
def reference(name, variant):
    """The float64 restatement and the float32 restatement's own error, shared by both routes."""
    run = make_run(name)
    t64, s64 = restatement(run, variant, torch.float64)
    return t64, s64, errors(*restatement(run, variant, torch.float32), t64, s64)


def device_step(name, variant, route, nslots=STEPS):
    from omnisafe_amd import bcq_step

    run, (npairs, _, w) = make_run(name), VARIANTS[variant]
    st = bcq_step.BcqStep(make_desc(name, npairs), {k: v.to(DEV) for k, v in run['data'].items()}, gamma=GAMMA,
                          polyak=POLYAK, phi=PHI, minimum_weighting=w, lr_actor=LR, lr_critic=LR, nslots=nslots,
                          cost_gamma=COST_GAMMA, cost_limit=COST_LIMIT, lambda_lr=LAMBDA_LR, lambda_init=LAMBDA0,
                          route=route, device=DEV)
    st.load_state_dict(run['actor'])
    for u in range(npairs):
        st.load_critic_state_dict(u, run['pairs'][u])
    st.target.copy_(st.critic)
    st.set_draws(0, run['idx'], run['z_r'], run['eps'], run['z_a'], run['z_c'])
    return st


def device_tensors(st):
    out = {'lambda': st.lagrange[:1].double().cpu().numpy()}
    for tag, which, cwhich in (('p', '', 'critic'), ('m', '_m', 'critic_m'), ('v', '_v', 'critic_v')):
        out.update({f'{tag}/actor/{k}': v.double().cpu().numpy() for k, v in st.state_dict(which).items()
                    if k != '_phi' and not k.startswith('vae._')})
        for u in range(st.pairs):
            out.update({f'{tag}/pair{u}/{k}': v.double().cpu().numpy() for k, v in st.critic_state_dict(u, cwhich).items()})
    for u in range(st.pairs):
        out.update({f't/pair{u}/{k}': v.double().cpu().numpy() for k, v in st.critic_state_dict(u, 'target').items()})
    return out


def check(tag, err, e32):
    ratios = _RATIOS[tag] = {q: err[q] / max(e32[q], FLOOR) for q in err}
    for q in sorted(ratios):
        print(f'{tag} {q}: error {err[q]:.3e} e32 {e32[q]:.3e} ratio {ratios[q]:.2f}')
    bad = {q: r for q, r in ratios.items() if not r <= K}
    assert not bad, bad


SUPPORTED = [n for n in CASES if n != 'over']


@pytest.mark.parametrize('route', ['layer', 'fused'])
@pytest.mark.parametrize('name', SUPPORTED)
def test_chain_against_float64(name, route):
    """``target_q`` of both pairs and ``predict`` at 1, 35 and 130 plain rows with given latents."""
    run = make_run(name)
    st = device_step(name, 'lag-closed', route)
    g = torch.Generator().manual_seed(3)
    obs = {n: torch.randn(n, run['D'], generator=g) for n in (1, 35, 130)}
    z = {n: torch.randn(n, 2 * run['A'], generator=g) for n in (1, 35, 130)}
    nobs = torch.repeat_interleave(run['data']['next_obs'][run['idx'][0]], run['S'], dim=0)
    got = {f'predict{n}': st.predict(obs[n].to(DEV), z[n].to(DEV)) for n in obs}
    got.update({f'target_q{u}': st.target_q(u, run['z_c' if u else 'z_r'][0]) for u in range(2)})
    ref = {}
    for dtype in (torch.float64, torch.float32):
        pa = {k: v.to(dtype) for k, v in run['actor'].items()}
        with torch.no_grad():
            ref[dtype] = {f'predict{n}': predict(run, pa, obs[n].to(dtype), z[n].to(dtype)).double() for n in obs}
            for u in range(2):
                pt = {k: v.to(dtype) for k, v in run['pairs'][u].items()}
                ref[dtype][f'target_q{u}'] = chain(run, pa, pt, nobs.to(dtype), run['z_c' if u else 'z_r'][0].to(dtype),
                                                   0.75).squeeze(-1).double()
    r64 = ref[torch.float64]
    rel = lambda x, q: float((x - r64[q]).norm() / r64[q].norm())  # noqa: E731
    check(f'chain/{name}/{route}', {q: rel(got[q].double().cpu(), q) for q in r64},
          {q: rel(ref[torch.float32][q], q) for q in r64})


def test_predict_determinism():
    st = device_step('ragged', 'bcq', None)
    obs = torch.randn(35, 5, generator=torch.Generator().manual_seed(1)).to(DEV)
    a, b, c = (st.predict(obs, None, seed=s) for s in (3, 3, 4))
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all()


@pytest.mark.parametrize('route', ['layer', 'fused'])
@pytest.mark.parametrize('variant', ['bcq', 'lag-open', 'lag-closed'])
@pytest.mark.parametrize('name', SUPPORTED)
def test_steps_against_float64(name, variant, route):
    steps_against_float64(name, variant, route)


@pytest.mark.parametrize('route', ['layer', 'fused'])
def test_steps_minimum_weighting_one(route):
    steps_against_float64('ragged', 'w1', route)


def steps_against_float64(name, variant, route):
    t64, s64, e32 = reference(name, variant)
    st = device_step(name, variant, route)
    st.run(STEPS, lagrange_open=VARIANTS[variant][1])
    assert st.steps.tolist() == [STEPS, STEPS] and st.adam_step.tolist() == [STEPS, STEPS] + [STEPS] * st.pairs + [0] * (2 - st.pairs)
    check(f'{name}/{variant}/{route}', errors(device_tensors(st), st.stats[:, :13].double().cpu().numpy(), t64, s64), e32)
    lay = st.layout  # padding lanes stay zero, the dataset keeps its bits
    pads = [(~lay.vae.real_mask(), (st.vae, st.vae_m, st.vae_v)), (~lay.real_mask(0), (st.pert, st.pert_m, st.pert_v)),
            (~lay.real_mask(1), (st.critic.T, st.critic_m.T, st.critic_v.T, st.target.T))]
    for mask, blocks in pads:
        for blk in blocks:
            assert not blk[torch.from_numpy(mask).to(DEV)].any()
    for k, v in make_run(name)['data'].items():
        assert torch.equal(st.data[k].cpu(), v), k


def test_over_falls_back_to_layer_and_refuses_fused():
    from omnisafe_amd import _lib, bcq_step

    assert device_step('over', 'bcq', None).route == bcq_step.ROUTES['layer']
    with pytest.raises(_lib.OsaError):
        device_step('over', 'bcq', 'fused')
    steps_against_float64('over', 'lag-open', None)


@pytest.fixture(scope='module', autouse=True)
def write_profile():
    yield
    if os.environ.get('OSA_WRITE_PROFILES') == '1' and _RATIOS:
        with open(os.path.join(ROOT, 'profiles', 'bcq_twin_error.md'), 'w', encoding='utf-8') as f:
            f.write('# BCQ / BCQ-Lag: error / max(e32, 2^-22) against the float64 restatement (bound 16)\n\n')
            f.write('| case/variant/route | quantities | worst | worst quantity |\n|---|---|---|---|\n')
            for name, r in _RATIOS.items():
                q = max(r, key=r.get)
                f.write(f'| {name} | {len(r)} | {r[q]:.2f} | {q} |\n')


def test_replay_and_determinism():
    eager, again, graphed = (device_step('ragged', 'lag-open', None) for _ in range(3))
    eager.run(3, lagrange_open=True)
    again.run(3, lagrange_open=True)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        graphed.run(1, lagrange_open=True)
        graph.capture_end()
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for other in (again, graphed):
        for blk in ('vae', 'vae_m', 'vae_v', 'pert', 'pert_m', 'pert_v', 'critic', 'critic_m', 'critic_v', 'target',
                    'lagrange', 'stats', 'steps'):
            assert torch.equal(getattr(eager, blk), getattr(other, blk)), blk


def test_draws_equal_numpy():
    st = device_step('ragged', 'lag-open', None, nslots=8)
    seed, first, n, N = 0x1234ABCD5678, 7, 5, st.n_rows
    st.draw(seed, first, n)
    for k in range(n):
        step, slot = first + k, (first + k) % 8
        w = philox(seed ^ 0x42435149445831, step, np.arange(st.B))
        assert st.idx[slot].tolist() == [((int(a) | (int(b) << 32)) * N) >> 64 for a, b in zip(w[0], w[1])]
        for buf, key in ((st.z_r, 0x4243515A523031), (st.z_c, 0x4243515A433031), (st.eps, 0x42435145505331),
                         (st.z_a, 0x4243515A413031)):
            w = philox(seed ^ key, step, np.arange(buf[slot].numel()))
            assert np.array_equal(buf[slot].cpu().numpy().reshape(-1), normal(w[0], w[1]))


@pytest.mark.parametrize('algo', ['BCQ', 'BCQLag'])
def test_agent_end_to_end(algo, tmp_path):
    import csv

    import omnisafe_amd
    from omnisafe_amd import bcq_step, offline
    from omnisafe_amd.saved_policy import device_env_class, load_checkpoint

    D, A = device_env_class('SynthReach-v0').dims('SynthReach-v0')
    rng = np.random.default_rng(5)
    obs = rng.standard_normal((2000, D)).astype(np.float32)
    W = rng.standard_normal((D, A)).astype(np.float32) / np.sqrt(D)
    arrays = {'obs': obs, 'action': (np.tanh(obs @ W) + 0.01 * rng.standard_normal((2000, A))).astype(np.float32),
              'reward': rng.standard_normal((2000, 1)).astype(np.float32),
              'cost': rng.random((2000, 1)).astype(np.float32), 'next_obs': obs[::-1].copy(),
              'done': np.zeros((2000, 1), np.float32)}
    path = offline.write_dataset(str(tmp_path), 'SynthReach-v0', arrays)
    hidden = {'hidden_sizes': [32, 32]}
    cfgs = {'train_cfgs': {'dataset': path, 'total_steps': 100, 'evaluate_epoisodes': 2},
            'algo_cfgs': {'batch_size': 64, 'steps_per_epoch': 50, 'sampled_action_num': 4},
            'model_cfgs': {'actor': hidden, 'critic': hidden},
            'logger_cfgs': {'log_dir': str(tmp_path / 'runs'), 'save_model_freq': 1, 'verbose': False},
            'env_cfgs': {'horizon': 8}}
    agent = omnisafe_amd.Agent(algo, 'SynthReach-v0', custom_cfgs=cfgs)
    agent.learn()
    step, log_dir = agent.agent._step, agent.agent.logger.log_dir
    with open(os.path.join(log_dir, 'progress.csv'), encoding='utf-8') as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 2
    for col in agent.agent._stat_columns():
        assert all(np.isfinite(float(r[bcq_step.STAT_KEYS[col]])) for r in rows), col
    assert float(rows[1]['Loss/Loss_recon']) < float(rows[0]['Loss/Loss_recon'])
    assert sorted(agent.evaluate(num_episodes=2)) == ['epoch-1.pt', 'epoch-2.pt']
    _, cfg, ck = load_checkpoint(log_dir, 'epoch-2.pt')
    assert list(ck['actor']) == list(step.state_dict()) and list(ck['actor'])[:2] == ['_phi', 'vae._encoder.0.weight']
    assert 'pi' in ck
    again = bcq_step.BcqActor(bcq_step.make_desc(D, A, [32, 32], [32, 32], 'relu', 'relu'), DEV)
    again.load_state_dict(ck['actor'])
    o, z = torch.from_numpy(obs[:9]).to(DEV), torch.ones(9, 2 * A, device=DEV)
    assert again.phi == step.phi and torch.equal(again.predict(o, z), step.predict(o, z))
