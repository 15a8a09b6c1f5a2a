"""GPU: the offline VAE-BC train step (csrc/vae_kernels.hip through vae_step.VaeStep) against a plain torch restatement
of ``VAE.loss`` + ``torch.optim.Adam`` run on the CPU in float64, on both routes of ``OSA_VAE_GEMM``; its draws against
their numpy restatement, determinism, graph replay, ``decode``, and the algorithm end to end through
``omnisafe_amd.Agent``.

Tolerance: error <= K * max(e32, 2^-22) with the project's K = 16 and e32 the error of the same restatement run in
float32 against the float64 run -- relative L2 per parameter tensor and Adam moment of both networks, relative per loss
(worst step).  Nothing is excluded.  With OSA_WRITE_PROFILES=1 the ratios go to profiles/vae_twin_error.md.
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K = 16.0
FLOOR = 2.0 ** -22
LR = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT = {'tanh': torch.tanh, 'relu': torch.relu, 'softplus': torch.nn.functional.softplus}
# name: D, A, hidden, activation, B, steps, scale of the encoder's log_std rows
CASES = {'one': (3, 1, [8], 'tanh', 1, 3, 1.0),
         'ragged': (12, 2, [70, 50], 'relu', 70, 3, 1.0),
         'batch256': (60, 2, [130, 130], 'relu', 256, 3, 1.0),
         'deep': (100, 3, [64, 64, 64], 'softplus', 33, 3, 1.0),
         'clamp': (12, 2, [70, 50], 'relu', 70, 3, 150.0),
         'yaml': (12, 2, [750, 750], 'relu', 256, 1, 1.0)}
_RATIOS = {}


def make_run(name):
    from omnisafe_amd import vae_step

    D, A, hidden, act, B, steps, ls_scale = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    torch.manual_seed(7)
    sd = vae_step.initial_state_dict(vae_step.make_desc(D, A, hidden, act, B))
    top = f'encoder.{2 * len(hidden)}'
    sd[f'{top}.weight'][2 * A:] *= ls_scale  # (the clamp case: log_std far outside [-20, 2] on some rows)
    N = 3 * B + 5
    obs = torch.randn(N, D, generator=g)
    data = {'obs': obs, 'action': torch.tanh(torch.randn(N, A, generator=g)), 'reward': torch.zeros(N, 1),
            'cost': torch.zeros(N, 1), 'next_obs': obs.clone(), 'done': torch.zeros(N, 1)}
    return dict(D=D, A=A, hidden=hidden, act=act, B=B, steps=steps, sd=sd, data=data,
                idx=torch.randint(0, N, (steps, B), generator=g), eps=torch.randn(steps, B, 2 * A, generator=g))


def mlp(p, name, n_layers, x, act):
    for j in range(n_layers):
        x = x @ p[f'{name}.{2 * j}.weight'].T + p[f'{name}.{2 * j}.bias']
        if j + 1 < n_layers:
            x = ACT[act](x)
    return x


def restatement(run, dtype):
    """VAE.loss (vae_actor.py:100-112) and one Adam step over all parameters (vae_bc.py:85-89), ``steps`` times."""
    p = {k: v.to(dtype).clone().requires_grad_() for k, v in run['sd'].items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR)
    L, losses, raws = len(run['hidden']) + 1, [], []
    for s in range(run['steps']):
        obs, act = run['data']['obs'][run['idx'][s]].to(dtype), run['data']['action'][run['idx'][s]].to(dtype)
        mean, raw = torch.chunk(mlp(p, 'encoder', L, torch.cat([obs, act], -1), run['act']), 2, dim=-1)
        dist = torch.distributions.Normal(mean, torch.clamp(raw, min=-20, max=2).exp())
        z = dist.mean + run['eps'][s].to(dtype) * dist.stddev  # rsample with the injected noise
        recon = torch.nn.functional.mse_loss(mlp(p, 'decoder', L, torch.cat([obs, z], -1), run['act']), act)
        kl = torch.distributions.kl.kl_divergence(dist, torch.distributions.Normal(0, 1)).mean()
        opt.zero_grad()
        (recon + kl).backward()
        opt.step()
        losses.append([(recon + kl).item(), recon.item(), kl.item()])
        raws.append(raw.detach())
    out = {}
    for k, v in p.items():
        out[f'p/{k}'] = v.detach().double().numpy()
        out[f'm/{k}'] = opt.state[v]['exp_avg'].double().numpy()
        out[f'v/{k}'] = opt.state[v]['exp_avg_sq'].double().numpy()
    return out, np.array(losses), raws


@functools.lru_cache(maxsize=None)
def reference(name):
    """The run, its float64 restatement and the float32 restatement's own error, shared by both routes."""
    run = make_run(name)
    t64, l64, raws = restatement(run, torch.float64)
    t32, l32, _ = restatement(run, torch.float32)
    return run, t64, l64, errors(t32, l32, t64, l64), raws


def errors(t, losses, t64, l64):
    err = {q: float(np.linalg.norm(t[q] - t64[q]) / np.linalg.norm(t64[q])) for q in t64}
    for c, key in enumerate(('Loss_vae', 'Loss_recon', 'Loss_kl')):
        err[key] = float(np.max(np.abs(losses[:, c] - l64[:, c]) / np.abs(l64[:, c])))
    return err


def device_step(run, route, nslots=None):
    from omnisafe_amd import vae_step

    desc = vae_step.make_desc(run['D'], run['A'], run['hidden'], run['act'], run['B'])
    st = vae_step.VaeStep(desc, {k: v.to(DEV) for k, v in run['data'].items()}, lr=LR,
                          nslots=nslots or run['steps'], route=route, device=DEV)
    st.load_state_dict(run['sd'])
    st.set_draws(0, run['idx'], run['eps'])
    return st


def device_tensors(st):
    out = {}
    for which, tag in (('params', 'p'), ('m', 'm'), ('v', 'v')):
        for k, v in st.state_dict(which).items():
            if not k.startswith('_'):
                out[f'{tag}/{k}'] = v.double().cpu().numpy()
    return out


@pytest.mark.parametrize('route', ['tile', 'skinny'])
@pytest.mark.parametrize('name', list(CASES))
def test_steps_against_float64(name, route):
    run, t64, l64, e32, raws = reference(name)
    if name == 'clamp':  # both clamp branches and the open interval are hit, in every step
        for raw in raws:
            assert (raw > 2).any() and (raw < -20).any() and ((raw > -20) & (raw < 2)).any()
    st = device_step(run, route)
    st.run(run['steps'])
    assert int(st.step.item()) == run['steps'] and int(st.adam_step.item()) == run['steps']
    err = errors(device_tensors(st), st.stats[:run['steps'], :3].double().cpu().numpy(), t64, l64)
    ratios = _RATIOS[f'{name}/{route}'] = {q: err[q] / max(e32[q], FLOOR) for q in err}
    for q in sorted(ratios):
        print(f'{name}/{route} {q}: error {err[q]:.3e} e32 {e32[q]:.3e} ratio {ratios[q]:.2f}')
    bad = {q: r for q, r in ratios.items() if not r <= K}
    assert not bad, bad
    pad = torch.from_numpy(~st.layout.real_mask()).to(DEV)  # padding lanes stay zero, the dataset keeps its bits
    for blk in (st.params, st.m, st.v):
        assert not blk[pad].any()
    for k, v in run['data'].items():
        assert torch.equal(st.data[k].cpu(), v), k


@pytest.fixture(scope='module', autouse=True)
def write_profile():
    yield
    if os.environ.get('OSA_WRITE_PROFILES') == '1' and _RATIOS:
        with open(os.path.join(ROOT, 'profiles', 'vae_twin_error.md'), 'w', encoding='utf-8') as f:
            f.write('# VAE-BC step: error / max(e32, 2^-22) against the float64 restatement (bound 16)\n\n')
            f.write('| case/route | quantities | worst | worst quantity |\n|---|---|---|---|\n')
            for name, r in _RATIOS.items():
                q = max(r, key=r.get)
                f.write(f'| {name} | {len(r)} | {r[q]:.2f} | {q} |\n')


def test_replay_and_determinism():
    run = reference('ragged')[0]
    eager, again, graphed = (device_step(run, None) for _ in range(3))
    eager.run(3)
    again.run(3)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        graphed.run(1)
        graph.capture_end()
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for other in (again, graphed):
        for blk in ('params', 'm', 'v', 'stats', 'step'):
            assert torch.equal(getattr(eager, blk), getattr(other, blk)), blk


def philox(key, hi, lo):
    """Philox4x32-10 of counter (hi, lo) under a 64-bit key; lo an array."""
    lo = np.asarray(lo, np.uint64)
    c = [lo & 0xFFFFFFFF, lo >> np.uint64(32), np.full_like(lo, hi & 0xFFFFFFFF), np.full_like(lo, hi >> 32)]
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & 0xFFFFFFFF, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def normal(w0, w1):
    u = [((w >> np.uint64(8)).astype(np.float32) + np.float32(1)) * np.float32(1 / 16777216) for w in (w0, w1)]
    return (np.sqrt(-2.0 * np.log(u[0].astype(np.float64))) * np.cos(6.28318530717958647692 * u[1].astype(np.float64))
            ).astype(np.float32)


def test_draws_equal_numpy():
    run = reference('ragged')[0]
    st = device_step(run, None, nslots=8)
    seed, first, n, B, A2, N = 0x1234ABCD5678, 7, 5, run['B'], 2 * run['A'], st.n_rows
    st.draw(seed, first, n)
    for k in range(n):
        step, slot = first + k, (first + k) % 8
        w = philox(seed ^ 0x56414549445831, step, np.arange(B))
        bits = [int(a) | (int(b) << 32) for a, b in zip(w[0], w[1])]
        assert st.idx[slot].tolist() == [(x * N) >> 64 for x in bits]
        w = philox(seed ^ 0x56414545505331, step, np.arange(B * A2))
        assert np.array_equal(st.eps[slot].cpu().numpy().reshape(-1), normal(w[0], w[1]))


@pytest.mark.parametrize('route', ['tile', 'skinny'])
@pytest.mark.parametrize('n', [1, 70, 300])
def test_decode(n, route):
    run, t64 = reference('ragged')[:2]
    st = device_step(run, route)
    g = torch.Generator().manual_seed(n)
    obs, z = torch.randn(n, run['D'], generator=g), torch.randn(n, 2 * run['A'], generator=g)
    L = len(run['hidden']) + 1
    out = {}
    for dtype in (torch.float64, torch.float32):
        p = {k: v.to(dtype) for k, v in run['sd'].items()}
        out[dtype] = mlp(p, 'decoder', L, torch.cat([obs, z], -1).to(dtype), run['act']).double()
    ref = out[torch.float64]
    e32 = float((out[torch.float32] - ref).norm() / ref.norm())
    err = float((st.decode(obs.to(DEV), z.to(DEV)).double().cpu() - ref).norm() / ref.norm())
    print(f'decode n={n} {route}: error {err:.3e} e32 {e32:.3e}')
    assert err <= K * max(e32, FLOOR)
    a, b, c = (st.decode(obs.to(DEV), None, seed=s) for s in (3, 3, 4))
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all()


def test_agent_end_to_end(tmp_path):
    import csv

    import omnisafe_amd
    from omnisafe_amd import offline, vae_step
    from omnisafe_amd.saved_policy import device_env_class, load_checkpoint

    D, A = device_env_class('SynthReach-v0').dims('SynthReach-v0')
    rng = np.random.default_rng(5)
    obs = rng.standard_normal((2000, D)).astype(np.float32)
    W = rng.standard_normal((D, A)).astype(np.float32) / np.sqrt(D)
    arrays = {'obs': obs, 'action': (np.tanh(obs @ W) + 0.01 * rng.standard_normal((2000, A))).astype(np.float32),
              'reward': np.zeros((2000, 1), np.float32), 'cost': np.zeros((2000, 1), np.float32), 'next_obs': obs,
              'done': np.zeros((2000, 1), np.float32)}
    path = offline.write_dataset(str(tmp_path), 'SynthReach-v0', arrays)
    cfgs = {'train_cfgs': {'dataset': path, 'total_steps': 100, 'evaluate_epoisodes': 2},
            'algo_cfgs': {'batch_size': 64, 'steps_per_epoch': 50},
            'model_cfgs': {'hidden_sizes': [32, 32]},
            'logger_cfgs': {'log_dir': str(tmp_path / 'runs'), 'save_model_freq': 1, 'verbose': False},
            'env_cfgs': {'horizon': 8}}
    agent = omnisafe_amd.Agent('VAEBC', 'SynthReach-v0', custom_cfgs=cfgs)
    agent.learn()
    log_dir = agent.agent.logger.log_dir
    with open(os.path.join(log_dir, 'progress.csv'), encoding='utf-8') as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 2
    for key in ('Loss/Loss_vae', 'Loss/Loss_recon', 'Loss/Loss_kl'):
        assert all(np.isfinite(float(r[key])) for r in rows), key
    assert float(rows[1]['Loss/Loss_recon']) < float(rows[0]['Loss/Loss_recon'])
    assert sorted(agent.evaluate(num_episodes=2)) == ['epoch-1.pt', 'epoch-2.pt']
    _, cfg, ck = load_checkpoint(log_dir, 'epoch-2.pt')
    assert list(ck['vae']) == list(agent.agent._step.state_dict()) and 'pi' in ck
    again = vae_step.VaeDecoder(vae_step.make_desc(D, A, [32, 32], cfg.model_cfgs.activation, 1), DEV)
    again.load_state_dict(ck['vae'])
    o, z = torch.from_numpy(obs[:9]).to(DEV), torch.ones(9, 2 * A, device=DEV)
    assert torch.equal(again.decode(o, z), agent.agent._step.decode(o, z))
