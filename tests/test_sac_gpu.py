"""GPU: SacStep (csrc/sac_kernels.hip) against a plain float64 torch-autograd statement of sac.py:93-207 on
ddpg.py:350-547 -- four steps with injected draws, so with policy_delay 2 two actor, temperature and Polyak steps -- on
both head routes; osa_sac_act and osa_sac_draws against the host's Philox; one end-to-end Agent('SAC') run.

Bound per quantity, as test_td3_gpu.py's: 4 x the error of a float32 torch replay of the same steps against the same
float64 reference, floor 16 float32 ulps = 1.9e-6.  Conditions, asserted from the two CPU replays alone: every kink's
argument (ReLU pre-activations, tq1 - tq2, q1 - q2, log_std against -20 and 2) is further from its kink than 4 x what the
float32 replay misses it by.  Measured on an MI355X, worst quantity per case (layer / fused kernel / float32 replay):
sac_ragged 2.0e-7 / 2.2e-7 / 3.6e-7, sac_tail 3.6e-7 / 1.7e-7 / 2.9e-7, sac_full 2.3e-7 / 1.8e-7 / 1.6e-7, sac_a32
1.7e-7 / 2.1e-7 / 1.9e-7, sac_cost 2.0e-7 / 2.2e-7 / 3.6e-7, sac_auto 2.2e-7 / 3.3e-7 / 1.9e-7, sac_clamp 2.1e-7 /
2.1e-7 / 1.9e-7, sac_wide 3.6e-7 / refused / 1.9e-7, sac_clip_l2 2.1e-7 / 1.5e-7 / 9.8e-8 (profiles/sac_twin_error.md)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RAGGED = dict(D=5, A=3, hid=[24, 40], B=37)
CASES = {
    'sac_ragged': RAGGED,                                   # ragged 32-row tile; 2A = 6 and the widths off the tiles
    'sac_tail': dict(RAGGED, hid=[24, 42]),                 # last width 42, ldk 44: the K tail forward, padding backward
    'sac_full': dict(D=17, A=6, hid=[256, 256], B=64),      # two row tiles, full K split, two column slabs backward
    'sac_a32': dict(RAGGED, A=32),                          # both 32-column tiles full
    'sac_cost': dict(RAGGED, cost=True),                    # tanh mu from the shared forward into the cost target
    'sac_auto': dict(RAGGED, auto=True),                    # third draw, scalar Adam, alpha moving between steps
    'sac_clamp': dict(RAGGED, shift=[-25.0, 4.0, 0.0]),     # log_std below -20 and above 2 in every step
    'sac_wide': dict(RAGGED, hid=[24, 516]),                # last hidden width above osa_sac_head_supported's 512
    'sac_clip_l2': dict(RAGGED, max_grad_norm=0.05, coeff=0.001),  # clip (every norm exceeds it), L2
}
SEEDS = dict(sac_ragged=3, sac_tail=3, sac_full=3, sac_a32=3, sac_cost=3, sac_auto=3, sac_clamp=3, sac_wide=3, sac_clip_l2=3)
STEPS, N, GAMMA, POLYAK, LR, ALPHA, DELAY = 4, 48, 0.99, 0.005, 3e-4, 0.2, 2
QUANTITIES = ('actor', 'actor_t', 'actor_m', 'actor_v', 'critic', 'critic_t', 'critic_m', 'critic_v', 'log_alpha',
              'stats')


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a - b))


def _cfg(case):
    return dict(dict(cost=False, auto=False, shift=None, max_grad_norm=0.0, coeff=0.0), **CASES[case])


@functools.lru_cache(maxsize=None)
def problem(case):
    from omnisafe_amd.crr_step import _init_mlp

    c = _cfg(case)
    D, A, B = c['D'], c['A'], c['B']
    g = torch.Generator().manual_seed(SEEDS[case])
    torch.manual_seed(SEEDS[case])
    flat = lambda sizes: [t.detach() for wb in _init_mlp(sizes, 'kaiming_uniform') for t in wb]
    nets = {'pi': flat([D] + c['hid'] + [2 * A])}
    if c['shift']:
        nets['pi'][-1][A:] += torch.tensor(c['shift'])
    for k in ['q0', 'q1'] + (['qc'] if c['cost'] else []):
        nets[k] = flat([D + A] + c['hid'] + [1])
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    ring = dict(obs=r(N, D), act=r(N, A), reward=torch.randn(N, generator=g), cost=torch.rand(N, generator=g),
                done=(torch.rand(N, generator=g) < 0.2).float(), next_obs=torch.randn(N, D, generator=g))
    idx = torch.randint(0, N, (STEPS, B), generator=g)
    eps = torch.randn(STEPS, 3, B, A, generator=g)
    return c, nets, ring, idx, eps


@functools.lru_cache(maxsize=None)
def replay(case, dtype):
    """sac.py:93-207 on ddpg.py:382-547 in ``dtype`` on the CPU: the final quantities, every kink's arguments in
    order, the smallest gradient norm a network optimiser saw and the range of log_std per step."""
    c, nets, ring, idx, eps = problem(case)
    ring = {k: v.to(dtype) for k, v in ring.items()}
    eps = eps.to(dtype)
    P = {k: [t.to(dtype).clone().requires_grad_(True) for t in v] for k, v in nets.items()}
    T = {k: [t.detach().clone() for t in v] for k, v in P.items()}
    groups = {'pi': P['pi'], 'r': P['q0'] + P['q1']}
    if c['cost']:
        groups['c'] = P['qc']
    opt = {k: torch.optim.Adam(v, lr=LR) for k, v in groups.items()}
    la = torch.tensor([0.0 if c['auto'] else math.log(ALPHA)], dtype=dtype, requires_grad=c['auto'])
    opt_a = torch.optim.Adam([la], lr=LR) if c['auto'] else None
    kinks, norms, ls_range, stats = [], [], [], np.zeros((STEPS, 7))

    def fwd(p, x):
        for l in range(0, len(p), 2):
            x = x @ p[l].T + p[l + 1]
            if l + 2 < len(p):
                kinks.append(x.detach().double().ravel())
                x = torch.relu(x)
        return x

    def actor(x, e):  # GaussianSACActor.predict(deterministic=False) + log_prob; tanh(mean)
        mu, ls = fwd(P['pi'], x).chunk(2, dim=-1)
        kinks.extend([(ls.detach().double() + 20).ravel(), (ls.detach().double() - 2).ravel()])
        ls_range.append((float(ls.detach().min()), float(ls.detach().max())))
        ls = ls.clamp(-20, 2)
        u = mu + ls.exp() * e
        # Normal(mu, std).log_prob(u) with (u - mu) / std = e stated, not recovered: at std = e^-20 a float32 replay
        # would lose e in u - mu and stop being a yardstick
        logp = (-0.5 * e * e - ls - 0.5 * math.log(2 * math.pi)).sum(-1)
        logp = logp - (2 * (math.log(2.0) - u - torch.nn.functional.softplus(-2 * u))).sum(-1)
        return torch.tanh(u), logp, torch.tanh(mu)

    def update(name, loss):
        opt[name].zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(groups[name], c['max_grad_norm'] or math.inf)))
        opt[name].step()

    def critic_loss(keys, y):
        q = [fwd(P[k], torch.cat([o, a], 1))[:, 0] for k in keys]
        loss = sum(torch.nn.functional.mse_loss(qk, y) for qk in q)
        if c['coeff']:
            loss = loss + sum(p.pow(2).sum() for k in keys for p in P[k]) * c['coeff']
        return loss, float(q[0].mean().detach())

    for t in range(STEPS):
        o, a, rew, cst, d, no = (ring[k][idx[t]] for k in ('obs', 'act', 'reward', 'cost', 'done', 'next_obs'))
        alpha = la.exp().item()
        with torch.no_grad():
            a2, logp2, am = actor(no, eps[t, 0])
            tq = [fwd(T[k], torch.cat([no, a2], 1))[:, 0] for k in ('q0', 'q1')]
            kinks.append((tq[0] - tq[1]).double())
            y = rew + GAMMA * (1 - d) * (torch.min(*tq) - logp2 * alpha)
            if c['cost']:
                yc = cst + GAMMA * (1 - d) * fwd(T['qc'], torch.cat([no, am], 1))[:, 0]
        loss, stats[t, 1] = critic_loss(['q0', 'q1'], y)
        stats[t, 0] = float(loss.detach())
        update('r', loss)
        if c['cost']:
            loss, stats[t, 4] = critic_loss(['qc'], yc)
            stats[t, 3] = float(loss.detach())
            update('c', loss)
        if (t + 1) % DELAY == 0:
            ap, logp, _ = actor(o, eps[t, 1])
            q = [fwd(P[k], torch.cat([o, ap], 1))[:, 0] for k in ('q0', 'q1')]
            kinks.append((q[0] - q[1]).detach().double())
            loss = (alpha * logp - torch.min(*q)).mean()
            stats[t, 2] = float(loss.detach())
            update('pi', loss)
            if c['auto']:
                with torch.no_grad():
                    _, logp, _ = actor(o, eps[t, 2])
                loss = -la * (logp - c['A']).mean()
                stats[t, 6] = float(loss.detach())
                opt_a.zero_grad()
                loss.backward()
                opt_a.step()
            with torch.no_grad():
                for k in P:
                    for tp, p in zip(T[k], P[k]):
                        tp.copy_(POLYAK * p + (1 - POLYAK) * tp)
        stats[t, 5] = la.exp().item()
    cat = lambda ts: np.concatenate([t.detach().double().numpy().ravel() for t in ts])
    ck = ['q0', 'q1'] + (['qc'] if c['cost'] else [])
    mom = lambda keys, name: cat([opt['pi' if keys == ['pi'] else ('c' if k == 'qc' else 'r')].state[p][name]
                                  for k in keys for p in P[k]])
    am = [opt_a.state[la][n] for n in ('exp_avg', 'exp_avg_sq')] if c['auto'] else [torch.zeros(1), torch.zeros(1)]
    out = {'actor': cat(P['pi']), 'actor_t': cat(T['pi']), 'actor_m': mom(['pi'], 'exp_avg'),
           'actor_v': mom(['pi'], 'exp_avg_sq'), 'critic': cat([p for k in ck for p in P[k]]),
           'critic_t': cat([p for k in ck for p in T[k]]), 'critic_m': mom(ck, 'exp_avg'),
           'critic_v': mom(ck, 'exp_avg_sq'), 'log_alpha': cat([la] + am), 'stats': stats}
    return out, kinks, min(norms), ls_range


def conditions(case):
    """The float64 reference, the float32 replay, and the asserts that keep the reference inside its own conditions."""
    ref, k64, min_norm, ls_range = replay(case, torch.float64)
    f32, k32, _, _ = replay(case, torch.float32)
    for i, (x, y) in enumerate(zip(k64, k32)):
        bad = x.abs() <= 4 * (x - y).abs()
        assert not bool(bad.any()), f'{case}: kink {i} within the float32 replay\'s error; pick another seed'
    c = _cfg(case)
    if c['max_grad_norm']:
        assert min_norm > c['max_grad_norm'], f'{case}: a gradient norm {min_norm} is not clipped'
    if c['shift']:
        assert all(lo < -20 and hi > 2 for lo, hi in ls_range), ls_range
    return ref, f32


def run_kernel(case, head=None):
    from omnisafe_amd import sac_step

    c, nets, ring, idx, eps = problem(case)
    desc = sac_step.make_desc(c['D'], c['A'], c['hid'], c['hid'], 'relu', 'relu', c['B'], 2, c['cost'])
    st = sac_step.SacStep(desc, size=N, gamma=GAMMA, polyak=POLYAK, lr_actor=LR, lr_critic=LR, nslots=STEPS, alpha=ALPHA,
                          auto_alpha=c['auto'], policy_delay=DELAY, max_grad_norm=c['max_grad_norm'],
                          critic_norm_coeff=c['coeff'], head=head)
    names = lambda p, pre: {f'{pre}.{2 * (i // 2)}.{"weight" if i % 2 == 0 else "bias"}': t for i, t in enumerate(p)}
    st.load_state_dict(names(nets['pi'], 'net'))
    rsd = {}
    for j in range(2):
        rsd.update(names(nets[f'q{j}'], f'critic_{j}.0'))
    st.load_critic_state_dict(rsd, 'reward')
    if c['cost']:
        st.load_critic_state_dict(names(nets['qc'], 'critic_0.0'), 'cost')
    st.actor_t.copy_(st.actor)
    st.critic_t.copy_(st.critic)
    for k, v in ring.items():
        st.ring[k].copy_(v)
    st.pos.copy_(torch.tensor([0, N]))
    st.set_draws(0, idx, eps)
    st.run(STEPS)
    torch.cuda.synchronize()
    cat = lambda sd: np.concatenate([v.double().cpu().numpy().ravel() for k, v in sd.items() if k != '_log2'])
    out = {'stats': st.stats[:, :7].double().cpu().numpy(), 'log_alpha': st.log_alpha.double().cpu().numpy()}
    for q in ('actor', 'actor_t', 'actor_m', 'actor_v'):
        out[q] = cat(st.state_dict(q))
    for q in ('critic', 'critic_t', 'critic_m', 'critic_v'):
        out[q] = np.concatenate([cat(st.critic_state_dict(n, q)) for n in ['reward'] + (['cost'] if c['cost'] else [])])
    return out, st


@pytest.mark.parametrize('head', ['layer', 'fused'])
@pytest.mark.parametrize('case', list(CASES))
def test_step_matches_float64_reference(case, head):
    from omnisafe_amd import _lib, sac_step

    ref, f32 = conditions(case)
    if case == 'sac_wide':  # above the fused head's limit: the default picks layer, fused is refused, not replaced
        c = _cfg(case)
        desc = sac_step.make_desc(c['D'], c['A'], c['hid'], c['hid'], 'relu', 'relu', c['B'])
        assert sac_step.head_of(desc, '') == sac_step.HEADS['layer']
        if head == 'fused':
            with pytest.raises(_lib.OsaError):
                sac_step.head_of(desc, 'fused')
            return
        head = None
    got, st = run_kernel(case, head)
    assert st.head == sac_step.HEADS[head or 'layer']
    bad = []
    for q in QUANTITIES:
        e_k, e_32 = rel_l2(got[q], ref[q]), rel_l2(f32[q], ref[q])
        print(f'{case} {head or "default"} {q}: kernel {e_k:.3e} float32 replay {e_32:.3e}')
        if not e_k <= max(4 * e_32, 16 * 2.0 ** -23):
            bad.append((q, e_k, e_32))
    assert not bad, bad


def host_normal(key, hi, n):
    """The first Box-Muller normal of Philox(key, hi, 0 .. n - 1), as the kernels draw it (nav_twin's host Philox)."""
    from nav_twin import philox4x32_10, u01

    w = philox4x32_10(key, hi, np.arange(n))
    u1, u2 = u01(w[:, 0]).astype(np.float64), u01(w[:, 1]).astype(np.float64)
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.28318530717958647692 * u2)).astype(np.float32), w


@pytest.mark.parametrize('mode', ['sample', 'mean', 'uniform'])
def test_act_matches_the_formula(mode):
    """osa_sac_act against the float64 forward with the draw restated on the host: Philox(seed ^ key, offset,
    row act_dim + d); sac_clamp's actor, so sigma is e^-20 in column 0, e^2 in column 1 and moderate in column 2."""
    from omnisafe_amd import sac_step

    c, nets, ring, _, _ = problem('sac_clamp')
    A, n, seed, offset = c['A'], 9, 0x1234ABCD5678, 3
    act = sac_step.SacActor(sac_step.make_desc(c['D'], A, c['hid'], c['hid'], 'relu', 'relu'), 'cuda:0')
    act.load_state_dict({f'net.{2 * (i // 2)}.{"weight" if i % 2 == 0 else "bias"}': t
                         for i, t in enumerate(nets['pi'])})
    obs = ring['obs'][:n].cuda()
    x = ring['obs'][:n].double()
    p = [t.double() for t in nets['pi']]
    for l in range(0, len(p), 2):
        x = x @ p[l].T + p[l + 1]
        x = torch.relu(x) if l + 2 < len(p) else x
    mu, ls = x.chunk(2, dim=-1)
    eps, w = host_normal(seed ^ 0x53414341435431, offset, n * A)
    got = act.act(obs, mode=getattr(sac_step, f'ACT_{mode.upper()}'), seed=seed, offset=offset).cpu()
    if mode == 'uniform':
        from nav_twin import u01

        assert np.array_equal(got.numpy().ravel(), np.float32(2) * u01(w[:, 0]) - np.float32(1))
        return
    u = mu + ls.clamp(-20, 2).exp() * torch.from_numpy(eps).double().reshape(n, A) if mode == 'sample' else mu
    assert rel_l2(got.double(), torch.tanh(u)) < 16 * 2.0 ** -23


def test_draws_equal_numpy():
    """osa_sac_draws: idx [nslots][B] below the fill count pos[1], eps [nslots][3][B][A], both keys, the slot of a step."""
    from omnisafe_amd import sac_step

    B, A, size, fill, nslots, seed, first, n = 37, 3, 64, 41, 8, 0x1234ABCD5678, 7, 5
    st = sac_step.SacStep(sac_step.make_desc(5, A, [8], [8], 'relu', 'relu', B), size=size, gamma=GAMMA, polyak=POLYAK,
                          lr_actor=LR, lr_critic=LR, nslots=nslots)
    st.pos.copy_(torch.tensor([fill % size, fill]))
    st.draw(seed, first, n)
    for k in range(n):
        step, slot = first + k, (first + k) % nslots
        _, w = host_normal(seed ^ 0x53414349445831, step, B)
        assert st.idx[slot].tolist() == [((int(a) | (int(b) << 32)) * fill) >> 64 for a, b in zip(w[:, 0], w[:, 1])]
        eps, _ = host_normal(seed ^ 0x53414345505331, step, 3 * B * A)
        assert np.array_equal(st.eps[slot].cpu().numpy().reshape(-1), eps)


def test_agent_sac_end_to_end(tmp_path):
    import omnisafe_amd
    from omnisafe_amd.evaluator import Evaluator

    cfgs = {'train_cfgs': {'total_steps': 128}, 'logger_cfgs': {'log_dir': str(tmp_path), 'verbose': False,
                                                                'save_model_freq': 1},
            'algo_cfgs': {'steps_per_epoch': 64, 'start_learning_steps': 16, 'batch_size': 32, 'size': 256,
                          'auto_alpha': True},
            'model_cfgs': {'actor': {'hidden_sizes': [32, 32]}, 'critic': {'hidden_sizes': [32, 32]}}}
    agent = omnisafe_amd.Agent('SAC', 'SynthNavGoal0-v0', custom_cfgs=cfgs)
    agent.learn()
    algo = agent.agent
    rows = np.asarray(algo.epoch_stats[0])  # the first epoch's rows, one per round
    assert rows.shape == (64, 7) and np.all(rows[:17, :5] == 0.0) and np.all(rows[:17, 5] == 1.0)
    assert np.all(np.isfinite(rows)) and np.all(rows[17:, 0] != 0.0) and np.all(rows[17:, 5] > 0.0)
    assert np.any(rows[17:, 2] != 0.0) and np.any(rows[17:, 6] != 0.0)
    assert algo.total_env_steps == 128
    ev = Evaluator(verbose=False)
    ev.load_saved(algo.logger.log_dir, agent._saved_models()[-1])  # noqa: SLF001
    rets, _ = ev.evaluate(num_episodes=1)
    assert len(rets) == 1 and np.isfinite(rets[0]) and ev.episode_lengths[0] >= 1
    played = agent.evaluate(num_episodes=1)
    assert played and all(len(r) == 1 and np.isfinite(r[0]) for r, _ in played.values())
