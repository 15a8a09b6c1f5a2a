"""GPU: Td3Step (csrc/td3_kernels.hip) against a plain float64 torch-autograd statement of ddpg.py:402-547 and
td3.py:50-116 -- four steps with injected draws, so with policy_delay 2 two actor and Polyak steps -- on both routes;
the replay ring against a numpy ring; one end-to-end Agent('TD3') run.

Bound per quantity: 4 x the error of a float32 torch replay of the same steps against the same float64 reference (the
factor covers the K-split summation orders of the MFMA tiles), floor 16 float32 ulps = 1.9e-6.  Measured on an MI355X,
worst quantity per case (kernel / float32 replay): td3_ragged 3.7e-7 / 2.8e-7, td3_full 3.1e-7 / 1.9e-7, ddpg
2.8e-7 / 2.6e-7, td3_cost 3.7e-7 / 2.8e-7, td3_wide 2.8e-7 / 2.0e-7, td3_clip_l2 3.2e-7 / 1.2e-7; the layer and the
fused route differ from each other by less than either differs from the reference.

EDGES, each on both routes under the same bound: the shared target action of DDPG with a cost critic (ddpg_cost),
partial second tiles, a half K step and networks of different depths (td3_tiles), one hidden layer (td3_shallow), the
four other activations, one per network (td3_smooth, td3_sigmoid), nine row tiles and one row (td3_b260, td3_b1), six
steps in calls of 2, 1, 2, 1 through two slots with policy_delay 3 (td3_chunks), a clip that never binds (td3_noclip);
td3_cost and ddpg on the fused route; LIMIT: the widest observation the fused route takes (td3_lds, D = 609) and the
layer fallback 4 above it (td3_lds4).  After every case the padding of every block is exactly zero.  Conditions -- the
kink margin, every norm above (td3_clip_l2) or below (td3_noclip) the clip -- are asserted from the CPU replays alone.
Worst quantity per case and route: profiles/td3_twin_error.md (kernel 1.2e-7 ... 9.9e-7, the latter td3_b260's actor_v
against a float32 replay at 2.1e-7: on the floor, not on the factor)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RAGGED = dict(nq=2, D=5, A=3, hid=[24, 40], B=37)
CASES = {
    'td3_ragged': RAGGED,                                    # ragged 32-row tile, widths and obs || act off the tiles
    'td3_full': dict(nq=2, D=17, A=6, hid=[256, 256], B=64),  # full-width buffers, two row tiles
    'ddpg': dict(RAGGED, nq=1),                              # one critic, delay 1, no noise, online actor in the target
    'td3_cost': dict(RAGGED, cost=True),                     # the cost critic
    'td3_wide': dict(RAGGED, hid=[260]),                     # layer route chosen by osa_td3_chain_supported
    'td3_clip_l2': dict(RAGGED, max_grad_norm=0.05, coeff=0.001),  # clip (every norm of the reference exceeds it), L2
}
# what the six above leave unrun; each on both routes.  A case may give actor_hid / critic_hid, actor_act / critic_act,
# delay, steps, nslots and chunks (the sizes of consecutive run(n) calls)
EDGES = {
    'ddpg_cost': dict(RAGGED, nq=1, cost=True),  # both targets share one action: fused skips the second actor pass
    # partial second tiles (200, 136), one wave with 2 live columns (34), ldw 36 = half a K step, three hidden critic
    # layers against two actor layers
    'td3_tiles': dict(RAGGED, actor_hid=[200, 34], critic_hid=[136, 200, 34]),
    'td3_shallow': dict(RAGGED, actor_hid=[24], critic_hid=[40]),              # the first layer feeds the head
    'td3_smooth': dict(RAGGED, actor_act='tanh', critic_act='softplus', cost=True),  # each network's own activation
    'td3_sigmoid': dict(RAGGED, actor_act='sigmoid', critic_act='identity'),   # the remaining two
    'td3_b260': dict(RAGGED, B=260),  # 9 row tiles, the last with 4 rows; second trip of the += 256 row loops
    'td3_b1': dict(RAGGED, B=1),      # one live row in a 32-row tile
    # slot wrap, host parity against the device step across calls; actor steps at t = 2 and t = 5 (first in its call)
    'td3_chunks': dict(RAGGED, delay=3, steps=6, nslots=2, chunks=[2, 1, 2, 1]),
    'td3_noclip': dict(RAGGED, max_grad_norm=2.0),  # above every norm of the reference (1.16): the scale's min(., 1)
}
# the fused route at its LDS limit: the widest observation osa_td3_chain_supported takes, and 4 above it
LIMIT = {'td3_lds': dict(RAGGED, D='widest'), 'td3_lds4': dict(RAGGED, D='widest+4')}
STEPS, N, SEED, GAMMA, POLYAK, LR = 4, 48, 3, 0.99, 0.005, 3e-4
# one seed per case, so that one case's conditions can be met without moving the others
SEEDS = dict({case: SEED for case in (*CASES, *EDGES, *LIMIT)}, td3_lds=6)  # td3_lds at 3: a margin of 7e-5
QUANTITIES = ('actor', 'actor_t', 'actor_m', 'actor_v', 'critic', 'critic_t', 'critic_m', 'critic_v', 'stats')
ACT = {'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid, 'softplus': torch.nn.functional.softplus,
       'identity': lambda x: x}  # models.ACTIVATIONS


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a - b))


@functools.lru_cache(maxsize=None)
def widest_obs():
    """The largest obs_dim the fused route takes at RAGGED's other sizes, asked of the product (a host call)."""
    import ctypes

    from omnisafe_amd import _lib, td3_step

    r = RAGGED
    ok = lambda D: bool(_lib.load().osa_td3_chain_supported(ctypes.byref(
        td3_step.make_desc(D, r['A'], r['hid'], r['hid'], 'relu', 'relu', r['B']))))
    D = r['D']
    assert ok(D)
    while ok(D + 1):
        D += 1
    return D


def _cfg(case):
    c = dict(cost=False, max_grad_norm=0.0, coeff=0.0, steps=STEPS, actor_act='relu', critic_act='relu')
    c.update(CASES.get(case) or EDGES.get(case) or LIMIT[case])
    if isinstance(c['D'], str):
        c['D'] = widest_obs() + (4 if c['D'].endswith('+4') else 0)
    td3 = c['nq'] == 2
    c.setdefault('delay', 2 if td3 else 1)
    c.setdefault('actor_hid', c['hid'])
    c.setdefault('critic_hid', c['hid'])
    c.setdefault('nslots', c['steps'])
    c.setdefault('chunks', [c['steps']])
    assert sum(c['chunks']) == c['steps'] and max(c['chunks']) <= c['nslots']
    c.update(pn=0.2 if td3 else 0.0, clip=0.5 if td3 else 0.0, target_actor=td3)
    return c


@functools.lru_cache(maxsize=None)
def problem(case):
    from omnisafe_amd.crr_step import _init_mlp

    c = _cfg(case)
    D, A, B = c['D'], c['A'], c['B']
    g = torch.Generator().manual_seed(SEEDS[case])
    torch.manual_seed(SEEDS[case])
    flat = lambda sizes: [t.detach() for wb in _init_mlp(sizes, 'kaiming_uniform') for t in wb]
    nets = {'pi': flat([D] + c['actor_hid'] + [A])}
    for k in ['q0', 'q1'][:c['nq']] + (['qc'] if c['cost'] else []):
        nets[k] = flat([D + A] + c['critic_hid'] + [1])
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    ring = dict(obs=r(N, D), act=r(N, A), reward=torch.randn(N, generator=g), cost=torch.rand(N, generator=g),
                done=(torch.rand(N, generator=g) < 0.2).float(), next_obs=torch.randn(N, D, generator=g))
    idx = torch.randint(0, N, (c['steps'], B), generator=g)
    eps = torch.randn(c['steps'], B, A, generator=g)
    return c, nets, ring, idx, eps


def _fwd(p, x, act, head=None):
    """``act``: the hidden activation; ``head``: the actor's tanh."""
    for l in range(0, len(p), 2):
        x = x @ p[l].T + p[l + 1]
        x = ACT[act](x) if l + 2 < len(p) else (torch.tanh(x) if head else x)
    return x


@functools.lru_cache(maxsize=None)
def replay(case, dtype):
    """ddpg.py:382-547 / td3.py:50-116 in ``dtype`` on the CPU: the final quantities, the margin of every kink's
    argument and the smallest and the largest gradient norm an optimiser saw."""
    c, nets, ring, idx, eps = problem(case)
    ring = {k: v.to(dtype) for k, v in ring.items()}
    P = {k: [t.to(dtype).clone().requires_grad_(True) for t in v] for k, v in nets.items()}
    T = {k: [t.detach().clone() for t in v] for k, v in P.items()}
    rk = ['q0', 'q1'][:c['nq']]
    groups = {'pi': P['pi'], 'r': [t for k in rk for t in P[k]]}
    if c['cost']:
        groups['c'] = P['qc']
    opt = {k: torch.optim.Adam(v, lr=LR) for k, v in groups.items()}
    margin, norms, stats = [], [], np.zeros((c['steps'], 5))
    pi = lambda p, x: _fwd(p, x, c['actor_act'], head=True)
    qf = lambda p, x: _fwd(p, x, c['critic_act'])[:, 0]

    def update(name, loss):
        opt[name].zero_grad()
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(groups[name], c['max_grad_norm'] or math.inf)))
        opt[name].step()

    def critic_loss(keys, tkeys, sig, actor, noise):
        with torch.no_grad():
            a2 = pi(actor, no)
            if noise is not None:
                margin.append(float((c['clip'] - (noise * c['pn']).abs()).abs().min()))
                a2 = a2 + (noise * c['pn']).clamp(-c['clip'], c['clip'])
                margin.append(float((1 - a2.abs()).abs().min()))
                a2 = a2.clamp(-1.0, 1.0)
            tq = [qf(T[k], torch.cat([no, a2], 1)) for k in tkeys]
            if len(tq) == 2:
                margin.append(float((tq[0] - tq[1]).abs().min()))
            y = sig + GAMMA * (1 - d) * (torch.min(*tq) if len(tq) == 2 else tq[0])
        q = [qf(P[k], torch.cat([o, a], 1)) for k in keys]
        loss = sum(torch.nn.functional.mse_loss(qk, y) for qk in q)
        if c['coeff']:
            loss = loss + sum(p.pow(2).sum() for k in keys for p in P[k]) * c['coeff']
        return loss, float(q[0].mean().detach())

    for t in range(c['steps']):
        o, a, rew, cst, d, no = (ring[k][idx[t]] for k in ('obs', 'act', 'reward', 'cost', 'done', 'next_obs'))
        loss, stats[t, 1] = critic_loss(rk, rk, rew, T['pi'] if c['target_actor'] else P['pi'],
                                        eps[t].to(dtype) if c['pn'] else None)
        stats[t, 0] = float(loss)
        update('r', loss)
        if c['cost']:
            loss, stats[t, 4] = critic_loss(['qc'], ['qc'], cst, P['pi'], None)
            stats[t, 3] = float(loss)
            update('c', loss)
        if (t + 1) % c['delay'] == 0:
            loss = -qf(P['q0'], torch.cat([o, pi(P['pi'], o)], 1)).mean()
            stats[t, 2] = float(loss)
            update('pi', loss)
            with torch.no_grad():
                for k in P:
                    for tp, p in zip(T[k], P[k]):
                        tp.copy_(POLYAK * p + (1 - POLYAK) * tp)
    cat = lambda ts: np.concatenate([t.detach().double().numpy().ravel() for t in ts])
    ck = rk + (['qc'] if c['cost'] else [])
    mom = lambda keys, name: cat([opt['pi' if keys == ['pi'] else ('c' if k == 'qc' else 'r')].state[p][name]
                                  for k in keys for p in P[k]])
    out = {'actor': cat(P['pi']), 'actor_t': cat(T['pi']), 'actor_m': mom(['pi'], 'exp_avg'),
           'actor_v': mom(['pi'], 'exp_avg_sq'), 'critic': cat([p for k in ck for p in P[k]]),
           'critic_t': cat([p for k in ck for p in T[k]]), 'critic_m': mom(ck, 'exp_avg'),
           'critic_v': mom(ck, 'exp_avg_sq'), 'stats': stats}
    return out, min(margin, default=1.0), min(norms), max(norms)


def run_kernel(case, route=None):
    from omnisafe_amd import td3_step

    c, nets, ring, idx, eps = problem(case)
    desc = td3_step.make_desc(c['D'], c['A'], c['actor_hid'], c['critic_hid'], c['actor_act'], c['critic_act'], c['B'],
                              c['nq'], c['cost'])
    st = td3_step.Td3Step(desc, size=N, gamma=GAMMA, polyak=POLYAK, lr_actor=LR, lr_critic=LR, nslots=c['nslots'],
                          policy_noise=c['pn'], policy_noise_clip=c['clip'], policy_delay=c['delay'],
                          max_grad_norm=c['max_grad_norm'], critic_norm_coeff=c['coeff'], route=route)
    names = lambda p, pre: {f'{pre}.{2 * (i // 2)}.{"weight" if i % 2 == 0 else "bias"}': t for i, t in enumerate(p)}
    st.load_state_dict(names(nets['pi'], 'net'))
    rsd = {}
    for j in range(c['nq']):
        rsd.update(names(nets[f'q{j}'], f'critic_{j}.0'))
    st.load_critic_state_dict(rsd, 'reward')
    if c['cost']:
        st.load_critic_state_dict(names(nets['qc'], 'critic_0.0'), 'cost')
    st.actor_t.copy_(st.actor)
    st.critic_t.copy_(st.critic)
    for k, v in ring.items():
        st.ring[k].copy_(v)
    st.pos.copy_(torch.tensor([0, N]))
    stats, t0 = np.zeros((c['steps'], 5)), 0
    for n in c['chunks']:  # a call's draws into their slots, its steps, its rows out before a later call reuses them
        st.set_draws(t0, idx[t0:t0 + n], eps[t0:t0 + n])
        st.run(n)
        torch.cuda.synchronize()
        slots = (torch.arange(n) + t0) % c['nslots']
        stats[t0:t0 + n] = st.stats[slots.to(st.device), :5].double().cpu().numpy()
        t0 += n
    assert st.update_count == c['steps'] == int(st.step.item())
    if c['nslots'] < c['steps']:  # a reused slot keeps the Loss_pi of an earlier actor step; learn() filters it so
        stats[(np.arange(c['steps']) + 1) % c['delay'] != 0, 2] = 0.0
    cat = lambda sd: np.concatenate([v.double().cpu().numpy().ravel() for v in sd.values()])
    out = {'stats': stats}
    for q, w in (('actor', 'actor'), ('actor_t', 'actor_t'), ('actor_m', 'actor_m'), ('actor_v', 'actor_v')):
        out[q] = cat(st.state_dict(w))
    for q in ('critic', 'critic_t', 'critic_m', 'critic_v'):
        out[q] = np.concatenate([cat(st.critic_state_dict(n, q)) for n in ['reward'] + (['cost'] if c['cost'] else [])])
    return out, st


def padding_nonzeros(st):
    """Elements of the padded blocks (parameters, targets, moments) that no state-dict index covers and that are not
    exactly zero: the fused cost branch re-runs the actor over the previous action's columns, and the L2 term sums a
    whole block -- both are right only while this is 0."""
    def count(block, flat_ix):
        pad = torch.ones(block.numel(), dtype=torch.bool, device=block.device)
        pad[flat_ix] = False
        return int(torch.count_nonzero(block[pad]))

    bad = sum(count(getattr(st, w), st._ix['actor'][1]) for w in ('actor', 'actor_t', 'actor_m', 'actor_v'))
    for w in ('critic', 'critic_t', 'critic_m', 'critic_v'):
        for name in ['reward'] + (['cost'] if st.use_cost else []):
            bad += sum(count(blk, ix[1]) for blk, ix in zip(st._critic_blocks(name, w), st._ix[name]))
    return bad


def check(case, route):
    ref, margin, min_norm, max_norm = replay(case, torch.float64)
    f32 = replay(case, torch.float32)[0]
    c = _cfg(case)
    assert margin > 1e-4, f'{case}: a kink argument within {margin:.2e} of its kink; pick another SEED'
    if case == 'td3_noclip':
        assert max_norm < c['max_grad_norm'], f'{case}: a gradient norm {max_norm} is clipped'
    elif c['max_grad_norm']:
        assert min_norm > c['max_grad_norm'], f'{case}: a gradient norm {min_norm} is not clipped'
    got, st = run_kernel(case, route)
    assert padding_nonzeros(st) == 0
    bad = []
    for q in QUANTITIES:
        e_k, e_32 = rel_l2(got[q], ref[q]), rel_l2(f32[q], ref[q])
        print(f'{case} {route or "default"} {q}: kernel {e_k:.3e} float32 replay {e_32:.3e}')
        if not e_k <= max(4 * e_32, 16 * 2.0 ** -23):
            bad.append((q, e_k, e_32))
    assert not bad, bad
    return st


@pytest.mark.parametrize('case', list(CASES))
def test_step_matches_float64_reference(case):
    from omnisafe_amd import _lib, td3_step

    st = check(case, None)
    assert st.route == td3_step.ROUTES['layer' if case == 'td3_wide' else td3_step.DEFAULT_ROUTE]
    if case == 'td3_wide':  # a width above 256: the fused route is refused, not replaced
        assert td3_step.route_of(st.desc, '') == td3_step.ROUTES['layer']
        with pytest.raises(_lib.OsaError):
            td3_step.route_of(st.desc, 'fused')


@pytest.mark.parametrize('case', ['td3_ragged', 'td3_full'])
@pytest.mark.parametrize('route', ['layer', 'fused'])
def test_routes_agree_within_the_bound(case, route):
    check(case, route)


@pytest.mark.parametrize('case', list(EDGES))
@pytest.mark.parametrize('route', ['layer', 'fused'])
def test_edge_step_matches_float64_reference(case, route):
    from omnisafe_amd import td3_step

    assert set(ACT) == set(td3_step.ACTIVATIONS)
    assert check(case, route).route == td3_step.ROUTES[route]


@pytest.mark.parametrize('case', ['td3_cost', 'ddpg'])
def test_fused_route_with_a_cost_critic_and_with_one_critic(case):
    """td3_cost: the fused kernel's second group -- the online actor over xin while its padding columns still hold the
    first group's action (D = 5: columns 5 .. 7) -- and the cost target from pt[2]; ddpg: nq 1, no noise."""
    check(case, 'fused')


def test_fused_route_at_its_lds_limit():
    """The widest observation the fused route accepts runs the kernel at its full dynamic LDS request; 4 above it the
    route is refused, not replaced, and the default falls back to layer."""
    from omnisafe_amd import _lib, td3_step

    D = widest_obs()
    st = check('td3_lds', 'fused')
    assert st.D == D and st.route == td3_step.ROUTES['fused']
    st = check('td3_lds4', None)
    assert st.D == D + 4 and st.route == td3_step.ROUTES['layer'] == td3_step.route_of(st.desc, '')
    with pytest.raises(_lib.OsaError):
        td3_step.route_of(st.desc, 'fused')


def test_ring_wraps_and_draws_stay_below_fill():
    from omnisafe_amd import td3_step

    n, size, D, A, B = 3, 8, 4, 2, 16
    st = td3_step.Td3Step(td3_step.make_desc(D, A, [8], [8], 'relu', 'relu', B), size=size, gamma=GAMMA, polyak=POLYAK,
                          lr_actor=LR, lr_critic=LR, nslots=2)
    rng = np.random.default_rng(0)
    want = {k: np.zeros((size, w), np.float32) for k, w in (('obs', D), ('act', A), ('next_obs', D), ('reward', 1),
                                                             ('cost', 1), ('done', 1))}
    dev = lambda x: torch.as_tensor(x).cuda()
    for k in range(4):  # 12 rows through 8
        rows = {key: rng.standard_normal((n, v.shape[1])).astype(np.float32) for key, v in want.items()}
        rows['done'] = (rng.random((n, 1)) < 0.5).astype(np.float32)
        final, mask = rng.standard_normal((n, D)).astype(np.float32), np.array([0, 1, 0], np.uint8)
        st.store(dev(rows['obs']), dev(rows['act']), dev(rows['reward'][:, 0]), dev(rows['cost'][:, 0]),
                 dev(rows['done'][:, 0].astype(np.uint8)), dev(np.zeros(n, np.uint8)), dev(rows['next_obs']),
                 dev(final), dev(mask))
        rows['next_obs'][1] = final[1]
        for i in range(n):
            for key in want:
                want[key][(k * n + i) % size] = rows[key][i]
        if k == 1:  # part full: 6 of 8 rows
            st.draw(seed=5, first_step=0, nsteps=2)
            assert 0 <= int(st.idx.min()) and int(st.idx.max()) < 6 and st.idx.unique().numel() > 3
            assert abs(float(st.eps.mean())) < 0.5 and 0.5 < float(st.eps.std()) < 1.5
    assert st.pos.tolist() == [12 % size, size]
    for key, v in want.items():
        assert np.array_equal(st.ring[key].cpu().numpy().reshape(size, -1), v), key


def test_agent_td3_end_to_end(tmp_path):
    import omnisafe_amd
    from omnisafe_amd.evaluator import Evaluator

    cfgs = {'train_cfgs': {'total_steps': 128}, 'logger_cfgs': {'log_dir': str(tmp_path), 'verbose': False,
                                                                'save_model_freq': 1},
            'algo_cfgs': {'steps_per_epoch': 64, 'start_learning_steps': 16, 'batch_size': 32, 'size': 256},
            'model_cfgs': {'actor': {'hidden_sizes': [32, 32]}, 'critic': {'hidden_sizes': [32, 32]}}}
    agent = omnisafe_amd.Agent('TD3', 'SynthNavGoal0-v0', custom_cfgs=cfgs)
    agent.learn()
    algo = agent.agent
    rows = np.asarray(algo.epoch_stats[0])  # the first epoch's rows, one per round
    assert rows.shape[0] == 64 and np.all(rows[:17] == 0.0)  # step <= start_learning_steps logs zeros
    assert np.all(np.isfinite(rows)) and np.all(rows[17:, 0] != 0.0) and np.any(rows[17:, 2] != 0.0)
    assert algo.total_env_steps == 128
    ev = Evaluator(verbose=False)
    ev.load_saved(algo.logger.log_dir, agent._saved_models()[-1])  # noqa: SLF001
    rets, costs = ev.evaluate(num_episodes=1)
    assert len(rets) == 1 and np.isfinite(rets[0]) and ev.episode_lengths[0] >= 1
