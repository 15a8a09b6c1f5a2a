"""GPU: Td3LagStep against a float64 autograd statement of ddpg_lag.py / td3_lag.py on both OSA_TD3_LAG_DACT settings
(problems, kernel runs, padding check and bound are test_td3_gpu's; only the replay's actor loss differs); the store's
normaliser and the PID multiplier against float64 restatements for equality, the Adam multiplier under the 16-ulp
floor; one Agent('TD3Lag') run.  One hidden actor layer: the head's dz outlives the step (profiles/td3_lag_twin_error.md)."""
import functools

import numpy as np
import pytest
import test_td3_gpu as T
import torch

pytestmark = pytest.mark.gpu

BASE = dict(nq=2, D=7, A=3, hid=[24, 40], actor_hid=[24], B=33, cost=True, steps=3)
CASES = {
    'lag_b33': BASE,                                   # a second row tile of one row, widths off the tiles
    'lag_ddpg_b5_a1': dict(BASE, nq=1, B=5, A=1),      # one critic, delay 1: every step an actor step; one action column
    'lag_b260_a32': dict(BASE, B=260, A=32),           # nine row tiles, the full 32-column output tile
    'lag_ddpg_h4': dict(BASE, nq=1, hid=[4], actor_hid=[4], actor_act='tanh', critic_act='tanh'),  # K = 8: one K step
    'lag_256': dict(BASE, hid=[256, 256], actor_hid=[256]),  # the YAML's critic: one full slab chunk per critic
    'lag_chunked': dict(BASE, hid=[264, 40]),          # a first width above 256: two chunks, the second of one K step
    'lag_limit': dict(BASE, hid=[1028]),               # above DACT_MAX_WIDTH: gemm refused; unasked, stacked runs
}
T.LIMIT.update(CASES)  # test_td3_gpu looks a case up by name: problem(), run_kernel()
T.SEEDS.update(dict.fromkeys(CASES, 3))
LAG = dict(cost_limit=25.0, lagrangian_multiplier_init=0.001, lambda_lr=0.035, lambda_optimizer='Adam',
           lagrangian_upper_bound=0.3)
PID = dict(pid_kp=0.1, pid_ki=0.01, pid_kd=0.01, pid_d_delay=10, pid_delta_p_ema_alpha=0.95,
           pid_delta_d_ema_alpha=0.9, sum_norm=False, diff_norm=False, cost_limit=25.0, penalty_max=1.5,
           lagrangian_multiplier_init=0.001)


@functools.lru_cache(maxsize=None)
def replay(case, lam, dtype):
    """test_td3_gpu.replay with the actor loss of ddpg_lag.py:73-100: the final quantities and the kinks' margin."""
    c, nets, ring, idx, eps = T.problem(case)
    ring = {k: v.to(dtype) for k, v in ring.items()}
    P = {k: [t.to(dtype).clone().requires_grad_(True) for t in v] for k, v in nets.items()}
    Tg = {k: [t.detach().clone() for t in v] for k, v in P.items()}
    rk = ['q0', 'q1'][:c['nq']]
    groups = {'pi': P['pi'], 'r': [t for k in rk for t in P[k]], 'c': P['qc']}
    opt = {k: torch.optim.Adam(v, lr=T.LR) for k, v in groups.items()}
    margin, stats = [], np.zeros((c['steps'], 5))
    pi = lambda p, x: T._fwd(p, x, c['actor_act'], head=True)
    qf = lambda p, x: T._fwd(p, x, c['critic_act'])[:, 0]

    def critic_step(name, keys, sig, actor, noise, row):
        with torch.no_grad():
            a2 = pi(actor, no)
            if noise is not None:
                margin.append(float((c['clip'] - (noise * c['pn']).abs()).abs().min()))
                a2 = a2 + (noise * c['pn']).clamp(-c['clip'], c['clip'])
                margin.append(float((1 - a2.abs()).abs().min()))
                a2 = a2.clamp(-1.0, 1.0)
            tq = [qf(Tg[k], torch.cat([no, a2], 1)) for k in keys]
            if len(tq) == 2:
                margin.append(float((tq[0] - tq[1]).abs().min()))
            y = sig + T.GAMMA * (1 - d) * (torch.min(*tq) if len(tq) == 2 else tq[0])
        q = [qf(P[k], torch.cat([o, a], 1)) for k in keys]
        loss = sum(torch.nn.functional.mse_loss(qk, y) for qk in q)
        row[:] = float(loss.detach()), float(q[0].mean().detach())
        update(name, loss)

    def update(name, loss):
        opt[name].zero_grad()
        loss.backward()
        opt[name].step()

    for t in range(c['steps']):
        o, a, rew, cst, d, no = (ring[k][idx[t]] for k in ('obs', 'act', 'reward', 'cost', 'done', 'next_obs'))
        critic_step('r', rk, rew, Tg['pi'] if c['target_actor'] else P['pi'], eps[t].to(dtype) if c['pn'] else None,
                    stats[t, 0:2])
        critic_step('c', ['qc'], cst, P['pi'], None, stats[t, 3:5])
        if (t + 1) % c['delay'] == 0:
            x = torch.cat([o, pi(P['pi'], o)], 1)
            loss = (-qf(P['q0'], x) + lam * qf(P['qc'], x)).mean() / (1 + lam)
            stats[t, 2] = float(loss.detach())
            update('pi', loss)
            with torch.no_grad():
                for k in P:
                    for tp, p in zip(Tg[k], P[k]):
                        tp.copy_(T.POLYAK * p + (1 - T.POLYAK) * tp)
    cat = lambda ts: np.concatenate([t.detach().double().numpy().ravel() for t in ts])
    mom = lambda ps, name: cat([o.state[p][name] for p in ps for o in opt.values() if p in o.state])
    out = {'stats': stats}
    for q, ps, ts in (('actor', P['pi'], Tg['pi']),
                      ('critic', groups['r'] + groups['c'], [t for k in rk + ['qc'] for t in Tg[k]])):
        out.update({q: cat(ps), q + '_t': cat(ts), q + '_m': mom(ps, 'exp_avg'), q + '_v': mom(ps, 'exp_avg_sq')})
    return out, min(margin, default=1.0)


def lag_step(desc=None, dact=None, lam=None, cfgs=LAG, **kw):
    from omnisafe_amd import td3_step

    if desc is None:  # the store's and the multiplier's tests: any small step
        desc = td3_step.make_desc(2, 1, [4], [4], 'relu', 'relu', 4, 2, True)
        kw.update(gamma=T.GAMMA, polyak=T.POLYAK, lr_actor=T.LR, lr_critic=T.LR)
    st = td3_step.Td3LagStep(desc, lagrange_cfgs=cfgs, window_lens=4, dact=dact, **kw)
    st.multiplier.fill_(st.initial_multiplier if lam is None else lam)  # the device scalar the actor step reads
    return st


def check(monkeypatch, case, dact, lam, route=None):
    from omnisafe_amd import _lib, td3_step

    (ref, margin), f32 = replay(case, lam, torch.float64), replay(case, lam, torch.float32)[0]
    assert margin > 1e-4, f'{case}: a kink argument within {margin:.2e} of its kink'
    monkeypatch.setattr(td3_step, 'Td3Step', functools.partial(lag_step, dact=dact, lam=lam))  # what run_kernel builds
    if case == 'lag_limit' and dact == 'gemm':  # refused, not replaced; unasked, stacked runs
        with pytest.raises(_lib.OsaError):
            T.run_kernel(case)
        dact = ''
        monkeypatch.setattr(td3_step, 'Td3Step', functools.partial(lag_step, dact='', lam=lam))
    got, st = T.run_kernel(case, route)
    assert st.dact == td3_step.DACTS[dact or 'stacked'] and T.padding_nonzeros(st) == 0
    dz, A = st.head_dz(), CASES[case]['A']
    assert int(torch.count_nonzero(dz[:, A:])) == 0 and float(dz[:, :A].abs().sum()) > 0
    for q in T.QUANTITIES:
        e_k, e_32 = T.rel_l2(got[q], ref[q]), T.rel_l2(f32[q], ref[q])
        print(f'{case} {dact or "default"} {route} lambda {lam} {q}: kernel {e_k:.3e} float32 replay {e_32:.3e}')
        assert e_k <= max(4 * e_32, 16 * 2.0 ** -23), (q, e_k, e_32)


@pytest.mark.parametrize('case,lam,route', [(c, lam, None) for c in CASES for lam in (0.0, 0.7, 50.0)]
                         + [('lag_b33', 0.7, 'fused')])  # the route chooses the critics' forward only
@pytest.mark.parametrize('dact', ['gemm', 'stacked'])
def test_step_matches_float64_reference(monkeypatch, case, lam, route, dact):
    check(monkeypatch, case, dact, lam, route)


def push(state, cost):
    """Normalizer._push and normalize (clip 5) in float64, sums in row order: the new state, the normalised costs."""
    (mean, sumsq, cnt), m, x = state, len(cost), np.asarray(cost, np.float64)
    mean_raw = float(np.cumsum(x)[-1]) / m  # (cumsum adds in row order)
    sq = float(np.cumsum((x - mean_raw) * (x - mean_raw))[-1])
    if cnt == 0:
        mean, sumsq, cnt = mean_raw, sq, float(m)
    else:
        total, delta = cnt + m, mean_raw - mean
        mean, sumsq, cnt = mean + delta * m / total, sumsq + (sq + delta * delta * cnt * m / total), total
    std = max(np.sqrt(sumsq / (cnt - 1)), 1e-2) if cnt > 1 else 1.0
    return (mean, sumsq, cnt), [v if cnt <= 1 else min(max((v - mean) / std, -5.0), 5.0) for v in cost]


@pytest.mark.parametrize('n', [1, 3, 300])
def test_store_normalises_the_cost_as_the_reference_normalizer(n):
    """1 row (count <= 1: the raw cost), then n rows each: a constant (std floor 1e-2), a spread and, from a state the
    test writes (100 000 samples of small variance), the +-5 clip; the episodes' sums keep the raw, integer costs."""
    st = lag_step(cost_normalize=True, size=2048, nslots=1)
    spread = [float(v) for v in np.random.default_rng(n).integers(0, 9, n)]
    acc, out = torch.zeros(n, 3, device='cuda'), torch.zeros(n, 3, device='cuda')
    count = torch.zeros(1, dtype=torch.int64, device='cuda')
    state, want, calls = (0.0, 0.0, 0.0), [], [[2.0], [2.0] * n, spread, None, ([1000.0, -1000.0] * n)[:n], spread]
    for k, cost in enumerate(calls):
        if cost is None:
            state = (2.0, 5000.0, 100000.0)
            st.cost_normalizer.copy_(torch.tensor(state, dtype=torch.float64))
            continue
        (state, z), m = push(state, cost), len(cost)
        want += z
        x, done = torch.zeros(m, 2, device='cuda'), torch.full((m,), int(k == 5), dtype=torch.uint8, device='cuda')
        st.store(x, x[:, :1], x[:, 0].contiguous(), torch.tensor(cost, device='cuda'), done, done, x,
                 episodes=(acc[:m], out, count))  # every episode ends with the last call
    got, want = st.ring['cost'][:len(want)].cpu().numpy(), np.asarray(want, np.float64).astype(np.float32)
    assert np.array_equal(got, want) and np.abs(want).max() == 5.0 and want[0] == 2.0 and want[1] == 0.0
    assert tuple(st.state_dict()['cost_normalizer'].tolist()) == state
    assert int(count) == n and float(out[:, 1].double().sum()) == sum(sum(c) for c in calls if c)


@pytest.mark.parametrize('cfgs', [LAG, PID], ids=['lag', 'pid'])
def test_multiplier_matches_the_host_classes(cfgs):
    """window_lens 4: an empty log (lambda stays), then 14 updates (> pid_d_delay): one episode and no carry, 1, 2 and 3
    running episodes behind 3 carried ones (Jc mixes both), windows inside the epoch; bound and ceiling are reached."""
    from omnisafe_amd.lagrange import Lagrange
    from omnisafe_amd.pid_lagrange import PIDLagrangian

    pid = 'pid_kp' in cfgs
    host = PIDLagrangian(**cfgs) if pid else Lagrange(**cfgs)
    st = lag_step(cfgs=cfgs, size=8, nslots=2)
    st.step.fill_(4)  # the round's last row: (4 - 1) % 2
    costs = np.random.default_rng(1).integers(10, 60, 40).astype(np.float32)
    carried, out = [31.0, 7.0, 44.0], torch.zeros(40, 3, device='cuda')
    carry = torch.tensor(carried + [0.0], device='cuda')
    out[:, 1] = torch.as_tensor(costs).cuda()
    count = torch.zeros(1, dtype=torch.int64, device='cuda')
    st.update_multiplier(carry, 0, (None, out, count))
    assert float(st.multiplier) == float(np.float32(st.initial_multiplier)) == float(st.stats[1, 5])
    for u in range(14):
        ncarry, n_ep = (0, 1) if u == 0 else (3, u if u < 4 else 2 * u)
        window = (carried[:ncarry] + [float(v) for v in costs[:n_ep]])[-4:]
        jc = float(np.cumsum(window)[-1]) / len(window)  # oldest first
        host.pid_update(jc) if pid else host.update_lagrange_multiplier(jc)
        count.fill_(n_ep)
        st.update_multiplier(carry, ncarry, (None, out, count))
        got, want = float(st.multiplier), float(np.float32(host.lagrangian_multiplier))
        print(f'update {u}: device {got!r} host {want!r}')
        assert got == want if pid else abs(got - want) <= 16 * 2.0 ** -23 * abs(want), (u, got, want)
        assert float(st.stats[1, 5]) == got
    assert got == np.float32(1.5 if pid else 0.3) and int(st.lag_count) == 14


def test_agent_td3lag_end_to_end(tmp_path):
    import omnisafe_amd

    cfgs = {'train_cfgs': {'total_steps': 128}, 'env_cfgs': {'horizon': 8},
            'logger_cfgs': {'log_dir': str(tmp_path), 'verbose': False, 'save_model_freq': 1, 'window_lens': 4},
            'algo_cfgs': {'steps_per_epoch': 64, 'start_learning_steps': 16, 'batch_size': 8, 'size': 256,
                          'warmup_epochs': 0},
            'lagrange_cfgs': {'lambda_lr': 0.01, 'lagrangian_multiplier_init': 0.5},  # Jc < 25: lambda sinks 0.01 a round
            'model_cfgs': {'actor': {'hidden_sizes': [16, 16]}, 'critic': {'hidden_sizes': [16, 16]}}}
    agent = omnisafe_amd.Agent('TD3Lag', 'SynthNavGoal1-v0', custom_cfgs=cfgs)
    algo = agent.agent
    inner = algo._train_epoch  # noqa: SLF001

    def guarded(epoch):  # the second epoch (the env is reset in the first) enqueues without a host synchronisation
        torch.cuda.set_sync_debug_mode('error' if epoch else 'default')
        try:
            return inner(epoch)
        finally:
            torch.cuda.set_sync_debug_mode('default')

    algo._train_epoch = guarded  # noqa: SLF001
    agent.learn()
    first, second = (np.asarray(algo.epoch_stats[e])[:, 5] for e in (0, 1))
    assert np.all(first == 0.5)  # epoch 0 is not > warmup_epochs: logged as it stands
    assert np.all(np.isfinite(second)) and len(set(second.tolist())) > 1
    assert float(algo._step.cost_normalizer[2]) == 128  # noqa: SLF001  every raw cost went through the normaliser
    played = agent.evaluate(num_episodes=1)
    assert len(played) >= 1 and all(np.isfinite(r[0]) for r, _ in played.values())
