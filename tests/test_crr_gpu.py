"""GPU: the offline CRR / CCRR train step (csrc/crr_kernels.hip through crr_step.CrrStep) against the float64 twin
(tests/crr_twin.py), its draws against their numpy restatement, determinism, graph replay, and the algorithms end to
end through ``omnisafe_amd.Agent``.

Tolerance: error <= K * max(e32, 2^-22) with the project's K = 16 and e32 the float32 twin's own error against the
float64 twin for the same run (tests/golden/crr_twin_f32_error.json, worst of four row orders; written by
test_crr_twin.py) -- relative L2 per parameter tensor, target and Adam moment, relative per logged scalar (worst
step).  Nothing is excluded.  Every ratio error / max(e32, 2^-22) is written out with OSA_WRITE_PROFILES=1 and kept in
profiles/crr_twin_error.md.

Measured: 3042 quantities in 28 runs, worst ratio 10.92, two above 8, both in `one/CRR/1` (B = 1):
Loss_reward_critic 10.92 and the last layer's bias moment of critic_1 9.57.  Their unit is the cancellation in q - y:
the device's q1 = 0.6118 is 1.8 float32 ulp from the float64 value (accumulation order of a 34- and a 96-term dot
product), y = 0.4534, so q - y = 0.158 carries that error 3.9 times larger, the bias gradient 2 (q - y) the same and
the loss (q - y)^2 twice that; the float32 twin lands 0.2 ulp from the float64 q on this one row, and with B = 1 its
four row orders are one order, so e32 is a single sample there.  K stays 16.
"""
import csv
import json
import os

import numpy as np
import pytest
import torch

import crr_twin as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K = 16.0
FLOOR = 2.0 ** -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP, LAG = T.HP, T.LAG
_RATIOS = {}


def _e32():
    with open(os.path.join(ROOT, 'tests', 'golden', 'crr_twin_f32_error.json'), encoding='utf-8') as f:
        return json.load(f)


def device_step(run, wiring='intended', nslots=None, **hp):
    from omnisafe_amd import crr_step

    D, A, a_h, c_h, a_act, c_act, B, S, _ = T.CASES[run['case']]
    desc = crr_step.make_desc(D, A, a_h, c_h, a_act, c_act, B, S, run['pairs'])
    data = {k: torch.from_numpy(v).to(DEV) for k, v in run['data'].items()}
    kw = dict(HP, **hp)
    st = crr_step.CrrStep(desc, data, nslots=nslots or run['nsteps'], wiring=wiring, device=DEV, **kw)
    st.load_actor_state_dict(run['actor'])
    st.load_actor_state_dict(run['adam_actor'][0], 'actor_m')
    st.load_actor_state_dict(run['adam_actor'][1], 'actor_v')
    for p in range(run['pairs']):
        st.load_critic_state_dict(p, run['pair_sds'][p])
        st.load_critic_state_dict(p, run['targets'][p], 'target')
        st.load_critic_state_dict(p, run['adam_pairs'][p][0], 'critic_m')
        st.load_critic_state_dict(p, run['adam_pairs'][p][1], 'critic_v')
    st.adam_step.fill_(T.ADAM_T0)
    st.set_draws(0, run['idx'], run['eps_next'], run['eps_samp'], run['eps_next_c'])
    return st


def device_snapshot(st):
    out = {}

    def put(prefix, sd):
        for k, v in sd.items():
            out[f'{prefix}/{k}'] = v.double().cpu().numpy()
    put('actor', st.actor_state_dict())
    put('actor_m', st.actor_state_dict('actor_m'))
    put('actor_v', st.actor_state_dict('actor_v'))
    for i in range(st.pairs):
        put(f'pair{i}', st.critic_state_dict(i))
        put(f'target{i}', st.critic_state_dict(i, 'target'))
        put(f'pair{i}_m', st.critic_state_dict(i, 'critic_m'))
        put(f'pair{i}_v', st.critic_state_dict(i, 'critic_v'))
    if st.pairs == 2:
        out['lagrange/lambda'] = st.lagrange[:1].double().cpu().numpy()
    return out


def device_stats(st, n, ccrr):
    from omnisafe_amd.crr_step import CRR_STATS, STAT_KEYS

    rows = st.stats[:n].double().cpu().numpy()
    cols = range(len(STAT_KEYS)) if ccrr else CRR_STATS
    return [{STAT_KEYS[c]: float(r[c]) for c in cols} for r in rows]


def padding_is_zero(st):
    lay = st.layout
    am = torch.from_numpy(~lay.real_mask(0)).to(DEV)
    cm = torch.from_numpy(~lay.real_mask(1)).to(DEV)
    for blk in (st.actor, st.actor_m, st.actor_v):
        assert not blk[am].any()
    for blk in (st.critic, st.critic_m, st.critic_v, st.target):
        assert not blk[:, cm].any()


def check(name, st, run, tw64, stats64):
    """Every quantity of the device run within K * max(e32, 2^-22) of the float64 twin; the ratios are kept."""
    err = T.error_table(device_snapshot(st), device_stats(st, run['nsteps'], run['pairs'] == 2), T.snapshot(tw64),
                        stats64)
    e32 = T.unpack_errors(_e32()[name], err)  # (refuses a file whose quantities are not exactly these)
    ratios = {q: err[q] / max(e32[q], FLOOR) for q in err}
    _RATIOS[name] = ratios
    for q in sorted(ratios):
        print(f'{name} {q}: error {err[q]:.3e} e32 {e32[q]:.3e} ratio {ratios[q]:.2f}')
    bad = {q: r for q, r in ratios.items() if not r <= K}
    assert not bad, bad
    padding_is_zero(st)
    for k, v in run['data'].items():  # the dataset keeps its bits
        assert torch.equal(st.data[k].cpu(), torch.from_numpy(v)), k


TABLE = T.run_table()


def run_named(name):
    """A table entry on the device and on the float64 twin, compared."""
    spec = TABLE[name]
    run, tw, stats64 = T.twin_of(spec, torch.float64)
    st = device_step(run, wiring=spec['wiring'], **spec['hp'])
    st.run(run['nsteps'], lagrange_open=spec['open'])
    assert int(st.step.item()) == run['nsteps']
    check(name, st, run, tw, stats64)
    return st, tw


@pytest.mark.parametrize('name', [n for n in TABLE if n.count('/') == 2 and n.rsplit('/', 1)[1].isdigit()])
def test_step_against_float64_twin(name):
    st, _ = run_named(name)
    assert st.adam_step.tolist() == [T.ADAM_T0 + int(name.rsplit('/', 1)[1])] * (1 + st.pairs)


@pytest.mark.parametrize('done_mode', ['zeros', 'ones'])
def test_done_flags(done_mode):
    run_named(f'tiny/CCRR/done-{done_mode}')


@pytest.mark.parametrize('algo', ['CRR', 'CCRR'])
def test_clamp(algo):
    """beta = 0.05 on `tiny`: CCRR clamps a weight at 1e10, CRR stays finite (both asserted on the twin in
    test_crr_twin.py)."""
    st, tw = run_named(f'tiny/{algo}/clamp')
    assert torch.isfinite(st.actor).all()
    if algo == 'CCRR':
        assert float(tw.last['w'].max()) == 1e10  # the clamp is reached


@pytest.mark.parametrize('mode', ['closed', 'open', 'zero'])
def test_multiplier(mode):
    """8 chained steps where step k's weight reads step k - 1's multiplier: gate closed (lambda keeps its bits), open,
    and driven to the 0 clamp (a cost limit far above every Q value, a large step)."""
    lam0 = torch.tensor([T.run_table()[f'tiny/CCRR/lambda-{mode}']['hp']['lambda_init'], 0.0, 0.0, 0.0])
    st, tw = run_named(f'tiny/CCRR/lambda-{mode}')
    if mode == 'closed':
        assert torch.equal(st.lagrange.cpu(), lam0)
    if mode == 'zero':
        assert st.lagrange[0].item() == 0.0 and tw.lam.item() == 0.0


def test_reference_wiring():
    st, _ = run_named('tiny/CCRR/reference-wiring')
    assert st.adam_step.tolist() == [T.ADAM_T0 + 3, T.ADAM_T0 + 6, T.ADAM_T0]  # the reward pair took both updates


def test_wiring_env(monkeypatch):
    from omnisafe_amd import crr_step

    run = T.make_run('tiny', 2, 1)
    monkeypatch.setenv('OSA_CCRR_WIRING', 'reference')
    assert device_step(run, wiring=None).wiring == 'reference'
    monkeypatch.setenv('OSA_CCRR_WIRING', 'sideways')
    with pytest.raises(ValueError):
        device_step(run, wiring=None)
    monkeypatch.delenv('OSA_CCRR_WIRING')
    assert device_step(run, wiring=None).wiring == 'intended'
    assert crr_step.STAT_KEYS[10] == 'Metrics/LagrangeMultiplier'


def test_draws_equal_numpy_restatement():
    """Device indices and both noise blocks of two steps at a non-zero step offset equal crr_twin's numpy draws
    exactly; a block run with device draws equals the same block with those draws injected, bit for bit."""
    D, A, _, _, _, _, B, S, N = T.CASES['tiny']
    run = T.make_run('tiny', 2, 2)
    seed, first = 0x1234ABCD5678, 5
    st = device_step(run, nslots=4, **LAG)
    st.step.fill_(first)
    st.draw(seed, first, 2)
    for k in range(2):
        slot = (first + k) % 4
        assert np.array_equal(st.idx[slot].cpu().numpy(), T.draw_idx(seed, first + k, B, N))
        for buf, key, rows in ((st.eps_next, T.KEY_NEXT, B), (st.eps_next_c, T.KEY_NEXTC, B),
                               (st.eps_samp, T.KEY_SAMP, B * S)):
            want = T.draw_eps(seed, key, first + k, rows, A)
            assert np.array_equal(buf[slot].cpu().numpy().view(np.uint32), want.view(np.uint32))
    slots = [(first + k) % 4 for k in range(2)]
    drawn = [b[slots].cpu() for b in (st.idx, st.eps_next, st.eps_samp, st.eps_next_c)]
    st.run(2, lagrange_open=True)
    st2 = device_step(run, nslots=4, **LAG)
    st2.step.fill_(first)
    st2.set_draws(first, *drawn)
    st2.run(2, lagrange_open=True)
    for a, b in ((st.actor, st2.actor), (st.critic, st2.critic), (st.target, st2.target), (st.lagrange, st2.lagrange),
                 (st.stats, st2.stats)):
        assert torch.equal(a, b)


def test_index_draws_cover_a_one_row_dataset():
    run = T.make_run('one', 1, 1)
    st = device_step(run)
    st.draw(7, 0, 1)
    assert st.idx.tolist() == [[0]]


def test_determinism_and_graph_replay():
    """`tile`, 4 steps: two eager runs give equal bits; a captured single-stream graph of ONE step replayed 4 times
    equals the 4 eager steps bit for bit, the per-step scalars included."""
    run = T.make_run('tile', 2, 4)

    def state(st):
        return [t.clone() for t in (st.actor, st.actor_m, st.actor_v, st.critic, st.critic_m, st.critic_v, st.target,
                                    st.lagrange, st.stats, st.adam_step, st.step)]

    eager = []
    for _ in range(2):
        st = device_step(run, **LAG)
        st.run(4, lagrange_open=True)
        eager.append(state(st))
    for a, b in zip(*eager):
        assert torch.equal(a, b)
    st = device_step(run, **LAG)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        st.run(1, lagrange_open=True)
        graph.capture_end()
    torch.cuda.synchronize()
    for _ in range(4):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager[0], state(st)):
        assert torch.equal(a, b)


def test_argument_checks_on_device_pointers():
    import ctypes as C

    from omnisafe_amd import _lib

    run = T.make_run('tiny', 1, 1)
    st = device_step(run)
    lib = _lib.load()
    before = st.actor.clone()
    rc = lib.osa_crr_step(C.byref(st.desc), C.byref(st.hp), C.byref(st._state), C.byref(st._data), C.byref(st._draws),
                          _lib.ptr(st.stats), _lib.ptr(st.ws), st.ws_floats - 4, 1, _lib.stream_ptr())
    assert rc == -1  # a short workspace: refused before any launch
    torch.cuda.synchronize()
    assert torch.equal(st.actor, before) and int(st.step.item()) == 0


# ---------------------------------------------------------------------------------------------------- end to end
def _dataset(tmp_path, env_id, D, A, N=512, linear=None, seed=3):
    from omnisafe_amd import offline

    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((N, D)).astype(np.float32)
    act = (rng.uniform(-1, 1, (N, A)) if linear is None
           else obs @ linear + 0.05 * rng.standard_normal((N, A))).astype(np.float32)
    arrays = {'obs': obs, 'action': act, 'reward': rng.standard_normal((N, 1)).astype(np.float32),
              'cost': (rng.random((N, 1)) < 0.2).astype(np.float32),
              'next_obs': rng.standard_normal((N, D)).astype(np.float32),
              'done': (rng.random((N, 1)) < 0.05).astype(np.float32)}
    return offline.write_dataset(str(tmp_path / 'data'), env_id, arrays), arrays


def _agent(algo, path, log_dir, total=20, **algo_cfgs):
    import omnisafe_amd

    cfgs = {'seed': 5,
            'train_cfgs': {'device': DEV, 'dataset': path, 'total_steps': total, 'evaluate_epoisodes': 2},
            'algo_cfgs': dict({'steps_per_epoch': 10, 'batch_size': 32, 'sampled_action_num': 3}, **algo_cfgs),
            'model_cfgs': {'actor': {'hidden_sizes': [32, 32]}, 'critic': {'hidden_sizes': [32, 32]}},
            'logger_cfgs': {'save_model_freq': 1, 'log_dir': str(log_dir), 'verbose': False}}
    if algo == 'CCRR':
        cfgs['algo_cfgs']['lagrange_start_step'] = 5
    return omnisafe_amd.Agent(algo, 'SynthReach-v0', custom_cfgs=cfgs)


BASE_KEYS = ['Metrics/EpRet', 'Metrics/EpCost', 'Metrics/EpLen', 'Time/Total', 'Time/Epoch', 'Time/Update',
             'Time/Evaluate', 'Train/Epoch', 'TotalSteps', 'Loss/Loss_reward_critic', 'Loss/Loss_actor', 'Qr/data_Qr',
             'Qr/target_Qr', 'Qr/current_Qr', 'Train/PolicyStd']
CCRR_KEYS = ['Loss/Loss_cost_critic', 'Qc/data_Qc', 'Qc/target_Qc', 'Qc/current_Qc', 'Metrics/LagrangeMultiplier']


@pytest.mark.parametrize('algo', ['CRR', 'CCRR'])
def test_agent_end_to_end(tmp_path, algo):
    from omnisafe_amd.evaluator import Evaluator
    from omnisafe_amd.offline import OfflineDataCollector
    from omnisafe_amd.saved_policy import device_env_class

    D, A = device_env_class('SynthReach-v0').dims('SynthReach-v0')
    path, _ = _dataset(tmp_path, 'SynthReach-v0', D, A)
    runs = []
    for k in range(2):
        agent = _agent(algo, path, tmp_path / f'runs{k}')
        ep_ret, ep_cost, ep_len = agent.learn()
        assert np.isfinite([ep_ret, ep_cost, ep_len]).all()
        log_dir = agent.agent.logger.log_dir
        assert os.path.basename(os.path.dirname(log_dir)) == f'{algo}-{{SynthReach-v0}}-SynthReach-v0_data'
        with open(os.path.join(log_dir, 'progress.csv'), encoding='utf-8') as f:
            rows = list(csv.DictReader(f))
        assert len(rows) == 2
        assert sorted(rows[0]) == sorted(BASE_KEYS + (CCRR_KEYS if algo == 'CCRR' else []))
        assert [float(r['TotalSteps']) for r in rows] == [10.0, 20.0]
        for r in rows:
            assert all(np.isfinite(float(v)) for v in r.values())
        cks = [torch.load(os.path.join(log_dir, 'torch_save', f'epoch-{e}.pt'), weights_only=False) for e in (1, 2)]
        for ck in cks:
            assert list(ck) == ['actor', 'pi'] and list(ck['pi'])[:3] == ['log_std', 'mean.0.weight', 'mean.0.bias']
            for name in ck['pi']:
                assert torch.equal(ck['pi'][name], ck['actor'][name])
        runs.append(([{k2: v for k2, v in r.items() if not k2.startswith('Time/')} for r in rows], cks, log_dir))
    assert runs[0][0] == runs[1][0]  # same seed: same numbers, timing aside
    for a, b in zip(runs[0][1], runs[1][1]):
        for name in a['pi']:
            assert torch.equal(a['pi'][name], b['pi'][name])
    log_dir = runs[0][2]
    ev = Evaluator(device=DEV, verbose=False)
    ev.load_saved(save_dir=log_dir, model_name='epoch-2.pt')
    rets, costs = ev.evaluate(2)
    assert len(rets) == 2 and len(costs) == 2
    col = OfflineDataCollector(64, 'SynthReach-v0', device=DEV)
    col.register_agent(log_dir, 'epoch-2.pt', 64)
    out = agent.evaluate(num_episodes=2)
    assert sorted(out) == ['epoch-1.pt', 'epoch-2.pt']


def test_dataset_from_a_collector_object(tmp_path):
    """`train_cfgs.dataset` may be an object whose `data` is on the device already."""
    import types

    from omnisafe_amd.saved_policy import device_env_class

    D, A = device_env_class('SynthReach-v0').dims('SynthReach-v0')
    _, arrays = _dataset(tmp_path, 'SynthReach-v0', D, A, N=64)
    col = types.SimpleNamespace(data={k: torch.from_numpy(v).to(DEV) for k, v in arrays.items()})
    agent = _agent('CRR', col, tmp_path / 'runs', total=10)
    agent.learn()
    assert agent.agent._step.data['obs'].data_ptr() == col.data['obs'].data_ptr()  # not copied


def test_direction(tmp_path):
    """Actions = a fixed linear map of the observation + small noise, beta = 1e3 (weights ~ 1): 300 CRR steps bring the
    mean distance between mu(obs) and the map's action below its value at step 0, on the device and on the float64
    twin from the same start."""
    from omnisafe_amd.saved_policy import device_env_class

    D, A = device_env_class('SynthReach-v0').dims('SynthReach-v0')
    W = (np.random.default_rng(9).standard_normal((D, A)) * 0.3).astype(np.float32)
    path, arrays = _dataset(tmp_path, 'SynthReach-v0', D, A, linear=W)
    agent = _agent('CRR', path, tmp_path / 'runs', total=300, steps_per_epoch=300, beta=1e3)
    st = agent.agent._step
    obs, target = torch.from_numpy(arrays['obs']).double(), torch.from_numpy(arrays['obs'] @ W).double()

    def distance(actor_sd):
        mean = T.Actor(actor_sd, 'relu', torch.float64).mean
        with torch.no_grad():
            return float((mean(obs) - target).norm(dim=1).mean())

    sd0, pair0 = st.actor_state_dict(), st.critic_state_dict(0)
    sd0, pair0 = ({k: v.cpu() for k, v in sd.items()} for sd in (sd0, pair0))
    d0 = distance(sd0)
    agent.learn()
    d_dev = distance({k: v.cpu() for k, v in st.actor_state_dict().items()})
    tw = T.Twin(sd0, [pair0], 'relu', 'relu', dtype=torch.float64, **dict(HP, beta=1e3))
    rng = np.random.default_rng(1)
    for _ in range(300):
        idx = rng.integers(0, 512, 32)
        tw.step(T.gather(arrays, idx), rng.standard_normal((32, A)), rng.standard_normal((96, A)))
    d_twin = distance({k: v.detach() for k, v in tw.actor.named().items()})
    print(f'distance: start {d0:.4f}, device {d_dev:.4f}, float64 twin {d_twin:.4f}')
    assert d_dev < d0 and d_twin < d0


def test_write_ratio_profile():
    """Runs last in this file: the ratios of every comparison above, for profiles/crr_twin_error.md."""
    if not _RATIOS:  # (selected alone)
        run_named('tiny/CRR/1')
    worst = max(max(r.values()) for r in _RATIOS.values())
    print(f'worst ratio {worst:.2f} over {sum(len(r) for r in _RATIOS.values())} quantities')
    if os.environ.get('OSA_WRITE_PROFILES') == '1':
        out = os.environ.get('OSA_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'crr_twin_error_gpu.json'), 'w', encoding='utf-8') as f:
            json.dump(_RATIOS, f, indent=1, sort_keys=True)
    assert worst <= K
