"""GPU: offline COptiDICE (csrc/dice_kernels.hip through dice_step.DiceStep) against the torch restatement of
``coptidice.py:162-290`` (tests/dice_twin.py) run on the CPU in float64: three train steps with injected row indices for
every case x fn_type, both clamps, graph replay and determinism, the draws against numpy, the batch bound, and the
algorithm end to end through ``omnisafe_amd.Agent``.

Tolerance: error <= K * max(e32, 2^-22) with the project's K = 16 and e32 the error of the same restatement run in
float32 against the float64 run -- relative L2 per tensor, relative per scalar (worst step).  Nothing is excluded.  With
OSA_WRITE_PROFILES=1 the ratios go to profiles/dice_twin_error.md.
"""
import functools
import os

import dice_twin as T
import numpy as np
import pytest
import torch
from test_vae_gpu import philox

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K, FLOOR = 16.0, 2.0 ** -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLAMPED = dict(lamb0=0.0, tau_init=0.0, cost_limit=1e3, eps=10.0)  # lambda stays at 0, tau at 1e-6
_RATIOS = {}


def errors(t, stats, t64, s64):
    """Relative L2 per tensor and relative per statistics column (worst step); absolute where the reference is zero."""
    err = {q: float(np.linalg.norm(t[q] - t64[q]) / (np.linalg.norm(t64[q]) or 1.0)) for q in t64}
    for c in range(s64.shape[1]):
        err[f'stat{c}'] = float(np.max(np.abs(stats[:, c] - s64[:, c]) / np.where(s64[:, c] == 0, 1.0, np.abs(s64[:, c]))))
    return err


@functools.lru_cache(maxsize=None)
def reference(name, fn, clamped=False):
    """The float64 restatement and the float32 restatement's own error; every branch the case must reach is reached."""
    run, kw = T.make_run(name), CLAMPED if clamped else {}
    t64, s64, seen = T.twin(run, fn, torch.float64, **kw)
    assert clamped or T.branches_wanted(fn) <= seen, (name, fn, seen)
    return t64, s64, errors(*T.twin(run, fn, torch.float32, **kw)[:2], t64, s64)


def device_step(name, fn, nslots=T.STEPS, batch=None, lamb0=T.LAMB0, tau_init=T.TAU_INIT, cost_limit=T.COST_LIMIT,
                eps=T.COST_UB_EPS):
    from omnisafe_amd import dice_step

    run = T.make_run(name)
    desc = dice_step.make_desc(run['D'], run['A'], run['hidden'], {n: run['act'] for n in T.NETS}, batch or run['B'], fn)
    st = dice_step.DiceStep(desc, {k: v.to(DEV) for k, v in run['data'].items()}, gamma=T.GAMMA, alpha=T.ALPHA,
                            cost_limit=cost_limit, cost_ub_eps=eps, lr_nu=T.LR['nu'], lr_chi=T.LR['chi'],
                            lr_actor=T.LR['actor'], lr_lamb=T.LR['lamb'], lr_tau=T.LR['tau'], lamb_init=lamb0,
                            tau_init=tau_init, nslots=nslots, device=DEV)
    for n in T.NETS:
        st.load_state_dict(run[n], n)
    st.set_draws(0, run['idx'])
    return st


def device_tensors(st):
    out = {'lambda': st.mult[:1].double().cpu().numpy(), 'tau': st.mult[4:5].double().cpu().numpy()}
    for tag, which in (('p', ''), ('m', '_m'), ('v', '_v')):
        for n in T.NETS:
            out.update({f'{tag}/{n}/{k}': v.double().cpu().numpy() for k, v in st.state_dict(n, which).items()})
    return out


def steps_against_float64(name, fn, clamped=False):
    t64, s64, e32 = reference(name, fn, clamped)
    st = device_step(name, fn, **(CLAMPED if clamped else {}))
    st.run(T.STEPS)
    assert st.step.tolist() == [T.STEPS] and st.adam_step.tolist() == [T.STEPS, T.STEPS]
    err = errors(device_tensors(st), st.stats[:, :10].double().cpu().numpy(), t64, s64)
    ratios = _RATIOS[f'{name}/{fn}' + '/clamped' * clamped] = {q: err[q] / max(e32[q], FLOOR) for q in err}
    for q in sorted(ratios):
        print(f'{name}/{fn} {q}: error {err[q]:.3e} e32 {e32[q]:.3e} ratio {ratios[q]:.2f}')
    bad = {q: r for q, r in ratios.items() if not r <= K}
    assert not bad, bad
    for k in range(3):  # padding lanes stay zero, the dataset keeps its bits
        mask = torch.from_numpy(~st.layout.real_mask(k)).to(DEV)
        for which in ('', '_m', '_v'):
            assert not getattr(st, T.NETS[k] + which)[mask].any()
    for k, v in T.make_run(name)['data'].items():
        assert torch.equal(st.data[k].cpu(), v), k
    return st


@pytest.mark.parametrize('fn', T.FNS)
@pytest.mark.parametrize('name', list(T.CASES))
def test_steps_against_float64(name, fn):
    steps_against_float64(name, fn)


def test_clamps():
    st = steps_against_float64('ragged', 'softchi', clamped=True)
    assert st.lamb == 0.0 and st.tau == float(np.float32(1e-6))


@pytest.fixture(scope='module', autouse=True)
def write_profile():
    yield
    if os.environ.get('OSA_WRITE_PROFILES') == '1' and _RATIOS:
        with open(os.path.join(ROOT, 'profiles', 'dice_twin_error.md'), 'w', encoding='utf-8') as f:
            f.write('# COptiDICE: error / max(e32, 2^-22) against the float64 restatement (bound 16)\n\n')
            f.write('| case/fn_type | quantities | worst | worst quantity |\n|---|---|---|---|\n')
            for name, r in _RATIOS.items():
                q = max(r, key=r.get)
                f.write(f'| {name} | {len(r)} | {r[q]:.2f} | {q} |\n')


def test_replay_and_determinism():
    eager, again, graphed = (device_step('ragged', 'softchi') for _ in range(3))
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
        for blk in [n + w for n in T.NETS for w in ('', '_m', '_v')] + ['mult', 'stats', 'step', 'adam_step']:
            assert torch.equal(getattr(eager, blk), getattr(other, blk)), blk


def test_draws_equal_numpy():
    st = device_step('ragged', 'kl', nslots=8)
    seed, first, n, N = 0x1234ABCD5678, 7, 5, st.n_rows
    st.draw(seed, first, n)
    for k in range(n):
        w = philox(seed ^ 0x44494345494458, first + k, np.arange(st.B))
        assert st.idx[(first + k) % 8].tolist() == [((int(a) | (int(b) << 32)) * N) >> 64 for a, b in zip(w[0], w[1])]


def test_batch_above_the_bound_is_refused_by_the_layout():
    from omnisafe_amd import _lib, dice_step

    bound = device_step('one', 'kl').layout.max_batch
    assert bound >= 1024
    ok = dice_step.make_desc(3, 1, {n: [8] for n in T.NETS}, {n: 'tanh' for n in T.NETS}, bound, 'kl')
    assert dice_step.DiceLayout(ok).max_batch == bound
    ok.batch = bound + 1
    with pytest.raises(_lib.OsaError):
        dice_step.DiceLayout(ok)


def test_agent_end_to_end(tmp_path):
    import csv

    import omnisafe_amd
    from omnisafe_amd import dice_step
    from omnisafe_amd.saved_policy import load_checkpoint

    from omnisafe_amd import offline
    from omnisafe_amd.saved_policy import device_env_class

    env_id = 'SynthNavCircle1-v0'
    D, A = device_env_class(env_id).dims(env_id)
    rng = np.random.default_rng(5)  # 32 lanes of 16 chained rows, as the collector lays them; the file has no init_obs
    walk = rng.standard_normal((32, 17, D)).astype(np.float32)
    arrays = {'obs': walk[:, :-1].reshape(-1, D), 'next_obs': walk[:, 1:].reshape(-1, D),
              'action': np.tanh(rng.standard_normal((512, A))).astype(np.float32),
              'reward': rng.standard_normal((512, 1)).astype(np.float32),
              'cost': rng.random((512, 1)).astype(np.float32), 'done': np.zeros((512, 1), np.float32)}
    path = offline.write_dataset(str(tmp_path), env_id, arrays)
    small = {'hidden_sizes': [32, 32]}
    cfgs = {'train_cfgs': {'dataset': path, 'total_steps': 8, 'evaluate_epoisodes': 2},
            'algo_cfgs': {'batch_size': 64, 'steps_per_epoch': 4},
            'model_cfgs': {'actor': small, 'nu': small, 'chi': {'hidden_sizes': [32]}},
            'logger_cfgs': {'log_dir': str(tmp_path / 'runs'), 'save_model_freq': 1, 'verbose': False},
            'env_cfgs': {'horizon': 8}}
    agent = omnisafe_amd.Agent('COptiDICE', env_id, custom_cfgs=cfgs)
    agent.learn()
    step, log_dir = agent.agent._step, agent.agent.logger.log_dir
    with open(os.path.join(log_dir, 'progress.csv'), encoding='utf-8') as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 2
    for key in dice_step.STAT_KEYS:
        assert all(np.isfinite(float(r[key])) for r in rows), key
    assert sorted(agent.evaluate(num_episodes=2)) == ['epoch-1.pt', 'epoch-2.pt']
    _, _, ck = load_checkpoint(log_dir, 'epoch-2.pt')
    assert list(ck['actor']) == list(step.state_dict()) and list(ck['actor'])[:2] == ['log_std', 'mean.0.weight']
    init = step.data['init_obs'].cpu().numpy().reshape(32, 16, D)
    assert np.array_equal(init, np.repeat(walk[:, :1], 16, axis=1))
    col = offline.OfflineDataCollector(64, env_id, device=DEV)
    col.register_agent(log_dir, 'epoch-2.pt', 64)
    assert len(col.agents) == 1
