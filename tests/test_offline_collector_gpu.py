"""GPU: omnisafe_amd.OfflineDataCollector -- the persistent collection kernel (osa_collect_episodes and a custom
library's osa_custom_collect_episodes) against the per-step path bit for bit, against the numpy twins of the envs from
the seed alone, its sampling against ConstraintActorCritic.step, its stores against sentinels, and collect() end to
end.  Horizon 7 throughout: a lane's 20 - 50 rows hold several in-kernel resets and a cut-off last episode."""
import json
import math
import os

import numpy as np
import pytest
import torch

import car_twin
import circle_twin
import custom_env_twin
import ledge_twin as L
import nav_twin

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HERE = os.path.dirname(os.path.abspath(__file__))
H = 7
SEED = 3
FIELDS = ('obs', 'action', 'reward', 'cost', 'next_obs', 'done')
F = np.float32

# env id -> (obs_dim, act_dim, twin of the vector env or None)
ENVS = {
    'SynthReach-v0': (60, 2, None),
    'SynthNavGoal2-v0': (60, 2, lambda K, seed: nav_twin.NavTwin(2, K, H, seed)),
    'SynthNavCircle1-v0': (28, 2, lambda K, seed: circle_twin.CircleTwin(1, K, H, seed)),
    'SynthNavCarGoal1-v0': (72, 2, lambda K, seed: car_twin.CarGoalTwin(1, K, H, seed)),
    'Glider1-v0': (70, 3, lambda K, seed: custom_env_twin.GliderTwin(1, K, H, seed)),
    'Ledge1-v0': (20, 2, None),
}


@pytest.fixture
def custom():
    """glider.h and ledge.h registered for the test."""
    import omnisafe_amd

    ids = {'glider.h': ('Glider', {'Glider0-v0': 0, 'Glider1-v0': 1}), 'ledge.h': ('Ledge', {'Ledge0-v0': 0, 'Ledge1-v0': 1})}
    for name, (struct, levels) in ids.items():
        omnisafe_amd.register_device_env(os.path.join(HERE, 'custom_envs', name), struct, levels, default_horizon=40)
    yield
    omnisafe_amd.unregister_device_env(*[e for _, levels in ids.values() for e in levels])


def make_checkpoint(root, env_id, algo='PPOLag', obs_normalize=True, hidden_sizes=None, seed=0, push_up=False):
    """config.json + torch_save/epoch-0.pt as the logger writes them: a randomly initialised actor with a log_std that
    differs per dimension, and observation statistics pushed from random data.  push_up: the last layer's mean is
    (about) (0, 3) with a small std -- a policy that always pushes the second action against its upper bound."""
    from omnisafe_amd.config import Config, get_default_kwargs
    from omnisafe_amd.models import ConstraintActorCritic
    from omnisafe_amd.normalizer import Normalizer
    from omnisafe_amd.spaces import Box

    obs_dim, act_dim, _ = ENVS[env_id]
    d = get_default_kwargs(algo)
    d.update({'algo': algo, 'env_id': env_id, 'exp_name': f'{algo}-{{{env_id}}}', 'seed': seed,
              'env_cfgs': {'horizon': H}})
    d['algo_cfgs']['obs_normalize'] = obs_normalize
    if hidden_sizes:
        d['model_cfgs']['actor']['hidden_sizes'] = list(hidden_sizes)
        d['model_cfgs']['critic']['hidden_sizes'] = list(hidden_sizes)
    cfg = Config.dict2config(d)
    os.makedirs(os.path.join(root, 'torch_save'), exist_ok=True)
    with open(os.path.join(root, 'config.json'), 'w', encoding='utf-8') as f:
        json.dump(d, f)
    torch.manual_seed(seed)
    ac = ConstraintActorCritic(Box(-np.inf, np.inf, (obs_dim,)), Box(-1.0, 1.0, (act_dim,)), cfg.model_cfgs, epochs=1,
                               device=DEV)
    pi = {k: v.detach().cpu().clone() for k, v in ac.actor.state_dict().items()}
    pi['log_std'] = torch.tensor([-0.6 + 0.25 * i for i in range(act_dim)], dtype=torch.float32)
    if push_up:
        last = sorted(k for k in pi if k.endswith('.bias'))[-1]
        pi[last] = torch.tensor([0.0, 3.0])
        pi[last.replace('bias', 'weight')] *= 0.01
        pi['log_std'] = torch.full((act_dim,), -3.0)
    ck = {'pi': pi}
    if obs_normalize:
        norm = Normalizer((obs_dim,), clip=5, device=DEV)
        g = torch.Generator(device='cpu').manual_seed(seed + 1)
        for _ in range(3):
            norm.push((torch.randn(256, obs_dim, generator=g) * 0.7 + 0.1).to(DEV))
        ck['obs_normalizer'] = {k: v.detach().cpu() for k, v in norm.state_dict().items()}
    torch.save(ck, os.path.join(root, 'torch_save', 'epoch-0.pt'))
    return root


def collect(agents, env_id, K, path, monkeypatch, out_dir, seed=SEED):
    """collect() of `agents` = [(root, rows)] on a forced path; returns (arrays, collector)."""
    import omnisafe_amd

    if path:
        monkeypatch.setenv('OSA_COLLECT_PATH', path)
    else:
        monkeypatch.delenv('OSA_COLLECT_PATH', raising=False)
    col = omnisafe_amd.OfflineDataCollector(sum(n for _, n in agents), env_id, seed=seed, device=DEV, num_envs=K,
                                            env_cfgs={'horizon': H})
    for root, n in agents:
        col.register_agent(str(root), 'epoch-0.pt', n)
    col.collect(str(out_dir))
    assert path in ('', col.path)
    with np.load(os.path.join(str(out_dir), f'{env_id}_data.npz')) as f:
        data = {k: f[k] for k in FIELDS}
    for k in FIELDS:
        assert np.array_equal(col.data[k].cpu().numpy(), data[k])
    return data, col


def rows_for(K, Q=23):
    """S with ceil(S / K) = Q that is no multiple of K (K > 1): a short last lane, and past K = 46 empty ones."""
    S = K * Q - K // 2
    assert -(-S // K) == Q and (K == 1 or S % K)
    return S


def lanes(S, K):
    from omnisafe_amd.offline import lane_layout

    return lane_layout(S, K)


# ------------------------------------------------------------------ 1. persistent = per-step
@pytest.mark.parametrize('K', [1, 3, 17, 130])
@pytest.mark.parametrize('env_id', ['SynthReach-v0', 'SynthNavGoal2-v0', 'SynthNavCircle1-v0', 'SynthNavCarGoal1-v0',
                                    'Glider1-v0'])
def test_persistent_equals_per_step(custom, tmp_path, monkeypatch, env_id, K):
    """K = 1, 3: a partly filled wave; 17: a second workgroup with one lane; 130: nine workgroups, a short lane and
    empty lanes.  With and without the normaliser."""
    S = rows_for(K)
    for normalize in (True, False):
        root = make_checkpoint(str(tmp_path / f'ck{int(normalize)}'), env_id, obs_normalize=normalize)
        a, ca = collect([(root, S)], env_id, K, 'persistent', monkeypatch, tmp_path / 'a')
        b, cb = collect([(root, S)], env_id, K, 'per-step', monkeypatch, tmp_path / 'b')
        for k in FIELDS:
            assert a[k].shape == b[k].shape and a[k].dtype == np.float32
            assert np.array_equal(a[k], b[k]), (k, normalize)
        assert ca.summaries == cb.summaries
        assert a['done'].sum() >= S // H - K and np.isfinite(a['obs']).all() and np.abs(a['action']).max() > 0


# ------------------------------------------------------------------ 2. the numpy twins, from the seed alone
def scaled(action):
    """ActionScale of the recorded sample in float32 (bounds -1 / 1 on both sides), as osa_action_scale1."""
    a = np.asarray(action, np.float32)
    return (F(-1) + ((F(2) * (a - F(-1)).astype(np.float32)).astype(np.float32) / F(2)).astype(np.float32)).astype(
        np.float32)


def lane_rows(data, S, K):
    """The six arrays as [Q][K] rows (NaN where a lane has no row) and the mask of the rows that exist."""
    Q, ranges = lanes(S, K)
    out = {k: np.full((Q, K) + data[k].shape[1:], np.nan, np.float32) for k in FIELDS}
    live = np.zeros((Q, K), bool)
    for lane, (a, b) in enumerate(ranges):
        for k in FIELDS:
            out[k][:b - a, lane] = data[k][a:b]
        live[:b - a, lane] = True
    return out, live


@pytest.mark.parametrize('env_id', ['SynthNavGoal2-v0', 'SynthNavCircle1-v0', 'SynthNavCarGoal1-v0', 'Glider1-v0'])
def test_rows_replay_through_the_twin(custom, tmp_path, monkeypatch, env_id):
    K = 17
    S = rows_for(K)
    root = make_checkpoint(str(tmp_path / 'ck'), env_id)
    data, _ = collect([(root, S)], env_id, K, 'persistent', monkeypatch, tmp_path / 'a')
    rows, live = lane_rows(data, S, K)
    twin = ENVS[env_id][2](K, SEED)  # (agent 0: the env seed is the collector's)
    obs = twin.reset()
    ends = 0
    for t in range(rows['obs'].shape[0]):
        m = live[t]
        assert np.array_equal(rows['obs'][t][m], obs[m]), t
        act = np.where(m[:, None], scaled(rows['action'][t]), F(0))
        out = twin.step(act)
        nobs, r, c, trunc, final = out[:5]
        assert np.array_equal(rows['reward'][t][m, 0], r[m]) and np.array_equal(rows['cost'][t][m, 0], c[m]), t
        assert np.array_equal(rows['next_obs'][t][m], (final if trunc else nobs)[m]), t
        assert np.array_equal(rows['done'][t][m, 0], np.full(m.sum(), F(trunc))), t
        ends += int(trunc)
        obs = nobs
    assert ends == 3  # (23 steps at horizon 7)


def test_terminating_class_ends_rows_as_the_twin(custom, tmp_path, monkeypatch):
    """ledge.h has terminal(): persistent path only.  The checkpoint pushes the second action against its bound, which
    decides every lane's y-path whatever the noise does: under that action the twin ALONE (below, before anything is
    compared) says that these K, Q and seed hold terminating and truncating lanes."""
    env_id, K, level = 'Ledge1-v0', 17, 1
    S = rows_for(K)
    Q, _ = lanes(S, K)
    tw = L.LedgeTwin(level, K, H, SEED)
    tw.reset()
    expect = np.zeros(2, int)
    for t in range(Q):
        out = tw.step(np.tile(np.array([[0.3, 3.0]], np.float32), (K, 1)))
        expect += [out[3].sum(), out[4].sum()]
    assert expect[0] >= 10 and expect[1] >= 10
    root = make_checkpoint(str(tmp_path / 'ck'), env_id, push_up=True)
    data, col = collect([(root, S)], env_id, K, '', monkeypatch, tmp_path / 'a')
    assert col.path == 'persistent'
    rows, live = lane_rows(data, S, K)
    state = L.ledge_reset(SEED, 0, K)
    steps = np.zeros(K, np.int32)
    n_term = n_trunc = 0
    for t in range(Q):
        m = live[t]
        assert np.array_equal(rows['obs'][t][m], L.ledge_obs(state)[m]), t  # after an end: the reset at that position
        act = np.where(m[:, None], scaled(rows['action'][t]), F(0))
        assert (act[m, 1] > 1).all()
        state, r, c = L.ledge_step(state, act, level, SEED, t + 1)
        term = L.ledge_terminal(state)
        count = steps + 1
        trunc = ~term & (count >= H)
        ended = term | trunc
        assert np.array_equal(rows['reward'][t][m, 0], r[m]) and np.array_equal(rows['cost'][t][m, 0], c[m]), t
        assert np.array_equal(rows['done'][t][m, 0], ended[m].astype(np.float32)), t
        assert np.array_equal(rows['next_obs'][t][m], L.ledge_obs(state)[m]), t  # the post-transition observation
        n_term += int((term & m).sum())
        n_trunc += int((trunc & m).sum())
        state[ended] = L.ledge_reset(SEED, t + 1, K)[ended]
        steps = np.where(ended, 0, count).astype(np.int32)
    assert n_term >= 10 and n_trunc >= 10
    monkeypatch.setenv('OSA_COLLECT_PATH', 'per-step')
    with pytest.raises(NotImplementedError, match='terminated step'):
        col.collect(str(tmp_path / 'b'))


# ------------------------------------------------------------------ 3. chain consistency
@pytest.mark.parametrize('env_id', ['SynthNavGoal2-v0', 'SynthNavCircle1-v0'])
def test_chain_consistency(tmp_path, monkeypatch, env_id):
    K = 17
    S = rows_for(K)
    root = make_checkpoint(str(tmp_path / 'ck'), env_id)
    data, _ = collect([(root, S)], env_id, K, 'persistent', monkeypatch, tmp_path / 'a')
    _, ranges = lanes(S, K)
    differs = 0
    for a, b in ranges:
        for i in range(a, b - 1):
            same = np.array_equal(data['obs'][i + 1], data['next_obs'][i])
            if data['done'][i, 0] == 0:
                assert same, i
            else:
                differs += not same
    assert differs >= 1
    assert set(np.unique(data['done'])) == {0.0, 1.0}


# ------------------------------------------------------------------ 4. sampling
def test_sampling(tmp_path, monkeypatch):
    """action = mean + exp(log_std) eps with the eps of a fresh actor seeded noise_seed: eps itself is read off an
    all-zero actor (mean 0, std 1: its sample IS eps) stepped at the same stream positions, and fed through
    ConstraintActorCritic.step(eps=...) of the loaded actor on the normalised obs."""
    from omnisafe_amd.models import ConstraintActorCritic
    from omnisafe_amd.offline import agent_seeds
    from omnisafe_amd.spaces import Box

    env_id, K, Q = 'SynthNavCircle1-v0', 130, 33
    S = K * Q - 65
    D, A, _ = ENVS[env_id]
    assert S * A >= 8192
    root = make_checkpoint(str(tmp_path / 'ck'), env_id)
    data, col = collect([(root, S)], env_id, K, 'persistent', monkeypatch, tmp_path / 'a')
    agent = col.agents[0]
    _, noise_seed = agent_seeds(SEED, 0)
    zero = ConstraintActorCritic(Box(-np.inf, np.inf, (D,)), Box(-1.0, 1.0, (A,)), _model_cfgs(root), epochs=1,
                                 device=DEV)
    zero.params.zero_()
    zero.set_seed(noise_seed)
    x0 = torch.zeros(K, D, device=DEV)
    eps = torch.stack([zero.step(x0, deterministic=False, nets_mask=1)[0].clone() for _ in range(Q)])  # [Q][K][A]
    eps = eps.permute(1, 0, 2).reshape(K * Q, A)[:S].contiguous()
    obs = torch.from_numpy(data['obs']).to(DEV)
    x = agent.normalizer.apply(obs)
    mean = agent.actor.step(x, deterministic=True, nets_mask=1)[0].clone()
    fed = agent.actor.step(x, deterministic=False, eps=eps, nets_mask=1)[0].clone()
    assert np.array_equal(fed.cpu().numpy(), data['action'])
    sd = np.exp(agent.actor.actor.log_std.detach().cpu().numpy().astype(np.float64))[:A]
    z = ((data['action'].astype(np.float64) - mean.cpu().numpy().astype(np.float64)) / sd).reshape(-1)
    n = z.size
    assert n >= 8192
    np.testing.assert_allclose(z, eps.cpu().numpy().astype(np.float64).reshape(-1), rtol=0, atol=1e-5)
    # the mean of n standard normals has standard deviation 1 / sqrt(n), their sample variance sqrt(2 / n): five of each
    assert abs(z.mean()) < 5 / math.sqrt(n)
    assert abs(z.var() - 1) < 5 * math.sqrt(2 / n)


def _model_cfgs(root):
    from omnisafe_amd.config import Config

    with open(os.path.join(root, 'config.json'), encoding='utf-8') as f:
        return Config.dict2config(json.load(f)).model_cfgs


def test_agents_differ_and_the_seed_reproduces_the_file(tmp_path, monkeypatch):
    env_id, K = 'SynthNavCircle1-v0', 3
    S = rows_for(K)
    root = make_checkpoint(str(tmp_path / 'ck'), env_id)
    a, _ = collect([(root, S), (root, S)], env_id, K, 'persistent', monkeypatch, tmp_path / 'a')
    for k in ('obs', 'action', 'reward', 'next_obs'):
        assert not np.array_equal(a[k][:S], a[k][S:]), k
    collect([(root, S), (root, S)], env_id, K, 'persistent', monkeypatch, tmp_path / 'b')
    name = f'{env_id}_data.npz'
    assert open(tmp_path / 'a' / name, 'rb').read() == open(tmp_path / 'b' / name, 'rb').read()
    c, _ = collect([(root, S), (root, S)], env_id, K, 'persistent', monkeypatch, tmp_path / 'c', seed=SEED + 1)
    assert not np.array_equal(a['obs'], c['obs']) and not np.array_equal(a['action'], c['action'])


# ------------------------------------------------------------------ 5. guards
SENTINEL = 0x7FC0BEEF  # a quiet NaN with a payload


@pytest.mark.parametrize('kind,D,K,S,Q', [(32 + 1, 28, 130, 131, 2), (32 + 1, 28, 17, 383, 23), (48 + 1, 72, 17, 383, 23),
                                          (48 + 1, 72, 5, 3, 1)])
def test_nothing_outside_the_block_is_touched(tmp_path, kind, D, K, S, Q):
    """The entry point on strided buffers (ld > width) inside sentinel rows: the short last lane and the lanes with an
    empty range (K = 130, S = 131; K = 5 > S = 3) write nothing past their rows."""
    from omnisafe_amd import _lib

    env_id = 'SynthNavCircle1-v0' if D == 28 else 'SynthNavCarGoal1-v0'
    root = make_checkpoint(str(tmp_path / 'ck'), env_id)
    import omnisafe_amd

    col = omnisafe_amd.OfflineDataCollector(S, env_id, device=DEV)
    col.register_agent(root, 'epoch-0.pt', S)
    ac, nm = col.agents[0].actor, col.agents[0].normalizer
    A, pad = 2, 5
    i32 = dict(dtype=torch.int32, device=DEV)

    def guarded(width, ld):
        return torch.full((S + 2 * pad, ld), SENTINEL, **i32)

    obs, nxt, act = guarded(D, D + 3), guarded(D, D + 9), guarded(A, A + 1)
    rew, cost, done = guarded(1, 1), guarded(1, 1), guarded(1, 1)
    sums = torch.full((2, K + 2), float('nan'), dtype=torch.float64, device=DEV)
    count = torch.full((K + 2,), -7, **i32)
    lo, hi = torch.full((A,), -1.0, device=DEV), torch.full((A,), 1.0, device=DEV)
    ptr = lambda t, row: t[row:].data_ptr()  # noqa: E731
    _lib.check(_lib.load().osa_collect_episodes(
        kind, K, Q, S, D, A, ac.hidden, _lib.ptr(ac.params), _lib.ptr(nm._mean), _lib.ptr(nm._std), _lib.ptr(nm._count),
        5.0, _lib.ptr(lo), _lib.ptr(hi), -1.0, 1.0, SEED, SEED + 1, H, 0.0, ptr(obs, pad), obs.stride(0), ptr(act, pad),
        act.stride(0), ptr(rew, pad), ptr(cost, pad), ptr(nxt, pad), nxt.stride(0), ptr(done, pad),
        sums[0, 1:].data_ptr(), sums[1, 1:].data_ptr(), count[1:].data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    for t, width in ((obs, D), (nxt, D), (act, A), (rew, 1), (cost, 1), (done, 1)):
        t = t.cpu().numpy()
        inside = t[pad:pad + S, :width]
        assert (inside != SENTINEL).all(), 'a row of the block was not written'
        assert np.isfinite(inside.view(np.float32)).all()
        t[pad:pad + S, :width] = SENTINEL
        assert (t == SENTINEL).all(), 'a store outside the block'
    sums, count = sums.cpu().numpy(), count.cpu().numpy()
    assert np.isnan(sums[:, [0, K + 1]]).all() and np.isfinite(sums[:, 1:K + 1]).all()
    assert count[0] == -7 and count[K + 1] == -7
    done = done.cpu().numpy().view(np.float32)[pad:pad + S, 0]
    assert count[1:K + 1].sum() == done.sum()
    _, ranges = lanes(S, K)
    for lane, (a, b) in enumerate(ranges):  # (an empty lane: zero sums and no episode)
        assert count[1 + lane] == done[a:b].sum()
        if a == b:
            assert sums[0, 1 + lane] == 0 and sums[1, 1 + lane] == 0


# ------------------------------------------------------------------ 6. end to end
def learn_checkpoint(algo, log_dir, env_id='SynthNavCircle1-v0'):
    """A one-epoch run (16 envs, horizon 7): (log_dir, name of its last checkpoint)."""
    import omnisafe_amd

    n = 16
    cfg = {'seed': 2, 'train_cfgs': {'device': DEV, 'total_steps': n * 2 * H, 'vector_env_nums': n},
           'algo_cfgs': {'steps_per_epoch': n * 2 * H},
           'logger_cfgs': {'log_dir': log_dir, 'verbose': False, 'save_model_freq': 1},
           'env_cfgs': {'horizon': H}}
    agent = omnisafe_amd.Agent(algo, env_id, custom_cfgs=cfg)
    agent.learn()
    log_dir = agent.agent.logger.log_dir
    names = sorted(os.listdir(os.path.join(log_dir, 'torch_save')), key=lambda s: int(s[len('epoch-'):-len('.pt')]))
    return log_dir, names[-1]


def recomputed(data, start, size, K):
    """data_collector.py:178-194 from the arrays: the lanes' sums in row order in float64, added up exactly."""
    _, ranges = lanes(size, K)
    ret, cost = [], []
    for a, b in ranges:
        r = c = 0.0
        for i in range(start + a, start + b):
            r += float(data['reward'][i, 0])
            c += float(data['cost'][i, 0])
        ret.append(r)
        cost.append(c)
    episodes = float(data['done'][start:start + size].sum())
    return math.fsum(ret) / episodes, math.fsum(cost) / episodes, size / episodes


def test_collect_end_to_end(tmp_path, monkeypatch, capsys):
    import omnisafe_amd
    from omnisafe_amd._lib import OsaError
    from omnisafe_amd.offline import default_num_envs

    env_id = 'SynthNavCircle1-v0'
    monkeypatch.delenv('OSA_COLLECT_PATH', raising=False)
    agents = [learn_checkpoint('PPOLag', str(tmp_path / 'ppolag')) + (60,),
              learn_checkpoint('CPO', str(tmp_path / 'cpo')) + (45,)]
    col = omnisafe_amd.OfflineDataCollector(105, env_id, seed=1, device=DEV, env_cfgs={'horizon': H})
    for agent in agents:
        col.register_agent(*agent)
    capsys.readouterr()
    col.collect(str(tmp_path / 'data'))
    out = capsys.readouterr().out
    assert col.path == 'persistent' and 'Warning' not in out
    with np.load(tmp_path / 'data' / f'{env_id}_data.npz') as f:
        data = {k: f[k] for k in f.files}
    assert sorted(data) == sorted(FIELDS)
    shapes = {'obs': (105, 28), 'action': (105, 2), 'reward': (105, 1), 'cost': (105, 1), 'next_obs': (105, 28),
              'done': (105, 1)}
    for k in FIELDS:
        assert data[k].shape == shapes[k] and data[k].dtype == np.float32 and np.isfinite(data[k]).all()
    printed = [float(line.split(': ')[1]) for line in out.splitlines() if line.startswith('Average ')]
    assert len(printed) == 6 and out.count('data points.') == 2
    start = 0
    for i, (_, _, size) in enumerate(agents):
        K = default_num_envs(size, H)
        assert K == size // H
        assert tuple(printed[3 * i:3 * i + 3]) == recomputed(data, start, size, K)
        start += size
    col.collect(str(tmp_path / 'data'))
    assert 'will be overwritten' in capsys.readouterr().out
    # a general network takes the per-step path and yields a file of the same form
    general = make_checkpoint(str(tmp_path / 'general'), env_id, hidden_sizes=[48, 24])
    g, gc = collect([(general, 105)], env_id, None, '', monkeypatch, tmp_path / 'g')
    assert gc.path == 'per-step' and gc.agents[0].actor.general
    for k in FIELDS:
        assert g[k].shape == shapes[k] and g[k].dtype == np.float32 and np.isfinite(g[k]).all()
    assert g['done'].sum() >= 105 // H - default_num_envs(105, H)
    monkeypatch.setenv('OSA_COLLECT_PATH', 'persistent')
    with pytest.raises(OsaError, match='OSA_COLLECT_PATH=persistent'):
        gc.collect(str(tmp_path / 'g2'))
