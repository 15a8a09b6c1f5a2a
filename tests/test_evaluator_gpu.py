"""GPU: omnisafe_amd.Evaluator / Agent.evaluate -- checkpoints written by this package played back on the persistent
kernel (osa_eval_episodes) and on the per-step path, compared with each other bit for bit and with the numpy
statement of the policy and of SynthReach (oracle/np_oracle.py) on the kernel's trace."""
import json
import os

import numpy as np
import pytest
import torch

import np_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HORIZON = 50


def make_checkpoint(root, algo, env_id, env_cfgs=None, model_cfgs=None, algo_cfgs=None, seed=0):
    """config.json + torch_save/epoch-0.pt as the logger writes them, with a randomly initialised actor and
    observation statistics pushed from random data (so that the normaliser is active)."""
    from omnisafe_amd.config import Config, get_default_kwargs
    from omnisafe_amd.envs import SYNTH_DIMS
    from omnisafe_amd.models import ConstraintActorCritic
    from omnisafe_amd.normalizer import Normalizer
    from omnisafe_amd.spaces import Box

    d = get_default_kwargs(algo)
    d.update({'algo': algo, 'env_id': env_id, 'exp_name': f'{algo}-{{{env_id}}}', 'seed': seed,
              'env_cfgs': dict(env_cfgs or {})})
    for k, v in (model_cfgs or {}).items():
        d['model_cfgs'][k].update(v)
    if algo_cfgs:
        d['algo_cfgs'].update(algo_cfgs)
    cfg = Config.dict2config(d)
    os.makedirs(os.path.join(root, 'torch_save'), exist_ok=True)
    with open(os.path.join(root, 'config.json'), 'w', encoding='utf-8') as f:
        json.dump(d, f)
    obs_dim, act_dim = dict(SYNTH_DIMS, **{'SynthReach-v0': (60, 2)})[env_id]
    saute = 'Saute' in algo or 'Simmer' in algo
    torch.manual_seed(seed)
    ac = ConstraintActorCritic(Box(-np.inf, np.inf, (obs_dim + saute,)), Box(-1.0, 1.0, (act_dim,)),
                               cfg.model_cfgs, epochs=1, device=DEV)
    norm = Normalizer((obs_dim,), clip=5, device=DEV)
    g = torch.Generator(device='cpu').manual_seed(seed + 1)
    for _ in range(3):
        norm.push((torch.randn(256, obs_dim, generator=g) * 0.7 + 0.1).to(DEV))
    torch.save({'pi': {k: v.detach().cpu() for k, v in ac.actor.state_dict().items()},
                'obs_normalizer': {k: v.detach().cpu() for k, v in norm.state_dict().items()}},
               os.path.join(root, 'torch_save', 'epoch-0.pt'))
    return root


def play(root, path, monkeypatch, K=64, cost_criteria=1.0, seed=3, trace=True, env=None):
    from omnisafe_amd.evaluator import Evaluator

    monkeypatch.setenv('OSA_EVAL_PATH', path)
    ev = Evaluator(seed=seed, device=DEV, verbose=False, env=env)
    ev.load_saved(str(root), 'epoch-0.pt')
    r, c = ev.evaluate(num_episodes=K, cost_criteria=cost_criteria, trace=trace)
    assert ev.path == path
    tr = ev.trace.cpu().numpy() if ev.trace is not None else None
    return np.array(r), np.array(c), np.array(ev.episode_lengths), tr, ev


def test_agent_evaluate_round_trip(tmp_path):
    """Agent.learn() then Agent.evaluate(): every epoch-N.pt of the run plays back (reference quick-start)."""
    import omnisafe_amd

    cfg = {'seed': 1, 'train_cfgs': {'device': DEV, 'total_steps': 2 * 32 * HORIZON, 'vector_env_nums': 32},
           'algo_cfgs': {'steps_per_epoch': 32 * HORIZON, 'update_iters': 2, 'batch_size': 64},
           'logger_cfgs': {'log_dir': str(tmp_path), 'verbose': False, 'save_model_freq': 1},
           'env_cfgs': {'horizon': HORIZON}}
    agent = omnisafe_amd.Agent('PPOLag', 'SynthReach-v0', custom_cfgs=cfg)
    agent.learn()
    out = agent.evaluate(num_episodes=64)
    names = list(out)
    assert len(names) >= 2 and names == sorted(names, key=lambda n: int(n[len('epoch-'):-len('.pt')]))
    for rewards, costs in out.values():
        assert len(rewards) == 64 and len(costs) == 64
        assert np.isfinite(rewards).all() and np.isfinite(costs).all()
    ev = omnisafe_amd.Evaluator(seed=0, device=DEV, verbose=False)
    ev.load_saved(agent.agent.logger.log_dir, names[-1])
    ev.evaluate(num_episodes=64)
    assert ev.path == 'persistent' and ev.episode_lengths == [float(HORIZON)] * 64


REACH_CASES = [('PPOLag', {}), ('PPOSaute', {'safety_budget': 2.0}), ('PPOEarlyTerminated', {'cost_limit': 1.0})]
SYNTH_SHAPES = ['SynthPointGoal1-v0', 'SynthCarGoal1-v0', 'SynthAnt-v0', 'SynthHumanoid-v0']


@pytest.mark.parametrize('algo,algo_cfgs', REACH_CASES)
def test_persistent_equals_per_step_reach(tmp_path, monkeypatch, algo, algo_cfgs):
    root = make_checkpoint(str(tmp_path), algo, 'SynthReach-v0', {'horizon': HORIZON}, algo_cfgs=algo_cfgs)
    a = play(root, 'persistent', monkeypatch)
    b = play(root, 'per-step', monkeypatch)
    for x, y in zip(a[:4], b[:4]):
        assert x.shape == y.shape and np.array_equal(x, y)
    if algo == 'PPOEarlyTerminated':
        assert (a[2] < HORIZON).any() and (a[2] == HORIZON).any()
    else:
        assert (a[2] == HORIZON).all()
    a2 = play(root, 'persistent', monkeypatch, cost_criteria=0.99, trace=False)
    b2 = play(root, 'per-step', monkeypatch, cost_criteria=0.99, trace=False)
    assert np.array_equal(a2[0], b2[0]) and np.array_equal(a2[2], b2[2])
    np.testing.assert_allclose(a2[1], b2[1], rtol=1e-12, atol=0)


@pytest.mark.parametrize('env_id', SYNTH_SHAPES)
def test_persistent_equals_per_step_synth(tmp_path, monkeypatch, env_id):
    root = make_checkpoint(str(tmp_path), 'PPOLag', env_id, {'horizon': 20, 'cost_p': 0.2})
    a = play(root, 'persistent', monkeypatch, K=40)
    b = play(root, 'per-step', monkeypatch, K=40)
    for x, y in zip(a[:4], b[:4]):
        assert x.shape == y.shape and np.array_equal(x, y)
    assert (a[2] == 20).all() and a[1].sum() > 0


@pytest.mark.parametrize('algo,algo_cfgs', REACH_CASES)
def test_trace_against_numpy_statement(tmp_path, monkeypatch, algo, algo_cfgs):
    """Teacher forcing on the kernel's trace: policy, ActionScale, SynthReach dynamics, sums, early termination and
    the Saute column recomputed in numpy."""
    from omnisafe_amd.config import get_default_kwargs

    root = make_checkpoint(str(tmp_path), algo, 'SynthReach-v0', {'horizon': HORIZON}, algo_cfgs=algo_cfgs)
    ret, cost, length, tr, ev = play(root, 'persistent', monkeypatch, K=64, cost_criteria=0.99)
    saute = algo == 'PPOSaute'
    in_w, A = 60 + saute, 2
    ck = torch.load(os.path.join(root, 'torch_save', 'epoch-0.pt'), weights_only=False)
    actor = O.Actor(in_w, A).double()
    actor.load_state_dict({k: v.double() for k, v in ck['pi'].items()})
    alive = tr[:, :, in_w + A + 2] == 1.0
    T, K = alive.shape
    assert np.array_equal(alive.sum(0), length)
    x, act = tr[:, :, :in_w], tr[:, :, in_w:in_w + A]
    rew, cst, state = tr[:, :, in_w + A], tr[:, :, in_w + A + 1], tr[:, :, in_w + A + 3:in_w + A + 9]
    with torch.no_grad():
        mu = actor.mean(torch.from_numpy(x[alive].astype(np.float64))).numpy()
    lo, hi = -1.0, 1.0
    np.testing.assert_allclose(act[alive], lo + (hi - lo) * (mu + 1.0) / 2.0, rtol=1e-5, atol=1e-6)
    d = get_default_kwargs(algo)['algo_cfgs']
    d.update(algo_cfgs)
    if saute:
        budget = np.float32(d['safety_budget'] * (1 - d['saute_gamma'] ** d['max_ep_len'])
                            / (1 - d['saute_gamma']) / d['max_ep_len'])
        z = np.ones(K, np.float32)
    r_acc, c_acc = np.zeros(K), np.zeros(K)
    for t in range(T):
        m = alive[t]
        if not m.any():
            break
        q, r, c, _ = O.reach_env_step(state[t][m], act[t][m])
        assert np.array_equal(r, rew[t][m]) and np.array_equal(c, cst[t][m])
        nxt = m & alive[t + 1] if t + 1 < T else np.zeros(K, bool)
        if t + 1 < T:
            assert np.array_equal(state[t + 1][nxt][:, :2], q[nxt[m]])
        if saute:
            assert np.array_equal(x[t][m][:, 60], z[m])
            z = ((z - cst[t] / budget).astype(np.float32) / np.float32(d['saute_gamma'])).astype(np.float32)
        r_acc[m] += rew[t][m].astype(np.float64)
        c_acc[m] += (0.99 ** t) * cst[t][m].astype(np.float64)
        if algo == 'PPOEarlyTerminated':  # an episode ends exactly at its first step with cost >= limit
            assert np.array_equal(nxt[m], c_acc[m] < d['cost_limit']) or t + 1 == T
    assert np.array_equal(r_acc, ret)
    np.testing.assert_allclose(c_acc, cost, rtol=1e-12, atol=0)


def test_determinism_and_seed(tmp_path, monkeypatch):
    root = make_checkpoint(str(tmp_path), 'PPOLag', 'SynthReach-v0', {'horizon': HORIZON})
    a = play(root, 'persistent', monkeypatch, seed=7, trace=False)
    b = play(root, 'persistent', monkeypatch, seed=7, trace=False)
    c = play(root, 'persistent', monkeypatch, seed=8, trace=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], c[0])


class _CountdownEnv:
    """A user env with this package's env interface (envs.py docstring): random observations, reward -|a|^2,
    cost 1 when a[0] > 0, terminates after 7 steps."""

    need_auto_reset_wrapper = False
    need_time_limit_wrapper = False

    def __init__(self, num_envs=4):
        from omnisafe_amd.spaces import Box

        self.num_envs = num_envs
        self.observation_space = Box(-np.inf, np.inf, (6,))
        self.action_space = Box(-2.0, 2.0, (2,))
        self._t = 0
        self._g = torch.Generator(device='cpu').manual_seed(0)

    def _obs(self):
        return torch.randn(self.num_envs, 6, generator=self._g).to(DEV)

    def reset(self, seed=None, options=None):
        self._t = 0
        return self._obs(), {}

    def step(self, action):
        self._t += 1
        r = -(action * action).sum(1)
        c = (action[:, 0] > 0).float()
        term = torch.full((self.num_envs,), self._t >= 7, dtype=torch.bool, device=DEV)
        return self._obs(), r, c, term, torch.zeros_like(term), {}

    def set_seed(self, seed):
        pass

    def close(self):
        pass


def test_general_network_and_user_env(tmp_path, monkeypatch):
    monkeypatch.delenv('OSA_EVAL_PATH', raising=False)
    from omnisafe_amd.evaluator import Evaluator

    big = {'actor': {'hidden_sizes': [96, 40, 24]}, 'critic': {'hidden_sizes': [96, 40, 24]}}
    root = make_checkpoint(str(tmp_path / 'g'), 'PPOLag', 'SynthReach-v0', {'horizon': HORIZON}, model_cfgs=big)
    ev = Evaluator(seed=0, device=DEV, verbose=False)
    ev.load_saved(root, 'epoch-0.pt')
    r, c = ev.evaluate(num_episodes=16)
    assert ev.path == 'per-step' and np.isfinite(r).all() and np.isfinite(c).all()
    assert ev.episode_lengths == [float(HORIZON)] * 16
    root = make_checkpoint(str(tmp_path / 'u'), 'PPOLag', 'SynthTiny-v0')
    ev = Evaluator(seed=0, device=DEV, verbose=False, env=_CountdownEnv(4))
    ev.load_saved(root, 'epoch-0.pt')
    r, c = ev.evaluate(num_episodes=10)
    assert ev.path == 'per-step' and len(r) == 10 and np.isfinite(r).all() and np.isfinite(c).all()
    assert ev.episode_lengths == [7.0] * 10
