"""GPU: the SynthNavGoal{0,1,2}-v0 device envs (osa_nav_env_step, the SynthNavGoal instantiation of
osa_eval_episodes) against their numpy twin (tests/nav_twin.py) bit for bit, and through the layers that use them:
the captured rollout graph, the evaluator's two paths, AgentGroup, and a directional learning check."""
import csv
import glob
import json
import os

import numpy as np
import pytest
import torch

import nav_twin as T
import raw_env

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = {0: 'SynthNavGoal0-v0', 1: 'SynthNavGoal1-v0', 2: 'SynthNavGoal2-v0'}


# ------------------------------------------------------------------ 1. reset from the seed alone
@pytest.mark.parametrize('level', [0, 1, 2])
@pytest.mark.parametrize('seed', [5, 2 ** 40 + 17])
def test_reset_from_the_seed_alone(level, seed):
    """Pins Philox, the draw allocation and pick_goal together: nothing but the seed goes in."""
    from omnisafe_amd import envs

    N = 1024
    env = envs.make(IDS[level], num_envs=N, device=DEV)
    assert env.level == level and env.max_episode_steps == 1000 and env.graph_safe
    assert env.observation_space.shape == (60,) and env.action_space.shape == (2,)
    env.set_seed(seed)
    obs, _ = env.reset()
    assert env.state.shape == (N, 64)
    state = env.state.cpu().numpy()
    np.testing.assert_array_equal(state, T.nav_reset(seed, 0, N, level))
    np.testing.assert_array_equal(obs.cpu().numpy(), T.nav_obs(state, level))
    obs2, _ = env.reset()  # the next stream position: a different layout
    np.testing.assert_array_equal(env.state.cpu().numpy(), T.nav_reset(seed, 1, N, level))
    assert not np.array_equal(obs2.cpu().numpy(), obs.cpu().numpy())


# ------------------------------------------------------------------ 2. trace
@pytest.mark.parametrize('level', [0, 1, 2])
@pytest.mark.parametrize('N', [1, 3, 130])
def test_raw_launches_equal_the_twin(level, N):
    """Raw launches of osa_nav_env_step on buffers of the test's own (the Point and the Car Goal kernels are one
    template; test_car_env_gpu.py does the same for the Car): 7 steps at horizon 3 (truncations with same-position
    resets at steps 3 and 6) from stream base 2 under actions 1.5 randn, at obs_dim = ld_obs = 60 and at obs_dim = 68 in
    rows of 72: everything the launch writes equals the twin at every step, the pad columns are zero, the final
    observation is written on the truncating step only, and nothing else is written."""
    W, H, seed, steps = 60, 3, 11 + level, 7
    for obs_dim, ld in ((W, W), (W + 8, W + 12)):
        env = raw_env.RawEnv('osa_nav_env_step', 64, level, N, obs_dim, ld, H, seed)
        twin = T.NavTwin(level, N, H, seed)
        env.base.fill_(2)  # the device part of the stream position (graph replay): the episode starts at position 2
        twin.pos = 2
        assert env.launch(0, None, 1) == 0
        np.testing.assert_array_equal(env.obs[:N, :W].cpu().numpy(), twin.reset())
        assert not env.obs[:N, W:obs_dim].any() and int(env.steps[:N].abs().sum()) == 0
        assert bool((env.final == raw_env.SENTINEL).all()) and bool((env.reward == raw_env.SENTINEL).all())
        gen = torch.Generator(device='cpu').manual_seed(100 * level + N)
        for t in range(steps):
            act = torch.randn(N, 2, generator=gen) * 1.5
            assert env.launch(t + 1, act.to(DEV), 0) == 0
            o_exp, r_exp, c_exp, done, final, _ = twin.step(act.numpy())
            assert done == ((t + 1) % H == 0)
            np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp)
            np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp)
            assert not env.term[:N].any() and bool((env.trunc[:N] == int(done)).all())
            assert bool((env.steps[:N] == (t + 1) % H).all())
            if done:
                np.testing.assert_array_equal(env.final[:N, :W].cpu().numpy(), final)
                assert not env.final[:N, W:obs_dim].any()
                env.final.fill_(raw_env.SENTINEL)
            else:
                assert bool((env.final == raw_env.SENTINEL).all())  # written on the truncating step only
            np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state)
            np.testing.assert_array_equal(env.obs[:N, :W].cpu().numpy(), o_exp)
            assert not env.obs[:N, W:obs_dim].any()
            assert env.pads_untouched(), (obs_dim, t)


@pytest.mark.parametrize('level', [0, 1, 2])
def test_trace_equals_the_twin(level):
    """2 H + 3 steps at H = 20 under actions 1.5 randn (about half of the components clamp): everything the env
    returns and its state equal the twin at every step.  The branch counts are the issue's (goals > 10, cost steps
    > 500); the twin alone gives 158 / 138 / 160 goals and 0 / 4476 / 7075 cost steps for these seeds."""
    from omnisafe_amd import envs

    N, H, seed = 1024, 20, 5
    env = envs.make(IDS[level], num_envs=N, device=DEV, horizon=H, seed=seed)
    twin = T.NavTwin(level, N, H, seed)
    obs, _ = env.reset()
    np.testing.assert_array_equal(obs.cpu().numpy(), twin.reset())
    gen = torch.Generator(device='cpu').manual_seed(level)
    n_reached = n_cost = 0
    for t in range(2 * H + 3):
        act = torch.randn(N, 2, generator=gen) * 1.5
        obs, reward, cost, term, trunc, info = env.step(act.to(DEV))
        o_exp, r_exp, c_exp, done, final, reached = twin.step(act.numpy())
        assert done == ((t + 1) % H == 0)
        assert bool(trunc.all()) == done and bool(trunc.any()) == done and not bool(term.any())
        np.testing.assert_array_equal(reward.cpu().numpy(), r_exp)
        np.testing.assert_array_equal(cost.cpu().numpy(), c_exp)
        if done:
            assert bool(info['_final_observation'].all())
            np.testing.assert_array_equal(info['final_observation'].cpu().numpy(), final)
        else:
            assert 'final_observation' not in info
        np.testing.assert_array_equal(env.state.cpu().numpy(), twin.state)
        np.testing.assert_array_equal(obs.cpu().numpy(), o_exp)
        n_reached += int(reached.sum())
        n_cost += int(c_exp.sum())
    print(f'level {level}: goals reached {n_reached}, cost steps {n_cost}')
    assert n_reached > 10
    if level == 0:
        assert n_cost == 0
    else:
        assert n_cost > 500


def test_strided_actions_and_argument_checks():
    from omnisafe_amd import _lib, envs

    env = envs.make(IDS[2], num_envs=64, device=DEV, horizon=7, seed=1)
    twin = T.NavTwin(2, 64, 7, 1)
    env.reset()
    twin.reset()
    wide = torch.randn(64, 5, generator=torch.Generator(device='cpu').manual_seed(0)).to(DEV)
    obs, reward, *_ = env.step(wide[:, 1:3])  # a row stride of 5
    o_exp, r_exp, *_ = twin.step(wide[:, 1:3].cpu().numpy())
    np.testing.assert_array_equal(obs.cpu().numpy(), o_exp)
    np.testing.assert_array_equal(reward.cpu().numpy(), r_exp)
    lib = _lib.load(require_gpu=True)
    p = _lib.ptr
    st, steps, o = env.state, env._steps, env._obs[0]
    bad_level = lib.osa_nav_env_step(0, 0, None, 64, 60, 7, 3, p(st), p(steps), None, 0, p(o), 60, None, None, None,
                                     None, None, 0, 1, _lib.stream_ptr())
    narrow = lib.osa_nav_env_step(0, 0, None, 64, 59, 7, 1, p(st), p(steps), None, 0, p(o), 60, None, None, None,
                                  None, None, 0, 1, _lib.stream_ptr())
    no_action = lib.osa_nav_env_step(0, 0, None, 64, 60, 7, 1, p(st), p(steps), None, 0, p(o), 60, None, None, None,
                                     None, None, 0, 0, _lib.stream_ptr())
    assert bad_level == -1 and narrow == -1 and no_action == -1


# ------------------------------------------------------------------ 3. graph replay
def test_rollout_graph_replay_equals_eager_launches(tmp_path, monkeypatch):
    """OnPolicyAdapter.rollout on the env inside the captured hipGraph against eager launches: the buffers of every
    epoch are identical (four epochs: the graph is captured on the second and replayed afterwards)."""
    import omnisafe_amd

    def run(graph):
        monkeypatch.setenv('OSA_ROLLOUT_GRAPH', '1' if graph else '0')
        cfg = {'seed': 7, 'train_cfgs': {'device': DEV, 'total_steps': 4 * 64 * 24, 'vector_env_nums': 64},
               'algo_cfgs': {'steps_per_epoch': 64 * 24, 'update_iters': 2},
               'logger_cfgs': {'log_dir': str(tmp_path / ('g' if graph else 'e')), 'verbose': False},
               'env_cfgs': {'horizon': 10}}  # truncations at steps 10 and 20 of the 24
        algo = omnisafe_amd.Agent('PPOLag', IDS[1], custom_cfgs=cfg).agent
        snaps = []
        for _ in range(4):
            algo._env.rollout(steps_per_epoch=algo._steps_per_epoch, agent=algo._actor_critic, buffer=algo._buf,
                              logger=algo._logger)
            snap = {k: v.clone() for k, v in algo._buf.data.items()}
            snap['norm_mean'] = algo._env._obs_normalizer._mean.clone()
            snap['env_state'] = algo._env._env.state.clone()
            algo._update()
            snap['params'] = algo._actor_critic.params.clone()
            snaps.append(snap)
            algo._logger.dump_tabular()
        return algo, snaps

    a_g, s_g = run(True)
    a_e, s_e = run(False)
    assert a_g._env.last_rollout_graphed is True and not getattr(a_e._env, 'last_rollout_graphed', False)
    for ep, (g, e) in enumerate(zip(s_g, s_e)):
        for k in g:
            assert torch.equal(g[k].cpu(), e[k].cpu()), (ep, k)
    assert float(s_g[0]['cost'].sum()) > 0 and not torch.equal(s_g[2]['obs'], s_g[3]['obs'])


# ------------------------------------------------------------------ 4. evaluator
def make_checkpoint(root, algo, env_id, env_cfgs, seed=0):
    """config.json + torch_save/epoch-0.pt as the logger writes them: a randomly initialised actor and observation
    statistics pushed from random data (so that the normaliser is active)."""
    from omnisafe_amd.config import Config, get_default_kwargs
    from omnisafe_amd.models import ConstraintActorCritic
    from omnisafe_amd.normalizer import Normalizer
    from omnisafe_amd.spaces import Box

    d = get_default_kwargs(algo)
    d.update({'algo': algo, 'env_id': env_id, 'exp_name': f'{algo}-{{{env_id}}}', 'seed': seed,
              'env_cfgs': dict(env_cfgs)})
    cfg = Config.dict2config(d)
    os.makedirs(os.path.join(root, 'torch_save'), exist_ok=True)
    with open(os.path.join(root, 'config.json'), 'w', encoding='utf-8') as f:
        json.dump(d, f)
    torch.manual_seed(seed)
    ac = ConstraintActorCritic(Box(-np.inf, np.inf, (60,)), Box(-1.0, 1.0, (2,)), cfg.model_cfgs, epochs=1,
                               device=DEV)
    norm = Normalizer((60,), clip=5, device=DEV)
    g = torch.Generator(device='cpu').manual_seed(seed + 1)
    for _ in range(3):
        norm.push((torch.randn(256, 60, generator=g) * 0.3 + 0.1).to(DEV))
    torch.save({'pi': {k: v.detach().cpu() for k, v in ac.actor.state_dict().items()},
                'obs_normalizer': {k: v.detach().cpu() for k, v in norm.state_dict().items()}},
               os.path.join(root, 'torch_save', 'epoch-0.pt'))
    return root


def play(root, path, monkeypatch, K, seed=3):
    from omnisafe_amd.evaluator import Evaluator

    if path:
        monkeypatch.setenv('OSA_EVAL_PATH', path)
    else:
        monkeypatch.delenv('OSA_EVAL_PATH', raising=False)
    ev = Evaluator(seed=seed, device=DEV, verbose=False)
    ev.load_saved(str(root), 'epoch-0.pt')
    r, c = ev.evaluate(num_episodes=K, trace=True)
    return np.array(r), np.array(c), np.array(ev.episode_lengths), ev.trace.cpu().numpy(), ev


def test_evaluator_persistent_equals_per_step_and_replays_through_the_twin(tmp_path, monkeypatch):
    H, K, seed = 40, 72, 3  # 72 episodes: four full waves and a half-filled one
    root = make_checkpoint(str(tmp_path), 'PPOLag', IDS[1], {'horizon': H})
    a = play(root, 'persistent', monkeypatch, K, seed)
    b = play(root, 'per-step', monkeypatch, K, seed)
    assert a[4].path == 'persistent' and b[4].path == 'per-step'
    for x, y in zip(a[:4], b[:4]):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x, y)
    assert play(root, '', monkeypatch, K, seed)[4].path == 'persistent'  # the default
    ret, cost, length, tr, ev = a
    assert (length == H).all() and tr.shape == (H, K, 60 + 2 + 3 + 64)
    x, act = tr[:, :, :60], tr[:, :, 60:62]
    rew, cst, alive, state = tr[:, :, 62], tr[:, :, 63], tr[:, :, 64], tr[:, :, 65:]
    assert (alive == 1).all()
    mean, std = ev._normalizer._mean.cpu().numpy(), ev._normalizer._std.cpu().numpy()
    np.testing.assert_array_equal(state[0], T.nav_reset(seed, 0, K, 1))
    for t in range(H):
        o = T.nav_obs(state[t], 1)
        np.testing.assert_array_equal(x[t], np.clip(((o - mean).astype(np.float32) / std).astype(np.float32), -5, 5))
        s2, r, c, _ = T.nav_step(state[t], act[t], 1, seed, t + 1)
        np.testing.assert_array_equal(rew[t], r)
        np.testing.assert_array_equal(cst[t], c)
        if t + 1 < H:
            np.testing.assert_array_equal(state[t + 1], s2)
    np.testing.assert_array_equal(ret, rew.astype(np.float64).cumsum(0)[-1])
    np.testing.assert_array_equal(cost, cst.astype(np.float64).sum(0))
    assert cost.sum() > 0


# ------------------------------------------------------------------ 5. group
def _outcome(agent):
    ac = agent.agent._actor_critic  # noqa: SLF001
    torch.cuda.synchronize()
    lines = [ln for ln in open(os.path.join(agent.agent.logger.log_dir, 'progress.csv')).read().split('\n') if ln]
    hdr = lines[0].split(',')
    keep = [i for i, h in enumerate(hdr) if not h.startswith('Time/')]
    return ac.params.clone(), [[ln.split(',')[i] for i in keep] for ln in lines]


def test_group_of_two_seeds_equals_two_solo_agents(tmp_path):
    import omnisafe_amd

    def cfgs(log_dir):
        return {'train_cfgs': {'device': DEV, 'total_steps': 2 * 64 * 40, 'vector_env_nums': 64},
                'algo_cfgs': {'steps_per_epoch': 64 * 40},
                'logger_cfgs': {'log_dir': log_dir, 'save_model_freq': 1000},
                'env_cfgs': {'horizon': 20}}

    seeds = [3, 4]
    solos = []
    for s in seeds:
        a = omnisafe_amd.Agent('PPOLag', IDS[1], custom_cfgs=dict(cfgs(str(tmp_path / f'solo{s}')), seed=s))
        a.learn()
        solos.append(_outcome(a))
    group = omnisafe_amd.AgentGroup('PPOLag', IDS[1], seeds=seeds, custom_cfgs=cfgs(str(tmp_path / 'group')))
    assert len(group.learn()) == 2
    for s, member, solo in zip(seeds, group.agents, solos):
        params, rows = _outcome(member)
        assert torch.equal(params, solo[0]), s
        assert rows == solo[1] and len(rows) == 3, s
    assert not torch.equal(solos[0][0], solos[1][0])


# ------------------------------------------------------------------ 6. learning, directional
LEARN = {'vector_env_nums': 256, 'steps_per_epoch': 51_200, 'epochs': 10, 'horizon': 200, 'seeds': 4,
         # the YAML's cost_limit of 25 is meant for 1000-step episodes; at 200 steps the same rate is 5, which binds
         # against the untrained policy's EpCost (the unscaled 25 would leave the multiplier at zero)
         'cost_limit': 5.0}


def train(algo, level, seed, log_dir):
    import omnisafe_amd

    c = LEARN
    custom = {'seed': seed,
              'train_cfgs': {'device': DEV, 'total_steps': c['steps_per_epoch'] * c['epochs'],
                             'vector_env_nums': c['vector_env_nums']},
              'algo_cfgs': {'steps_per_epoch': c['steps_per_epoch']},
              'logger_cfgs': {'log_dir': log_dir, 'save_model_freq': 1000},
              'env_cfgs': {'horizon': c['horizon']}}
    if algo == 'PPOLag':
        custom['lagrange_cfgs'] = {'cost_limit': c['cost_limit']}
    omnisafe_amd.Agent(algo, IDS[level], custom_cfgs=custom).learn()
    path = glob.glob(os.path.join(log_dir, '*', f'seed-{str(seed).zfill(3)}-*', 'progress.csv'))[0]
    rows = list(csv.DictReader(open(path)))
    return {k: np.array([float(r[f'Metrics/{k}']) for r in rows]) for k in ('EpRet', 'EpCost')}


def twin_untrained_policy_rates(level, horizon, std):
    """Per-episode return and cost of 1024 twin episodes under actions N(0, std^2): what an untrained Gaussian policy
    (mean near 0) does."""
    env = T.NavTwin(level, 1024, horizon, 123)
    env.reset()
    rng = np.random.default_rng(0)
    ret, cost = np.zeros(1024), np.zeros(1024)
    for _ in range(horizon):
        _, r, c, *_ = env.step((rng.standard_normal((1024, 2)) * std).astype(np.float32))
        ret += r
        cost += c
    return ret, cost


def consistent(ours, twin, rel):
    """|seed-mean of ours - mean of the twin's episodes| within four standard errors of the difference (ours: over
    seeds; the twin's: over episodes) plus `rel` of the twin's value for what the twin's stand-in policy leaves out
    (the untrained actor's mean is small, not zero, and it sees normalised observations)."""
    se = np.sqrt(ours.std(ddof=1) ** 2 / len(ours) + twin.std(ddof=1) ** 2 / len(twin))
    return abs(ours.mean() - twin.mean()) <= 4 * se + rel * abs(twin.mean())


@pytest.mark.parametrize('algo,level', [('PPOLag', 1), ('PPO', 0)])
def test_learning_directional(algo, level, tmp_path):
    """A sanity statement, not a parity claim (no reference curve exists for an env of this package's own): over 4
    seeds, the seed-mean EpRet of the last three epochs exceeds the first epoch's by more than two standard errors of
    the difference; for PPOLag the tail EpCost is not above the first epoch's by more than two standard errors.  The
    first epoch itself must look like the twin under an untrained policy's actions."""
    c = LEARN
    curves = [train(algo, level, s, str(tmp_path / f's{s}')) for s in range(c['seeds'])]
    ret = np.stack([cv['EpRet'] for cv in curves])
    cost = np.stack([cv['EpCost'] for cv in curves])
    assert ret.shape == (c['seeds'], c['epochs'])
    print(algo, level, 'EpRet seed-mean per epoch', np.round(ret.mean(0), 3).tolist())
    print(algo, level, 'EpCost seed-mean per epoch', np.round(cost.mean(0), 3).tolist())
    d_ret = ret[:, -3:].mean(1) - ret[:, 0]
    se_ret = d_ret.std(ddof=1) / np.sqrt(len(d_ret))
    print(algo, level, 'EpRet tail - first', d_ret.mean(), 'se', se_ret)
    # the untrained policy: near-zero-mean Gaussian actions with the actor's initial log_std of 0
    t_ret, t_cost = twin_untrained_policy_rates(level, c['horizon'], std=1.0)
    print(algo, level, 'first epoch EpRet / EpCost', ret[:, 0].mean(), cost[:, 0].mean(), 'twin', t_ret.mean(),
          t_cost.mean())
    assert consistent(ret[:, 0], t_ret, 0.25)
    if level == 0:
        assert (cost == 0).all()
    else:
        assert consistent(cost[:, 0], t_cost, 0.25)
    assert d_ret.mean() > 2 * se_ret
    if algo == 'PPOLag':
        d_cost = cost[:, -3:].mean(1) - cost[:, 0]
        se_cost = d_cost.std(ddof=1) / np.sqrt(len(d_cost))
        print(algo, level, 'EpCost tail - first', d_cost.mean(), 'se', se_cost)
        assert d_cost.mean() <= 2 * se_cost
