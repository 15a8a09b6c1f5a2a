"""GPU: the SynthNavCircle{0,1,2}-v0 device envs (osa_circle_env_step: half a wave per env; the SynthNavCircle
instantiation of osa_eval_episodes) against their numpy twin (tests/circle_twin.py) bit for bit, and through the layers
that use them at observation width 28: the captured rollout graph, the evaluator's two paths, AgentGroup, the
trust-region updates, and a directional learning check."""
import csv
import functools
import os

import numpy as np
import pytest
import torch

import circle_twin as T
import raw_env

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
IDS = {0: 'SynthNavCircle0-v0', 1: 'SynthNavCircle1-v0', 2: 'SynthNavCircle2-v0'}
SENTINEL = -777.0


# ------------------------------------------------------------------ 1. reset from the seed alone
@pytest.mark.parametrize('level', [0, 1, 2])
@pytest.mark.parametrize('seed', [5, 2 ** 40 + 17])
def test_reset_from_the_seed_alone(level, seed):
    """Pins Philox, the env's own key and the draw allocation: nothing but the seed goes in.  N = 3: one full
    workgroup and one whose second half-wave has no env."""
    from omnisafe_amd import envs

    N = 3
    env = envs.make(IDS[level], num_envs=N, device=DEV)
    assert env.level == level and env.max_episode_steps == 500 and env.graph_safe
    assert env.observation_space.shape == (28,) and env.action_space.shape == (2,)
    assert float(env.action_space.low.min()) == -1 and float(env.action_space.high.max()) == 1
    env.set_seed(seed)
    obs, _ = env.reset()
    assert env.state.shape == (N, 8) and obs.shape == (N, 28)
    state = env.state.cpu().numpy()
    np.testing.assert_array_equal(state, T.circle_reset(seed, 0, N))
    np.testing.assert_array_equal(obs.cpu().numpy(), T.circle_obs(state))
    assert int(env._steps.abs().sum()) == 0
    obs2, _ = env.reset()  # the next stream position: another start
    np.testing.assert_array_equal(env.state.cpu().numpy(), T.circle_reset(seed, 1, N))
    assert not np.array_equal(obs2.cpu().numpy(), obs.cpu().numpy()) and obs2.data_ptr() != obs.data_ptr()


# ------------------------------------------------------------------ 2. trace
RawEnv = functools.partial(raw_env.RawEnv, 'osa_circle_env_step', 8)


@pytest.mark.parametrize('level', [0, 1, 2])
@pytest.mark.parametrize('N', [1, 3, 130])
def test_trace_equals_the_twin(level, N):
    """20 steps at horizon 7 (truncations with same-position resets at steps 7 and 14) under actions 1.5 randn (about
    half of the components clamp), N = 1 (a lone half-wave), 3 (an idle half-wave) and 130 (65 workgroups), at
    obs_dim = ld_obs = 28 and at obs_dim 40 in rows of 48: everything the launch writes equals the twin at every step,
    columns 28 .. 39 are zero, and nothing else is written."""
    H, seed, steps = 7, 11 + level, 20
    for obs_dim, ld in ((28, 28), (40, 48)):
        env = RawEnv(level, N, obs_dim, ld, H, seed)
        twin = T.CircleTwin(level, N, H, seed)
        env.base.fill_(2)  # the device part of the stream position (graph replay): the episode starts at position 2
        twin.pos = 2
        assert env.launch(0, None, 1) == 0
        np.testing.assert_array_equal(env.obs[:N, :28].cpu().numpy(), twin.reset())
        assert not env.obs[:N, 28:obs_dim].any() and int(env.steps[:N].abs().sum()) == 0
        assert bool((env.final == SENTINEL).all()) and bool((env.reward == SENTINEL).all())
        gen = torch.Generator(device='cpu').manual_seed(100 * level + N)
        n_cost = n_clamped = 0
        for t in range(steps):
            act = torch.randn(N, 2, generator=gen) * 1.5
            assert env.launch(t + 1, act.to(DEV), 0) == 0
            o_exp, r_exp, c_exp, done, final = twin.step(act.numpy())
            assert done == ((t + 1) % H == 0)
            np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp)
            np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp)
            assert not env.term[:N].any() and bool((env.trunc[:N] == int(done)).all())
            assert bool((env.steps[:N] == (t + 1) % H).all())
            if done:
                np.testing.assert_array_equal(env.final[:N, :28].cpu().numpy(), final)
                assert not env.final[:N, 28:obs_dim].any()
                env.final.fill_(SENTINEL)
            else:
                assert bool((env.final == SENTINEL).all())  # written on the truncating step only
            np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state)
            np.testing.assert_array_equal(env.obs[:N, :28].cpu().numpy(), o_exp)
            assert not env.obs[:N, 28:obs_dim].any()
            assert env.pads_untouched(), (obs_dim, t)
            n_cost += int(c_exp.sum())
            n_clamped += int((act.abs() > 1).sum())
        assert n_clamped > N * steps // 2
        if level == 0:
            assert n_cost == 0
    print(f'level {level} N {N}: cost steps {n_cost}, clamped components {n_clamped}')


@pytest.mark.parametrize('level', [0, 1, 2])
def test_costs_and_walls_from_states_of_the_callers_own(level):
    """The short episodes above seldom leave the corridor.  The state matrix is the caller's: 130 envs placed all over
    the arena [-2, 2]^2 at speed, one step each -- costs on both walls of both pairs, positions clipped at the arena's
    edge, rewards of either sign at every radius."""
    N = 130
    env = RawEnv(level, N, 28, 28, 7, 1)
    assert env.launch(0, None, 1) == 0
    rng = np.random.default_rng(level)
    s = np.zeros((N, 8), np.float32)
    s[:, 0:2] = rng.uniform(-2, 2, (N, 2))
    h = rng.standard_normal((N, 2))
    s[:, 2:4] = h / np.linalg.norm(h, axis=1, keepdims=True)
    s[:, 4] = rng.uniform(-0.2, 0.2, N)
    s[:, 5] = rng.uniform(-0.2, 0.2, N)
    s[:4, 0:2] = [[0.75, 0.0], [-0.75, 0.0], [0.0, 0.75], [0.0, 0.0]]  # on a wall (no cost); at the origin (reward 0)
    s[:4, 4] = 0
    env.state[:N] = torch.from_numpy(s).to(DEV)
    act = (rng.standard_normal((N, 2)) * 1.5).astype(np.float32)
    act[:4] = 0
    assert env.launch(1, torch.from_numpy(act).to(DEV), 0) == 0
    s_exp, r_exp, c_exp = T.circle_step(s, act, level)
    np.testing.assert_array_equal(env.state[:N].cpu().numpy(), s_exp)
    np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp)
    np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp)
    np.testing.assert_array_equal(env.obs[:N].cpu().numpy(), T.circle_obs(s_exp))
    assert env.pads_untouched()
    assert not c_exp[:4].any() and r_exp[3] == 0 and (r_exp > 0).any() and (r_exp < 0).any()
    assert (np.abs(s_exp[:, 0:2]) == 2).any()
    assert c_exp.sum() == 0 if level == 0 else 30 < c_exp.sum() < N


@pytest.mark.parametrize('level', [0, 1, 2])
def test_env_class_returns_what_the_twin_returns(level):
    """The same through envs.NavCircleVectorEnv: double-buffered observations, final_observation in the info of the
    truncating step only."""
    from omnisafe_amd import envs

    N, H, seed = 5, 7, 3
    env = envs.make(IDS[level], num_envs=N, device=DEV, horizon=H, seed=seed)
    twin = T.CircleTwin(level, N, H, seed)
    obs, _ = env.reset()
    np.testing.assert_array_equal(obs.cpu().numpy(), twin.reset())
    gen = torch.Generator(device='cpu').manual_seed(level)
    for t in range(20):
        act = torch.randn(N, 2, generator=gen) * 1.5
        prev = obs
        obs, reward, cost, term, trunc, info = env.step(act.to(DEV))
        o_exp, r_exp, c_exp, done, final = twin.step(act.numpy())
        assert obs.data_ptr() != prev.data_ptr()
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
        np.testing.assert_array_equal(env._steps.cpu().numpy(), np.full(N, (t + 1) % H, np.int32))


def test_strided_actions_and_argument_checks():
    env = RawEnv(2, 3, 28, 28, 7, 1)
    twin = T.CircleTwin(2, 3, 7, 1)
    assert env.launch(0, None, 1) == 0
    twin.reset()
    wide = (torch.randn(3, 5, generator=torch.Generator(device='cpu').manual_seed(0)) * 1.5).to(DEV)
    assert env.launch(1, wide[:, 1:3], 0) == 0  # a row stride of 5
    o_exp, r_exp, c_exp, *_ = twin.step(wide[:, 1:3].cpu().numpy())
    np.testing.assert_array_equal(env.obs[:3].cpu().numpy(), o_exp)
    np.testing.assert_array_equal(env.reward[:3].cpu().numpy(), r_exp)
    np.testing.assert_array_equal(env.cost[:3].cpu().numpy(), c_exp)
    # refused before any launch: every buffer stays as it is
    kept = {k: getattr(env, k).clone() for k in ('state', 'steps', 'obs', 'final', 'reward', 'cost', 'term', 'trunc')}
    act = wide[:, 1:3]
    assert env.launch(2, act, 0, obs_dim=27) == -1
    assert env.launch(2, act, 0, state=None) == -1
    assert env.launch(2, None, 0) == -1  # a step without actions
    env.level = 3
    assert env.launch(2, act, 0) == -1
    env.level, env.N = 2, 0
    assert env.launch(2, act, 0) == -1
    env.N, env.ld = 3, 27
    assert env.launch(2, act, 0) == -1  # rows narrower than obs_dim
    torch.cuda.synchronize()
    for k, v in kept.items():
        assert torch.equal(getattr(env, k), v), k


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
    assert s_g[0]['obs'].shape[-1] == 28 and s_g[0]['env_state'].shape == (64, 8)
    assert not torch.equal(s_g[2]['obs'], s_g[3]['obs'])


# ------------------------------------------------------------------ 4. evaluator
def short_cfgs(log_dir, n=16, horizon=8, epochs=2, **logger):
    return {'train_cfgs': {'device': DEV, 'total_steps': epochs * n * 2 * horizon, 'vector_env_nums': n},
            'algo_cfgs': {'steps_per_epoch': n * 2 * horizon},
            'logger_cfgs': dict({'log_dir': log_dir, 'verbose': False, 'save_model_freq': 1000}, **logger),
            'env_cfgs': {'horizon': horizon}}


@pytest.fixture(scope='module')
def checkpoint(tmp_path_factory):
    """A 2-epoch PPOLag run on level 1 at horizon 30: (log_dir, name of its last checkpoint)."""
    import omnisafe_amd

    cfg = dict(short_cfgs(str(tmp_path_factory.mktemp('ckpt')), n=16, horizon=30, save_model_freq=1), seed=2)
    agent = omnisafe_amd.Agent('PPOLag', IDS[1], custom_cfgs=cfg)
    agent.learn()
    log_dir = agent.agent.logger.log_dir
    names = sorted(os.listdir(os.path.join(log_dir, 'torch_save')), key=lambda n: int(n[len('epoch-'):-len('.pt')]))
    return log_dir, names[-1]


def play(checkpoint, path, monkeypatch, K, seed=3):
    from omnisafe_amd.evaluator import Evaluator

    if path:
        monkeypatch.setenv('OSA_EVAL_PATH', path)
    else:
        monkeypatch.delenv('OSA_EVAL_PATH', raising=False)
    ev = Evaluator(seed=seed, device=DEV, verbose=False)
    ev.load_saved(*checkpoint)
    r, c = ev.evaluate(num_episodes=K, trace=True)
    return np.array(r), np.array(c), np.array(ev.episode_lengths), ev.trace.cpu().numpy(), ev


@pytest.mark.parametrize('K', [5, 33])
def test_evaluator_persistent_equals_per_step_and_replays_through_the_twin(checkpoint, monkeypatch, K):
    """K = 5: a quarter-filled wave; K = 33: two full waves and one episode of a third."""
    from omnisafe_amd import _lib

    H, seed = 30, 3
    assert _lib.load().osa_eval_trace_floats(32 + 1, 28, 2, 0) == 28 + 2 + 3 + 8
    a = play(checkpoint, 'persistent', monkeypatch, K, seed)
    b = play(checkpoint, 'per-step', monkeypatch, K, seed)
    assert a[4].path == 'persistent' and b[4].path == 'per-step'
    for x, y in zip(a[:4], b[:4]):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x, y)
    assert play(checkpoint, '', monkeypatch, K, seed)[4].path == 'persistent'  # the default
    ret, cost, length, tr, ev = a
    assert (length == H).all() and tr.shape == (H, K, 28 + 2 + 3 + 8)
    x, act = tr[:, :, :28], tr[:, :, 28:30]
    rew, cst, alive, state = tr[:, :, 30], tr[:, :, 31], tr[:, :, 32], tr[:, :, 33:]
    assert (alive == 1).all()
    mean, std = ev._normalizer._mean.cpu().numpy(), ev._normalizer._std.cpu().numpy()
    np.testing.assert_array_equal(state[0], T.circle_reset(seed, 0, K))
    for t in range(H):
        o = T.circle_obs(state[t])
        np.testing.assert_array_equal(x[t], np.clip(((o - mean).astype(np.float32) / std).astype(np.float32), -5, 5))
        s2, r, c = T.circle_step(state[t], act[t], 1)
        np.testing.assert_array_equal(rew[t], r)
        np.testing.assert_array_equal(cst[t], c)
        if t + 1 < H:
            np.testing.assert_array_equal(state[t + 1], s2)
    np.testing.assert_array_equal(ret, rew.astype(np.float64).cumsum(0)[-1])
    np.testing.assert_array_equal(cost, cst.astype(np.float64).sum(0))
    assert np.abs(act).max() > 0 and np.abs(rew).max() > 0


# ------------------------------------------------------------------ 5. group, trust region
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
        return short_cfgs(log_dir, n=64, horizon=20)

    seeds = [0, 1]
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


@pytest.mark.parametrize('algo', ['CPO', 'TRPOLag'])
def test_trust_region_update_at_width_28(algo, tmp_path):
    """Two epochs on level 1 (N = 16, horizon 8): the Fisher products, conjugate gradients and line searches run at a
    policy input of 28 columns, the parameters stay finite, and the same seed gives the same run bit for bit."""
    import omnisafe_amd

    runs = []
    for k in range(2):
        a = omnisafe_amd.Agent(algo, IDS[1], custom_cfgs=dict(short_cfgs(str(tmp_path / f'run{k}')), seed=4))
        a.learn()
        runs.append(_outcome(a))
    assert torch.isfinite(runs[0][0]).all() and len(runs[0][1]) == 3
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


# ------------------------------------------------------------------ 6. learning, directional
LEARN = {'vector_env_nums': 256, 'steps_per_epoch': 51_200, 'epochs': 10, 'horizon': 200, 'seeds': 4}


def train_group(algo, level, log_dir):
    """The four seeds in one AgentGroup; per seed the EpRet / EpCost columns of its progress.csv.  PPOLag keeps the
    YAML's cost_limit of 25, which binds from the first epoch (an untrained policy costs about 70 per episode)."""
    import omnisafe_amd

    c = LEARN
    custom = {'train_cfgs': {'device': DEV, 'total_steps': c['steps_per_epoch'] * c['epochs'],
                             'vector_env_nums': c['vector_env_nums']},
              'algo_cfgs': {'steps_per_epoch': c['steps_per_epoch']},
              'logger_cfgs': {'log_dir': log_dir, 'verbose': False, 'save_model_freq': 1000},
              'env_cfgs': {'horizon': c['horizon']}}
    group = omnisafe_amd.AgentGroup(algo, IDS[level], seeds=list(range(c['seeds'])), custom_cfgs=custom)
    group.learn()
    if algo == 'PPOLag':
        assert float(group.agents[0].agent._cfgs.lagrange_cfgs.cost_limit) == 25.0  # noqa: SLF001
    curves = []
    for member in group.agents:
        rows = list(csv.DictReader(open(os.path.join(member.agent.logger.log_dir, 'progress.csv'))))
        curves.append({k: np.array([float(r[f'Metrics/{k}']) for r in rows]) for k in ('EpRet', 'EpCost')})
    return curves


def twin_untrained_policy_rates(level, horizon, std):
    """Per-episode return and cost of 1024 twin episodes under actions N(0, std^2): what an untrained Gaussian policy
    (mean near 0) does."""
    env = T.CircleTwin(level, 1024, horizon, 123)
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
    seeds trained in one AgentGroup, the seed-mean EpRet of the last three epochs exceeds the first epoch's by more
    than two standard errors of the difference; for PPOLag (YAML cost_limit 25, binding from the start) the tail EpCost
    is not above the first epoch's by more than two standard errors, and the first epoch's EpCost must look like the
    twin under an untrained policy's actions; on level 0 the cost is identically 0."""
    c = LEARN
    curves = train_group(algo, level, str(tmp_path))
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
