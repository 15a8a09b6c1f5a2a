"""GPU: device envs registered from a header (register_device_env).  The generic per-step kernel
(osa_custom_env_kernel) against the specialised kernels of two built-in descriptions and, for the example env
tests/custom_envs/glider.h, against its numpy twin (tests/custom_env_twin.py); then through the layers: the captured
rollout graph, the evaluator's two paths, Agent and AgentGroup.  Every comparison is bit for bit."""
import os

import numpy as np
import pytest
import torch

import custom_env_twin as T
import raw_env

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = raw_env.SENTINEL


def header(name):
    return os.path.join(HERE, 'custom_envs', name)


@pytest.fixture
def register():
    """register_device_env that unregisters at the end of the test."""
    import omnisafe_amd

    entered = []

    def enter(name, struct, ids, **kwargs):
        cls = omnisafe_amd.register_device_env(header(name), struct, ids, **kwargs)
        entered.extend(ids)
        return cls

    yield enter
    omnisafe_amd.unregister_device_env(*[e for e in entered if e in omnisafe_amd.custom_envs()])


@pytest.fixture
def glider(register):
    return register('glider.h', 'Glider', {'Glider0-v0': 0, 'Glider1-v0': 1}, default_horizon=40)


# ------------------------------------------------------------------ 1. the generic kernel equals the specialised ones
@pytest.mark.parametrize('name, struct, level, builtin', [
    ('reach_again.h', 'ReachAgain', 0, 'SynthReach-v0'),
    ('circle_again.h', 'CircleAgain', 1, 'SynthNavCircle1-v0'),
], ids=['reach', 'circle1'])
def test_generic_kernel_equals_the_specialised_kernel(register, name, struct, level, builtin):
    """The same description through osa_custom_env_kernel and through the kernel written for it: same seed, N = 130,
    horizon 7, 20 steps (truncations at 7 and 14) under the same random actions."""
    from omnisafe_amd import envs

    N, H, seed = 130, 7, 9
    register(name, struct, {'Again-v0': level})
    ours = envs.make('Again-v0', num_envs=N, device=DEV, horizon=H, seed=seed)
    theirs = envs.make(builtin, num_envs=N, device=DEV, horizon=H, seed=seed)
    assert ours.action_space.shape == theirs.action_space.shape == (2,) and type(ours).lanes == 32
    assert ours.state.shape == theirs.state.shape and ours.level == theirs.level == level
    # SynthReach-v0 pads its 6 native columns with zeros to 60, ours keeps the description's OBS: compare that part
    D = ours.observation_space.shape[0]
    assert D == {'ReachAgain': 6, 'CircleAgain': 28}[struct]
    o1, _ = ours.reset()
    o2, _ = theirs.reset()
    assert torch.equal(o1, o2[:, :D]) and not o2[:, D:].any() and torch.equal(ours.state, theirs.state)
    gen = torch.Generator(device='cpu').manual_seed(1)
    for t in range(20):
        act = (torch.randn(N, 2, generator=gen) * 1.5).to(DEV)
        a = ours.step(act)
        b = theirs.step(act)
        assert torch.equal(a[0], b[0][:, :D]), t
        for k in (1, 2, 3, 4):  # reward, cost, terminated, truncated
            assert torch.equal(a[k], b[k]), (t, k)
        assert ('final_observation' in a[5]) == ('final_observation' in b[5]) == ((t + 1) % H == 0)
        if 'final_observation' in a[5]:
            assert torch.equal(a[5]['final_observation'], b[5]['final_observation'][:, :D])
            assert bool(a[5]['_final_observation'].all())
        assert torch.equal(ours.state, theirs.state), t
        assert torch.equal(ours._steps, theirs._steps)
    assert bool(a[1].abs().sum() > 0)


# ------------------------------------------------------------------ 2. glider against its twin
def raw_glider(cls, level, N, obs_dim, ld, horizon, seed):
    env = raw_env.RawEnv('osa_nav_env_step', T.STATE, level, N, obs_dim, ld, horizon, seed)
    env.fn = cls.library().osa_custom_env_step  # (the same argument list)
    return env


@pytest.mark.parametrize('level', [0, 1])
@pytest.mark.parametrize('N', [1, 3, 130])
def test_glider_trace_equals_the_twin_at_every_lane_count(register, level, N):
    """25 steps at horizon 9 (truncations with same-position resets at steps 9 and 18) under actions 1.5 randn, N = 1 (a
    lone env), 3 (an odd count) and 130 (past one workgroup at every LANES), at obs_dim = 70 in rows of 70 and at
    obs_dim 75 in rows of 80 (sentinels behind): everything the launch writes equals the twin at every step, and the
    libraries built at 16, 32 and 64 lanes per env write the same bits."""
    H, seed, steps = 9, 21 + level, 25
    classes = {lanes: register('glider.h', struct, [f'Glider-lanes{lanes}-v0'])
               for lanes, struct in ((32, 'Glider'), (16, 'Glider16'), (64, 'Glider64'))}
    assert {lanes: cls.lanes for lanes, cls in classes.items()} == {16: 16, 32: 32, 64: 64}
    assert len({cls.lib_path for cls in classes.values()}) == 3
    for obs_dim, ld in ((T.OBS, T.OBS), (75, 80)):
        envs_ = {lanes: raw_glider(cls, level, N, obs_dim, ld, H, seed) for lanes, cls in classes.items()}
        twin = T.GliderTwin(level, N, H, seed)
        o_exp = twin.reset()
        for env in envs_.values():
            assert env.launch(0, None, 1) == 0  # reset from the seed alone
            np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state)
            np.testing.assert_array_equal(env.obs[:N, :T.OBS].cpu().numpy(), o_exp)
            assert not env.obs[:N, T.OBS:obs_dim].any() and int(env.steps[:N].abs().sum()) == 0
            assert bool((env.final == SENTINEL).all()) and bool((env.reward == SENTINEL).all())
        gen = torch.Generator(device='cpu').manual_seed(100 * level + N)
        n_cost = n_clamped = n_goal = 0
        tail_nonzero = False
        for t in range(steps):
            act = torch.randn(N, 3, generator=gen) * 1.5
            o_exp, r_exp, c_exp, done, final = twin.step(act.numpy())
            assert done == ((t + 1) % H == 0)
            for lanes, env in envs_.items():
                assert env.launch(t + 1, act.to(DEV), 0) == 0
                np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp, err_msg=f'{lanes} lanes')
                np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp)
                assert not env.term[:N].any() and bool((env.trunc[:N] == int(done)).all())
                assert bool((env.steps[:N] == (t + 1) % H).all())
                if done:
                    np.testing.assert_array_equal(env.final[:N, :T.OBS].cpu().numpy(), final)
                    assert not env.final[:N, T.OBS:obs_dim].any()
                    env.final.fill_(SENTINEL)
                else:
                    assert bool((env.final == SENTINEL).all())  # written on the truncating step only
                np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state)
                np.testing.assert_array_equal(env.obs[:N, :T.OBS].cpu().numpy(), o_exp, err_msg=f'{lanes} lanes')
                assert not env.obs[:N, T.OBS:obs_dim].any()
                assert env.pads_untouched(), (lanes, obs_dim, t)
            n_cost += int(c_exp.sum())
            n_goal += int((r_exp > 0.5).sum())
            n_clamped += int((act.abs() > 1).sum())
            tail_nonzero = tail_nonzero or bool((o_exp[:, 64:T.OBS] != 0).any(0).all())  # the second round's columns
        assert n_clamped > N * steps // 2 and tail_nonzero
        if level == 0:
            assert n_cost == 0
    print(f'level {level} N {N}: cost steps {n_cost}, goals {n_goal}, clamped components {n_clamped}')


def test_glider_costs_goals_and_walls_from_states_of_the_callers_own(glider):
    """Short episodes from a reset seldom reach a goal or the slab's edge.  The state matrix is the caller's: 130 envs
    placed all over the box at speed, some next to their goal, one step each -- the goal redrawn from the transition's
    own Philox block, the count, costs above and below the slab on level 1, positions clipped at the box."""
    N, seed = 130, 4
    rng = np.random.default_rng(0)
    s = np.zeros((N, T.STATE), np.float32)
    s[:, 0:3] = rng.uniform(-2, 2, (N, 3))
    s[:, 3:6] = rng.uniform(-0.5, 0.5, (N, 3))
    s[:, 6:9] = rng.uniform(-1.5, 1.5, (N, 3))
    s[:40, 6:9] = s[:40, 0:3] + s[:40, 3:6] * np.float32(0.9)  # about where the glide ends
    s[:, 9] = rng.integers(0, 3, N)
    act = (rng.standard_normal((N, 3)) * 1.5).astype(np.float32)
    for level in (0, 1):
        env = raw_glider(glider, level, N, T.OBS, T.OBS, 9, seed)
        assert env.launch(0, None, 1) == 0
        env.state[:N] = torch.from_numpy(s).to(DEV)
        assert env.launch(5, torch.from_numpy(act).to(DEV), 0) == 0
        s_exp, r_exp, c_exp = T.glider_step(s, act, level, seed, 5)
        np.testing.assert_array_equal(env.state[:N].cpu().numpy(), s_exp)
        np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp)
        np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp)
        np.testing.assert_array_equal(env.obs[:N].cpu().numpy(), T.glider_obs(s_exp))
        assert env.pads_untouched()
        reached = s_exp[:, 9] != s[:, 9]
        assert 20 < reached.sum() < N and (r_exp[reached] > 0.5).all() and (s_exp[reached, 6:9] != s[reached, 6:9]).all()
        assert (np.abs(s_exp[:, 0:3]) == 2).any()
        assert c_exp.sum() == 0 if level == 0 else 20 < c_exp.sum() < N


def test_glider_argument_checks(glider):
    """Refused before any launch: a row narrower than the env, two action columns for three, a level the description
    does not have."""
    env = raw_glider(glider, 1, 3, T.OBS, T.OBS, 9, 1)
    assert env.launch(0, None, 1) == 0
    wide = (torch.randn(3, 5, generator=torch.Generator(device='cpu').manual_seed(0)) * 1.5).to(DEV)
    twin = T.GliderTwin(1, 3, 9, 1)
    twin.reset()
    assert env.launch(1, wide[:, 1:4], 0) == 0  # a row stride of 5
    o_exp, r_exp, *_ = twin.step(wide[:, 1:4].cpu().numpy())
    np.testing.assert_array_equal(env.obs[:3].cpu().numpy(), o_exp)
    np.testing.assert_array_equal(env.reward[:3].cpu().numpy(), r_exp)
    kept = {k: getattr(env, k).clone() for k in ('state', 'steps', 'obs', 'final', 'reward', 'cost', 'term', 'trunc')}
    act = wide[:, 1:4]
    assert env.launch(2, act, 0, obs_dim=69) == -1
    assert env.launch(2, act, 0, state=None) == -1
    assert env.launch(2, None, 0) == -1
    assert env.launch(2, torch.zeros(3, 2, device=DEV), 0) == -1  # ld_action 2 < ACT
    env.level = 2
    assert env.launch(2, act, 0) == -1  # LEVELS = 1
    env.level, env.N = 1, 0
    assert env.launch(2, act, 0) == -1
    torch.cuda.synchronize()
    for k, v in kept.items():
        assert torch.equal(getattr(env, k), v), k


# ------------------------------------------------------------------ 3. graph replay
def test_rollout_graph_replay_equals_eager_launches(glider, tmp_path, monkeypatch):
    """OnPolicyAdapter.rollout on the custom env inside the captured hipGraph against eager launches: the buffers of
    every epoch are identical (four epochs: the graph is captured on the second and replayed for two more; commit()
    advances the stream position, so the epochs differ)."""
    import omnisafe_amd

    def run(graph):
        monkeypatch.setenv('OSA_ROLLOUT_GRAPH', '1' if graph else '0')
        cfg = {'seed': 7, 'train_cfgs': {'device': DEV, 'total_steps': 4 * 64 * 24, 'vector_env_nums': 64},
               'algo_cfgs': {'steps_per_epoch': 64 * 24, 'update_iters': 2},
               'logger_cfgs': {'log_dir': str(tmp_path / ('g' if graph else 'e')), 'verbose': False},
               'env_cfgs': {'horizon': 10}}  # truncations at steps 10 and 20 of the 24
        algo = omnisafe_amd.Agent('PPOLag', 'Glider1-v0', custom_cfgs=cfg).agent
        snaps = []
        for _ in range(4):
            algo._env.rollout(steps_per_epoch=algo._steps_per_epoch, agent=algo._actor_critic, buffer=algo._buf,
                              logger=algo._logger)
            snap = {k: v.clone() for k, v in algo._buf.data.items()}
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
    assert s_g[0]['obs'].shape[-1] == T.OBS and s_g[0]['env_state'].shape == (64, T.STATE)
    assert s_g[0]['act'].shape[-1] == 3
    assert not torch.equal(s_g[2]['obs'], s_g[3]['obs'])


# ------------------------------------------------------------------ 4. evaluator
def short_cfgs(log_dir, n=16, horizon=8, epochs=2, **logger):
    return {'train_cfgs': {'device': DEV, 'total_steps': epochs * n * 2 * horizon, 'vector_env_nums': n},
            'algo_cfgs': {'steps_per_epoch': n * 2 * horizon},
            'logger_cfgs': dict({'log_dir': log_dir, 'verbose': False, 'save_model_freq': 1000}, **logger),
            'env_cfgs': {'horizon': horizon}}


def train_checkpoint(algo, log_dir, env_id='Glider1-v0'):
    """A 2-epoch run (glider: level 1) at horizon 12 ([64, 64] actor, obs_normalize): (log_dir, name of its last
    checkpoint)."""
    import omnisafe_amd

    cfg = dict(short_cfgs(log_dir, n=16, horizon=12, save_model_freq=1), seed=2)
    agent = omnisafe_amd.Agent(algo, env_id, custom_cfgs=cfg)
    assert list(agent.agent._cfgs.model_cfgs.actor.hidden_sizes) == [64, 64] and agent.agent._cfgs.algo_cfgs.obs_normalize
    agent.learn()
    log_dir = agent.agent.logger.log_dir
    names = sorted(os.listdir(os.path.join(log_dir, 'torch_save')), key=lambda n: int(n[len('epoch-'):-len('.pt')]))
    return log_dir, names[-1]


def play(checkpoint, path, monkeypatch, K, seed=3):
    from omnisafe_amd.evaluator import Evaluator

    monkeypatch.setenv('OSA_EVAL_PATH', path)
    ev = Evaluator(seed=seed, device=DEV, verbose=False)
    ev.load_saved(*checkpoint)
    r, c = ev.evaluate(num_episodes=K, trace=True)
    return np.array(r), np.array(c), np.array(ev.episode_lengths), ev.trace.cpu().numpy(), ev


@pytest.mark.parametrize('algo', ['PPOLag', 'PPOSaute'])
def test_evaluator_persistent_equals_per_step_and_replays_through_the_twin(glider, tmp_path, monkeypatch, algo):
    """K = 5: a quarter-filled wave; K = 33: two full waves and one episode of a third.  PPOSaute: the policy input has
    the safety column behind the 70 observation columns."""
    H, seed = 12, 3
    checkpoint = train_checkpoint(algo, str(tmp_path))
    saute = int(algo == 'PPOSaute')
    in_w = T.OBS + saute
    for K in (5, 33):
        a = play(checkpoint, 'persistent', monkeypatch, K, seed)
        b = play(checkpoint, 'per-step', monkeypatch, K, seed)
        assert a[4].path == 'persistent' and b[4].path == 'per-step'
        for x, y in zip(a[:4], b[:4]):
            assert x.shape == y.shape
            np.testing.assert_array_equal(x, y)
        ret, cost, length, tr, ev = a
        assert (length == H).all() and tr.shape == (H, K, in_w + 3 + 3 + T.TRACE)
        x, act = tr[:, :, :T.OBS], tr[:, :, in_w:in_w + 3]
        rew, cst, alive, state = tr[:, :, in_w + 3], tr[:, :, in_w + 4], tr[:, :, in_w + 5], tr[:, :, in_w + 6:]
        assert (alive == 1).all()
        mean, std = ev._normalizer._mean.cpu().numpy(), ev._normalizer._std.cpu().numpy()
        twin = T.GliderTwin(1, K, H, seed)  # a replay of the traced actions
        o = twin.reset()
        for t in range(H):
            np.testing.assert_array_equal(state[t], twin.state[:, :T.TRACE])
            np.testing.assert_array_equal(x[t], np.clip(((o - mean).astype(np.float32) / std).astype(np.float32), -5, 5))
            if t + 1 < H:
                o, r, c, *_ = twin.step(act[t])
            else:  # (the twin would reset on the last step; the record is the transition's)
                _, r, c = T.glider_step(twin.state, act[t], 1, seed, t + 1)
            np.testing.assert_array_equal(rew[t], r)
            np.testing.assert_array_equal(cst[t], c)
        np.testing.assert_array_equal(ret, rew.astype(np.float64).cumsum(0)[-1])
        np.testing.assert_array_equal(cost, cst.astype(np.float64).sum(0))
        if saute:
            assert (tr[0, :, T.OBS] == 1).all()  # the safety budget starts full
        assert np.abs(act).max() > 0 and np.abs(rew).max() > 0 and np.abs(act[:, :, 2]).max() > 0
    monkeypatch.delenv('OSA_EVAL_PATH')
    from omnisafe_amd.evaluator import Evaluator

    ev = Evaluator(seed=seed, device=DEV, verbose=False)
    ev.load_saved(*checkpoint)
    ev.evaluate(num_episodes=2)
    assert ev.path == 'persistent'  # the default for a custom env as well
    with pytest.raises(ValueError, match='no state row to draw'):
        ev.render(num_episodes=1, save_replay_path=str(tmp_path / 'video'))


# ------------------------------------------------------------------ 4b. one action column
def test_one_action_column_steps_and_evaluates(register, tmp_path, monkeypatch):
    """ACT = 1 in the two-column form (tests/custom_envs/slider.h): the (N, 1) action tensor has a row stride of 1, the
    entry point takes it, and a1 arrives as 0 -- the env adds it to the velocity, so the next env's action (or, for the
    last env, the 1000 behind the rows) would show.  The raw entry point refuses a stride of 0 and takes a wider one.
    Then both evaluator paths on a trained checkpoint, replayed through the twin."""
    from omnisafe_amd import envs

    N, H, seed = 130, 5, 6
    cls = register('slider.h', 'Slider', ['Slider-v0'])
    assert cls.dims('Slider-v0') == (3, 1) and cls.state_width == 2 and cls.max_level == 0
    env = envs.make('Slider-v0', num_envs=N, device=DEV, horizon=H, seed=seed)
    obs, _ = env.reset()
    state = T.slider_reset(seed, 0, N)
    np.testing.assert_array_equal(env.state.cpu().numpy(), state)
    np.testing.assert_array_equal(obs.cpu().numpy(), T.slider_obs(state))
    flat = torch.full((N + 1,), 1000.0, device=DEV)
    gen = torch.Generator(device='cpu').manual_seed(0)
    for t in range(12):
        a = torch.randn(N, 1, generator=gen) * 1.5
        flat[:N] = a[:, 0].to(DEV)
        act = flat[:N].view(N, 1)
        assert act.stride(0) == 1
        obs, reward, cost, term, trunc, info = env.step(act)
        state, r, c = T.slider_step(state, a.numpy())
        np.testing.assert_array_equal(reward.cpu().numpy(), r)
        np.testing.assert_array_equal(cost.cpu().numpy(), c)
        if (t + 1) % H == 0:
            np.testing.assert_array_equal(info['final_observation'].cpu().numpy(), T.slider_obs(state))
            state = T.slider_reset(seed, t + 1, N)
        np.testing.assert_array_equal(env.state.cpu().numpy(), state)
        np.testing.assert_array_equal(obs.cpu().numpy(), T.slider_obs(state))
    raw = raw_env.RawEnv('osa_nav_env_step', 2, 0, 3, 3, 3, H, seed)
    raw.fn = cls.library().osa_custom_env_step
    assert raw.launch(0, None, 1) == 0
    wide = torch.zeros(3, 4, device=DEV)
    assert raw.launch(1, wide[:, 2:3], 0) == 0  # a row stride of 4
    assert raw.launch(2, wide[0:1, 0:1].expand(3, 1), 0) == -1  # a row stride of 0: refused before the launch
    assert raw.pads_untouched()
    with pytest.raises(ValueError, match='no state row to draw'):
        env.render()
    # the evaluator: the persistent kernel hands the two-column form a1 = 0 as well
    checkpoint = train_checkpoint('PPOLag', str(tmp_path), 'Slider-v0')
    a = play(checkpoint, 'persistent', monkeypatch, 5)
    b = play(checkpoint, 'per-step', monkeypatch, 5)
    for x, y in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y)
    tr = a[3]
    assert tr.shape == (12, 5, 3 + 1 + 3 + 2)
    state = T.slider_reset(3, 0, 5)
    for t in range(12):
        np.testing.assert_array_equal(tr[t, :, 7:9], state)
        state, r, c = T.slider_step(state, tr[t, :, 3:4])
        np.testing.assert_array_equal(tr[t, :, 4], r)
        np.testing.assert_array_equal(tr[t, :, 5], c)
    assert np.abs(tr[:, :, 3]).max() > 0


# ------------------------------------------------------------------ 5. end to end
def _outcome(agent):
    ac = agent.agent._actor_critic  # noqa: SLF001
    torch.cuda.synchronize()
    lines = [ln for ln in open(os.path.join(agent.agent.logger.log_dir, 'progress.csv')).read().split('\n') if ln]
    hdr = lines[0].split(',')
    keep = [i for i, h in enumerate(hdr) if not h.startswith('Time/')]
    return ac.params.clone(), [[ln.split(',')[i] for i in keep] for ln in lines]


def test_agent_group_and_evaluate_end_to_end(glider, tmp_path):
    """Agent('PPOLag', 'Glider1-v0'): two epochs of 16 envs x 16 steps; the same configuration as member 0 of an
    AgentGroup of seeds [0, 1] equals it in parameters and in every column but Time/*; Agent.evaluate() plays every saved
    model."""
    import omnisafe_amd

    def cfgs(log_dir):
        return short_cfgs(log_dir, n=16, horizon=8, save_model_freq=1)

    solo = omnisafe_amd.Agent('PPOLag', 'Glider1-v0', custom_cfgs=dict(cfgs(str(tmp_path / 'solo')), seed=0))
    solo.learn()
    params, rows = _outcome(solo)
    assert torch.isfinite(params).all() and len(rows) == 3
    assert os.path.exists(os.path.join(solo.agent.logger.log_dir, 'progress.csv'))
    assert type(solo.agent._env._env) is glider and solo.agent._env._env.level == 1
    group = omnisafe_amd.AgentGroup('PPOLag', 'Glider1-v0', seeds=[0, 1], custom_cfgs=cfgs(str(tmp_path / 'group')))
    assert len(group.learn()) == 2
    g_params, g_rows = _outcome(group.agents[0])
    assert torch.equal(g_params, params) and g_rows == rows
    assert not torch.equal(_outcome(group.agents[1])[0], params)
    saved = os.listdir(os.path.join(solo.agent.logger.log_dir, 'torch_save'))
    out = solo.evaluate(num_episodes=3)
    assert sorted(out) == sorted(saved) and len(saved) >= 2
    for rewards, costs in out.values():
        assert len(rewards) == len(costs) == 3 and np.isfinite(rewards).all()
