"""GPU: the SynthNavCarGoal{0,1,2}-v0 and SynthNavCarCircle{0,1,2}-v0 device envs (osa_car_goal_env_step: one wave per
env over a row wider than the wave; osa_car_circle_env_step: half a wave per env over a row wider than the half; their
instantiations of osa_eval_episodes) against the numpy twin (tests/car_twin.py) bit for bit, and through the layers
that use them at observation widths 72 and 40: the captured rollout graph, the evaluator's two paths, AgentGroup, the
trust-region updates, and a directional learning check."""
import csv
import os

import numpy as np
import pytest
import torch

import car_twin as T
import nav_twin
import raw_env

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOAL = {0: 'SynthNavCarGoal0-v0', 1: 'SynthNavCarGoal1-v0', 2: 'SynthNavCarGoal2-v0'}
CIRCLE = {0: 'SynthNavCarCircle0-v0', 1: 'SynthNavCarCircle1-v0', 2: 'SynthNavCarCircle2-v0'}
POINT_GOAL = {0: 'SynthNavGoal0-v0', 1: 'SynthNavGoal1-v0', 2: 'SynthNavGoal2-v0'}
POINT_CIRCLE = {0: 'SynthNavCircle0-v0', 1: 'SynthNavCircle1-v0', 2: 'SynthNavCircle2-v0'}
SENTINEL = -777.0
# per task: entry point, floats per state row, observation columns, the env's default horizon
TASK = {'goal': ('osa_car_goal_env_step', 64, 72, 1000), 'circle': ('osa_car_circle_env_step', 12, 40, 500)}


def make_twin(task, level, N, H, seed):
    return T.CarGoalTwin(level, N, H, seed) if task == 'goal' else T.CarCircleTwin(level, N, H, seed)


def twin_obs(task, state, level):
    return T.car_goal_obs(state, level) if task == 'goal' else T.car_circle_obs(state)


def twin_step(task, state, action, level, seed, pos):
    """(new state, reward, cost) of one transition of the task's twin."""
    if task == 'goal':
        return T.car_goal_step(state, action, level, seed, pos)[:3]
    return T.car_circle_step(state, action, level)


# ------------------------------------------------------------------ 1. reset from the seed alone
@pytest.mark.parametrize('level', [0, 1, 2])
@pytest.mark.parametrize('seed', [5, 2 ** 40 + 17])
@pytest.mark.parametrize('task', ['goal', 'circle'])
def test_reset_from_the_seed_alone(task, level, seed):
    """Nothing but the seed goes in.  N = 3 (CarCircle: one full workgroup and one whose second half-wave has no env).
    The arena is the point env's of the same seed: the reset shares its Philox key and draw allocation on purpose."""
    from omnisafe_amd import envs

    N = 3
    _, width, D, horizon = TASK[task]
    env = envs.make((GOAL if task == 'goal' else CIRCLE)[level], num_envs=N, device=DEV)
    assert env.level == level and env.max_episode_steps == horizon and env.graph_safe
    assert env.observation_space.shape == (D,) and env.action_space.shape == (2,)
    assert float(env.action_space.low.min()) == -1 and float(env.action_space.high.max()) == 1
    env.set_seed(seed)
    obs, _ = env.reset()
    assert env.state.shape == (N, width) and obs.shape == (N, D)
    state = env.state.cpu().numpy()
    exp = T.car_goal_reset(seed, 0, N, level) if task == 'goal' else T.car_circle_reset(seed, 0, N)
    np.testing.assert_array_equal(state, exp)
    np.testing.assert_array_equal(obs.cpu().numpy(), twin_obs(task, state, level))
    assert int(env._steps.abs().sum()) == 0
    point = envs.make((POINT_GOAL if task == 'goal' else POINT_CIRCLE)[level], num_envs=N, device=DEV)
    point.set_seed(seed)
    p_obs, _ = point.reset()
    p_state = point.state.cpu().numpy()
    np.testing.assert_array_equal(state[:, :p_state.shape[1]], p_state)
    np.testing.assert_array_equal(obs[:, 24:].cpu().numpy(), p_obs[:, 12:].cpu().numpy())  # the same lidars
    obs2, _ = env.reset()  # the next stream position: another start
    exp2 = T.car_goal_reset(seed, 1, N, level) if task == 'goal' else T.car_circle_reset(seed, 1, N)
    np.testing.assert_array_equal(env.state.cpu().numpy(), exp2)
    assert not np.array_equal(obs2.cpu().numpy(), obs.cpu().numpy()) and obs2.data_ptr() != obs.data_ptr()


# ------------------------------------------------------------------ 2. trace
def RawEnv(task, *args):
    return raw_env.RawEnv(*TASK[task][:2], *args)


@pytest.mark.parametrize('level', [0, 1, 2])
@pytest.mark.parametrize('N', [1, 3, 130])
@pytest.mark.parametrize('task', ['goal', 'circle'])
def test_trace_equals_the_twin(task, level, N):
    """20 steps at horizon 7 (truncations with same-position resets at steps 7 and 14) from stream base 2 under actions
    1.5 randn, N = 1, 3 and 130, at obs_dim = ld_obs = the env's width and at a wider obs_dim in still wider rows
    (CarGoal 72, and 80 in rows of 84; CarCircle 40, and 48 in rows of 52): everything the launch writes equals the twin
    at every step, the pad columns are zero, and nothing else is written.  On CarGoal level 2 columns 64 .. 71 -- the
    ones a second lane round writes -- must be lit somewhere."""
    W = TASK[task][2]
    H, seed, steps = 7, 11 + level, 20
    for obs_dim, ld in ((W, W), (W + 8, W + 12)):
        env = RawEnv(task, level, N, obs_dim, ld, H, seed)
        twin = make_twin(task, level, N, H, seed)
        env.base.fill_(2)  # the device part of the stream position (graph replay): the episode starts at position 2
        twin.pos = 2
        assert env.launch(0, None, 1) == 0
        np.testing.assert_array_equal(env.obs[:N, :W].cpu().numpy(), twin.reset())
        assert not env.obs[:N, W:obs_dim].any() and int(env.steps[:N].abs().sum()) == 0
        assert bool((env.final == SENTINEL).all()) and bool((env.reward == SENTINEL).all())
        gen = torch.Generator(device='cpu').manual_seed(100 * level + N)
        n_cost = n_clamped = n_tail = 0
        for t in range(steps):
            act = torch.randn(N, 2, generator=gen) * 1.5
            assert env.launch(t + 1, act.to(DEV), 0) == 0
            o_exp, r_exp, c_exp, done, final, *_ = twin.step(act.numpy())
            assert done == ((t + 1) % H == 0)
            np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp)
            np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp)
            assert not env.term[:N].any() and bool((env.trunc[:N] == int(done)).all())
            assert bool((env.steps[:N] == (t + 1) % H).all())
            if done:
                np.testing.assert_array_equal(env.final[:N, :W].cpu().numpy(), final)
                assert not env.final[:N, W:obs_dim].any()
                env.final.fill_(SENTINEL)
            else:
                assert bool((env.final == SENTINEL).all())  # written on the truncating step only
            np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state)
            np.testing.assert_array_equal(env.obs[:N, :W].cpu().numpy(), o_exp)
            assert not env.obs[:N, W:obs_dim].any()
            assert env.pads_untouched(), (obs_dim, t)
            n_cost += int(c_exp.sum())
            n_clamped += int((act.abs() > 1).sum())
            n_tail += int(np.count_nonzero(o_exp[:, 64:]))
        assert n_clamped > 2 * N * steps // 4  # more than a quarter of the 2 N steps components
        if level == 0:
            assert n_cost == 0
        if task == 'goal' and level == 2:
            assert n_tail > 0
    print(f'{task} level {level} N {N}: cost steps {n_cost}, clamped components {n_clamped}, lit tail bins {n_tail}')


# ------------------------------------------------------------------ 3. states of the caller's own
def one_launch(task, level, s, act, seed=3, pos=9):
    """The state matrix `s` written into the launch's buffers, one step at stream position `pos`."""
    N, W = s.shape[0], TASK[task][2]
    env = RawEnv(task, level, N, W, W, 7, seed)
    assert env.launch(0, None, 1) == 0
    env.state[:N] = torch.from_numpy(s).to(DEV)
    assert env.launch(pos, torch.from_numpy(act).to(DEV), 0) == 0
    s_exp, r_exp, c_exp = twin_step(task, s, act, level, seed, pos)
    np.testing.assert_array_equal(env.state[:N].cpu().numpy(), s_exp)
    np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp)
    np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp)
    np.testing.assert_array_equal(env.obs[:N].cpu().numpy(), twin_obs(task, s_exp, level))
    assert env.pads_untouched()
    return s_exp, r_exp, c_exp


@pytest.mark.parametrize('level', [0, 1, 2])
def test_goal_branches_from_states_of_the_callers_own(level):
    """The goal-resample and cost branches do not occur in 20 steps from rest.  The crafted states of
    tests/test_car_twin.py (a goal within reach, a hazard and a vase under the wheels, a wall) in rows 0 .. 4 and 125
    envs placed at speed all over real arenas behind them, one launch."""
    N = 130
    s = T.car_goal_reset(21, 0, N, level)
    rng = np.random.default_rng(level)
    s[:, 0:2] = rng.uniform(-2, 2, (N, 2))
    s[:, 10:12] = rng.uniform(-0.2, 0.2, (N, 2))
    s[:, 4] = (np.float32(0.5) * (s[:, 10] + s[:, 11]).astype(np.float32)).astype(np.float32)
    s[:, 5:8] = rng.uniform(-0.1, 0.1, (N, 3))
    near = rng.uniform(-0.25, 0.25, (N // 4, 2)).astype(np.float32)
    s[5:5 + N // 4, 8:10] = s[5:5 + N // 4, 0:2] + near  # a quarter of the envs next to their goals
    s[:5, 0:2], s[:5, 2:4], s[:5, 8:10] = (0, 0), (1, 0), (1.2, 1.2)
    s[:5, 12:32], s[:5, 32:52] = 1.9, -1.9
    s[:5, 5:8] = 0
    s[0, 8:10], s[0, 10:12] = (0.45, 0), (0.2, 0.2)              # reaches its goal: d1 = 0.25 < 0.3
    s[1:4, 10:12] = (0.1, 0.1)                                    # q = (0.11, 0)
    s[1, 12:14] = (0.25, 0.0)                                     # a hazard at 0.14
    s[2, 32:34] = (0.18, 0.0)                                     # a vase at 0.07
    s[3, 12:14] = (0.36, 0.0)                                     # a hazard just out of reach
    s[4, 0:2], s[4, 10:12] = (1.99, -1.0), (0.5, 0.5)             # into the wall
    s[:5, 4] = (np.float32(0.5) * (s[:5, 10] + s[:5, 11]).astype(np.float32)).astype(np.float32)
    act = (rng.standard_normal((N, 2)) * 1.5).astype(np.float32)
    act[:5] = 1
    s_exp, r_exp, c_exp = one_launch('goal', level, s, act)
    reached = (s_exp[:, 8:10] != s[:, 8:10]).any(1)
    assert reached[0] and r_exp[0] > 1 and not reached[1:5].any() and reached.sum() > 10
    cands = nav_twin.draws(3, 9, N, 14, 8).reshape(N, 4, 2)
    assert tuple(s_exp[0, 8:10]) == tuple(cands[0, 0])  # every hazard of row 0 is far from the first candidate
    assert c_exp[:5].tolist() == {0: [0, 0, 0, 0, 0], 1: [0, 1, 0, 0, 0], 2: [0, 1, 1, 0, 0]}[level]
    assert tuple(s_exp[4, 0:2]) == (2.0, -1.0) and (np.abs(s_exp[:, 0:2]) == 2).sum() > 1
    if level:
        assert c_exp[5:].sum() > 0


@pytest.mark.parametrize('level', [0, 1, 2])
def test_circle_costs_and_walls_from_states_of_the_callers_own(level):
    """130 envs placed all over the arena [-2, 2]^2 at speed, wheels apart, one step each: costs on both walls of both
    pairs, positions clipped at the arena's edge, rewards of either sign."""
    N = 130
    rng = np.random.default_rng(level)
    s = np.zeros((N, 12), np.float32)
    s[:, 0:2] = rng.uniform(-2, 2, (N, 2))
    h = rng.standard_normal((N, 2))
    s[:, 2:4] = h / np.linalg.norm(h, axis=1, keepdims=True)
    s[:, 10:12] = rng.uniform(-0.2, 0.2, (N, 2))
    s[:, 4] = (np.float32(0.5) * (s[:, 10] + s[:, 11]).astype(np.float32)).astype(np.float32)
    s[:, 5:8] = rng.uniform(-0.1, 0.1, (N, 3))
    s[:4, 0:2] = [[0.75, 0.0], [-0.75, 0.0], [0.0, 0.75], [0.0, 0.0]]  # on a wall (no cost); at the origin (reward 0)
    s[:4, 4:] = 0
    s[4, 0:4], s[4, 10:12] = (0.74, 0, 1, 0), (0.2, 0.2)   # the corridor case of tests/test_car_twin.py: q = (0.94, 0)
    s[5, 0:4], s[5, 10:12] = (0, -0.74, 0, -1), (0.2, 0.2)
    s[6, 0:4], s[6, 10:12], s[6, 4] = (0, -1.95, 0, -1), (0.5, 0.5), 0.5  # into the arena's edge
    s[4:6, 4] = 0.2
    act = (rng.standard_normal((N, 2)) * 1.5).astype(np.float32)
    act[:4] = 0
    act[4:7] = 1
    s_exp, r_exp, c_exp = one_launch('circle', level, s, act)
    assert not c_exp[:4].any() and r_exp[3] == 0 and (r_exp > 0).any() and (r_exp < 0).any()
    assert c_exp[4:6].tolist() == {0: [0, 0], 1: [1, 0], 2: [1, 1]}[level]
    assert tuple(s_exp[6, 0:2]) == (0.0, -2.0) and (np.abs(s_exp[:, 0:2]) == 2).any()
    assert c_exp.sum() == 0 if level == 0 else 30 < c_exp.sum() < N


@pytest.mark.parametrize('task', ['goal', 'circle'])
def test_strided_actions_and_argument_checks(task):
    W = TASK[task][2]
    env = RawEnv(task, 2, 3, W, W, 7, 1)
    twin = make_twin(task, 2, 3, 7, 1)
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
    assert env.launch(2, act, 0, obs_dim=W - 1) == -1
    assert env.launch(2, act, 0, obs_dim=64 if task == 'goal' else 32) == -1  # one lane round is not the row
    assert env.launch(2, act, 0, state=None) == -1
    assert env.launch(2, None, 0) == -1  # a step without actions
    env.level = 3
    assert env.launch(2, act, 0) == -1
    env.level, env.N = 2, 0
    assert env.launch(2, act, 0) == -1
    env.N, env.ld = 3, W - 1
    assert env.launch(2, act, 0) == -1  # rows narrower than obs_dim
    torch.cuda.synchronize()
    for k, v in kept.items():
        assert torch.equal(getattr(env, k), v), k


@pytest.mark.parametrize('level', [0, 1, 2])
@pytest.mark.parametrize('task', ['goal', 'circle'])
def test_env_class_returns_what_the_twin_returns(task, level):
    """The same through the env classes: double-buffered observations, final_observation in the info of the
    truncating step only."""
    from omnisafe_amd import envs

    N, H, seed = 5, 7, 3
    env = envs.make((GOAL if task == 'goal' else CIRCLE)[level], num_envs=N, device=DEV, horizon=H, seed=seed)
    twin = make_twin(task, level, N, H, seed)
    obs, _ = env.reset()
    np.testing.assert_array_equal(obs.cpu().numpy(), twin.reset())
    gen = torch.Generator(device='cpu').manual_seed(level)
    for t in range(20):
        act = torch.randn(N, 2, generator=gen) * 1.5
        prev = obs
        obs, reward, cost, term, trunc, info = env.step(act.to(DEV))
        o_exp, r_exp, c_exp, done, final, *_ = twin.step(act.numpy())
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


# ------------------------------------------------------------------ 4. graph replay
@pytest.mark.parametrize('task', ['goal', 'circle'])
def test_rollout_graph_replay_equals_eager_launches(task, tmp_path, monkeypatch):
    """OnPolicyAdapter.rollout on the env inside the captured hipGraph against eager launches: the buffers of both
    epochs are identical (the graph is captured on the second)."""
    import omnisafe_amd

    def run(graph):
        monkeypatch.setenv('OSA_ROLLOUT_GRAPH', '1' if graph else '0')
        cfg = {'seed': 7, 'train_cfgs': {'device': DEV, 'total_steps': 2 * 64 * 24, 'vector_env_nums': 64},
               'algo_cfgs': {'steps_per_epoch': 64 * 24, 'update_iters': 2},
               'logger_cfgs': {'log_dir': str(tmp_path / ('g' if graph else 'e')), 'verbose': False},
               'env_cfgs': {'horizon': 10}}  # truncations at steps 10 and 20 of the 24
        algo = omnisafe_amd.Agent('PPOLag', (GOAL if task == 'goal' else CIRCLE)[1], custom_cfgs=cfg).agent
        snaps = []
        for _ in range(2):
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
    _, width, D, _ = TASK[task]
    assert s_g[0]['obs'].shape[-1] == D and s_g[0]['env_state'].shape == (64, width)
    assert not torch.equal(s_g[0]['obs'], s_g[1]['obs'])


# ------------------------------------------------------------------ 5. evaluator
def short_cfgs(log_dir, n=16, horizon=8, epochs=2, **logger):
    return {'train_cfgs': {'device': DEV, 'total_steps': epochs * n * 2 * horizon, 'vector_env_nums': n},
            'algo_cfgs': {'steps_per_epoch': n * 2 * horizon},
            'logger_cfgs': dict({'log_dir': log_dir, 'verbose': False, 'save_model_freq': 1000}, **logger),
            'env_cfgs': {'horizon': horizon}}


@pytest.fixture(scope='module', params=[('goal', 2), ('circle', 1)], ids=['goal2', 'circle1'])
def checkpoint(request, tmp_path_factory):
    """A 2-epoch PPOLag run at horizon 30: (task, level, log_dir, name of its last checkpoint)."""
    import omnisafe_amd

    task, level = request.param
    cfg = dict(short_cfgs(str(tmp_path_factory.mktemp('ckpt')), n=16, horizon=30, save_model_freq=1), seed=2)
    agent = omnisafe_amd.Agent('PPOLag', (GOAL if task == 'goal' else CIRCLE)[level], custom_cfgs=cfg)
    agent.learn()
    log_dir = agent.agent.logger.log_dir
    names = sorted(os.listdir(os.path.join(log_dir, 'torch_save')), key=lambda n: int(n[len('epoch-'):-len('.pt')]))
    return task, level, log_dir, names[-1]


def play(checkpoint, path, monkeypatch, K, seed=3):
    from omnisafe_amd.evaluator import Evaluator

    if path:
        monkeypatch.setenv('OSA_EVAL_PATH', path)
    else:
        monkeypatch.delenv('OSA_EVAL_PATH', raising=False)
    ev = Evaluator(seed=seed, device=DEV, verbose=False)
    ev.load_saved(*checkpoint[2:])
    r, c = ev.evaluate(num_episodes=K, trace=True)
    return np.array(r), np.array(c), np.array(ev.episode_lengths), ev.trace.cpu().numpy(), ev


@pytest.mark.parametrize('K', [5, 33])
def test_evaluator_persistent_equals_per_step_and_replays_through_the_twin(checkpoint, monkeypatch, K):
    """K = 5: a quarter-filled wave; K = 33: two full waves and one episode of a third.  The four lanes of an episode
    share the 72 (40) columns."""
    from omnisafe_amd import _lib

    task, level = checkpoint[:2]
    _, width, D, _ = TASK[task]
    H, seed = 30, 3
    kind = (48 if task == 'goal' else 64) + level
    assert _lib.load().osa_eval_trace_floats(kind, D, 2, 0) == D + 2 + 3 + width
    a = play(checkpoint, 'persistent', monkeypatch, K, seed)
    b = play(checkpoint, 'per-step', monkeypatch, K, seed)
    assert a[4].path == 'persistent' and b[4].path == 'per-step'
    for x, y in zip(a[:4], b[:4]):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x, y)
    assert play(checkpoint, '', monkeypatch, K, seed)[4].path == 'persistent'  # the default
    ret, cost, length, tr, ev = a
    assert (length == H).all() and tr.shape == (H, K, D + 2 + 3 + width)
    x, act = tr[:, :, :D], tr[:, :, D:D + 2]
    rew, cst, alive, state = tr[:, :, D + 2], tr[:, :, D + 3], tr[:, :, D + 4], tr[:, :, D + 5:]
    assert (alive == 1).all()
    mean, std = ev._normalizer._mean.cpu().numpy(), ev._normalizer._std.cpu().numpy()
    fresh = T.car_goal_reset(seed, 0, K, level) if task == 'goal' else T.car_circle_reset(seed, 0, K)
    np.testing.assert_array_equal(state[0], fresh)
    for t in range(H):
        o = twin_obs(task, state[t], level)
        np.testing.assert_array_equal(x[t], np.clip(((o - mean).astype(np.float32) / std).astype(np.float32), -5, 5))
        s2, r, c = twin_step(task, state[t], act[t], level, seed, t + 1)
        np.testing.assert_array_equal(rew[t], r)
        np.testing.assert_array_equal(cst[t], c)
        if t + 1 < H:
            np.testing.assert_array_equal(state[t + 1], s2)
    np.testing.assert_array_equal(ret, rew.astype(np.float64).cumsum(0)[-1])
    np.testing.assert_array_equal(cost, cst.astype(np.float64).sum(0))
    assert np.abs(act).max() > 0 and np.abs(rew).max() > 0
    assert state[-1][:, 10:12].any() and state[-1][:, 7].any()  # the wheels and t_prev are part of the record


# ------------------------------------------------------------------ 6. group, trust region
def _outcome(agent):
    ac = agent.agent._actor_critic  # noqa: SLF001
    torch.cuda.synchronize()
    lines = [ln for ln in open(os.path.join(agent.agent.logger.log_dir, 'progress.csv')).read().split('\n') if ln]
    hdr = lines[0].split(',')
    keep = [i for i, h in enumerate(hdr) if not h.startswith('Time/')]
    return ac.params.clone(), [[ln.split(',')[i] for i in keep] for ln in lines], hdr


@pytest.mark.parametrize('env_id', [GOAL[1], CIRCLE[1]])
def test_group_of_two_seeds_equals_two_solo_agents(env_id, tmp_path):
    import omnisafe_amd

    def cfgs(log_dir):
        return short_cfgs(log_dir, n=64, horizon=20)

    seeds = [0, 1]
    solos = []
    for s in seeds:
        a = omnisafe_amd.Agent('PPOLag', env_id, custom_cfgs=dict(cfgs(str(tmp_path / f'solo{s}')), seed=s))
        a.learn()
        solos.append(_outcome(a))
    group = omnisafe_amd.AgentGroup('PPOLag', env_id, seeds=seeds, custom_cfgs=cfgs(str(tmp_path / 'group')))
    assert len(group.learn()) == 2
    for s, member, solo in zip(seeds, group.agents, solos):
        params, rows, _ = _outcome(member)
        assert torch.equal(params, solo[0]), s
        assert rows == solo[1] and len(rows) == 3, s
    assert not torch.equal(solos[0][0], solos[1][0])


def test_cpo_on_car_goal1_end_to_end(tmp_path):
    """BASELINE config 3's algorithm at its shape (72 / 2) on an env with a real constraint: two small epochs, finite
    parameters and a logged Misc/OptimCase; the same seed gives the same run bit for bit."""
    import omnisafe_amd

    runs = []
    for k in range(2):
        a = omnisafe_amd.Agent('CPO', GOAL[1], custom_cfgs=dict(short_cfgs(str(tmp_path / f'run{k}')), seed=4))
        a.learn()
        runs.append(_outcome(a))
    params, rows, hdr = runs[0]
    assert torch.isfinite(params).all() and len(rows) == 3
    assert a.agent._env._env.observation_space.shape == (72,)  # noqa: SLF001
    cases = [int(float(r[rows[0].index('Misc/OptimCase')])) for r in rows[1:]]
    assert all(0 <= c <= 4 for c in cases), cases
    ret = [float(r[rows[0].index('Metrics/EpRet')]) for r in rows[1:]]
    assert np.isfinite(ret).all()
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


@pytest.mark.parametrize('algo', ['CPO', 'TRPOLag'])
def test_trust_region_update_at_width_40(algo, tmp_path):
    """Two epochs on CarCircle level 1 (N = 16, horizon 8): the Fisher products, conjugate gradients and line searches
    run at a policy input of 40 columns, the parameters stay finite, and the same seed gives the same run bit for
    bit."""
    import omnisafe_amd

    runs = []
    for k in range(2):
        a = omnisafe_amd.Agent(algo, CIRCLE[1], custom_cfgs=dict(short_cfgs(str(tmp_path / f'run{k}')), seed=4))
        a.learn()
        runs.append(_outcome(a))
    assert torch.isfinite(runs[0][0]).all() and len(runs[0][1]) == 3
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


# ------------------------------------------------------------------ 7. learning, directional
LEARN = {'vector_env_nums': 256, 'steps_per_epoch': 51_200, 'epochs': 10, 'horizon': 200, 'seeds': 4,
         # the point robot's check (profiles/nav_learning.md): the YAML's cost_limit of 25 per 1000-step episode at the
         # same rate for 200 steps
         'cost_limit': 5.0}


def train_group(algo, env_id, log_dir, cfg=None):
    """The seeds in one AgentGroup; per seed the EpRet / EpCost columns of its progress.csv."""
    import omnisafe_amd

    c = dict(LEARN, **(cfg or {}))
    custom = {'train_cfgs': {'device': DEV, 'total_steps': c['steps_per_epoch'] * c['epochs'],
                             'vector_env_nums': c['vector_env_nums']},
              'algo_cfgs': {'steps_per_epoch': c['steps_per_epoch']},
              'logger_cfgs': {'log_dir': log_dir, 'verbose': False, 'save_model_freq': 1000},
              'env_cfgs': {'horizon': c['horizon']}}
    if algo == 'PPOLag' and c['cost_limit'] is not None:
        custom['lagrange_cfgs'] = {'cost_limit': c['cost_limit']}
    group = omnisafe_amd.AgentGroup(algo, env_id, seeds=list(range(c['seeds'])), custom_cfgs=custom)
    group.learn()
    curves = []
    for member in group.agents:
        rows = list(csv.DictReader(open(os.path.join(member.agent.logger.log_dir, 'progress.csv'))))
        curves.append({k: np.array([float(r[f'Metrics/{k}']) for r in rows]) for k in ('EpRet', 'EpCost')})
    return curves


def test_learning_directional(tmp_path):
    """A sanity statement, not a parity claim (no reference curve exists for an env of this package's own): PPOLag on
    SynthNavCarGoal1-v0 with the point robot's budget (4 seeds in one AgentGroup, 256 envs, horizon 200, cost_limit 5,
    10 epochs of 51 200 steps).  The seed-mean EpRet of epochs 8 - 10 exceeds the first epoch's by more than two
    standard errors of the difference, and the tail EpCost is not above the first epoch's by more than two standard
    errors.  Figures: profiles/car_learning.md."""
    c = LEARN
    curves = train_group('PPOLag', GOAL[1], str(tmp_path))
    ret = np.stack([cv['EpRet'] for cv in curves])
    cost = np.stack([cv['EpCost'] for cv in curves])
    assert ret.shape == (c['seeds'], c['epochs'])
    print('EpRet seed-mean per epoch', np.round(ret.mean(0), 3).tolist())
    print('EpCost seed-mean per epoch', np.round(cost.mean(0), 3).tolist())
    d_ret = ret[:, -3:].mean(1) - ret[:, 0]
    se_ret = d_ret.std(ddof=1) / np.sqrt(len(d_ret))
    d_cost = cost[:, -3:].mean(1) - cost[:, 0]
    se_cost = d_cost.std(ddof=1) / np.sqrt(len(d_cost))
    print('EpRet tail - first', d_ret.mean(), 'se', se_ret)
    print('EpCost tail - first', d_cost.mean(), 'se', se_cost)
    assert d_ret.mean() > 2 * se_ret
    assert d_cost.mean() <= 2 * se_cost
