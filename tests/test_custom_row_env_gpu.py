"""GPU: custom device envs with an object row in LDS (LDS_ROW = true).  The generic row kernel
(osa_custom_row_env_kernel) against the specialised kernel of the built-in Goal descriptions at every lane count, the
examples tests/custom_envs/button.h and field.h against their numpy twins (tests/button_twin.py), then through the
layers: a captured graph, the evaluator's two paths and its pictures, the collector, Agent and AgentGroup.  Every
comparison is bit for bit."""
import ctypes
import gc
import os

import numpy as np
import pytest
import torch

import button_twin as B
import raw_env

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HERE = os.path.dirname(os.path.abspath(__file__))
ENVS = os.path.join(HERE, 'custom_envs')
SENTINEL = raw_env.SENTINEL
BUTTON_IDS = {False: {f'SynthNavButton{l}-v0': l for l in range(3)},
              True: {f'SynthNavCarButton{l}-v0': l for l in range(3)}}
KIND = {False: 'point', True: 'car'}


def library(header, struct):
    from omnisafe_amd import build, envs

    return envs._bind_custom(build.build_custom_env(os.path.join(ENVS, header), struct))[0]


def raw(lib, state_width, level, N, obs_dim, ld, horizon, seed):
    env = raw_env.RawEnv('osa_nav_env_step', state_width, level, N, obs_dim, ld, horizon, seed)
    if lib is not None:
        env.fn = lib.osa_custom_env_step  # (the same argument list)
    return env


@pytest.fixture
def register():
    """register_device_env of an example struct that unregisters at the end of the test."""
    import omnisafe_amd

    entered = []

    def enter(header, struct, ids, **kwargs):
        cls = omnisafe_amd.register_device_env(os.path.join(ENVS, header), struct, ids, **kwargs)
        entered.extend(ids)
        return cls

    yield enter
    omnisafe_amd.unregister_device_env(*[e for e in entered if e in omnisafe_amd.custom_envs()])


@pytest.fixture
def button(register):
    return register('button.h', 'Button', BUTTON_IDS[False], default_horizon=1000)


def everything(env, N):
    return {k: getattr(env, k).cpu().numpy() for k in ('state', 'obs', 'final', 'reward', 'cost', 'term', 'trunc',
                                                       'steps')}


# ------------------------------------------------------------------ 1. the generic kernel against the built-in one
@pytest.mark.parametrize('level', [0, 1, 2])
@pytest.mark.parametrize('car', [False, True], ids=['point', 'car'])
def test_the_row_kernel_equals_the_goal_kernel_at_every_lane_count(car, level):
    """GoalAgain / CarGoalAgain (OsaNavEnv<robot, OsaGoal> re-declared out of tree) in the generic row kernel at 16, 32
    and 64 lanes per env against osa_nav_env_step / osa_car_goal_env_step: N = 1, 3 and 130, horizon 7, 24 steps (three
    truncations) under actions uniform in [-1.5, 1.5], at the native width and in rows wider than the observation.  Every
    buffer the launches write -- sentinel rows and columns included -- holds the same bytes after every launch."""
    name, entry, obs_w = ('CarGoalAgain', 'osa_car_goal_env_step', 72) if car else ('GoalAgain', 'osa_nav_env_step', 60)
    libs = {lanes: library('goal_again.h', f'{name}{lanes}') for lanes in (16, 32, 64)}
    info = (ctypes.c_int * 8)()
    for lanes, lib in libs.items():
        assert lib.osa_custom_env_info(info) == 0 and info[6] == lanes and info[0] == 64 and info[1] == obs_w
    rng = np.random.default_rng(level + 3 * car)
    H, steps, seed = 7, 24, 17
    for N in (1, 3, 130):
        for obs_dim, ld in ((obs_w, obs_w), (obs_w + 3, obs_w + 8)):
            ref = raw_env.RawEnv(entry, 64, level, N, obs_dim, ld, H, seed)
            mine = {lanes: raw(lib, 64, level, N, obs_dim, ld, H, seed) for lanes, lib in libs.items()}
            n_trunc = 0
            for t in range(steps + 1):
                act = None if t == 0 else torch.from_numpy(rng.uniform(-1.5, 1.5, (N, 2)).astype(np.float32)).to(DEV)
                assert ref.launch(t, act, int(t == 0)) == 0
                want = everything(ref, N)
                assert ref.pads_untouched()
                for lanes, env in mine.items():
                    assert env.launch(t, act, int(t == 0)) == 0
                    for k, v in everything(env, N).items():
                        np.testing.assert_array_equal(v, want[k], err_msg=f'{k}: {lanes} lanes, N {N}, step {t}')
                n_trunc += int(want['trunc'][:N].sum()) if t else 0
                if t and want['trunc'][:N].any():  # the final rows were written: the next ones start from sentinels
                    assert not (want['final'][:N, :obs_dim] == SENTINEL).any()
                    for env in (ref, *mine.values()):
                        env.final.fill_(SENTINEL)
            assert n_trunc == 3 * N
            assert (want['state'][:N, 12:52] != 0).any() == (level > 0)


# ------------------------------------------------------------------ 2. Button against its twin
def play_button(lib, car, level, N, horizon, seed, steps, obs_dim=None, ld=None):
    """The scripted run of the twin, replayed launch by launch: the reset from the seed alone, then every step."""
    obs_w = B.OBS[car]
    obs_dim, ld = obs_dim or obs_w, ld or obs_w
    env = raw(lib, 64, level, N, obs_dim, ld, horizon, seed)
    twin = B.RowTwin(KIND[car], level, N, horizon, seed)
    o_exp = twin.reset()
    assert env.launch(0, None, 1) == 0
    np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state)
    np.testing.assert_array_equal(env.obs[:N, :obs_w].cpu().numpy(), o_exp)
    assert bool((env.final == SENTINEL).all()) and bool((env.reward == SENTINEL).all()) and env.pads_untouched()
    seen = {}
    for t in range(steps):
        act = twin.controller(t)
        o_exp, r_exp, c_exp, term, trunc, final = twin.step(act)
        assert env.launch(t + 1, torch.from_numpy(act).to(DEV), 0) == 0
        where = f'level {level}, N {N}, step {t}'
        np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state, err_msg=where)
        np.testing.assert_array_equal(env.obs[:N, :obs_w].cpu().numpy(), o_exp, err_msg=where)
        assert not env.obs[:N, obs_w:obs_dim].any(), where
        np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp, err_msg=where)
        np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp, err_msg=where)
        np.testing.assert_array_equal(env.trunc[:N].cpu().numpy(), trunc.astype(np.uint8), err_msg=where)
        np.testing.assert_array_equal(env.steps[:N].cpu().numpy(), twin.steps, err_msg=where)
        assert not env.term[:N].any() and env.pads_untouched(), where
        got_final = env.final[:N].cpu().numpy()
        np.testing.assert_array_equal(got_final[trunc, :obs_w], final[trunc], err_msg=where)
        assert (got_final[~trunc] == SENTINEL).all(), where
        if trunc.any():
            env.final.fill_(SENTINEL)
        for k, on in twin.events.items():
            seen[k] = seen.get(k, 0) + int(on.sum())
        seen['truncation'] = seen.get('truncation', 0) + int(trunc.sum())
    return seen


@pytest.mark.parametrize('level', [0, 1, 2])
@pytest.mark.parametrize('car', [False, True], ids=['point', 'car'])
def test_button_equals_its_twin_step_for_step(car, level):
    """The scripted run whose events tests/test_button_twin.py establishes (130 envs, horizon 40, 90 steps: presses,
    wrong buttons, hazards, gremlins, two truncations), and short runs at N = 1 and 3 (workgroups with a slot that has
    no env, at the default 32 lanes) in rows wider than the observation."""
    lib = library('button.h', 'CarButton' if car else 'Button')
    seen = play_button(lib, car, level, B.SCRIPT_N, B.SCRIPT_HORIZON, B.SCRIPT_SEED, B.SCRIPT_STEPS)
    assert seen['press'] > 0 and seen['wrong'] > 0 and seen['truncation'] == 2 * B.SCRIPT_N
    assert (seen['hazard'] > 0) == (level > 0) and (seen['gremlin'] > 0) == (level > 0)
    for N in (1, 3):
        obs_w = B.OBS[car]
        seen = play_button(lib, car, level, N, 7, B.SCRIPT_SEED + N, 20, obs_w + 3, obs_w + 8)
        assert seen['truncation'] == 2 * N


@pytest.mark.parametrize('car', [False, True], ids=['point', 'car'])
def test_button_in_a_captured_graph_replayed_twice(register, car):
    """make(...) on level 2, N = 130: ten steps and the commit() that folds the stream position into its device part,
    captured once and replayed twice with the scripted actions of steps 1 .. 10 and 11 .. 20 in the graph's action
    buffer (horizon 7: both replays truncate, at different places).  Every step's outputs equal the twin's."""
    from omnisafe_amd import envs

    cls = register('button.h', 'CarButton' if car else 'Button', BUTTON_IDS[car])
    assert cls.graph_safe is True and cls.lds_row is True
    N, H, K, seed = 130, 7, 10, B.SCRIPT_SEED
    env_id = list(BUTTON_IDS[car])[2]
    twin = B.RowTwin(KIND[car], 2, N, H, seed)
    twin.reset()
    acts, want = [], []
    for t in range(2 * K):
        acts.append(twin.controller(t))
        want.append(twin.step(acts[-1]) + (twin.state.copy(),))
    env = envs.make(env_id, num_envs=N, device=DEV, horizon=H, seed=seed)
    env.reset()
    env.commit()
    static_act = torch.zeros(K, N, 2, device=DEV)
    out = {k: torch.zeros(K, N, *shape, device=DEV, dtype=dt) for k, shape, dt in (
        ('obs', (B.OBS[car],), torch.float32), ('reward', (), torch.float32), ('cost', (), torch.float32),
        ('trunc', (), torch.uint8), ('final', (B.OBS[car],), torch.float32), ('state', (64,), torch.float32))}

    def ten_steps():
        for k in range(K):
            obs, reward, cost, _, trunc, _ = env.step(static_act[k])
            for name, src in (('obs', obs), ('reward', reward), ('cost', cost), ('trunc', trunc),
                              ('final', env._final), ('state', env.state)):
                out[name][k].copy_(src)
        env.commit()

    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    gc.collect()
    gc_was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            ten_steps()
    finally:
        if gc_was_enabled:
            gc.enable()
    n_trunc = 0
    for half in range(2):
        static_act.copy_(torch.from_numpy(np.stack(acts[half * K:(half + 1) * K])))
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for k in range(K):
            o_exp, r_exp, c_exp, _, trunc, final, state = want[half * K + k]
            where = f'replay {half}, step {k}'
            np.testing.assert_array_equal(got['obs'][k], o_exp, err_msg=where)
            np.testing.assert_array_equal(got['reward'][k], r_exp, err_msg=where)
            np.testing.assert_array_equal(got['cost'][k], c_exp, err_msg=where)
            np.testing.assert_array_equal(got['trunc'][k], trunc.astype(np.uint8), err_msg=where)
            np.testing.assert_array_equal(got['state'][k], state, err_msg=where)
            np.testing.assert_array_equal(got['final'][k][trunc], final[trunc], err_msg=where)
            n_trunc += int(trunc.sum())
    assert n_trunc == 2 * N


# ------------------------------------------------------------------ 3. Field against its twin
@pytest.mark.parametrize('N', [1, 3, B.FIELD_N])
def test_field_equals_its_twin_where_neighbours_end_on_different_steps(N):
    """Field (a row of 150 floats, 146 object columns, terminal()) at 16, 32 (the default) and 64 lanes: N = 5 shares
    workgroups between envs that terminate on different steps and one that only truncates
    (tests/test_button_twin.py), N = 1 and 3 leave slots of a workgroup without an env.  State, observation, reward,
    cost, both flags, the counters and the final rows equal the twin after every launch, sentinels intact."""
    H, seed, steps = B.FIELD_HORIZON, B.FIELD_SEED, B.FIELD_STEPS
    libs = {struct: library('field.h', struct) for struct in ('Field16', 'Field', 'Field64')}
    W = B.FIELD_OBS
    for obs_dim, ld in ((W, W), (W + 3, W + 8)):
        envs_ = {s: raw(lib, B.FIELD_STATE, 0, N, obs_dim, ld, H, seed) for s, lib in libs.items()}
        twin = B.RowTwin('field', 0, N, H, seed)
        o_exp = twin.reset()
        for env in envs_.values():
            assert env.launch(0, None, 1) == 0
            np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state)
            np.testing.assert_array_equal(env.obs[:N, :W].cpu().numpy(), o_exp)
            assert env.pads_untouched() and bool((env.term == 9).all())
        n_term = n_trunc = n_cost = 0
        for t in range(steps):
            act = twin.controller(t)
            o_exp, r_exp, c_exp, term, trunc, final = twin.step(act)
            for struct, env in envs_.items():
                where = f'{struct}, N {N}, obs_dim {obs_dim}, step {t}'
                assert env.launch(t + 1, torch.from_numpy(act).to(DEV), 0) == 0
                np.testing.assert_array_equal(env.term[:N].cpu().numpy(), term.astype(np.uint8), err_msg=where)
                np.testing.assert_array_equal(env.trunc[:N].cpu().numpy(), trunc.astype(np.uint8), err_msg=where)
                np.testing.assert_array_equal(env.steps[:N].cpu().numpy(), twin.steps, err_msg=where)
                np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp, err_msg=where)
                np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp, err_msg=where)
                np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state, err_msg=where)
                np.testing.assert_array_equal(env.obs[:N, :W].cpu().numpy(), o_exp, err_msg=where)
                assert not env.obs[:N, W:obs_dim].any(), where
                got_final = env.final[:N].cpu().numpy()
                np.testing.assert_array_equal(got_final[trunc, :W], final[trunc], err_msg=where)
                assert (got_final[~trunc] == SENTINEL).all() and env.pads_untouched(), where
                if trunc.any():
                    env.final.fill_(SENTINEL)
            n_term, n_trunc, n_cost = n_term + int(term.sum()), n_trunc + int(trunc.sum()), n_cost + int(c_exp.sum())
        assert n_term >= 1 and n_cost >= 1 and (n_trunc >= 1 or N == 1)


# ------------------------------------------------------------------ 4. evaluator: both paths, the twin, the pictures
def cfgs(log_dir, horizon, n=16, epochs=2):
    return {'train_cfgs': {'device': DEV, 'total_steps': epochs * n * 2 * horizon, 'vector_env_nums': n},
            'algo_cfgs': {'steps_per_epoch': n * 2 * horizon, 'update_iters': 2},
            'logger_cfgs': {'log_dir': log_dir, 'verbose': False, 'save_model_freq': 1},
            'env_cfgs': {'horizon': horizon}}


def progress(agent):
    """progress.csv of a run without its Time/ columns, and the parameters."""
    torch.cuda.synchronize()
    lines = [ln for ln in open(os.path.join(agent.agent.logger.log_dir, 'progress.csv')).read().split('\n') if ln]
    keep = [i for i, h in enumerate(lines[0].split(',')) if not h.startswith('Time/')]
    return agent.agent._actor_critic.params.clone(), [[ln.split(',')[i] for i in keep] for ln in lines]


def last_checkpoint(agent):
    log_dir = agent.agent.logger.log_dir
    names = sorted(os.listdir(os.path.join(log_dir, 'torch_save')), key=lambda s: int(s[len('epoch-'):-len('.pt')]))
    return log_dir, names[-1]


def files_of(folder):
    return {n: open(os.path.join(folder, n), 'rb').read() for n in sorted(os.listdir(folder))}


def evaluate_both_paths(checkpoint, monkeypatch, K, seed):
    from omnisafe_amd.evaluator import Evaluator

    out = {}
    for path in ('persistent', 'per-step'):
        monkeypatch.setenv('OSA_EVAL_PATH', path)
        ev = Evaluator(seed=seed, device=DEV, verbose=False)
        ev.load_saved(*checkpoint)
        r, c = ev.evaluate(num_episodes=K, trace=True)
        assert ev.path == path
        out[path] = (np.array(r), np.array(c), np.array(ev.episode_lengths), ev.trace.cpu().numpy())
    for x, y in zip(out['persistent'], out['per-step']):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x, y)
    return out['persistent']


def replay(twin, tr, in_w, H, K):
    """The traced actions through the twin: states, rewards and costs of the live episodes; returns the lengths."""
    act, rew, cst = tr[:, :, in_w:in_w + 2], tr[:, :, in_w + 2], tr[:, :, in_w + 3]
    alive, state = tr[:, :, in_w + 4], tr[:, :, in_w + 5:]
    twin.reset()
    live, length = np.ones(K, bool), np.zeros(K, np.int64)
    for t in range(H):
        np.testing.assert_array_equal(alive[t], live.astype(np.float32))
        np.testing.assert_array_equal(state[t, live], twin.state[live])
        _, r, c, term, trunc, _ = twin.step(act[t])
        np.testing.assert_array_equal(rew[t, live], r[live])
        np.testing.assert_array_equal(cst[t, live], c[live])
        length += live
        live = live & ~(term | trunc)
    assert not live.any()
    return length


def test_evaluator_paths_agree_on_button_and_draw_the_twins_pictures(button, tmp_path, monkeypatch):
    """Two epochs of PPOLag on SynthNavButton1-v0 (16 envs, horizon 16; the log holds finite numbers), then the saved
    policy on both evaluator paths: returns, costs, lengths and traces agree bit for bit and replay through the twin;
    Evaluator.render writes the same files on both paths, whose frames are tests/scene_twin.py's picture of the traced
    rows under the twin's draw()."""
    import omnisafe_amd
    import scene_twin as T
    from omnisafe_amd import apng
    from omnisafe_amd.evaluator import Evaluator

    H, K, seed = 16, 6, 3
    agent = omnisafe_amd.Agent('PPOLag', 'SynthNavButton1-v0', custom_cfgs=dict(cfgs(str(tmp_path / 'run'), H), seed=2))
    agent.learn()
    assert type(agent.agent._env._env) is button and agent.agent._env._env.graph_safe
    params, rows = progress(agent)
    assert torch.isfinite(params).all() and len(rows) == 3
    assert all(np.isfinite(float(v)) for row in rows[1:] for v in row if v != '')
    checkpoint = last_checkpoint(agent)
    ret, cost, length, tr = evaluate_both_paths(checkpoint, monkeypatch, K, seed)
    in_w = B.OBS[False]
    assert tr.shape == (H, K, in_w + 2 + 3 + 64)
    np.testing.assert_array_equal(length, replay(B.RowTwin('point', 1, K, H, seed), tr, in_w, H, K))
    np.testing.assert_array_equal(length, np.full(K, H))
    np.testing.assert_array_equal(ret, tr[:, :, in_w + 2].astype(np.float64).cumsum(0)[-1])
    np.testing.assert_array_equal(cost, tr[:, :, in_w + 3].astype(np.float64).sum(0))
    written = {}
    for path in ('persistent', 'per-step'):
        monkeypatch.setenv('OSA_EVAL_PATH', path)
        ev = Evaluator(seed=seed, device=DEV, verbose=False)
        ev.load_saved(*checkpoint)
        out = str(tmp_path / path)
        ev.render(num_episodes=2, width=64, height=48, trail=4, save_replay_path=out)
        written[path] = files_of(out)
    assert written['persistent'] == written['per-step']
    for k in range(2):
        states = tr[:, k, in_w + 5:]
        hit = np.zeros(H, np.uint8)
        hit[1:] = tr[:-1, k, in_w + 3] > 0
        frames = apng.read_apng(os.path.join(str(tmp_path / 'persistent'), f'eval-episode-{k}.png'))
        want = T.render(B.button_draw(False), B.button_position, B.BUTTON_VIEW, states, 0, H, 4, hit, 0, 64, 48, 2,
                        level=1)
        assert len(frames) == H and np.array_equal(np.stack(frames), want)


def test_evaluator_paths_agree_on_field(register, tmp_path, monkeypatch):
    """Field (150 state floats in every trace record, episodes that end themselves): both paths agree, and the twin
    gives the lengths -- some below the horizon, some at it."""
    import test_offline_collector_gpu as OC

    H, K, seed = 10, 33, B.FIELD_SEED
    cls = register('field.h', 'Field', ['Field-v0'], default_horizon=H)
    assert cls.lds_row and cls.terminates and cls.trace_state_floats == 150
    # a policy that pushes the second action against its bound: the mass runs up, v_y -> 0.5, and passes y = 2 within
    # nine steps from y0 > 0.26, on the tenth from y0 > -0.07, and not at all from further down (y0 = 0.5 u >= -0.75)
    monkeypatch.setattr(OC, 'H', H)
    monkeypatch.setitem(OC.ENVS, 'Field-v0', (B.FIELD_OBS, 2, None))
    root = OC.make_checkpoint(str(tmp_path / 'ck'), 'Field-v0', push_up=True)
    ret, cost, length, tr = evaluate_both_paths((root, 'epoch-0.pt'), monkeypatch, K, seed)
    assert tr.shape == (H, K, B.FIELD_OBS + 2 + 3 + 150)
    np.testing.assert_array_equal(length, replay(B.RowTwin('field', 0, K, H, seed), tr, B.FIELD_OBS, H, K))
    print(f'Field lengths {sorted(length.tolist())}')
    assert (length < H).any() and (length == H).any() and (length >= 1).all()
    np.testing.assert_array_equal(cost, tr[:, :, B.FIELD_OBS + 3].astype(np.float64).sum(0))


def test_env_render_draws_the_twins_picture(register):
    import scene_twin as T
    from omnisafe_amd import envs

    for car in (False, True):
        register('button.h', 'CarButton' if car else 'Button', BUTTON_IDS[car])
        env = envs.make(list(BUTTON_IDS[car])[2], num_envs=3, device=DEV, horizon=9, seed=4)
        env.reset()
        for _ in range(5):
            env.step(torch.full((3, 2), 0.7, device=DEV))
        state = env.state.cpu().numpy()
        assert state[:, B.K_COL].tolist() == [5, 5, 5]
        for lane, camera in ((0, 'fixed'), (2, 'track')):
            img = env.render(lane=lane, width=64, height=48, camera_name=camera)
            want = T.render(B.button_draw(car), B.button_position, B.BUTTON_VIEW, state[lane:lane + 1], 0, 1, 0, None,
                            int(camera == 'track'), 64, 48, 2, level=2)[0]
            assert img.shape == (48, 64, 3) and np.array_equal(img, want)


# ------------------------------------------------------------------ 5. collector
def test_collector_rows_replay_through_the_twin(button, tmp_path, monkeypatch):
    """OfflineDataCollector on SynthNavButton1-v0, 17 lanes of 23 rows at horizon 7: the persistent path's rows equal
    the per-step path's and replay through the twin from the seed alone."""
    import test_offline_collector_gpu as OC

    env_id, K = 'SynthNavButton1-v0', 17
    S = OC.rows_for(K)
    OC.ENVS[env_id] = (B.OBS[False], 2, None)
    try:
        root = OC.make_checkpoint(str(tmp_path / 'ck'), env_id)
        data, _ = OC.collect([(root, S)], env_id, K, 'persistent', monkeypatch, tmp_path / 'a')
        other, _ = OC.collect([(root, S)], env_id, K, 'per-step', monkeypatch, tmp_path / 'b')
    finally:
        del OC.ENVS[env_id]
    for k in OC.FIELDS:
        assert np.array_equal(data[k], other[k]), k
    rows, live = OC.lane_rows(data, S, K)
    twin = B.RowTwin('point', 1, K, OC.H, OC.SEED)
    obs = twin.reset()
    ends = 0
    for t in range(rows['obs'].shape[0]):
        m = live[t]
        assert np.array_equal(rows['obs'][t][m], obs[m]), t
        act = np.where(m[:, None], OC.scaled(rows['action'][t]), np.float32(0))
        nobs, r, c, _, trunc, final = twin.step(act)
        assert np.array_equal(rows['reward'][t][m, 0], r[m]) and np.array_equal(rows['cost'][t][m, 0], c[m]), t
        assert np.array_equal(rows['next_obs'][t][m], np.where(trunc[:, None], final, nobs)[m]), t
        assert np.array_equal(rows['done'][t][m, 0], trunc[m].astype(np.float32)), t
        ends += int(trunc.all())
        obs = nobs
    assert ends == 3  # (23 steps at horizon 7)


# ------------------------------------------------------------------ 6. Agent and AgentGroup
def test_agent_group_equals_the_solo_agents(button, tmp_path):
    """Agent('PPOLag', 'SynthNavButton1-v0'), two epochs of 16 envs x 32 steps at horizon 16: member s of an
    AgentGroup of seeds [0, 1] equals the solo agent of seed s in parameters and in every column but Time/*."""
    import omnisafe_amd

    solos = []
    for seed in (0, 1):
        solo = omnisafe_amd.Agent('PPOLag', 'SynthNavButton1-v0',
                                  custom_cfgs=dict(cfgs(str(tmp_path / f'solo{seed}'), 16), seed=seed))
        solo.learn()
        solos.append(progress(solo))
    group = omnisafe_amd.AgentGroup('PPOLag', 'SynthNavButton1-v0', seeds=[0, 1],
                                    custom_cfgs=cfgs(str(tmp_path / 'group'), 16))
    assert len(group.learn()) == 2
    for member, (s_params, s_rows) in zip(group.agents, solos):
        g_params, g_rows = progress(member)
        assert torch.equal(g_params, s_params) and g_rows == s_rows
    assert not torch.equal(solos[0][0], solos[1][0]) and torch.isfinite(solos[0][0]).all()


# ------------------------------------------------------------------ 7. runtime parameters with an object row
def test_runtime_parameters_combine_with_an_object_row(register):
    """FieldParam (field.h with the discs' radius as a runtime parameter) through the parameter-taking entry point of
    the row kernel, 5 envs that end on different steps: at the default radius every output is Field's twin's; at radius
    0 nothing costs and everything else is unchanged; the envs' parameter rows hold the value after every reset."""
    from omnisafe_amd import envs

    cls = register('field.h', 'FieldParam', ['FieldParam-v0'], default_horizon=B.FIELD_HORIZON)
    assert cls.lds_row is True and cls.param_names == ('radius',) and cls.entry_point == 'osa_custom_env_step_params'
    assert np.float32(cls.param_defaults[0]) == np.float32(0.15)
    N, H, seed = B.FIELD_N, B.FIELD_HORIZON, B.FIELD_SEED
    for cfgs_, radius in (({}, 0.15), ({'radius': 0.0}, 0.0)):
        env = envs.make('FieldParam-v0', num_envs=N, device=DEV, horizon=H, seed=seed, **cfgs_)
        twin = B.RowTwin('field', 0, N, H, seed)
        obs, _ = env.reset()
        np.testing.assert_array_equal(obs.cpu().numpy(), twin.reset())
        n_term = n_cost = 0
        for t in range(B.FIELD_STEPS):
            act = twin.controller(t)
            o_exp, r_exp, c_exp, term, trunc, _ = twin.step(act)
            obs, reward, cost, terminated, truncated, _ = env.step(torch.from_numpy(act).to(DEV))
            np.testing.assert_array_equal(obs.cpu().numpy(), o_exp)
            np.testing.assert_array_equal(env.state.cpu().numpy(), twin.state)
            np.testing.assert_array_equal(reward.cpu().numpy(), r_exp)
            np.testing.assert_array_equal(cost.cpu().numpy(), c_exp if radius > 0 else np.zeros(N, np.float32))
            np.testing.assert_array_equal(terminated.cpu().numpy(), term.astype(np.uint8))
            np.testing.assert_array_equal(truncated.cpu().numpy(), trunc.astype(np.uint8))
            np.testing.assert_array_equal(env.params.cpu().numpy(), np.full((N, 1), radius, np.float32))
            n_term, n_cost = n_term + int(term.sum()), n_cost + int(c_exp.sum())
        assert n_term >= 1 and n_cost >= 1
