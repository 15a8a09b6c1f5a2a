"""GPU: runtime parameters of custom device envs (include/omnisafe_amd_env.h, PARAMETERS).  The example env
tests/custom_envs/gust.h against its numpy twin (tests/gust_twin.py) in the generic per-step kernel, then through the
layers: make() and env_cfgs, set_param under a replaying rollout graph, the evaluator's and the collector's two paths,
the pictures, Agent and AgentGroup.  Every comparison is bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import gust_twin as G
import raw_env
import scene_twin

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HERE = os.path.dirname(os.path.abspath(__file__))
GUST = os.path.join(HERE, 'custom_envs', 'gust.h')
SENTINEL = raw_env.SENTINEL
EINVAL, EUNSUPPORTED = -1, -3
RANGED = {'wind': (0.0, 0.5), 'band': (0.4, 0.8)}  # two ranged, two fixed (drag and reach at their defaults)
FIELDS = ('obs', 'action', 'reward', 'cost', 'next_obs', 'done')


@pytest.fixture
def gust():
    """Gust (ends episodes by arriving) and GustEndless (the collector's per-step path takes no terminating class)."""
    import omnisafe_amd

    cls = omnisafe_amd.register_device_env(GUST, 'Gust', ['Gust-v0'], default_horizon=40)
    omnisafe_amd.register_device_env(GUST, 'GustEndless', ['GustEndless-v0'], default_horizon=40)
    yield cls
    omnisafe_amd.unregister_device_env('Gust-v0', 'GustEndless-v0')


class RawGust(raw_env.RawEnv):
    """osa_custom_env_step_params on buffers of the test's own: the parameter rows in a matrix of stride P + 3 with
    PAD sentinel rows in front of env 0 and behind env N - 1."""

    def __init__(self, cls, rng, N, horizon, seed, obs_dim=G.OBS, ld=G.OBS):
        super().__init__('osa_nav_env_step', G.STATE, 0, N, obs_dim, ld, horizon, seed)
        self.fn = cls.library().osa_custom_env_step_params
        self.plain = cls.library().osa_custom_env_step
        self.ld_par = G.P + 3
        self.par_all = torch.full((N + 2 * self.PAD, self.ld_par), SENTINEL, dtype=torch.float32, device=DEV)
        self.par = self.par_all[self.PAD:self.PAD + N]
        self.range = torch.from_numpy(np.asarray(rng, np.float32)).to(DEV)

    def launch(self, pos, action, reset_only, rng='own', par='own', ld_par=None, fn=None):
        p = self._lib.ptr
        ld_a = action.stride(0) if action is not None else 0
        tail = () if fn is self.plain else (p(self.range) if rng == 'own' else None,
                                            p(self.par) if par == 'own' else None,
                                            self.ld_par if ld_par is None else ld_par)
        return (fn or self.fn)(
            self.seed, pos, p(self.base), self.N, self.D, self.horizon, self.level, p(self.state), p(self.steps),
            p(action), ld_a, p(self.obs), self.ld, p(self.reward), p(self.cost), p(self.term), p(self.trunc),
            p(self.final), self.ld, reset_only, *tail, self._lib.stream_ptr())

    def par_pads_untouched(self):
        N, PAD = self.N, self.PAD
        return (bool((self.par_all[:PAD] == SENTINEL).all()) and bool((self.par_all[PAD + N:] == SENTINEL).all())
                and bool((self.par_all[:, G.P:] == SENTINEL).all()))


def play_against_the_twin(cls, rng, N, H, steps, seed, steered):
    """Reset, then `steps` steps: everything the launch writes equals the twin at every step.  Returns the counts of
    terminations, truncations and cost steps."""
    env = RawGust(cls, rng, N, H, seed)
    twin = G.GustTwin(rng, N, H, seed)
    o_exp = twin.reset()
    assert env.launch(0, None, 1) == 0
    np.testing.assert_array_equal(env.par[:, :G.P].cpu().numpy(), twin.par)
    np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state)
    np.testing.assert_array_equal(env.obs[:N].cpu().numpy(), o_exp)
    assert bool((env.final == SENTINEL).all()) and env.par_pads_untouched()
    noise = np.random.default_rng(N).uniform(-1.5, 1.5, (steps, N, 2)).astype(np.float32)
    n_term = n_trunc = n_cost = 0
    resets = np.zeros(N, int)
    for t in range(steps):
        act = G.steer(twin.state, noise[t]) if steered else noise[t]
        old_par = twin.par.copy()
        o_exp, r_exp, c_exp, term, trunc, final = twin.step(act)
        where = f'N {N}, step {t}'
        assert env.launch(t + 1, torch.from_numpy(act).to(DEV), 0) == 0
        np.testing.assert_array_equal(env.term[:N].cpu().numpy(), term.astype(np.uint8), err_msg=where)
        np.testing.assert_array_equal(env.trunc[:N].cpu().numpy(), trunc.astype(np.uint8), err_msg=where)
        np.testing.assert_array_equal(env.steps[:N].cpu().numpy(), twin.steps, err_msg=where)
        np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp, err_msg=where)
        np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp, err_msg=where)
        np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state, err_msg=where)
        np.testing.assert_array_equal(env.obs[:N].cpu().numpy(), o_exp, err_msg=where)
        np.testing.assert_array_equal(env.par[:, :G.P].cpu().numpy(), twin.par, err_msg=where)
        got_final = env.final[:N].cpu().numpy()
        np.testing.assert_array_equal(got_final[trunc], final[trunc], err_msg=where)  # under the OLD parameters
        assert (got_final[~trunc] == SENTINEL).all(), where
        assert env.pads_untouched() and env.par_pads_untouched(), where
        ended = term | trunc
        # a row changes at its env's reset and nowhere else; the final observation shows the old band (column 6)
        np.testing.assert_array_equal(twin.par[~ended], old_par[~ended])
        np.testing.assert_array_equal(got_final[trunc, 6], old_par[trunc, 2])
        if trunc.any():
            env.final.fill_(SENTINEL)
        resets += ended
        n_term, n_trunc, n_cost = n_term + int(term.sum()), n_trunc + int(trunc.sum()), n_cost + int(c_exp.sum())
    assert (resets >= 3).all()
    return n_term, n_trunc, n_cost


# ------------------------------------------------------------------ 1. the per-step kernel against the twin
@pytest.mark.parametrize('N', [1, 3, 130])
def test_trace_equals_the_twin(gust, N):
    """17 steps at horizon 5 (every env resets at least three times) under actions uniform in [-1.5, 1.5], two
    parameters ranged and two fixed: obs, reward, cost, flags, counters, state, the parameter rows and the final
    observation -- under the ended episode's parameters -- equal the twin at every step; the rows live at stride P + 3
    between sentinel rows, which survive."""
    rng = G.ranges(**RANGED)
    n_term, n_trunc, _ = play_against_the_twin(gust, rng, N, 5, 17, 7, steered=False)
    assert n_trunc >= 3 * N - n_term


# ------------------------------------------------------------------ 2. defaults, make() and env_cfgs
def test_defaults_and_env_cfgs(gust):
    """No env_cfgs: the twin's trace at PARAM_DEFAULT.  wind=0.45 changes the trace, and to the twin's at 0.45.  (On
    the parent commit the class has no param_names and the key is dropped.)"""
    from omnisafe_amd import envs

    assert gust.param_names == G.NAMES
    np.testing.assert_array_equal(np.float32(gust.param_defaults), G.DEFAULT)
    N, H, seed = 3, 5, 2
    acts = np.random.default_rng(0).uniform(-1.5, 1.5, (17, N, 2)).astype(np.float32)
    traces = []
    for cfgs in ({}, {'wind': 0.45}, RANGED):
        env = envs.make('Gust-v0', num_envs=N, device=DEV, horizon=H, seed=seed, **cfgs)
        assert type(env) is gust and env.graph_safe
        twin = G.GustTwin(G.ranges(**cfgs), N, H, seed)
        np.testing.assert_array_equal(env.param_ranges.cpu().numpy(), twin.rng)
        np.testing.assert_array_equal(env.reset()[0].cpu().numpy(), twin.reset())
        assert env.params.shape == (N, G.P) and env.param_ranges.shape == (2, G.P)
        rows = []
        for t in range(17):
            obs, r, c, term, trunc, _ = env.step(torch.from_numpy(acts[t]).to(DEV))
            o_exp, r_exp, c_exp, term_exp, trunc_exp, _ = twin.step(acts[t])
            np.testing.assert_array_equal(obs.cpu().numpy(), o_exp)
            np.testing.assert_array_equal(r.cpu().numpy(), r_exp)
            np.testing.assert_array_equal(c.cpu().numpy(), c_exp)
            np.testing.assert_array_equal(term.cpu().numpy(), term_exp.astype(np.uint8))
            np.testing.assert_array_equal(trunc.cpu().numpy(), trunc_exp.astype(np.uint8))
            np.testing.assert_array_equal(env.params.cpu().numpy(), twin.par)
            rows.append(o_exp)
        if not cfgs:
            np.testing.assert_array_equal(env.params.cpu().numpy(), np.broadcast_to(G.DEFAULT, (N, G.P)))
        traces.append(np.stack(rows))
    assert not np.array_equal(traces[0], traces[1]) and not np.array_equal(traces[0], traces[2])
    with pytest.raises(TypeError, match='wnid'):
        envs.make('Gust-v0', num_envs=N, device=DEV, wnid=0.3)
    with pytest.raises(ValueError):
        envs.make('Gust-v0', num_envs=N, device=DEV, wind=(0.5, 0.1))
    with pytest.raises(TypeError):
        env.set_param('wnid', 0.1)
    with pytest.raises(ValueError):
        env.set_param('wind', float('nan'))


# ------------------------------------------------------------------ 3. terminal() with parameters
def test_terminal_sees_the_parameters_and_the_redraw_is_at_the_ending_step(gust):
    """reach (the goal's radius: terminal() and the goal's place) and wind ranged, steered actions at horizon 12: envs
    arrive at differing steps, each is redrawn at the position of the step that ended it, all equal to the twin."""
    rng = G.ranges(wind=(0.0, 0.5), reach=(0.05, 0.3))
    n_term, n_trunc, n_cost = play_against_the_twin(gust, rng, 130, 12, 40, 11, steered=True)
    assert n_term >= 50 and n_trunc >= 50 and n_cost >= 10, (n_term, n_trunc, n_cost)


# ------------------------------------------------------------------ 4. set_param under a replaying rollout graph
def rollout_cfgs(log_dir, n, horizon, steps, epochs, env_cfgs=None, **algo):
    return {'seed': 7, 'train_cfgs': {'device': DEV, 'total_steps': epochs * n * steps, 'vector_env_nums': n},
            'algo_cfgs': dict({'steps_per_epoch': n * steps, 'update_iters': 2}, **algo),
            'logger_cfgs': {'log_dir': log_dir, 'verbose': False},
            'env_cfgs': dict({'horizon': horizon}, **(env_cfgs or {}))}


def test_set_param_reaches_a_replaying_graph(gust, tmp_path, monkeypatch):
    """Four epochs of OnPolicyAdapter.rollout (32 envs, 40 steps at horizon 16; the graph is captured on the second and
    replayed for two more) with set_param('wind', ...) between them: buffers, states and parameter rows equal eager
    launches with the same calls.  In the eager run every step is watched: a row changes only where its env was reset,
    so an epoch starts under the old range and every env moves into the new one at its first reset."""
    import omnisafe_amd

    N, H, T = 32, 16, 40
    winds = [None, (0.3, 0.5), (0.6, 0.9), 0.05]  # before epoch e

    def run(graph):
        monkeypatch.setenv('OSA_ROLLOUT_GRAPH', '1' if graph else '0')
        cfg = rollout_cfgs(str(tmp_path / ('g' if graph else 'e')), N, H, T, 4, env_cfgs={'wind': (0.0, 0.2)})
        algo = omnisafe_amd.Agent('PPOLag', 'Gust-v0', custom_cfgs=cfg).agent
        env = algo._env._env
        assert type(env) is gust and env.graph_safe
        step = env.step
        if not graph:
            def watched(action):
                before, out = env.params.clone(), step(action)
                changed = (env.params != before).any(1)
                assert not bool((changed & (env._steps != 0)).any())  # only at a reset
                return out
            env.step = watched
        snaps = []
        for epoch in range(4):
            if winds[epoch] is not None:
                env.set_param('wind', winds[epoch])
            start = env.params.clone()
            algo._env.rollout(steps_per_epoch=algo._steps_per_epoch, agent=algo._actor_critic, buffer=algo._buf,
                              logger=algo._logger)
            snap = {k: v.clone() for k, v in algo._buf.data.items()}
            snap.update(env_state=env.state.clone(), env_params=env.params.clone(), start_params=start,
                        env_ranges=env.param_ranges.clone())
            algo._update()
            snaps.append(snap)
            algo._logger.dump_tabular()
        return algo, snaps

    a_g, s_g = run(True)
    a_e, s_e = run(False)
    assert a_g._env.last_rollout_graphed is True and not getattr(a_e._env, 'last_rollout_graphed', False)
    for ep, (g, e) in enumerate(zip(s_g, s_e)):
        for k in g:
            assert torch.equal(g[k].cpu(), e[k].cpu()), (ep, k)
    for ep, lo, hi in ((1, 0.3, 0.5), (2, 0.6, 0.9), (3, 0.05, 0.05)):  # T > 2 H: every env was reset under the range
        wind = s_g[ep]['env_params'][:, 0].cpu().numpy()
        assert (wind >= np.float32(lo)).all() and (wind <= np.float32(hi)).all(), (ep, wind)
        before = s_g[ep]['start_params'][:, 0].cpu().numpy()  # ... and started the epoch under the one before
        assert torch.equal(s_g[ep]['start_params'], s_g[ep - 1]['env_params'])
        assert not ((before >= np.float32(lo)) & (before <= np.float32(hi))).any()


# ------------------------------------------------------------------ 5. argument checks
def test_argument_checks_launch_nothing(gust):
    N = 3
    env = RawGust(gust, G.ranges(**RANGED), N, 5, 1)
    act = torch.zeros(N, 2, device=DEV)
    for reset_only, action in ((1, None), (0, act)):
        assert env.launch(0, action, reset_only, rng=None) == EINVAL
        assert env.launch(0, action, reset_only, par=None) == EINVAL
        assert env.launch(0, action, reset_only, ld_par=G.P - 1) == EINVAL
        assert env.launch(0, action, reset_only, fn=env.plain) == EUNSUPPORTED  # (it would run with unbound parameters)
    torch.cuda.synchronize()
    assert bool((env.par_all == SENTINEL).all()) and bool((env.state == SENTINEL).all())
    assert bool((env.obs == SENTINEL).all()) and bool((env.steps == 99).all())


# ------------------------------------------------------------------ 6. evaluator
def make_checkpoint(root, env_id, env_cfgs, seed=0):
    """config.json + torch_save/epoch-0.pt as the logger writes them: a randomly initialised [64, 64] actor, no
    observation normaliser (the policy sees the env's rows)."""
    from omnisafe_amd.config import Config, get_default_kwargs
    from omnisafe_amd.models import ConstraintActorCritic
    from omnisafe_amd.spaces import Box

    d = get_default_kwargs('PPOLag')
    d.update({'algo': 'PPOLag', 'env_id': env_id, 'exp_name': f'PPOLag-{{{env_id}}}', 'seed': seed,
              'env_cfgs': env_cfgs})
    d['algo_cfgs']['obs_normalize'] = False
    cfg = Config.dict2config(d)
    os.makedirs(os.path.join(root, 'torch_save'), exist_ok=True)
    with open(os.path.join(root, 'config.json'), 'w', encoding='utf-8') as f:
        json.dump(d, f)
    torch.manual_seed(seed)
    ac = ConstraintActorCritic(Box(-np.inf, np.inf, (G.OBS,)), Box(-1.0, 1.0, (G.ACT,)), cfg.model_cfgs, epochs=1,
                               device=DEV)
    pi = {k: v.detach().cpu().clone() for k, v in ac.actor.state_dict().items()}
    pi['log_std'] = torch.tensor([-0.6, -0.35], dtype=torch.float32)
    last = sorted(k for k in pi if k.endswith('.bias'))[-1]
    pi[last] = torch.tensor([1.5, 0.0])  # flies in +x, towards the goal
    torch.save({'pi': pi}, os.path.join(root, 'torch_save', 'epoch-0.pt'))
    return root


def play(root, path, monkeypatch, K, seed, **kwargs):
    from omnisafe_amd.evaluator import Evaluator

    monkeypatch.setenv('OSA_EVAL_PATH', path)
    ev = Evaluator(seed=seed, device=DEV, verbose=False)
    ev.load_saved(root, 'epoch-0.pt')
    r, c = ev.evaluate(num_episodes=K, trace=True, **kwargs)
    assert ev.path == path
    return [np.array(r), np.array(c), np.array(ev.episode_lengths), ev.trace.cpu().numpy(), ev.episode_params], ev


def replay_through_the_twin(out, rng, K, H, seed):
    ret, cost, length, tr, par = out
    in_w = G.OBS
    np.testing.assert_array_equal(par, G.param_draw(rng, seed, 0, np.arange(K)))
    x, act = tr[:, :, :G.OBS], tr[:, :, in_w:in_w + 2]
    rew, cst, alive, state = tr[:, :, in_w + 2], tr[:, :, in_w + 3], tr[:, :, in_w + 4], tr[:, :, in_w + 5:]
    twin = G.GustTwin(rng, K, H, seed)
    o = twin.reset()
    live = np.ones(K, bool)
    twin_len = np.zeros(K, np.int64)
    for t in range(tr.shape[0]):
        np.testing.assert_array_equal(alive[t], live.astype(np.float32))
        np.testing.assert_array_equal(state[t, live], twin.state[live])
        np.testing.assert_array_equal(x[t, live], o[live])
        o, r, c, term, trunc, _ = twin.step(act[t])
        np.testing.assert_array_equal(rew[t, live], r[live])
        np.testing.assert_array_equal(cst[t, live], c[live])
        twin_len += live
        live = live & ~(term | trunc)
    assert not live.any()
    np.testing.assert_array_equal(length, twin_len)
    np.testing.assert_array_equal(ret, rew.astype(np.float64).cumsum(0)[-1])
    np.testing.assert_array_equal(cost, cst.astype(np.float64).sum(0))


def test_evaluator_paths_agree_and_replay_through_the_twin(gust, tmp_path, monkeypatch):
    """K = 1, 5 (partly filled waves) and 20 (past the 16 episodes of one wave): the persistent kernel and the per-step
    path give the same returns, costs, lengths, traces and episode_params; the rows are the twin's draw at position 0,
    and the traced actions replay through the twin under them.  env_params={'wind': 0.4} overlays the run's range."""
    H, seed = 16, 3
    root = make_checkpoint(str(tmp_path / 'ck'), 'Gust-v0', dict({'horizon': H}, **{k: list(v) for k, v in RANGED.items()}))
    rng = G.ranges(**RANGED)
    for K in (1, 5, 20):
        a, _ = play(root, 'persistent', monkeypatch, K, seed)
        b, _ = play(root, 'per-step', monkeypatch, K, seed)
        for x, y in zip(a, b):
            assert x.shape == y.shape
            np.testing.assert_array_equal(x, y)
        assert a[4].shape == (K, G.P) and a[3].shape == (H, K, G.OBS + 2 + 3 + G.TRACE)
        replay_through_the_twin(a, rng, K, H, seed)
    assert len(np.unique(a[4][:, 0])) == 20  # the episodes' rows differ
    print(f'lengths at K = 20: {sorted(a[2].tolist())}')
    for path in ('persistent', 'per-step'):
        c, ev = play(root, path, monkeypatch, 20, seed, env_params={'wind': 0.4})
        np.testing.assert_array_equal(c[4][:, 0], np.full(20, np.float32(0.4)))
        np.testing.assert_array_equal(c[4][:, 2], a[4][:, 2])  # band keeps the run's range (and its draw)
        assert not np.array_equal(c[3], a[3])
        replay_through_the_twin(c, G.ranges(wind=0.4, band=RANGED['band']), 20, H, seed)
    d, _ = play(root, 'persistent', monkeypatch, 20, seed)  # the overlay was for that call alone
    np.testing.assert_array_equal(d[3], a[3])


# ------------------------------------------------------------------ 7. collector
def scaled(action):
    """ActionScale of the recorded sample in float32 (bounds -1 / 1 on both sides), as osa_action_scale1."""
    F = np.float32
    a = np.asarray(action, np.float32)
    return (F(-1) + ((F(2) * (a - F(-1)).astype(np.float32)).astype(np.float32) / F(2)).astype(np.float32)).astype(
        np.float32)


def test_collector_paths_agree_and_replay_through_the_twin(gust, tmp_path, monkeypatch):
    """GustEndless-v0 with ranged parameters, K = 5 lanes of Q = 23 rows at horizon 7 (every lane plays three episodes
    and starts a fourth): the persistent kernel's file equals the per-step path's, and the rows replay through the twin,
    whose parameter rows are redrawn at every ending step."""
    import omnisafe_amd
    from omnisafe_amd.offline import lane_layout

    env_id, K, H, seed = 'GustEndless-v0', 5, 7, 11
    S = K * 23 - 2
    root = make_checkpoint(str(tmp_path / 'ck'), env_id, {'horizon': H})
    cfgs = dict({'horizon': H}, **RANGED)
    data = {}
    for path in ('persistent', 'per-step'):
        monkeypatch.setenv('OSA_COLLECT_PATH', path)
        col = omnisafe_amd.OfflineDataCollector(S, env_id, seed=seed, device=DEV, num_envs=K, env_cfgs=cfgs)
        col.register_agent(root, 'epoch-0.pt', S)
        col.collect(str(tmp_path / path))
        assert col.path == path
        with np.load(os.path.join(str(tmp_path / path), f'{env_id}_data.npz')) as f:
            assert sorted(f.files) == sorted(FIELDS)  # the file's keys are what they were
            data[path] = {k: f[k] for k in FIELDS}
    for k in FIELDS:
        np.testing.assert_array_equal(data['persistent'][k], data['per-step'][k], err_msg=k)
    Q, lanes = lane_layout(S, K)
    assert Q == 23 and Q // H >= 3
    d = data['persistent']
    twin = G.GustTwin(G.ranges(**RANGED), K, H, seed, terminates=False)
    obs = twin.reset()
    seen = [twin.par.copy()]
    for t in range(Q):
        m = np.array([a + t < b for a, b in lanes])
        row = np.array([min(a + t, S - 1) for a, _ in lanes])
        np.testing.assert_array_equal(d['obs'][row][m], obs[m], err_msg=str(t))
        act = np.where(m[:, None], scaled(d['action'][row]), np.float32(0))
        nobs, r, c, _, trunc, final = twin.step(act)
        np.testing.assert_array_equal(d['reward'][row][m, 0], r[m])
        np.testing.assert_array_equal(d['cost'][row][m, 0], c[m])
        np.testing.assert_array_equal(d['next_obs'][row][m], np.where(trunc[:, None], final, nobs)[m])
        np.testing.assert_array_equal(d['done'][row][m, 0], trunc[m].astype(np.float32))
        if trunc.all():
            seen.append(twin.par.copy())
        obs = nobs
    assert len(seen) == 4 and all((seen[i][:, 0] != seen[i + 1][:, 0]).all() for i in range(3))


# ------------------------------------------------------------------ 8. pictures
def gust_picture(par, rows, first, count, trail, hit, camera, W, H):
    return scene_twin.render(G.gust_draw(par), G.position, G.VIEW, rows, first, count, trail, hit, camera, W, H, 2,
                             level=0, track=G.TRACK)


def test_render_paints_the_episodes_own_parameters(gust, tmp_path, monkeypatch):
    """Evaluator.render of three Gust episodes with band and reach ranged: every frame is the scene twin's picture under
    that episode's row -- the corridor's walls at its band, the goal at its radius -- and two episodes with different
    rows give different frames.  env.render(lane) paints the env's current row."""
    from omnisafe_amd import apng, envs
    from omnisafe_amd.evaluator import Evaluator

    H, K, seed = 16, 3, 3
    cfgs = {'horizon': H, 'band': [0.3, 0.9], 'reach': [0.1, 0.3]}
    root = make_checkpoint(str(tmp_path / 'ck'), 'Gust-v0', cfgs)
    monkeypatch.delenv('OSA_EVAL_PATH', raising=False)
    ev = Evaluator(seed=seed, device=DEV, verbose=False)
    ev.load_saved(root, 'epoch-0.pt')
    out = str(tmp_path / 'video')
    ev.render(num_episodes=K, width=64, height=48, trail=4, save_replay_path=out)
    par, tr = ev.episode_params, ev.trace.cpu().numpy()
    np.testing.assert_array_equal(par, G.param_draw(G.ranges(band=(0.3, 0.9), reach=(0.1, 0.3)), seed, 0, np.arange(K)))
    rec, firsts = tr.shape[2], []
    for k in range(K):
        n = int(ev.episode_lengths[k])
        rows = tr[:, k, rec - G.TRACE:]
        hit = np.zeros(H, np.uint8)
        hit[1:] = tr[:-1, k, rec - G.TRACE - 2] > 0
        frames = apng.read_apng(os.path.join(out, f'eval-episode-{k}.png'))
        assert len(frames) == n
        assert np.array_equal(np.stack(frames), gust_picture(par[k], rows, 0, n, 4, hit, 0, 64, 48))
        still = apng.read_apng(os.path.join(out, f'eval-episode-{k}-path.png'))
        assert np.array_equal(still[0], gust_picture(par[k], rows, n - 1, 1, n, hit, 0, 64, 48)[0])
        # the wall: the pixel column at x = -0.36 (clear of the point and the goal) is floor inside the episode's band and cost colour outside it
        ys = (48 - 2 * np.arange(48) - 1) * (G.VIEW / 48)
        col = frames[0][:, 28]
        floor, costly = scene_twin.R.PALETTE[1], scene_twin.R.PALETTE[2]
        inside, outside = np.abs(ys) < par[k, 2] - 0.06, (np.abs(ys) > par[k, 2] + 0.06) & (np.abs(ys) < 1.9)
        assert (col[inside] == floor).all() and (col[outside] == costly).all() and inside.any() and outside.any()
        firsts.append(frames[0])
        # the same rows under another episode's parameters are another picture
        other = par[(k + 1) % K]
        assert not np.array_equal(frames[0], gust_picture(other, rows, 0, 1, 4, hit, 0, 64, 48)[0])
    assert not np.array_equal(firsts[0], firsts[1])

    env = envs.make('Gust-v0', num_envs=3, device=DEV, seed=4, band=(0.3, 0.9))
    env.reset()
    env.step(torch.full((3, 2), 0.7, device=DEV))
    state, rows = env.state.cpu().numpy(), env.params.cpu().numpy()
    for lane, camera in ((0, 'fixed'), (2, 'track')):
        img = env.render(lane=lane, width=64, height=48, camera_name=camera)
        want = gust_picture(rows[lane], state[lane:lane + 1], 0, 1, 0, None, int(camera == 'track'), 64, 48)[0]
        assert np.array_equal(img, want)
    from omnisafe_amd import render as render_mod
    with pytest.raises(ValueError, match='runtime parameters'):  # a scene of such a class names its row
        render_mod.rasterise(gust.render_kind('Gust-v0'), env.state, 0, G.STATE, 0, 1, 0, None, 0, 64, 48, 2)


# ------------------------------------------------------------------ 9. end to end
def _outcome(agent):
    ac = agent.agent._actor_critic  # noqa: SLF001
    torch.cuda.synchronize()
    lines = [ln for ln in open(os.path.join(agent.agent.logger.log_dir, 'progress.csv')).read().split('\n') if ln]
    hdr = lines[0].split(',')
    keep = [i for i, h in enumerate(hdr) if not h.startswith('Time/')]
    return ac.params.clone(), [[ln.split(',')[i] for i in keep] for ln in lines]


def test_agent_and_group_end_to_end(gust, tmp_path):
    """Agent('PPOLag', 'Gust-v0') with env_cfgs wind = (0, 0.5) for two short epochs: config.json carries the env_cfgs
    and Agent.evaluate() plays on them (and on an overlay).  An AgentGroup of two variants that differ only in wind runs
    on one library, and each member is bit for bit its solo Agent."""
    import omnisafe_amd

    N, H, T = 32, 16, 40

    def cfgs(log_dir, **env_cfgs):
        cfg = rollout_cfgs(log_dir, N, H, T, 2, env_cfgs=env_cfgs)
        cfg['logger_cfgs']['save_model_freq'] = 2
        return cfg

    agent = omnisafe_amd.Agent('PPOLag', 'Gust-v0', custom_cfgs=cfgs(str(tmp_path / 'one'), wind=(0.0, 0.5)))
    agent.learn()
    env = agent.agent._env._env
    np.testing.assert_array_equal(env.param_ranges.cpu().numpy(), G.ranges(wind=(0.0, 0.5)))
    assert len(np.unique(env.params[:, 0].cpu().numpy())) == N
    with open(os.path.join(agent.agent.logger.log_dir, 'config.json'), encoding='utf-8') as f:
        assert json.load(f)['env_cfgs'] == {'horizon': H, 'wind': [0.0, 0.5]}
    out = agent.evaluate(num_episodes=3)
    off = agent.evaluate(num_episodes=3, env_params={'wind': 0.9})
    assert len(out) >= 1 and out.keys() == off.keys()
    for name, (rewards, costs) in out.items():
        assert len(rewards) == len(costs) == 3 and np.isfinite(rewards).all()
        assert off[name][0] != rewards  # another wind, other episodes

    winds = (0.1, 0.4)
    solos = []
    for i, wind in enumerate(winds):
        solo = omnisafe_amd.Agent('PPOLag', 'Gust-v0', custom_cfgs=cfgs(str(tmp_path / f'solo{i}'), wind=wind))
        solo.learn()
        solos.append(_outcome(solo))
    group = omnisafe_amd.AgentGroup('PPOLag', 'Gust-v0', variants=[{'env_cfgs': {'wind': w}} for w in winds],
                                    custom_cfgs=cfgs(str(tmp_path / 'group')))
    classes = {type(m.agent._env._env) for m in group.agents}
    assert classes == {gust} and len({c.lib_path for c in classes}) == 1  # one class, one library
    assert len(group.learn()) == 2
    for member, wind, (s_params, s_rows) in zip(group.agents, winds, solos):
        g_params, g_rows = _outcome(member)
        assert torch.equal(g_params, s_params) and g_rows == s_rows
        assert bool((member.agent._env._env.params[:, 0] == np.float32(wind)).all())
    assert not torch.equal(solos[0][0], solos[1][0])
    assert len(group.evaluate(num_episodes=2, env_params={'wind': 0.3})) == 2
