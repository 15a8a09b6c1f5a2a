"""GPU: device envs that end their own episodes (the optional terminal() member of include/omnisafe_amd_env.h).  The
example env tests/custom_envs/ledge.h against its numpy twin (tests/ledge_twin.py) in the generic per-step kernel at
every lane count, then through the layers: the host protocol of a terminating class, the captured rollout graph and
its bootstrap values, the evaluator's two paths, Agent and AgentGroup.  Every comparison is bit for bit."""
import os

import numpy as np
import pytest
import torch

import ledge_twin as L
import raw_env

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HERE = os.path.dirname(os.path.abspath(__file__))
LEDGE = os.path.join(HERE, 'custom_envs', 'ledge.h')
SENTINEL = raw_env.SENTINEL


@pytest.fixture
def register():
    """register_device_env of a struct of ledge.h that unregisters at the end of the test."""
    import omnisafe_amd

    entered = []

    def enter(struct, ids, **kwargs):
        cls = omnisafe_amd.register_device_env(LEDGE, struct, ids, **kwargs)
        entered.extend(ids)
        return cls

    yield enter
    omnisafe_amd.unregister_device_env(*[e for e in entered if e in omnisafe_amd.custom_envs()])


@pytest.fixture
def ledge(register):
    return register('Ledge', {'Ledge0-v0': 0, 'Ledge1-v0': 1}, default_horizon=40)


def raw_ledge(cls, level, N, obs_dim, ld, horizon, seed):
    env = raw_env.RawEnv('osa_nav_env_step', L.STATE, level, N, obs_dim, ld, horizon, seed)
    env.fn = cls.library().osa_custom_env_step  # (the same argument list)
    return env


def near_the_edges(N):
    """State rows of the caller's own for the small env counts, where random play from a reset rarely falls: env 0
    one step from the upper edge (v_y' >= 0.18 - 0.05 - 0.04, so p_y' >= 1.04), the last env (N > 1) one step from the
    lower edge; an env between them keeps its reset row."""
    rows = {0: [0.25, 0.95, 0.1, 0.2, 0, 0]}
    if N > 1:
        rows[N - 1] = [0.5, -0.95, 0.05, -0.2, 0, 0]
    return {n: np.array(r, np.float32) for n, r in rows.items()}


# ------------------------------------------------------------------ 1. the per-step kernel against the twin
@pytest.mark.parametrize('level', [0, 1])
@pytest.mark.parametrize('N', [1, 3, 130])
def test_ledge_trace_equals_the_twin_at_every_lane_count(register, level, N):
    """48 steps at horizon 12 under actions uniform in [-1.5, 1.5], N = 1 (a lone env), 3 (an odd count: one workgroup
    at 16 lanes, two at 32) and 130 (past one workgroup at every LANES), at obs_dim = 20 in rows of 20 and at obs_dim 23
    in rows of 28 (zero columns, sentinels behind): everything the launch writes equals the twin at every step -- state,
    observation, reward, cost, both flags, the per-env step counters -- the final_obs rows of the truncating envs hold
    the pre-reset observation and every other row of final_obs still holds the sentinel.  The libraries built at 16, 32
    and 64 lanes per env write the same bits.  N = 130 plays the trace whose mix of ends test_ledge_twin.py
    establishes (workgroups with a terminating, a truncating and a continuing env on one step); N = 1 and 3 start from
    rows next to the edges."""
    H, seed, steps = L.TRACE_HORIZON, L.TRACE_SEED, L.TRACE_STEPS
    classes = {lanes: register(struct, [f'Ledge-lanes{lanes}-v0'])
               for lanes, struct in ((32, 'Ledge'), (16, 'Ledge16'), (64, 'Ledge64'))}
    assert {lanes: cls.lanes for lanes, cls in classes.items()} == {16: 16, 32: 32, 64: 64}
    assert all(cls.terminates for cls in classes.values()) and len({cls.lib_path for cls in classes.values()}) == 3
    acts = L.trace_actions(N, steps)
    for obs_dim, ld in ((L.OBS, L.OBS), (23, 28)):
        envs_ = {lanes: raw_ledge(cls, level, N, obs_dim, ld, H, seed) for lanes, cls in classes.items()}
        twin = L.LedgeTwin(level, N, H, seed)
        o_exp = twin.reset()
        for env in envs_.values():
            assert env.launch(0, None, 1) == 0  # reset from the seed alone
            np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state)
            np.testing.assert_array_equal(env.obs[:N, :L.OBS].cpu().numpy(), o_exp)
            assert not env.obs[:N, L.OBS:obs_dim].any() and int(env.steps[:N].abs().sum()) == 0
            assert bool((env.final == SENTINEL).all()) and bool((env.reward == SENTINEL).all())
            assert bool((env.term == 9).all()) and bool((env.trunc == 9).all())  # a reset writes no flags
        if N < 130:
            for n, row in near_the_edges(N).items():
                twin.state[n] = row
                for env in envs_.values():
                    env.state[n] = torch.from_numpy(row).to(DEV)
        n_term = n_trunc = n_cost = mixed4 = mixed2 = 0
        tail_nonzero = False
        for t in range(steps):
            act = torch.from_numpy(acts[t])
            o_exp, r_exp, c_exp, term, trunc, final = twin.step(acts[t])
            assert not (term & trunc).any()
            for lanes, env in envs_.items():
                where = f'{lanes} lanes, obs_dim {obs_dim}, step {t}'
                assert env.launch(t + 1, act.to(DEV), 0) == 0
                np.testing.assert_array_equal(env.term[:N].cpu().numpy(), term.astype(np.uint8), err_msg=where)
                np.testing.assert_array_equal(env.trunc[:N].cpu().numpy(), trunc.astype(np.uint8), err_msg=where)
                np.testing.assert_array_equal(env.steps[:N].cpu().numpy(), twin.steps, err_msg=where)
                np.testing.assert_array_equal(env.reward[:N].cpu().numpy(), r_exp, err_msg=where)
                np.testing.assert_array_equal(env.cost[:N].cpu().numpy(), c_exp, err_msg=where)
                np.testing.assert_array_equal(env.state[:N].cpu().numpy(), twin.state, err_msg=where)
                np.testing.assert_array_equal(env.obs[:N, :L.OBS].cpu().numpy(), o_exp, err_msg=where)
                assert not env.obs[:N, L.OBS:obs_dim].any(), where
                got_final = env.final[:N].cpu().numpy()
                np.testing.assert_array_equal(got_final[trunc, :L.OBS], final[trunc], err_msg=where)
                assert not got_final[trunc, L.OBS:obs_dim].any(), where
                # terminating and continuing envs: no final observation is written
                assert (got_final[~trunc] == SENTINEL).all(), where
                assert env.pads_untouched(), where
                if trunc.any():
                    env.final.fill_(SENTINEL)
            n_term, n_trunc, n_cost = n_term + int(term.sum()), n_trunc + int(trunc.sum()), n_cost + int(c_exp.sum())
            mixed4 += L.mixed_groups(term, trunc, 4)
            mixed2 += L.mixed_groups(term, trunc, 2)
            tail_nonzero = tail_nonzero or bool((o_exp[:, 16:L.OBS] != 0).any(0).all())  # the second round at 16 lanes
        assert tail_nonzero and n_trunc >= 1
        assert n_term >= (40 if N == 130 else min(N, 2))
        if N == 130:
            assert n_trunc >= 150 and mixed4 >= 3 and mixed2 >= 3
        assert n_cost == 0 if level == 0 else n_cost > 0
    print(f'level {level} N {N}: terminations {n_term}, truncations {n_trunc}, cost steps {n_cost}, mixed workgroups '
          f'{mixed4} / {mixed2}')


def test_ledge_endless_equals_ledge_wherever_ledge_does_not_terminate(register):
    """The same description without terminal(), from the same caller-written rows (130 envs all over the ledge, at
    speed, some about to fall or to arrive) at the same stream position: one step agrees bit for bit in reward and cost
    everywhere (it is the same transition) and in state and observation wherever Ledge does not terminate;
    LedgeEndless never sets `terminated`, walks on where Ledge resets, and truncates by the counter alone."""
    N, seed, H, pos = 130, 4, 9, 5
    ledge, endless = register('Ledge', ['LedgeA-v0']), register('LedgeEndless', ['LedgeB-v0'])
    assert ledge.terminates is True and endless.terminates is False
    rng = np.random.default_rng(0)
    s = np.zeros((N, L.STATE), np.float32)
    s[:, 0] = rng.uniform(0, 3, N)
    s[:, 1] = rng.uniform(-0.98, 0.98, N)
    s[:, 2] = rng.uniform(0, 0.4, N)
    s[:, 3] = rng.uniform(-0.3, 0.3, N)
    s[:, 4] = rng.integers(0, 5, N)
    s[8], s[17] = [0.5, 0.95, 0.1, 0.2, 2, 0], [2.9, 0.0, 0.3, 0.0, 3, 0]  # their time limit is due as they end (below)
    act = rng.uniform(-1.5, 1.5, (N, 2)).astype(np.float32)
    for level in (0, 1):
        s_exp, r_exp, c_exp = L.ledge_step(s, act, level, seed, pos)
        term = L.ledge_terminal(s_exp)
        assert 10 < term.sum() < N - 10 and (s_exp[:, 0] > 3).sum() > 3 and (np.abs(s_exp[:, 1]) > 1).sum() > 3
        out = {}
        for name, cls in (('ledge', ledge), ('endless', endless)):
            env = raw_ledge(cls, level, N, L.OBS, L.OBS, H, seed)
            assert env.launch(0, None, 1) == 0
            env.state[:N] = torch.from_numpy(s).to(DEV)
            env.steps[:N] = torch.arange(N, dtype=torch.int32, device=DEV) % H  # counts H - 1: the time limit is due
            assert env.launch(pos, torch.from_numpy(act).to(DEV), 0) == 0
            assert env.pads_untouched()
            out[name] = {k: getattr(env, k)[:N].cpu().numpy() for k in ('state', 'obs', 'reward', 'cost', 'term',
                                                                        'trunc', 'steps', 'final')}
        a, b = out['ledge'], out['endless']
        due = (np.arange(N) % H) == H - 1
        assert (due & term).any() and (due & ~term).any()
        for got in (a, b):
            np.testing.assert_array_equal(got['reward'], r_exp)
            np.testing.assert_array_equal(got['cost'], c_exp)
        np.testing.assert_array_equal(a['term'], term.astype(np.uint8))
        np.testing.assert_array_equal(a['trunc'], (due & ~term).astype(np.uint8))  # termination wins
        assert not b['term'].any()
        np.testing.assert_array_equal(b['trunc'], due.astype(np.uint8))
        keep = ~term & ~due
        np.testing.assert_array_equal(a['state'][keep], b['state'][keep])
        np.testing.assert_array_equal(a['state'][keep], s_exp[keep])
        np.testing.assert_array_equal(a['obs'][keep], b['obs'][keep])
        fresh = L.ledge_reset(seed, pos, N)
        np.testing.assert_array_equal(a['state'][term | due], fresh[term | due])
        np.testing.assert_array_equal(b['state'][due], fresh[due])
        np.testing.assert_array_equal(b['state'][~due], s_exp[~due])  # walks on, off the ledge and past the end
        np.testing.assert_array_equal(a['steps'], np.where(term | due, 0, np.arange(N) % H + 1))
        np.testing.assert_array_equal(b['steps'], np.where(due, 0, np.arange(N) % H + 1))
        np.testing.assert_array_equal(b['final'][due], L.ledge_obs(s_exp)[due])
        np.testing.assert_array_equal(a['final'][due & ~term], L.ledge_obs(s_exp)[due & ~term])
        assert (a['final'][term | ~due] == SENTINEL).all() and (b['final'][~due] == SENTINEL).all()


# ------------------------------------------------------------------ 2. the host protocol of a terminating class
def test_host_protocol_hands_out_final_observations_from_the_horizon_on(ledge, register):
    """make('Ledge1-v0', num_envs=130, horizon=12), 30 steps: no env can truncate before step 12 after the common
    reset, and from there on any step may, so info carries final_observation on exactly the steps with
    _since_reset >= 12, under a mask that is the device's `truncated`.  A reset starts the count again.  Flags,
    counters and the masked final rows equal the twin."""
    from omnisafe_amd import envs

    N, H, seed = 130, 12, L.TRACE_SEED
    env = envs.make('Ledge1-v0', num_envs=N, device=DEV, horizon=H, seed=seed)
    assert type(env) is ledge and env.terminates and env.graph_safe and env.max_episode_steps == H
    twin = L.LedgeTwin(1, N, H, seed)
    acts = L.trace_actions(N, 30 + 14)
    k = n_term = n_trunc = 0
    for steps in (30, 14):
        obs, info = env.reset()
        assert info == {}
        np.testing.assert_array_equal(obs.cpu().numpy(), twin.reset())
        for t in range(steps):
            obs, reward, cost, term, trunc, info = env.step(torch.from_numpy(acts[k]).to(DEV))
            o_exp, r_exp, c_exp, term_exp, trunc_exp, final = twin.step(acts[k])
            k += 1
            assert ('final_observation' in info) == ('_final_observation' in info) == (t + 1 >= H), (steps, t)
            np.testing.assert_array_equal(term.cpu().numpy(), term_exp.astype(np.uint8))
            np.testing.assert_array_equal(trunc.cpu().numpy(), trunc_exp.astype(np.uint8))
            if t + 1 < H:
                assert not trunc_exp.any()
            else:
                mask = info['_final_observation']
                assert torch.equal(mask, trunc) and mask.dtype == torch.uint8
                np.testing.assert_array_equal(info['final_observation'].cpu().numpy()[trunc_exp], final[trunc_exp])
            np.testing.assert_array_equal(obs.cpu().numpy(), o_exp)
            np.testing.assert_array_equal(reward.cpu().numpy(), r_exp)
            np.testing.assert_array_equal(cost.cpu().numpy(), c_exp)
            np.testing.assert_array_equal(env.state.cpu().numpy(), twin.state)
            np.testing.assert_array_equal(env._steps.cpu().numpy(), twin.steps)
            n_term, n_trunc = n_term + int(term_exp.sum()), n_trunc + int(trunc_exp.sum())
    assert n_term > 20 and n_trunc > 100
    # a class that does not terminate keeps the protocol it had: the truncating steps alone
    assert register('LedgeEndless', ['LedgeEndless-v0']).terminates is False
    other = envs.make('LedgeEndless-v0', num_envs=3, device=DEV, horizon=4, seed=seed)
    other.reset()
    act = torch.zeros(3, 2, device=DEV)
    seen = ['final_observation' in other.step(act)[5] for _ in range(9)]
    assert seen == [False, False, False, True, False, False, False, True, False]


# ------------------------------------------------------------------ 3. rollout: graph replay and bootstrap values
def rollout_cfgs(log_dir, n, horizon, steps, epochs, **algo):
    return {'seed': 7, 'train_cfgs': {'device': DEV, 'total_steps': epochs * n * steps, 'vector_env_nums': n},
            'algo_cfgs': dict({'steps_per_epoch': n * steps, 'update_iters': 2}, **algo),
            'logger_cfgs': {'log_dir': log_dir, 'verbose': False}, 'env_cfgs': {'horizon': horizon}}


def test_rollout_graph_replay_equals_eager_launches(ledge, tmp_path, monkeypatch):
    """OnPolicyAdapter.rollout on the terminating env (32 envs, 40 steps per env at horizon 16, so the final
    observations are handed out on 25 of the 40 steps) inside the captured hipGraph against eager launches: the buffers
    of every epoch are identical (four epochs: the graph is captured on the second and replayed for two more).  The
    logged episode length is below the horizon: some episodes end early."""
    import omnisafe_amd

    N, H, T = 32, 16, 40

    def run(graph):
        monkeypatch.setenv('OSA_ROLLOUT_GRAPH', '1' if graph else '0')
        cfg = rollout_cfgs(str(tmp_path / ('g' if graph else 'e')), N, H, T, 4)
        algo = omnisafe_amd.Agent('PPOLag', 'Ledge1-v0', custom_cfgs=cfg).agent
        assert algo._env._env.terminates and algo._env._env.graph_safe
        snaps, ep_len = [], []
        for _ in range(4):
            algo._env.rollout(steps_per_epoch=algo._steps_per_epoch, agent=algo._actor_critic, buffer=algo._buf,
                              logger=algo._logger)
            ep_len.append(float(algo._logger.get_stats('Metrics/EpLen')[0]))  # what dump_tabular() logs below
            snap = {k: v.clone() for k, v in algo._buf.data.items()}
            snap['env_state'] = algo._env._env.state.clone()
            snap['env_steps'] = algo._env._env._steps.clone()
            algo._update()
            snap['params'] = algo._actor_critic.params.clone()
            snaps.append(snap)
            algo._logger.dump_tabular()
        return algo, snaps, ep_len

    a_g, s_g, len_g = run(True)
    a_e, s_e, len_e = run(False)
    assert a_g._env.last_rollout_graphed is True and not getattr(a_e._env, 'last_rollout_graphed', False)
    for ep, (g, e) in enumerate(zip(s_g, s_e)):
        for k in g:
            assert torch.equal(g[k].cpu(), e[k].cpu()), (ep, k)
    assert s_g[0]['obs'].shape[-1] == L.OBS and s_g[0]['env_state'].shape == (N, L.STATE)
    assert not torch.equal(s_g[2]['obs'], s_g[3]['obs'])
    for snap in s_g:  # path ends inside the epoch, at steps that differ between the envs
        ends = snap['path_end'].reshape(T, N)[:-1].bool()
        assert ends.any() and bool((ends != ends[:, :1]).any())
    assert len_g == len_e and all(0 < v < H for v in len_g), len_g


def test_rollout_bootstraps_truncated_paths_only(ledge, tmp_path, monkeypatch):
    """The first epoch of a rollout (eager launches; no observation normaliser, so the rows the critic sees are the
    env's) with the env's actions and the critic's calls recorded: replayed through the twin, `path_end` is the twin's
    terminated | truncated (and the epoch's last step), `boot_r` / `boot_c` are 0 at terminated steps and the critic's
    values of the final observation -- the twin's pre-reset observation -- at truncated ones, and the env is never
    asked for a final observation before the horizon."""
    import omnisafe_amd

    N, H, T = 32, 16, 40
    monkeypatch.setenv('OSA_ROLLOUT_GRAPH', '0')
    cfg = rollout_cfgs(str(tmp_path), N, H, T, 1, obs_normalize=False)
    algo = omnisafe_amd.Agent('PPOLag', 'Ledge1-v0', custom_cfgs=cfg).agent
    env, ac = algo._env._env, algo._actor_critic
    acts, infos, critic_in = [], [], []
    step, values = env.step, ac.values

    def recording_step(action):
        acts.append(action.clone())
        out = step(action)
        infos.append('final_observation' in out[5])
        return out

    def recording_values(rows):
        critic_in.append(rows.clone())
        return values(rows)

    env.step, ac.values = recording_step, recording_values
    algo._env.rollout(steps_per_epoch=algo._steps_per_epoch, agent=ac, buffer=algo._buf, logger=algo._logger)
    env.step, ac.values = step, values
    torch.cuda.synchronize()
    assert len(acts) == T and infos == [t + 1 >= H for t in range(T)]
    assert len(critic_in) == sum(infos) + 1  # one call per final observation, one for the epoch's last observation
    b = {k: v.clone().reshape(T, N, *v.shape[2:]) if v.dim() > 1 else v.clone() for k, v in algo._buf.data.items()}
    twin = L.LedgeTwin(1, N, H, env._seed)
    twin.reset()
    n_term = n_trunc = 0
    call = 0
    for t in range(T):
        _, r_exp, c_exp, term, trunc, final = twin.step(acts[t].cpu().numpy())
        np.testing.assert_array_equal(b['reward'][t].cpu().numpy(), r_exp)
        np.testing.assert_array_equal(b['cost'][t].cpu().numpy(), c_exp)
        last = t == T - 1
        np.testing.assert_array_equal(b['path_end'][t].cpu().numpy() != 0, term | trunc | last)
        boot_r, boot_c = b['boot_r'][t].cpu().numpy(), b['boot_c'][t].cpu().numpy()
        assert not boot_r[term].any() and not boot_c[term].any()  # a terminated path has no bootstrap value
        if not last:
            assert not boot_r[~trunc].any() and not boot_c[~trunc].any()
        if infos[t]:
            rows = critic_in[call]
            call += 1
            np.testing.assert_array_equal(rows.cpu().numpy()[trunc], final[trunc])
            v_r, v_c = (v.clone().reshape(N).cpu().numpy() for v in ac.values(rows))
            np.testing.assert_array_equal(boot_r[trunc], v_r[trunc])
            np.testing.assert_array_equal(boot_c[trunc], v_c[trunc])
            if trunc.any():
                assert np.abs(v_r[trunc]).max() > 0
        else:
            assert not trunc.any()
        if last:  # the running paths are cut with the value of the next observation
            v_r, v_c = (v.clone().reshape(N).cpu().numpy() for v in ac.values(critic_in[-1]))
            run = ~term & ~trunc
            np.testing.assert_array_equal(critic_in[-1].cpu().numpy(), L.ledge_obs(twin.state))
            np.testing.assert_array_equal(boot_r[run], v_r[run])
            np.testing.assert_array_equal(boot_c[run], v_c[run])
        n_term, n_trunc = n_term + int(term.sum()), n_trunc + int(trunc.sum())
    np.testing.assert_array_equal(env.state.cpu().numpy(), twin.state)
    assert n_term >= 3 and n_trunc >= 20, (n_term, n_trunc)


# ------------------------------------------------------------------ 4. evaluator
def train_checkpoint(log_dir, horizon):
    """A 2-epoch PPOLag run on Ledge1-v0 (16 envs, [64, 64] actor, obs_normalize): (log_dir, its last checkpoint)."""
    import omnisafe_amd

    n = 16
    cfg = {'seed': 2, 'train_cfgs': {'device': DEV, 'total_steps': 2 * n * 2 * horizon, 'vector_env_nums': n},
           'algo_cfgs': {'steps_per_epoch': n * 2 * horizon},
           'logger_cfgs': {'log_dir': log_dir, 'verbose': False, 'save_model_freq': 1},
           'env_cfgs': {'horizon': horizon}}
    agent = omnisafe_amd.Agent('PPOLag', 'Ledge1-v0', custom_cfgs=cfg)
    assert agent.agent._cfgs.algo_cfgs.obs_normalize
    agent.learn()
    log_dir = agent.agent.logger.log_dir
    names = sorted(os.listdir(os.path.join(log_dir, 'torch_save')), key=lambda s: int(s[len('epoch-'):-len('.pt')]))
    return log_dir, names[-1]


def play(checkpoint, path, monkeypatch, K, seed):
    from omnisafe_amd.evaluator import Evaluator

    monkeypatch.setenv('OSA_EVAL_PATH', path)
    ev = Evaluator(seed=seed, device=DEV, verbose=False)
    ev.load_saved(*checkpoint)
    r, c = ev.evaluate(num_episodes=K, trace=True)
    return np.array(r), np.array(c), np.array(ev.episode_lengths), ev.trace.cpu().numpy(), ev


def test_evaluator_persistent_equals_per_step_and_replays_through_the_twin(ledge, tmp_path, monkeypatch):
    """K = 5: a quarter-filled wave; K = 33: two full waves and one episode of a third.  The persistent kernel ends an
    episode where the description's terminal() says so, the per-step path at the env's `terminated`: returns, costs,
    lengths and traces agree bit for bit, and replaying the traced actions through the twin gives the same lengths,
    states, rewards and costs.  Horizon 16 at seed 3: under a policy that does nothing 2 of the 33 episodes fall before
    the horizon (gusts alone), and no policy arrives behind x = 3 in fewer than 13 steps; of the 33 played here at least
    one ends early and at least one reaches the horizon."""
    H, seed = 16, 3
    checkpoint = train_checkpoint(str(tmp_path), H)
    in_w = L.OBS
    for K in (5, 33):
        a = play(checkpoint, 'persistent', monkeypatch, K, seed)
        b = play(checkpoint, 'per-step', monkeypatch, K, seed)
        assert a[4].path == 'persistent' and b[4].path == 'per-step'
        for x, y in zip(a[:4], b[:4]):
            assert x.shape == y.shape
            np.testing.assert_array_equal(x, y)
        ret, cost, length, tr, ev = a
        assert tr.shape == (H, K, in_w + 2 + 3 + L.TRACE) and (length >= 1).all() and (length <= H).all()
        x, act = tr[:, :, :L.OBS], tr[:, :, in_w:in_w + 2]
        rew, cst, alive, state = tr[:, :, in_w + 2], tr[:, :, in_w + 3], tr[:, :, in_w + 4], tr[:, :, in_w + 5:]
        mean, std = ev._normalizer._mean.cpu().numpy(), ev._normalizer._std.cpu().numpy()
        twin = L.LedgeTwin(1, K, H, seed)  # a replay of the traced actions
        o = twin.reset()
        live = np.ones(K, bool)
        twin_len = np.zeros(K, np.int64)
        for t in range(H):
            np.testing.assert_array_equal(alive[t], live.astype(np.float32))
            assert not tr[t, ~live].any()  # a finished episode leaves no record
            np.testing.assert_array_equal(state[t, live], twin.state[live, :L.TRACE])
            normed = np.clip(((o - mean).astype(np.float32) / std).astype(np.float32), -5, 5)
            np.testing.assert_array_equal(x[t, live], normed[live])
            before = twin.state.copy()
            o, _, _, term, trunc, _ = twin.step(act[t])
            _, r, c = L.ledge_step(before, act[t], 1, seed, t + 1)
            np.testing.assert_array_equal(rew[t, live], r[live])
            np.testing.assert_array_equal(cst[t, live], c[live])
            twin_len += live
            live = live & ~(term | trunc)
        assert not live.any()
        np.testing.assert_array_equal(length, twin_len)
        np.testing.assert_array_equal(ret, rew.astype(np.float64).cumsum(0)[-1])
        np.testing.assert_array_equal(cost, cst.astype(np.float64).sum(0))
        assert np.abs(act).max() > 0 and np.abs(rew).max() > 0
        print(f'K {K}: lengths {sorted(length.tolist())}')
        if K == 33:
            assert (length < H).any() and (length == H).any(), length
    monkeypatch.delenv('OSA_EVAL_PATH')
    from omnisafe_amd.evaluator import Evaluator

    ev = Evaluator(seed=seed, device=DEV, verbose=False)
    ev.load_saved(*checkpoint)
    ev.evaluate(num_episodes=2)
    assert ev.path == 'persistent'  # the default for a terminating custom env as well


# ------------------------------------------------------------------ 5. end to end
def _outcome(agent):
    ac = agent.agent._actor_critic  # noqa: SLF001
    torch.cuda.synchronize()
    lines = [ln for ln in open(os.path.join(agent.agent.logger.log_dir, 'progress.csv')).read().split('\n') if ln]
    hdr = lines[0].split(',')
    keep = [i for i, h in enumerate(hdr) if not h.startswith('Time/')]
    return ac.params.clone(), [[ln.split(',')[i] for i in keep] for ln in lines]


def test_agent_group_equals_the_solo_agents(ledge, tmp_path):
    """Agent('PPOLag', 'Ledge1-v0'): two epochs of 32 envs x 40 steps at horizon 16; the same configuration as member
    s of an AgentGroup of seeds [0, 1] equals the solo agent of seed s in parameters and in every column but Time/*.
    Episodes end at differing lengths: the logged mean length lies below the horizon."""
    import omnisafe_amd

    N, H, T = 32, 16, 40

    def cfgs(log_dir):
        cfg = rollout_cfgs(log_dir, N, H, T, 2)
        del cfg['seed']
        cfg['logger_cfgs']['save_model_freq'] = 1
        return cfg

    solos = []
    for seed in (0, 1):
        solo = omnisafe_amd.Agent('PPOLag', 'Ledge1-v0', custom_cfgs=dict(cfgs(str(tmp_path / f'solo{seed}')), seed=seed))
        solo.learn()
        solos.append(_outcome(solo))
        assert type(solo.agent._env._env) is ledge and solo.agent._env._env.level == 1
    params, rows = solos[0]
    assert torch.isfinite(params).all() and len(rows) == 3
    col = rows[0].index('Metrics/EpLen')
    assert all(0 < float(r[col]) < H for r in rows[1:]), [r[col] for r in rows[1:]]
    group = omnisafe_amd.AgentGroup('PPOLag', 'Ledge1-v0', seeds=[0, 1], custom_cfgs=cfgs(str(tmp_path / 'group')))
    assert len(group.learn()) == 2
    for member, (s_params, s_rows) in zip(group.agents, solos):
        g_params, g_rows = _outcome(member)
        assert torch.equal(g_params, s_params) and g_rows == s_rows
    assert not torch.equal(solos[0][0], solos[1][0])
    out = solo.evaluate(num_episodes=3)
    assert len(out) >= 2
    for rewards, costs in out.values():
        assert len(rewards) == len(costs) == 3 and np.isfinite(rewards).all()
