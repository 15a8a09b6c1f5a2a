"""CPU: the SynthNavCarGoal{0,1,2}-v0 and SynthNavCarCircle{0,1,2}-v0 ids are registered and their two entry points are
part of the C ABI; the numpy twin of the Car (tests/car_twin.py, which tests/test_car_env_gpu.py compares the device
with bit for bit) does what the specification says: known answers operation by operation, equality with the
already-pinned point twins under equal wheel commands, every branch of a transition on states written here, the lidar
on car states, and a sanity check that the task can be driven."""
import os
import re

import numpy as np
import pytest
import torch

import car_twin as T
import circle_twin
import nav_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GOAL_IDS = ('SynthNavCarGoal0-v0', 'SynthNavCarGoal1-v0', 'SynthNavCarGoal2-v0')
CIRCLE_IDS = ('SynthNavCarCircle0-v0', 'SynthNavCarCircle1-v0', 'SynthNavCarCircle2-v0')


def goal_state(p=(0, 0), u=(1, 0), g=(1.2, 1.2), w=(0, 0), n=1):
    """A CarGoal state row without objects (they are added by the caller), f consistent with the wheels."""
    s = np.zeros((n, 64), np.float32)
    s[:, 0:2], s[:, 2:4], s[:, 8:10], s[:, 10:12] = p, u, g, w
    s[:, 4] = (F(0.5) * (s[:, 10] + s[:, 11]).astype(np.float32)).astype(np.float32)
    return s


def circle_state(p=(0, 0), u=(1, 0), w=(0, 0)):
    s = np.zeros((1, 12), np.float32)
    s[0, 0:2], s[0, 2:4], s[0, 10:12] = p, u, w
    s[0, 4] = F(F(0.5) * F(s[0, 10] + s[0, 11]))
    return s


def gstep(s, a, level=0, seed=1, pos=1):
    return T.car_goal_step(s, np.asarray([a] * s.shape[0], np.float32), level, seed, pos)


# ------------------------------------------------------------------ registration (fails before the feature)
def test_ids_registered_and_entry_points_declared():
    from omnisafe_amd import _lib, envs

    ids = envs.support_envs()
    for level in range(3):
        assert GOAL_IDS[level] in ids and envs.CAR_GOAL_LEVELS[GOAL_IDS[level]] == level
        assert envs.ENV_REGISTRY[GOAL_IDS[level]] is envs.NavCarGoalVectorEnv
        assert CIRCLE_IDS[level] in ids and envs.CAR_CIRCLE_LEVELS[CIRCLE_IDS[level]] == level
        assert envs.ENV_REGISTRY[CIRCLE_IDS[level]] is envs.NavCarCircleVectorEnv
    assert envs.ENV_REGISTRY['SynthCarGoal1-v0'] is envs.SynthVectorEnv  # the noise env keeps its id
    src = open(os.path.join(ROOT, 'include', 'omnisafe_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in ('osa_car_goal_env_step', 'osa_car_circle_env_step'):
        assert name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES['osa_nav_env_step']  # the same argument list
        assert re.search(r'\bint\s+' + name + r'\s*\(', src)
    assert re.search(r'#define\s+OSA_EVAL_ENV_CARGOAL0\s+48\b', src)
    assert re.search(r'#define\s+OSA_EVAL_ENV_CARCIRCLE0\s+64\b', src)
    from omnisafe_amd import evaluator

    assert envs.NavCarGoalVectorEnv in evaluator.DEVICE_ENVS and envs.NavCarCircleVectorEnv in evaluator.DEVICE_ENVS


@pytest.mark.reference
@pytest.mark.skipif(torch.cuda.is_available(), reason='build-container wiring test')
def test_plugin_makes_the_ids_valid_for_the_reference_agent(tmp_path, monkeypatch):
    """After omnisafe_amd.install() the reference's own env-id check (envs/core.py:362-386) knows the ids, and its
    Agent gets as far as this package's class, which refuses to run without a GPU."""
    import ref_harness

    omnisafe = ref_harness.import_reference()
    import omnisafe_amd
    from omnisafe.algorithms import registry as ref_registry
    from omnisafe.envs import core as ref_env_core

    keep = dict(ref_registry.REGISTRY._module_dict)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *_a, **_k: None)  # algo_wrapper.py:164 on a box without a GPU
    try:
        assert 'CPO' in omnisafe_amd.install()
        ids = ref_env_core.ENV_REGISTRY.support_envs()
        assert set(GOAL_IDS) | set(CIRCLE_IDS) <= set(ids)
        cfg = {'train_cfgs': {'device': 'cuda:0', 'total_steps': 2000, 'vector_env_nums': 4},
               'algo_cfgs': {'steps_per_epoch': 1000},
               'logger_cfgs': {'use_wandb': False, 'use_tensorboard': False, 'log_dir': str(tmp_path)}}
        for env_id in (GOAL_IDS[1], CIRCLE_IDS[1]):
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                omnisafe.Agent('CPO', env_id, custom_cfgs=cfg)
    finally:
        omnisafe_amd.uninstall()
        ref_registry.REGISTRY._module_dict.clear()
        ref_registry.REGISTRY._module_dict.update(keep)


# ------------------------------------------------------------------ known answers, operation by operation
def test_equal_wheels_from_rest_drive_straight():
    s1, r, c, reached = gstep(goal_state(p=(0, 0), u=(0.6, 0.8)), (1.0, 1.0))
    w = F(F(F(0.9) * F(0)) + F(F(0.02) * F(1)))
    assert w == F(0.02) and s1[0, 10] == w and s1[0, 11] == w
    assert s1[0, 4] == F(0.02) and s1[0, 5] == 0 and s1[0, 6] == 0 and s1[0, 7] == 0
    nrm = np.sqrt(F(F(F(0.6) * F(0.6)) + F(F(0.8) * F(0.8))), dtype=np.float32)
    u2 = (F(F(0.6) / nrm), F(F(0.8) / nrm))
    assert tuple(s1[0, 2:4]) == u2
    assert tuple(s1[0, 0:2]) == (F(F(0.02) * u2[0]), F(F(0.02) * u2[1]))
    assert c[0] == 0 and not reached[0]
    d0 = nav_twin.dist(np.zeros((1, 2), np.float32), np.full((1, 2), 1.2, np.float32))
    assert r[0] == F(d0[0] - nav_twin.dist(s1[:, 0:2], s1[:, 8:10])[0]) and r[0] > 0


def test_opposite_wheels_from_rest_turn_on_the_spot():
    s0 = goal_state(p=(0.3, -0.7), u=(1, 0))
    s1, r, _, _ = gstep(s0, (-1.0, 1.0))
    assert s1[0, 10] == F(-0.02) and s1[0, 11] == F(0.02)
    assert s1[0, 4] == 0 and np.array_equal(s1[0, 0:2], s0[0, 0:2])  # f == 0 exactly: the position to the bit
    t = F(F(0.375) * F(F(0.02) - F(-0.02)))
    assert s1[0, 6] == t and t == F(F(0.375) * F(0.04)) and s1[0, 7] == 0
    tt = F(t * t)
    den = F(F(1) + tt)
    cs, sn = F(F(F(1) - tt) / den), F(F(F(2) * t) / den)
    nrm = np.sqrt(F(F(cs * cs) + F(sn * sn)), dtype=np.float32)
    assert tuple(s1[0, 2:4]) == (F(cs / nrm), F(sn / nrm)) and s1[0, 3] > 0  # counter-clockwise
    assert r[0] == 0
    # the mirrored command turns the other way
    s2 = gstep(s0, (1.0, -1.0))[0]
    assert s2[0, 6] == -t and s2[0, 3] == -s1[0, 3] and s2[0, 2] == s1[0, 2]


def test_the_action_is_clamped_first():
    s0 = goal_state(p=(0.1, 0.2), u=(0.6, 0.8), w=(0.05, -0.03))
    a, b = gstep(s0, (7.5, -9.0)), gstep(s0, (1.0, -1.0))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c0 = circle_state(p=(0.1, 0.2), u=(0.6, 0.8), w=(0.05, -0.03))
    for x, y in zip(T.car_circle_step(c0, np.asarray([[7.5, -9.0]], np.float32), 2),
                    T.car_circle_step(c0, np.asarray([[1.0, -1.0]], np.float32), 2)):
        assert np.array_equal(x, y)


def test_sensor_columns_after_two_steps():
    s1 = gstep(goal_state(u=(1, 0)), (1.0, 0.5))[0]
    s2 = gstep(s1, (-0.25, 1.0))[0]
    wl1, wr1 = F(F(0.02) * F(1)), F(F(0.02) * F(0.5))
    wl2 = F(F(F(0.9) * wl1) + F(F(0.02) * F(-0.25)))
    wr2 = F(F(F(0.9) * wr1) + F(F(0.02) * F(1)))
    f1, f2 = F(F(0.5) * F(wl1 + wr1)), F(F(0.5) * F(wl2 + wr2))
    t1, t2 = F(F(0.375) * F(wr1 - wl1)), F(F(0.375) * F(wr2 - wl2))
    assert (s2[0, 4], s2[0, 5], s2[0, 6], s2[0, 7], s2[0, 10], s2[0, 11]) == (f2, f1, t2, t1, wl2, wr2)
    for o in (T.car_goal_obs(s2, 0), T.car_circle_obs(s2[:, :12])):
        assert o.dtype == np.float32
        assert o[0, 0] == f2 and o[0, 1] == F(f2 - f1) and o[0, 2] == t2
        assert tuple(o[0, 3:5]) == tuple(s2[0, 2:4]) and o[0, 5] == wl2 and o[0, 6] == wr2
        assert o[0, 7] == F(t2 - t1) and o[0, 1] != 0 and o[0, 7] != 0
        assert not o[0, 8:24].any()
    assert T.car_goal_obs(s2, 0).shape == (1, 72) and T.car_circle_obs(s2[:, :12]).shape == (1, 40)
    wide = T.car_goal_obs(s2, 0, 80)
    assert wide.shape == (1, 80) and np.array_equal(wide[:, :72], T.car_goal_obs(s2, 0)) and not wide[:, 72:].any()


# ------------------------------------------------------------------ pinned to the point twins
@pytest.mark.parametrize('level', [0, 1, 2])
def test_equal_wheel_commands_are_the_point_robot_going_straight(level):
    """Under (a, a): w_l = w_r = w follows the point's f <- 0.9 f + 0.02 a, 0.5 (w + w) = w exactly, and t = 0 makes
    the rotation the identity -- position, heading, f, reward, cost and goal equal nav_twin under (a, 0) bit for bit,
    50 steps with resamplings, N = 64."""
    N, seed = 64, 17 + level
    car = T.car_goal_reset(seed, 0, N, level)
    pt = nav_twin.nav_reset(seed, 0, N, level)
    assert np.array_equal(car, pt)  # the same arena from the same seed
    rng = np.random.default_rng(level)
    n_reached = n_cost = 0
    for t in range(1, 51):
        a = (rng.standard_normal(N) * 1.5).astype(np.float32)
        car, r, c, reached = T.car_goal_step(car, np.stack([a, a], 1), level, seed, t)
        pt, r_p, c_p, reached_p = nav_twin.nav_step(pt, np.stack([a, np.zeros_like(a)], 1), level, seed, t)
        for cols in (slice(0, 7), slice(8, 10), slice(12, 64)):
            assert np.array_equal(car[:, cols], pt[:, cols]), (t, cols)
        assert np.array_equal(car[:, 10], car[:, 4]) and np.array_equal(car[:, 11], car[:, 4])
        assert not car[:, 6].any() and not car[:, 7].any()
        assert np.array_equal(r, r_p) and np.array_equal(c, c_p) and np.array_equal(reached, reached_p)
        assert np.array_equal(T.car_goal_obs(car, level)[:, 24:], nav_twin.nav_obs(pt, level)[:, 12:])
        n_reached += int(reached.sum())
        n_cost += int(c.sum())
    assert (n_cost > 0) == (level > 0)
    print(f'level {level}: goals {n_reached}, cost steps {n_cost}')


@pytest.mark.parametrize('level', [0, 1, 2])
def test_equal_wheel_commands_on_the_circle_task(level):
    N, seed = 64, 5
    car = T.car_circle_reset(seed, 0, N)
    pt = circle_twin.circle_reset(seed, 0, N)
    assert np.array_equal(car[:, :8], pt) and not car[:, 8:].any()
    rng = np.random.default_rng(level)
    for t in range(50):
        a = (rng.standard_normal(N) * 1.5).astype(np.float32)
        car, r, c = T.car_circle_step(car, np.stack([a, a], 1), level)
        pt, r_p, c_p = circle_twin.circle_step(pt, np.stack([a, np.zeros_like(a)], 1), level)
        assert np.array_equal(car[:, :8], pt) and np.array_equal(r, r_p) and np.array_equal(c, c_p), t
        assert np.array_equal(T.car_circle_obs(car)[:, 24:], circle_twin.circle_obs(pt)[:, 12:])


# ------------------------------------------------------------------ every branch, on states written here
def test_goal_reached_and_resampled():
    for level in (0, 1, 2):
        s0 = goal_state(p=(0, 0), u=(1, 0), g=(0.45, 0), w=(0.2, 0.2), n=4)
        s0[1:, 8:10] = (1.2, 1.2)  # only env 0 is near its goal
        s1, r, c, reached = gstep(s0, (1.0, 1.0), level, seed=3, pos=9)
        f1 = F(F(F(0.9) * F(0.2)) + F(0.02))
        assert s1[0, 4] == f1 and abs(float(f1) - 0.2) < 1e-7
        assert reached.tolist() == [True, False, False, False] and int(reached.sum()) == 1
        d0, d1 = F(0.45), F(F(0.45) - f1)
        assert d1 < F(0.3) and r[0] == F(F(d0 - d1) + F(1))
        cands = nav_twin.draws(3, 9, 4, 14, 8).reshape(4, 4, 2)
        assert tuple(s1[0, 8:10]) == tuple(cands[0, 0])  # no hazards in this state: the first candidate
        assert np.array_equal(s1[1:, 8:10], s0[1:, 8:10]) and (r[1:] < 1).all()
    # with a hazard on the first candidate the second one is taken
    s0 = goal_state(p=(0, 0), u=(1, 0), g=(0.45, 0), w=(0.2, 0.2))
    cands = nav_twin.draws(3, 9, 1, 14, 8).reshape(1, 4, 2)
    s0[0, 12:14] = cands[0, 0]
    s0[0, 14:28] = 1.9  # the other seven hazards of level 1 out of everybody's way
    assert nav_twin.dist(cands[:, 1], cands[:, 0])[0] >= nav_twin.KEEP
    s1, _, c, reached = gstep(s0, (1.0, 1.0), 1, seed=3, pos=9)
    assert reached[0] and tuple(s1[0, 8:10]) == tuple(cands[0, 1]) and c[0] == 0


def test_hazard_and_vase_costs_by_level():
    s0 = goal_state(p=(0, 0), u=(1, 0), w=(0.1, 0.1), n=3)
    f1 = F(F(F(0.9) * F(0.1)) + F(0.02))  # q = (0.11, 0)
    s0[:, 12:32] = 1.9
    s0[:, 32:52] = -1.9
    s0[0, 12:14] = (0.25, 0.0)           # env 0: a hazard at distance 0.14 of q
    s0[1, 32:34] = (0.18, 0.0)           # env 1: a vase at distance 0.07 of q
    s0[2, 12:14] = (F(f1) + F(0.25), 0)  # env 2: a hazard just out of reach
    cost = {level: gstep(s0, (1.0, 1.0), level)[2].tolist() for level in (0, 1, 2)}
    assert cost[0] == [0, 0, 0]          # level 0 has no objects, whatever the row holds
    assert cost[1] == [1, 0, 0]          # vases do not cost on level 1
    assert cost[2] == [1, 1, 0]
    assert sum(cost[1]) == 1 and sum(cost[2]) == 2


def test_wall_clip():
    s1 = gstep(goal_state(p=(1.99, -1.0), u=(1, 0), w=(0.5, 0.5)), (1.0, 1.0))[0]
    f1 = F(F(F(0.9) * F(0.5)) + F(0.02))
    assert s1[0, 4] == f1 and F(F(1.99) + f1) > 2 and tuple(s1[0, 0:2]) == (2.0, -1.0)
    c1 = T.car_circle_step(circle_state(p=(0.0, -1.95), u=(0, -1), w=(0.5, 0.5)), np.ones((1, 2), np.float32), 0)[0]
    assert tuple(c1[0, 0:2]) == (0.0, -2.0)
    assert int((np.abs(s1[0, 0:2]) == 2).sum()) + int((np.abs(c1[0, 0:2]) == 2).sum()) == 2


def test_corridor_costs_by_level():
    def cost(p, u, level):
        return float(T.car_circle_step(circle_state(p=p, u=u, w=(0.2, 0.2)), np.ones((1, 2), np.float32), level)[2][0])

    assert [cost((0.74, 0), (1, 0), level) for level in (0, 1, 2)] == [0, 1, 1]   # q = (0.94, 0)
    assert [cost((0, 0.74), (0, 1), level) for level in (0, 1, 2)] == [0, 0, 1]
    assert [cost((-0.74, 0), (-1, 0), level) for level in (0, 1, 2)] == [0, 1, 1]
    assert [cost((0, -0.74), (0, -1), level) for level in (0, 1, 2)] == [0, 0, 1]
    # and the reward is circle_twin's expression of the attempted displacement
    s1, r, _ = T.car_circle_step(circle_state(p=(1, 0), u=(0, 1)), np.ones((1, 2), np.float32), 0)
    p1, r_p, _ = circle_twin.circle_step(np.asarray([[1, 0, 0, 1, 0, 0, 0, 0]], np.float32),
                                         np.asarray([[1, 0]], np.float32), 0)
    assert tuple(s1[0, 0:2]) == (1.0, F(0.02)) and r[0] == r_p[0] and r[0] > 0


# ------------------------------------------------------------------ lidar on car states
def test_every_object_falls_in_exactly_one_lidar_bin():
    N, level = 512, 2
    env = T.CarGoalTwin(level, N, 1000, 4)
    env.reset()
    rng = np.random.default_rng(1)
    for _ in range(30):  # turning and driving: headings off the reset's, wheel speeds apart
        env.step((rng.standard_normal((N, 2)) * 1.5).astype(np.float32))
    s = env.state
    assert (s[:, 10] != s[:, 11]).all() and s[:, 6].any()
    p, u = s[:, 0:2], s[:, 2:4]
    for objs in (s[:, 8:10].reshape(N, 1, 2), s[:, 12:32].reshape(N, 10, 2), s[:, 32:52].reshape(N, 10, 2)):
        assert (nav_twin.lidar_bins(p, u, objs) == 1).all()
    o = T.car_goal_obs(s, level)
    assert ((o[:, 24:40] > 0).sum(1) <= 1).all() and o[:, 64:72].any() and o[:, 40:56].any()
    lvl1 = T.car_goal_obs(T.car_goal_reset(4, 0, N, 1), 1)
    assert ((lvl1[:, 56:72] > 0).sum(1) <= 1).all()  # one vase


# ------------------------------------------------------------------ vector twins
def test_vector_twins_truncate_and_reset_together():
    a = np.asarray([[1.0, 0.25]] * 8, np.float32)
    env = T.CarGoalTwin(1, 8, horizon=3, seed=9)
    assert np.array_equal(env.reset(), T.car_goal_obs(nav_twin.nav_reset(9, 0, 8, 1), 1))
    for t in range(1, 7):
        before = env.state
        o, r, c, trunc, final, _ = env.step(a)
        assert trunc == (t % 3 == 0) and (final is not None) == trunc
        if trunc:
            assert np.array_equal(final, T.car_goal_obs(T.car_goal_step(before, a, 1, 9, t)[0], 1))
            assert np.array_equal(env.state, T.car_goal_reset(9, t, 8, 1)) and not env.state[:, 10:12].any()
        else:
            assert np.array_equal(env.state, T.car_goal_step(before, a, 1, 9, t)[0])
        assert np.array_equal(o, T.car_goal_obs(env.state, 1))
    env = T.CarCircleTwin(2, 8, horizon=3, seed=9)
    assert np.array_equal(env.reset()[:, 24:], circle_twin.circle_obs(circle_twin.circle_reset(9, 0, 8))[:, 12:])
    for t in range(1, 7):
        before = env.state
        o, r, c, trunc, final = env.step(a)
        assert trunc == (t % 3 == 0) and (final is not None) == trunc
        if trunc:
            assert np.array_equal(final, T.car_circle_obs(T.car_circle_step(before, a, 2)[0]))
            assert np.array_equal(env.state, T.car_circle_reset(9, t, 8)) and not env.state[:, 4:].any()
        else:
            assert np.array_equal(env.state, T.car_circle_step(before, a, 2)[0])
        assert np.array_equal(o, T.car_circle_obs(env.state))


# ------------------------------------------------------------------ task sanity
def steer_to_goal(s):
    """Wheel commands from the state: turn towards the goal's body-frame bearing, drive when roughly facing it."""
    r = s[:, 8:10] - s[:, 0:2]
    u = s[:, 2:4]
    bearing = np.arctan2(u[:, 0] * r[:, 1] - u[:, 1] * r[:, 0], u[:, 0] * r[:, 0] + u[:, 1] * r[:, 1])
    turn = np.clip(2.0 * bearing, -1, 1)
    fwd = np.where(np.abs(bearing) < 0.6, 1.0, 0.0)
    return np.stack([fwd - turn, fwd + turn], 1).astype(np.float32)


def test_the_task_can_be_driven():
    """256 envs, level 1, horizon 200, seed 123.  On the twin the controller above returns 13.17 (standard error 0.12
    over the envs) and N(0, 1) wheel commands -0.08 (0.05): the gap, 13.25, is a hundred of its standard errors.  The
    bound is half of that gap."""
    def play(policy):
        env = T.CarGoalTwin(1, 256, 200, 123)
        env.reset()
        ret, cost = np.zeros(256), np.zeros(256)
        for _ in range(200):
            _, r, c, *_ = env.step(policy(env.state))
            ret += r
            cost += c
        return ret, cost

    rng = np.random.default_rng(0)
    ret_c, cost_c = play(steer_to_goal)
    ret_n, cost_n = play(lambda s: rng.standard_normal((s.shape[0], 2)).astype(np.float32))
    msg = (f'controller EpRet {ret_c.mean():.3f} EpCost {cost_c.mean():.2f}; '
           f'N(0, 1) EpRet {ret_n.mean():.3f} EpCost {cost_n.mean():.2f}')
    print(msg)
    assert ret_c.mean() - ret_n.mean() > 6.6, msg
