"""CPU: the SynthNavCircle{0,1,2}-v0 ids are registered and osa_circle_env_step is part of the C ABI; the numpy twin of
the env (tests/circle_twin.py, which tests/test_circle_env_gpu.py compares the device with bit for bit) does what the
specification says on hand-computed transitions, costs, resets and lidar readings."""
import os
import re

import numpy as np
import pytest
import torch

import circle_twin as T
import nav_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def make_state(p=(0, 0), u=(1, 0), f=0.0, f_prev=0.0):
    s = np.zeros((1, 8), np.float32)
    s[0, 0:2], s[0, 2:4], s[0, 4], s[0, 5] = p, u, f, f_prev
    return s


def step(s, a, level=0):
    return T.circle_step(s, np.asarray([a], np.float32), level)


def reward_of(m, q):
    """The specification's expression, operation by operation, on float32 scalars."""
    mx, my, qx, qy = F(m[0]), F(m[1]), F(q[0]), F(q[1])
    num = F(F(my * qx) - F(mx * qy))
    rad = np.sqrt(F(F(qx * qx) + F(qy * qy)), dtype=np.float32)
    dev = np.abs(F(rad - F(1)))
    return F(F(num / rad) / F(F(1) + dev)) if rad > 0 else F(0)


# ------------------------------------------------------------------ registration (fails before the feature)
def test_ids_registered_and_entry_point_declared():
    from omnisafe_amd import _lib, envs

    ids = envs.support_envs()
    for level, env_id in enumerate(('SynthNavCircle0-v0', 'SynthNavCircle1-v0', 'SynthNavCircle2-v0')):
        assert env_id in ids and envs.CIRCLE_LEVELS[env_id] == level
        assert envs.ENV_REGISTRY[env_id] is envs.NavCircleVectorEnv
    assert 'osa_circle_env_step' in _lib.SIGNATURES
    assert _lib.SIGNATURES['osa_circle_env_step'] == _lib.SIGNATURES['osa_nav_env_step']  # the same argument list
    src = open(os.path.join(ROOT, 'include', 'omnisafe_amd.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'\bint\s+osa_circle_env_step\s*\(', src)
    assert re.search(r'#define\s+OSA_EVAL_ENV_CIRCLE0\s+32\b', src)
    dev = open(os.path.join(ROOT, 'omnisafe_amd', 'csrc', 'env_device.h')).read()
    key = re.search(r'#define\s+OSA_CIRCLE_KEY\s+0x([0-9A-Fa-f]{16})ull', dev)
    assert key and int(key.group(1), 16) == T.CIRCLE_KEY
    others = {int(k, 16) for k in re.findall(r'0x([0-9A-Fa-f]{16})ull', dev)} - {T.CIRCLE_KEY}
    assert len(others) >= 3 and T.CIRCLE_KEY != nav_twin.NAV_KEY


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
        assert {'SynthNavCircle0-v0', 'SynthNavCircle1-v0', 'SynthNavCircle2-v0'} <= set(ids)
        cfg = {'train_cfgs': {'device': 'cuda:0', 'total_steps': 2000, 'vector_env_nums': 4},
               'algo_cfgs': {'steps_per_epoch': 1000},
               'logger_cfgs': {'use_wandb': False, 'use_tensorboard': False, 'log_dir': str(tmp_path)}}
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            omnisafe.Agent('CPO', 'SynthNavCircle1-v0', custom_cfgs=cfg)
    finally:
        omnisafe_amd.uninstall()
        ref_registry.REGISTRY._module_dict.clear()
        ref_registry.REGISTRY._module_dict.update(keep)


# ------------------------------------------------------------------ known-answer rewards
def test_tangential_move_counter_clockwise_pays():
    s1, r, c = step(make_state(p=(1, 0), u=(0, 1)), (1.0, 0.0))
    f1 = F(0.02)
    assert s1[0, 4] == f1 and s1[0, 5] == 0 and s1[0, 6] == 0
    assert tuple(s1[0, 2:4]) == (0.0, 1.0) and tuple(s1[0, 0:2]) == (1.0, f1) and s1[0, 7] == 0
    assert r[0] == reward_of((0, f1), (1, f1)) and r[0] > 0
    assert abs(float(r[0]) - 0.02 / np.sqrt(1.0004) / (np.sqrt(1.0004))) < 1e-7
    assert c[0] == 0
    # the action is clamped to [-1, 1] first
    s2, r2, _ = step(make_state(p=(1, 0), u=(0, 1)), (7.5, 0.0))
    assert np.array_equal(s1, s2) and r2[0] == r[0]


def test_tangential_move_clockwise_is_charged_the_same():
    _, r, _ = step(make_state(p=(1, 0), u=(0, 1)), (1.0, 0.0))
    s1, rn, _ = step(make_state(p=(1, 0), u=(0, -1)), (1.0, 0.0))
    assert tuple(s1[0, 0:2]) == (1.0, F(-0.02))
    assert rn[0] == reward_of((0, -F(0.02)), (1, -F(0.02))) and rn[0] == -r[0] and rn[0] < 0


def test_radial_move_pays_nothing():
    s1, r, _ = step(make_state(p=(1, 0), u=(1, 0)), (1.0, 0.0))
    assert tuple(s1[0, 0:2]) == (F(F(1) + F(0.02)), 0.0) and r[0] == 0
    s1, r, _ = step(make_state(p=(1, 0), u=(-1, 0)), (1.0, 0.0))
    assert tuple(s1[0, 0:2]) == (F(F(1) - F(0.02)), 0.0) and r[0] == 0
    # standing at the origin: |q| = 0 pays 0, not NaN
    s1, r, _ = step(make_state(), (0.0, 0.0))
    assert tuple(s1[0, 0:2]) == (0.0, 0.0) and r[0] == 0


def test_reward_is_damped_away_from_radius_one():
    r = {}
    for rad in (0.5, 1.0, 1.5):
        s1, rw, _ = step(make_state(p=(rad, 0), u=(0, 1)), (1.0, 0.0))
        assert rw[0] == reward_of((0, F(0.02)), (rad, F(0.02)))
        r[rad] = float(rw[0])
    assert r[1.0] > r[0.5] > 0 and r[1.0] > r[1.5] > 0
    assert abs(r[0.5] - 0.02 * 0.5 / 0.5004 / 1.4996) < 1e-5 and abs(r[1.5] - 0.02 * 1.5 / 1.50013 / 1.50013) < 1e-5


def test_a_turning_step_uses_the_new_heading():
    s1, r, _ = step(make_state(p=(1, 0), u=(1, 0), f=0.1), (0.0, 1.0))
    t = F(0.15)
    tt = F(t * t)
    den = F(F(1) + tt)
    c, sn = F(F(F(1) - tt) / den), F(F(F(2) * t) / den)
    nrm = np.sqrt(F(F(c * c) + F(sn * sn)), dtype=np.float32)
    u2 = (F(c / nrm), F(sn / nrm))
    f1 = F(F(0.9) * F(0.1))
    m = (F(f1 * u2[0]), F(f1 * u2[1]))
    assert s1[0, 6] == t and tuple(s1[0, 2:4]) == u2 and s1[0, 4] == f1 and s1[0, 5] == F(0.1)
    assert tuple(s1[0, 0:2]) == (F(F(1) + m[0]), m[1])
    assert r[0] == reward_of(m, s1[0, 0:2]) and r[0] > 0


# ------------------------------------------------------------------ costs
def test_costs_by_level():
    along_x = make_state(p=(0.74, 0), u=(1, 0), f=0.2)     # f = 0.18 + 0.02: q = (0.94, 0)
    along_y = make_state(p=(0, 0.74), u=(0, 1), f=0.2)
    assert abs(float(step(along_x, (1.0, 0.0))[0][0, 0]) - 0.94) < 1e-6
    assert [float(step(along_x, (1.0, 0.0), level)[2][0]) for level in (0, 1, 2)] == [0, 1, 1]
    assert [float(step(along_y, (1.0, 0.0), level)[2][0]) for level in (0, 1, 2)] == [0, 0, 1]
    # the other wall of each pair
    assert [float(step(make_state(p=(-0.74, 0), u=(-1, 0), f=0.2), (1.0, 0.0), level)[2][0])
            for level in (0, 1, 2)] == [0, 1, 1]
    assert [float(step(make_state(p=(0, -0.74), u=(0, -1), f=0.2), (1.0, 0.0), level)[2][0])
            for level in (0, 1, 2)] == [0, 0, 1]


def test_the_wall_itself_does_not_cost():
    on = make_state(p=(F(0.75), F(-0.75)))                # f = 0, action 0: q = p
    for level in (0, 1, 2):
        s1, _, c = step(on, (0.0, 0.0), level)
        assert tuple(s1[0, 0:2]) == (F(0.75), F(-0.75)) and c[0] == 0
    past = np.nextafter(F(0.75), F(1))
    assert [float(step(make_state(p=(past, 0)), (0.0, 0.0), level)[2][0]) for level in (0, 1, 2)] == [0, 1, 1]
    assert [float(step(make_state(p=(0, -past)), (0.0, 0.0), level)[2][0]) for level in (0, 1, 2)] == [0, 0, 1]


def test_wall_clip():
    s1, _, c = step(make_state(p=(1.99, -1.0), u=(1, 0), f=0.5), (1.0, 0.0), 2)
    f1 = F(F(F(0.9) * F(0.5)) + F(0.02))
    assert s1[0, 4] == f1 and F(F(1.99) + f1) > 2
    assert tuple(s1[0, 0:2]) == (2.0, -1.0) and c[0] == 1
    s2 = step(make_state(p=(0.0, -1.95), u=(0, -1), f=0.5), (1.0, 0.0))[0]
    assert tuple(s2[0, 0:2]) == (0.0, -2.0)


# ------------------------------------------------------------------ reset
def test_reset_layout():
    s = T.circle_reset(5, 0, 256)
    u = T.draws(5, 0, 256, 1, 4)
    assert s.shape == (256, 8) and s.dtype == np.float32
    assert u.min() > -1.5 and u.max() <= 1.5
    assert np.array_equal(s[:, 0:2], (F(0.4) * u[:, 0:2]).astype(np.float32))
    assert np.abs(s[:, 0:2]).max() <= 0.6 and np.abs(s[:, 0:2]).max() > 0.5
    nrm = np.sqrt(s[:, 2].astype(np.float64) ** 2 + s[:, 3].astype(np.float64) ** 2)
    assert np.abs(nrm - 1).max() <= np.finfo(np.float32).eps
    assert np.allclose(s[:, 2] * u[:, 3], s[:, 3] * u[:, 2], atol=1e-6)   # parallel to (u2, u3)
    assert not s[:, 4:].any()
    # the draws depend on seed, position and env index
    assert not np.array_equal(s, T.circle_reset(6, 0, 256))
    assert not np.array_equal(s, T.circle_reset(5, 1, 256))
    assert not np.array_equal(s[0], s[1])
    assert np.array_equal(s[:7], T.circle_reset(5, 0, 7))
    # and on the env's own key: not SynthNavGoal's numbers at the same seed
    assert not np.array_equal(u, nav_twin.draws(5, 0, 256, 1, 4))
    assert np.array_equal(T.draws(5 ^ T.CIRCLE_KEY ^ nav_twin.NAV_KEY, 0, 256, 1, 4), nav_twin.draws(5, 0, 256, 1, 4))


# ------------------------------------------------------------------ lidar of the centre
def seen_from(u, theta, d):
    """The position from which the origin lies at body-frame angle theta and distance d (float64, then rounded)."""
    ux, uy = u
    return (-d * (np.cos(theta) * ux - np.sin(theta) * uy), -d * (np.cos(theta) * uy + np.sin(theta) * ux))


def test_centre_lidar_sector_centres():
    u = (0.6, 0.8)
    for k in range(16):
        for d in (0.3, 1.2):
            o = T.circle_obs(make_state(p=seen_from(u, (k + 0.5) * np.pi / 8, d), u=u, f=0.25, f_prev=0.125))
            assert o.shape == (1, 28) and o.dtype == np.float32
            assert abs(float(o[0, 12 + k]) - (1 - d / 3)) < 1e-6, k
            assert not np.delete(o[0, 12:], k).any(), k
            assert tuple(o[0, :5]) == (F(0.25), F(0.125), 0.0, F(0.6), F(0.8)) and not o[0, 5:12].any()
    # the reading is the specification's expression of |p|
    s = make_state(p=(0.3, -0.4), u=u)
    rad = np.sqrt(F(F(F(0.3) * F(0.3)) + F(F(-0.4) * F(-0.4))), dtype=np.float32)
    assert T.circle_obs(s)[0, 12:].max() == F(F(1) - F(rad / F(3)))


def test_centre_lidar_at_the_origin_and_out_of_range():
    assert not T.circle_obs(make_state(p=(0, 0), u=(0.6, 0.8)))[0, 12:].any()
    far = make_state(p=seen_from((1, 0), 0.3, 3.2), u=(1, 0))
    assert not T.circle_obs(far)[0, 12:].any()
    near = make_state(p=seen_from((1, 0), 0.3, 2.9), u=(1, 0))
    assert (T.circle_obs(near)[0, 12:] > 0).sum() == 1
    wide = T.circle_obs(near, 40)
    assert wide.shape == (1, 40) and np.array_equal(wide[:, :28], T.circle_obs(near)) and not wide[:, 28:].any()


def test_every_position_but_the_origin_lights_exactly_one_bin():
    rng = np.random.default_rng(0)
    N = 20_000
    s = np.zeros((N, 8), np.float32)
    s[:, 0:2] = rng.uniform(-2, 2, (N, 2))
    h = rng.standard_normal((N, 2))
    s[:, 2:4] = h / np.linalg.norm(h, axis=1, keepdims=True)
    o = T.circle_obs(s)
    assert ((o[:, 12:] > 0).sum(1) == 1).all()            # |p| <= 2 sqrt 2 < 3: always in range


# ------------------------------------------------------------------ vector twin
def test_vector_twin_truncates_and_resets_together():
    env = T.CircleTwin(1, 8, horizon=3, seed=9)
    o0 = env.reset()
    assert np.array_equal(o0, T.circle_obs(T.circle_reset(9, 0, 8)))
    a = np.ones((8, 2), np.float32)
    for t in range(1, 7):
        before = env.state
        o, r, c, trunc, final = env.step(a)
        assert trunc == (t % 3 == 0) and (final is not None) == trunc
        if trunc:
            assert np.array_equal(final, T.circle_obs(T.circle_step(before, a, 1)[0]))
            assert np.array_equal(env.state, T.circle_reset(9, t, 8))
            assert np.array_equal(o, T.circle_obs(env.state)) and not np.array_equal(o, final)
        else:
            assert np.array_equal(env.state, T.circle_step(before, a, 1)[0])
            assert np.array_equal(o, T.circle_obs(env.state))
