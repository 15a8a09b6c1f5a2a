"""CPU: the host side of offline CRR / CCRR -- configuration, dataset loading and its errors, the argument checks of the
new C entry points (before any launch: no GPU is needed), the state-dict layout, the registry."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

FIELDS = ('obs', 'action', 'reward', 'cost', 'next_obs', 'done')


def _arrays(N=16, D=5, A=2):
    rng = np.random.default_rng(0)
    return {'obs': rng.standard_normal((N, D)).astype(np.float32), 'action': rng.standard_normal((N, A)).astype(np.float32),
            'reward': rng.standard_normal((N, 1)).astype(np.float32), 'cost': np.zeros((N, 1), np.float32),
            'next_obs': rng.standard_normal((N, D)).astype(np.float32), 'done': np.zeros((N, 1), np.float32)}


@pytest.mark.reference
@pytest.mark.parametrize('algo', ['CRR', 'CCRR'])
def test_defaults_equal_reference_yaml(algo):
    """config.OFFLINE_DEFAULTS restates configs/offline/{CRR,CCRR}.yaml; deliberate deviations: device (cuda:0),
    use_tensorboard (off), the `verbose` extension and the (empty) env_cfgs block."""
    import ref_harness

    ref_harness.import_reference()
    from omnisafe.utils.config import get_default_kwargs_yaml

    from omnisafe_amd import config

    ref = get_default_kwargs_yaml(algo, '', 'offline').todict()
    ours = config.get_default_kwargs(algo)

    def cmp(r, m, path=''):
        for k in r:
            assert k in m, f'missing {path}{k}'
            if isinstance(r[k], dict):
                cmp(r[k], m[k], path + k + '.')
            elif k not in ('device', 'use_tensorboard'):
                assert r[k] == m[k] and type(r[k]) is type(m[k]), f'{path}{k}: reference {r[k]!r}, ours {m[k]!r}'
        for k in m:
            assert k in r or k in ('env_cfgs', 'verbose'), f'extra {path}{k}'

    cmp(ref, ours)


def test_offline_defaults_are_a_table_of_their_own():
    from omnisafe_amd import config

    assert sorted(config.OFFLINE_DEFAULTS) == ['CCRR', 'CRR'] and not set(config.OFFLINE_DEFAULTS) & set(config.DEFAULTS)
    assert 'lagrange_cfgs' in config.get_default_kwargs('CCRR') and 'lagrange_cfgs' not in config.get_default_kwargs('CRR')
    with pytest.raises(KeyError):
        config.get_default_kwargs('BCQ')


def test_unknown_keys_are_refused_and_checks_branch_on_the_family():
    import omnisafe_amd
    from omnisafe_amd import config

    with pytest.raises(KeyError, match='Invalid key: update_iters'):
        omnisafe_amd.Agent('CRR', 'SynthReach-v0', custom_cfgs={'algo_cfgs': {'update_iters': 3}})
    with pytest.raises(KeyError, match='Invalid key: lagrange_cfgs'):
        omnisafe_amd.Agent('CRR', 'SynthReach-v0', custom_cfgs={'lagrange_cfgs': {'cost_limit': 1.0}})
    off = config.Config.dict2config(dict(config.get_default_kwargs('CCRR'), algo='CCRR'))
    config.check_all_configs(off)
    off.train_cfgs.parallel = 2
    with pytest.raises(AssertionError):
        config.check_all_configs(off)
    on = config.Config.dict2config(dict(config.get_default_kwargs('PPOLag'), algo='PPOLag'))
    config.check_all_configs(on)
    on.algo_cfgs.update_iters = 0  # the on-policy checks are as strict as before
    with pytest.raises(AssertionError):
        config.check_all_configs(on)


def test_dataset_errors(tmp_path):
    from omnisafe_amd import crr_step, offline

    arrays = _arrays()
    path = offline.write_dataset(str(tmp_path), 'Env-v0', arrays)
    data = crr_step.load_dataset(path, 5, 2, 'cpu')
    assert list(data) == list(FIELDS) and all(t.dtype == torch.float32 and t.is_contiguous() for t in data.values())
    assert np.array_equal(data['next_obs'].numpy(), arrays['next_obs'])
    with pytest.raises(FileNotFoundError):
        crr_step.load_dataset(str(tmp_path / 'nothing.npz'), 5, 2, 'cpu')
    with pytest.raises(FileNotFoundError):  # a dataset NAME: the reference would download it, this package never does
        crr_step.load_dataset('SafetyPointCircle1-v0_mixed_0.5', 5, 2, 'cpu')
    short = str(tmp_path / 'short.npz')
    np.savez(short, **{k: v for k, v in arrays.items() if k != 'cost'})
    with pytest.raises(KeyError, match='cost'):
        crr_step.load_dataset(short, 5, 2, 'cpu')
    with pytest.raises(ValueError, match='obs'):
        crr_step.load_dataset(path, 6, 2, 'cpu')
    with pytest.raises(ValueError, match='action'):
        crr_step.load_dataset(path, 5, 3, 'cpu')
    ragged = str(tmp_path / 'ragged.npz')
    np.savez(ragged, **dict(arrays, done=arrays['done'][:-1]))
    with pytest.raises(ValueError, match='done'):
        crr_step.load_dataset(ragged, 5, 2, 'cpu')


def test_entry_points_check_arguments_before_any_launch():
    from omnisafe_amd import _lib, crr_step

    lib = _lib.load()
    d = crr_step.make_desc(7, 3, [24, 40], [24, 40], 'relu', 'relu', 5, 3, 2)
    out = (C.c_int * 52)()
    assert lib.osa_crr_layout(None, out) == -1 and lib.osa_crr_layout(C.byref(d), None) == -1
    assert lib.osa_crr_layout(C.byref(d), out) == 0
    assert lib.osa_crr_ws_floats(None) == 0 and lib.osa_crr_ws_floats(C.byref(d)) > 0
    assert lib.osa_crr_draws(None, 0, 0, 1, 1, 5, None, None, None, None, None) == -1
    assert lib.osa_crr_draws(C.byref(d), 0, 0, 1, 1, 5, None, None, None, None, None) == -1
    assert lib.osa_crr_step(None, None, None, None, None, None, None, 0, 1, None) == -1
    hp, st, da, dr = crr_step.CrrHParams(), crr_step.CrrState(), crr_step.CrrData(), crr_step.CrrDrawBuffers()
    assert lib.osa_crr_step(C.byref(d), C.byref(hp), C.byref(st), C.byref(da), C.byref(dr), None, None, 0, 1, None) == -1
    bad = crr_step.make_desc(7, 3, [24], [24], 'relu', 'relu', 5, 3, 2)
    for field, value in (('pairs', 3), ('batch', 0), ('samples', 0), ('obs_dim', 0)):
        keep = getattr(bad, field)
        setattr(bad, field, value)
        assert lib.osa_crr_layout(C.byref(bad), out) == -1, field
        setattr(bad, field, keep)
    bad.n_layers[1] = 1  # no hidden layer
    bad.width[1][0] = 1
    assert lib.osa_crr_layout(C.byref(bad), out) == _lib.OSA_EUNSUPPORTED
    big = crr_step.make_desc(7, 3, [24], [24], 'relu', 'relu', 1 << 18, 10, 1)
    assert lib.osa_crr_layout(C.byref(big), out) == _lib.OSA_EUNSUPPORTED


def test_hidden_layer_limits():
    from omnisafe_amd import crr_step
    from omnisafe_amd.models import GMLP_MAX_LAYERS

    crr_step.make_desc(4, 2, [8] * (GMLP_MAX_LAYERS - 1), [8], 'relu', 'tanh', 4, 2, 1)
    for a_h, c_h in (([], [8]), ([8], []), ([8] * GMLP_MAX_LAYERS, [8]), ([8, 0], [8])):
        with pytest.raises(NotImplementedError):
            crr_step.make_desc(4, 2, a_h, c_h, 'relu', 'relu', 4, 2, 1)
    with pytest.raises(NotImplementedError):
        crr_step.make_desc(4, 2, [8], [8], 'gelu', 'relu', 4, 2, 1)


def test_state_dict_names_order_shapes_and_padding():
    from omnisafe_amd import crr_step

    d = crr_step.make_desc(7, 3, [24, 40], [10], 'relu', 'relu', 5, 3, 2)
    lay = crr_step.CrrLayout(d)
    actor = lay.tensors(0)
    assert [(n, s) for n, s, _ in actor] == [
        ('log_std', (3,)), ('mean.0.weight', (24, 7)), ('mean.0.bias', (24,)), ('mean.2.weight', (40, 24)),
        ('mean.2.bias', (40,)), ('mean.4.weight', (3, 40)), ('mean.4.bias', (3,))]
    critic = lay.tensors(1, 'critic_1.0')
    assert [(n, s) for n, s, _ in critic] == [
        ('critic_1.0.0.weight', (10, 10)), ('critic_1.0.0.bias', (10,)), ('critic_1.0.2.weight', (1, 10)),
        ('critic_1.0.2.bias', (1,))]
    for net, items in ((0, actor), (1, critic)):
        ix = np.concatenate([i for _, _, i in items])
        assert len(set(ix.tolist())) == len(ix) and ix.max() < (lay.Pa if net == 0 else lay.Pc)
        assert lay.real_mask(net).sum() == len(ix)
    assert lay.Pa % 16 == 0 and lay.Pc % 16 == 0 and lay.nstat == 12
    # rows of 7 and of 10 inputs are padded to 8 and 12 floats
    assert actor[1][2][7] - actor[1][2][0] == 8 and critic[0][2][10] - critic[0][2][0] == 12


@pytest.mark.reference
def test_initial_weights_equal_the_reference_builders():
    """Same torch seed: actor, reward critic pair, cost critic pair in the reference's construction order."""
    import ref_harness

    ref_harness.import_reference()
    from gymnasium.spaces import Box
    from omnisafe.models.actor.actor_builder import ActorBuilder
    from omnisafe.models.critic.critic_builder import CriticBuilder

    from omnisafe_amd import crr_step

    obs_space, act_space = Box(-np.inf, np.inf, (7,)), Box(-1.0, 1.0, (3,))
    torch.manual_seed(12)
    ref_actor = ActorBuilder(obs_space, act_space, [24, 40], 'relu', 'kaiming_uniform').build_actor('gaussian_learning')
    ref_pairs = [CriticBuilder(obs_space, act_space, [10], 'relu', 'kaiming_uniform', num_critics=2).build_critic('q')
                 for _ in range(2)]
    torch.manual_seed(12)
    actor, pairs = crr_step.initial_state_dicts(crr_step.make_desc(7, 3, [24, 40], [10], 'relu', 'relu', 5, 3, 2))
    for ours, ref in [(actor, ref_actor)] + list(zip(pairs, ref_pairs)):
        sd = ref.state_dict()
        assert list(ours) == list(sd)
        for k in sd:
            assert torch.equal(ours[k], sd[k]), k


def test_registry_and_plugin_lists():
    from omnisafe_amd import algorithms, plugin
    from omnisafe_amd.algorithms import registry
    from omnisafe_amd.algorithms.offline import CCRR, CRR, BaseOffline

    assert registry.get('CRR') is CRR and registry.get('CCRR') is CCRR and issubclass(CCRR, BaseOffline)
    assert len(plugin.ACCELERATED) == 23 and not {'CRR', 'CCRR'} & set(plugin.ACCELERATED)
    assert len(algorithms.ALGORITHMS['on-policy']) == 23 and algorithms.ALGORITHMS['offline'] == ('CCRR', 'CRR')


def test_offline_runs_have_no_normalizer_key():
    """saved_policy.build_policy reads algo_cfgs.obs_normalize as absent = False (an offline run's config.json)."""
    import inspect

    from omnisafe_amd import saved_policy

    assert "getattr(cfgs.algo_cfgs, 'obs_normalize', False)" in inspect.getsource(saved_policy.build_policy)
    assert os.path.basename(saved_policy.__file__) == 'saved_policy.py'
