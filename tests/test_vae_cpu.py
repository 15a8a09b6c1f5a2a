"""CPU: the host side of offline VAE-BC -- configuration, registry, the state-dict layout against the reference's VAE,
and the shapes refused before any GPU is touched."""
import numpy as np
import pytest
import torch


@pytest.mark.reference
def test_defaults_equal_reference_yaml():
    """config.BC_DEFAULTS restates configs/offline/VAEBC.yaml; deliberate deviations as for CRR: device (cuda:0),
    use_tensorboard (off), the `verbose` extension and the (empty) env_cfgs block."""
    import ref_harness

    ref_harness.import_reference()
    from omnisafe.utils.config import get_default_kwargs_yaml

    from omnisafe_amd import config

    ref = get_default_kwargs_yaml('VAEBC', '', 'offline').todict()
    ours = config.get_default_kwargs('VAEBC')

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


def test_registry_tables_and_config_branch():
    from omnisafe_amd import algorithms, config, plugin
    from omnisafe_amd.algorithms import registry
    from omnisafe_amd.algorithms.offline import VAEBC, BaseOffline

    assert registry.get('VAEBC') is VAEBC and issubclass(VAEBC, BaseOffline)
    assert algorithms.ALGORITHMS['offline-bc'] == ('VAEBC',) and len(plugin.ACCELERATED) == 23
    assert sorted(config.BC_DEFAULTS) == ['VAEBC'] and 'VAEBC' not in config.OFFLINE_DEFAULTS
    with pytest.raises(KeyError):
        config.get_default_kwargs('BCQ')
    cfgs = config.Config.dict2config(dict(config.get_default_kwargs('VAEBC'), algo='VAEBC'))
    config.check_all_configs(cfgs)  # no sampled_action_num / gamma / polyak to ask for
    cfgs.algo_cfgs.batch_size = 0
    with pytest.raises(AssertionError):
        config.check_all_configs(cfgs)


@pytest.mark.reference
def test_state_dict_equals_the_reference_vae():
    """Keys, order, shapes and (same torch seed) initial values of VAE.state_dict()."""
    import ref_harness

    ref_harness.import_reference()
    from gymnasium.spaces import Box
    from omnisafe.models.actor.actor_builder import ActorBuilder

    from omnisafe_amd import vae_step

    torch.manual_seed(12)
    ref = ActorBuilder(Box(-np.inf, np.inf, (7,)), Box(-1.0, 1.0, (3,)), [24, 40], 'relu',
                       'kaiming_uniform').build_actor('vae').state_dict()
    desc = vae_step.make_desc(7, 3, [24, 40], 'relu', 5)
    items = vae_step.VaeLayout(desc).tensors()
    assert [(n, s) for n, s, _ in items] == [(k, tuple(v.shape)) for k, v in ref.items()]
    torch.manual_seed(12)
    ours = vae_step.initial_state_dict(desc)
    for k, v in ours.items():
        assert torch.equal(v, ref[k]) and torch.equal(v, ref['_' + k]), k


def test_layout_padding():
    from omnisafe_amd import vae_step

    lay = vae_step.VaeLayout(vae_step.make_desc(7, 3, [24, 40], 'relu', 5))
    items = {n: ix for n, _, ix in lay.tensors()}
    assert lay.Pe % 16 == 0 and lay.Pd % 16 == 0 and lay.nstat == 4
    assert np.array_equal(items['_encoder.0.weight'], items['encoder.0.weight'])  # two names, one tensor
    # encoder rows of 7 + 3 inputs are padded to 12 floats, decoder rows of 7 + 6 to 16; the decoder follows at Pe
    assert items['encoder.0.weight'][10] - items['encoder.0.weight'][0] == 12
    assert items['decoder.0.weight'][13] - items['decoder.0.weight'][0] == 16 and items['decoder.0.weight'][0] == lay.Pe
    assert lay.real_mask().sum() == sum(len(ix) for n, ix in items.items() if not n.startswith('_'))


@pytest.mark.parametrize('kw', [dict(hidden_sizes=[]), dict(hidden_sizes=[8, 0]), dict(hidden_sizes=[8] * 8),
                                dict(activation='gelu'), dict(act_dim=33)])
def test_unsupported_shapes_raise_before_any_gpu(kw):
    from omnisafe_amd import vae_step

    args = dict(obs_dim=4, act_dim=2, hidden_sizes=[8], activation='relu', batch=4)
    vae_step.make_desc(**args)
    with pytest.raises(NotImplementedError):
        vae_step.make_desc(**dict(args, **kw))
