"""CPU: the host side of off-policy SAC -- configuration, registry, the state-dict layout against the reference's
GaussianSACActor and QCritic, and the shapes and options refused before any GPU is touched."""
import numpy as np
import pytest


@pytest.mark.reference
def test_defaults_equal_reference_yaml():
    """config.SAC_DEFAULTS restates configs/off-policy/SAC.yaml; deliberate deviations: device (cuda:0),
    use_tensorboard (off), the `verbose` extension and the (empty) env_cfgs block."""
    import ref_harness

    ref_harness.import_reference()
    from omnisafe.utils.config import get_default_kwargs_yaml

    from omnisafe_amd import config

    ref = get_default_kwargs_yaml('SAC', '', 'off-policy').todict()
    ours = config.default_kwargs('SAC')

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
    from omnisafe_amd import algorithms, config
    from omnisafe_amd.algorithms import registry
    from omnisafe_amd.algorithms.off_policy import SAC, BaseOffPolicy

    assert registry.get('SAC') is SAC and issubclass(SAC, BaseOffPolicy) and SAC.num_critics == 2
    assert algorithms.ALGORITHMS['off-policy-sac'] == ('SAC',) and 'SAC' not in config.OFFPOLICY_DEFAULTS
    cfgs = config.Config.dict2config(dict(config.default_kwargs('SAC'), algo='SAC'))
    config.check_all_configs(cfgs)
    cfgs.algo_cfgs.alpha = 0.0
    with pytest.raises(AssertionError):
        config.check_all_configs(cfgs)


@pytest.mark.reference
def test_layout_equals_the_reference_state_dicts():
    """Keys, order and shapes of GaussianSACActor.state_dict() (its ``_log2`` buffer included) and of a two-network
    QCritic.state_dict()."""
    import ref_harness

    ref_harness.import_reference()
    from gymnasium.spaces import Box
    from omnisafe.models.actor.actor_builder import ActorBuilder
    from omnisafe.models.critic.critic_builder import CriticBuilder

    from omnisafe_amd import sac_step

    spaces = Box(-np.inf, np.inf, (7,)), Box(-1.0, 1.0, (3,))
    actor = ActorBuilder(*spaces, [24, 40], 'relu', 'kaiming_uniform').build_actor('gaussian_sac').state_dict()
    critic = CriticBuilder(*spaces, [24, 40], 'relu', 'kaiming_uniform', num_critics=2).build_critic('q').state_dict()
    lay = sac_step.SacLayout(sac_step.make_desc(7, 3, [24, 40], [24, 40], 'relu', 'relu', 5))
    ours = [('_log2', ())] + [(n, s) for n, s, _ in lay.tensors()]
    assert ours == [(k, tuple(v.shape)) for k, v in actor.items()] and ours[-2][1] == (6, 40)
    ours = [(n, s) for block in lay.critic_tensors(2) for n, s, _ in block]
    assert ours == [(k, tuple(v.shape)) for k, v in critic.items()]
    assert lay.Pa % 16 == 0 and lay.Pc % 16 == 0


@pytest.mark.parametrize('kw', [dict(actor_hidden=[]), dict(critic_hidden=[8, 0]), dict(actor_hidden=[8] * 8),
                                dict(critic_hidden=[4097]), dict(actor_act='gelu'), dict(act_dim=33), dict(act_dim=0),
                                dict(num_critics=1), dict(num_critics=3)])
def test_unsupported_shapes_raise_before_any_gpu(kw):
    from omnisafe_amd import sac_step

    args = dict(obs_dim=4, act_dim=2, actor_hidden=[8], critic_hidden=[8], actor_act='relu', critic_act='relu', batch=4)
    sac_step.make_desc(**args)
    with pytest.raises(NotImplementedError):
        sac_step.make_desc(**dict(args, **kw))


@pytest.mark.parametrize('env_id,cfgs', [('SafetyPointGoal1-v0', {}),
                                         ('SynthNavGoal0-v0', {'algo_cfgs': {'obs_normalize': True}}),
                                         ('SynthNavGoal0-v0', {'algo_cfgs': {'cost_normalize': True}}),
                                         ('SynthNavGoal0-v0', {'model_cfgs': {'linear_lr_decay': True}})])
def test_unsupported_options_raise_before_any_gpu(env_id, cfgs):
    from omnisafe_amd import config
    from omnisafe_amd.algorithms.off_policy import SAC

    c = config.Config.dict2config(dict(config.default_kwargs('SAC'), algo='SAC', env_id=env_id))
    c.recurisve_update(cfgs)
    algo = SAC.__new__(SAC)
    algo._env_id, algo._cfgs = env_id, c  # noqa: SLF001
    with pytest.raises(NotImplementedError):
        algo._init_env()  # noqa: SLF001
