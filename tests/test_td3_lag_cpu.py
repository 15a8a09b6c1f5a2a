"""CPU: the host side of DDPGLag, TD3Lag, DDPGPID and TD3PID -- configuration, registry, the options accepted or
refused before any GPU is touched, and the carry of episode costs between epochs."""
import pytest
import test_td3_cpu
import torch

NAMES = ('DDPGLag', 'DDPGPID', 'TD3Lag', 'TD3PID')


@pytest.mark.reference
@pytest.mark.parametrize('algo', NAMES)
def test_defaults_equal_reference_yaml(algo):
    """config.OFFPOLICY_LAG_DEFAULTS restates the four YAMLs, under test_td3_cpu's comparison and its deviations."""
    test_td3_cpu.test_defaults_equal_reference_yaml(algo)


def _algo(name, custom=None):  # a bare object with its configuration, as test_td3_cpu builds TD3's
    from omnisafe_amd import config
    from omnisafe_amd.algorithms import registry

    algo = object.__new__(registry.get(name))
    algo._env_id = 'SynthNavGoal0-v0'  # noqa: SLF001
    algo._cfgs = config.Config.dict2config(dict(config.default_kwargs(name), algo=name))  # noqa: SLF001
    algo._cfgs.recurisve_update(custom or {})  # noqa: SLF001
    return algo


@pytest.mark.parametrize('name', NAMES)
def test_registry_config_branch_and_options(name):
    """The new tables; cost_normalize True (the YAML default) passes _init_env's refusals, to which test_td3_cpu holds
    the base class; obs_normalize and, for the Lag forms, a lambda_optimizer other than Adam still raise there."""
    from omnisafe_amd import algorithms, config, plugin, td3_step
    from omnisafe_amd.algorithms.off_policy import BaseOffPolicy

    assert algorithms.ALGORITHMS['off-policy-lag'] == NAMES == tuple(sorted(config.OFFPOLICY_LAG_DEFAULTS))
    assert td3_step.LAG_STAT_KEYS == td3_step.STAT_KEYS + ('Metrics/LagrangeMultiplier',)
    algo = _algo(name)
    assert isinstance(algo, BaseOffPolicy) and algo.num_critics == (2 if name.startswith('TD3') else 1)
    assert name not in plugin.ACCELERATED and algo._cfgs.algo_cfgs.use_cost  # noqa: SLF001
    with pytest.raises(KeyError):
        config.get_default_kwargs(name)
    config.check_all_configs(algo._cfgs)  # noqa: SLF001
    with pytest.raises(AssertionError):
        config.check_all_configs(_algo(name, {'algo_cfgs': {'warmup_epochs': -1}})._cfgs)  # noqa: SLF001
    with pytest.raises(AttributeError, match='_device'):  # past every refusal: the bare object has no device for the env
        algo._init_env()  # noqa: SLF001
    for who, custom in ((name, {'algo_cfgs': {'obs_normalize': True}}), ('TD3', {'algo_cfgs': {'cost_normalize': True}}),
                        (name, {'lagrange_cfgs': {'lambda_optimizer': 'SGD'}}))[:2 + name.endswith('Lag')]:
        with pytest.raises(NotImplementedError):
            _algo(who, custom)._init_env()  # noqa: SLF001


@pytest.mark.parametrize('ncarry,n_ep,want', [(2, 1, [5.0, 6.0, 7.0]), (3, 3, [7.0, 7.0, 8.0, 9.0]), (0, 0, [])])
def test_after_epoch_carries_the_last_window_of_episode_costs(ncarry, n_ep, want):
    algo = _algo('TD3Lag')
    algo._carry, algo._ncarry = torch.tensor([5.0, 6.0, 7.0, 0.0]), ncarry  # noqa: SLF001  window_lens 4
    algo._episodes = (None, torch.tensor([[0.0, 7.0, 1.0], [0.0, 8.0, 1.0], [0.0, 9.0, 1.0]]), None)  # noqa: SLF001
    algo._after_epoch(n_ep)  # noqa: SLF001
    assert algo._carry[:algo._ncarry].tolist() == want  # noqa: SLF001
