"""CPU: the host side of offline BCQ / BCQ-Lag -- the configuration tables against the values of the reference's YAML
files, the registry, the shapes refused before any GPU is touched, and the actor's state-dict names, order and shapes."""
import pytest


def test_config_tables_hold_the_yaml_values():
    """configs/offline/BCQ.yaml and BCQLag.yaml, `defaults` blocks."""
    from omnisafe_amd import algorithms, config
    from omnisafe_amd.algorithms import registry
    from omnisafe_amd.algorithms.offline import BCQ, BaseOffline, BCQLag

    model = {'hidden_sizes': [256, 256, 256], 'activation': 'relu', 'lr': 0.001}
    algo = {'gamma': 0.99, 'batch_size': 256, 'steps_per_epoch': 1000, 'phi': 0.05, 'sampled_action_num': 10,
            'minimum_weighting': 0.75, 'polyak': 0.005}
    bcq, lag = config.default_kwargs('BCQ'), config.default_kwargs('BCQLag')
    assert bcq['algo_cfgs'] == algo and 'lagrange_cfgs' not in bcq
    assert lag['algo_cfgs'] == dict(algo, cost_gamma=0.99, lagrange_start_step=150000)
    assert lag['lagrange_cfgs'] == {'cost_limit': 25.0, 'lagrangian_multiplier_init': 1.0, 'lambda_lr': 0.001,
                                    'lambda_optimizer': 'Adam'}
    for d in (bcq, lag):
        assert d['model_cfgs']['actor'] == model and d['model_cfgs']['critic'] == model and d['seed'] == 0
        assert d['train_cfgs']['total_steps'] == 1000000 and d['train_cfgs']['evaluate_epoisodes'] == 10
    assert registry.get('BCQ') is BCQ and registry.get('BCQLag') is BCQLag and issubclass(BCQLag, BCQ)
    assert issubclass(BCQ, BaseOffline) and algorithms.ALGORITHMS['offline-bcq'] == ('BCQ', 'BCQLag')
    assert config.default_kwargs('PPOLag') == config.get_default_kwargs('PPOLag')
    cfgs = config.Config.dict2config(dict(lag, algo='BCQLag'))
    config.check_all_configs(cfgs)  # (no beta to ask for)
    for key, bad in (('minimum_weighting', 1.5), ('phi', -0.1)):
        cfgs = config.Config.dict2config(dict(config.default_kwargs('BCQ'), algo='BCQ'))
        setattr(cfgs.algo_cfgs, key, bad)
        with pytest.raises(AssertionError):
            config.check_all_configs(cfgs)


@pytest.mark.parametrize('kw', [dict(actor_act='gelu'), dict(critic_act='gelu'), dict(actor_hidden=[]),
                                dict(critic_hidden=[]), dict(act_dim=33)])
def test_make_desc_refusals(kw):
    from omnisafe_amd import bcq_step

    args = dict(obs_dim=4, act_dim=2, actor_hidden=[8], critic_hidden=[8], actor_act='relu', critic_act='relu')
    bcq_step.make_desc(**args)
    with pytest.raises(NotImplementedError):
        bcq_step.make_desc(**dict(args, **kw))


def test_state_dict_names_order_and_shapes():
    """PerturbationActor.state_dict() behind ``_phi`` for obs 7, act 3, hidden [24, 40]: the VAE registers each network
    twice (``_encoder`` / ``_decoder``, then ``encoder`` / ``decoder``), then the perturbation network."""
    from omnisafe_amd import bcq_step

    desc = bcq_step.make_desc(7, 3, [24, 40], [16], 'relu', 'tanh', 5, 2, 2)
    lay = bcq_step.BcqLayout(desc)
    enc = [(24, 10), (24,), (40, 24), (40,), (12, 40), (12,)]
    dec = [(24, 13), (24,), (40, 24), (40,), (3, 40), (3,)]
    per = [(24, 10), (24,), (40, 24), (40,), (3, 40), (3,)]
    names = lambda prefix: [f'{prefix}.{2 * j}.{kind}' for j in range(3) for kind in ('weight', 'bias')]  # noqa: E731
    want = []
    for prefix, shapes in (('vae._encoder', enc), ('vae._decoder', dec), ('vae.encoder', enc), ('vae.decoder', dec),
                           ('perturbation', per)):
        want += list(zip(names(prefix), shapes))
    blocks = lay.actor_tensors()
    assert [(n, s) for n, s, _ in blocks['vae'] + blocks['pert']] == want
    assert [(n, s) for n, s, _ in lay.tensors(1, 'critic_1.0')] == [
        ('critic_1.0.0.weight', (16, 10)), ('critic_1.0.0.bias', (16,)), ('critic_1.0.2.weight', (1, 16)),
        ('critic_1.0.2.bias', (1,))]
    assert all(p % 16 == 0 for p in (lay.Pe, lay.Pd, lay.Pp, lay.Pc)) and lay.nstat == 16
    assert bcq_step._lib.load().osa_bcq_chain_supported(bcq_step.C.byref(desc)) == 1
