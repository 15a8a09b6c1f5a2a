"""CPU: the twin of the COptiDICE step (tests/dice_twin.py) against the unmodified reference step for step (marked
`reference`), ``load_init_obs``, the defaults against the YAML, and the closed form of the chi gradient."""
import types

import dice_twin as T
import numpy as np
import pytest
import torch


@pytest.mark.reference
@pytest.mark.parametrize('fn', T.FNS)
def test_float32_twin_equals_reference(fn):
    """``COptiDICE._train`` of the reference on the `ragged` case, fed the twin's batches: after every step each logged
    scalar, and after the last every parameter, lambda and tau, within 4 x max(e32, 2^-22) of the float32 twin, e32 the
    float32 twin's own error against float64 -- two float32 evaluations of one formula differ by at most the sum of
    their rounding errors; 4 is the factor tests/test_crr_twin.py uses."""
    import ref_harness

    ref_harness.import_reference()
    from gymnasium.spaces import Box
    from omnisafe.algorithms.offline.coptidice import COptiDICE
    from omnisafe.models.actor.actor_builder import ActorBuilder
    from omnisafe.models.offline import ObsEncoder

    run = T.make_run('ragged')
    spaces = Box(-np.inf, np.inf, (run['D'],)), Box(-1.0, 1.0, (run['A'],))
    stub, logged = types.SimpleNamespace(), {}
    stub._actor = ActorBuilder(*spaces, run['hidden']['actor'], run['act'], 'kaiming_uniform').build_actor('gaussian_learning')
    stub._nu_net, stub._chi_net = (ObsEncoder(*spaces, run['hidden'][n], run['act'], 'kaiming_uniform', 1) for n in ('nu', 'chi'))
    for mod, n in ((stub._actor, 'actor'), (stub._nu_net, 'nu'), (stub._chi_net, 'chi')):
        mod.load_state_dict(run[n])
    stub._lamb = torch.nn.Parameter(torch.tensor(T.LAMB0).clamp(0, 1e3))
    stub._tau = torch.nn.Parameter(torch.tensor(T.TAU_INIT) + 1e-6)
    for name, mod, lr in (('_actor', stub._actor.parameters(), 'actor'), ('_nu_net', stub._nu_net.parameters(), 'nu'),
                          ('_chi_net', stub._chi_net.parameters(), 'chi'), ('_lamb', [stub._lamb], 'lamb'),
                          ('_tau', [stub._tau], 'tau')):
        setattr(stub, name + '_optimizer', torch.optim.Adam(mod, lr=T.LR[lr]))
    stub._cfgs = types.SimpleNamespace(algo_cfgs=types.SimpleNamespace(
        gamma=T.GAMMA, alpha=T.ALPHA, cost_ub_eps=T.COST_UB_EPS, cost_limit=T.COST_LIMIT))
    stub._device = torch.device('cpu')
    stub._fn, stub._fn_inv = COptiDICE._get_f_divergence_fn(fn)
    stub.logger = types.SimpleNamespace(store=lambda *a, **kw: logged.update(*a, **kw))
    for name in ('_train', '_update_net', '_update_actor', '_advantage', '_w_sa'):
        setattr(stub, name, types.MethodType(getattr(COptiDICE, name), stub))
    t64, s64, _ = T.twin(run, fn, torch.float64)
    t32, s32, _ = T.twin(run, fn, torch.float32)
    keys = ('Loss/Loss_Nu', 'Loss/Loss_Chi', 'Loss/Loss_Lamb', 'Loss/Loss_Tau', 'Train/CostUB', 'Train/KL_divergence',
            'Train/tau', 'Train/lagrange_multiplier', 'Loss/Loss_actor', 'Train/PolicyStd')
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))  # noqa: E731
    for s in range(T.STEPS):
        d = {k: v[run['idx'][s]] for k, v in run['data'].items()}
        stub._train((d['obs'], d['action'], d['reward'][:, 0], d['cost'][:, 0], d['next_obs'], d['done'][:, 0],
                     d['init_obs']))
        for c, key in enumerate(keys):
            bound = 4 * max(rel(s32[s, c], s64[s, c]), 2.0 ** -22)
            assert rel(float(logged[key]), s32[s, c]) <= bound, (s, key, float(logged[key]), s32[s, c])
    got = {'lambda': stub._lamb.detach().reshape(1).numpy(), 'tau': stub._tau.detach().reshape(1).numpy()}
    for n, mod in (('actor', stub._actor), ('nu', stub._nu_net), ('chi', stub._chi_net)):
        got.update({f'p/{n}/{k}': v.detach().numpy() for k, v in mod.state_dict().items()})
    for q, v in got.items():
        assert rel(v, t32[q]) <= 4 * max(rel(t32[q], t64[q]), 2.0 ** -22), q


def test_load_init_obs(tmp_path):
    """Three episodes: rows 0-2 end by a lane break without ``done``, rows 3-4 by ``done``, rows 5-6 run out."""
    from omnisafe_amd.dice_step import episode_starts, load_init_obs

    obs = np.arange(14, dtype=np.float32).reshape(7, 2)
    next_obs = np.roll(obs, -1, axis=0).copy()
    next_obs[2] = 99.0  # the lane break: obs[3] != next_obs[2]
    done = np.zeros((7, 1), np.float32)
    done[4] = 1.0       # a done row whose next_obs IS the next row's obs
    assert episode_starts(obs, next_obs, done).tolist() == [True, False, False, True, False, True, False]
    data = {k: torch.from_numpy(v) for k, v in (('obs', obs), ('next_obs', next_obs), ('done', done))}
    want = obs[[0, 0, 0, 3, 3, 5, 5]]
    assert np.array_equal(load_init_obs(None, data).numpy(), want)
    for extra, expect in (({}, want), ({'init_obs': obs[::-1].copy()}, obs[::-1])):
        path = str(tmp_path / f'd{len(extra)}.npz')
        np.savez(path, obs=obs, next_obs=next_obs, done=done, **extra)
        assert np.array_equal(load_init_obs(path, data).numpy(), expect)


@pytest.mark.reference
def test_defaults_equal_reference_yaml():
    """config.DICE_DEFAULTS restates configs/offline/COptiDICE.yaml; deviations as for CRR: device, use_tensorboard, the
    `verbose` extension and the (empty) env_cfgs block."""
    import ref_harness

    ref_harness.import_reference()
    from omnisafe.utils.config import get_default_kwargs_yaml

    from omnisafe_amd import config

    def cmp(r, m, path=''):
        for k in r:
            assert k in m, f'missing {path}{k}'
            if isinstance(r[k], dict):
                cmp(r[k], m[k], path + k + '.')
            elif k not in ('device', 'use_tensorboard'):
                assert r[k] == m[k] and type(r[k]) is type(m[k]), f'{path}{k}: reference {r[k]!r}, ours {m[k]!r}'
        for k in m:
            assert k in r or k in ('env_cfgs', 'verbose'), f'extra {path}{k}'

    cmp(get_default_kwargs_yaml('COptiDICE', '', 'offline').todict(), config.default_kwargs('COptiDICE'))
    with pytest.raises(KeyError):
        config.get_default_kwargs('COptiDICE')  # (the lookup the older CPU tests pin keeps to its tables)


def test_registry_and_refusals():
    from omnisafe_amd import algorithms, config, dice_step
    from omnisafe_amd.algorithms import registry

    assert registry.get('COptiDICE') is algorithms.COptiDICE and algorithms.COptiDICE.saved_as == 'actor'
    config.check_all_configs(config.Config.dict2config(dict(config.default_kwargs('COptiDICE'), algo='COptiDICE')))
    nets = lambda v: {n: v for n in T.NETS}  # noqa: E731
    for hidden, act, fn in (([8], 'relu', 'tv'), ([8], 'gelu', 'kl'), ([], 'relu', 'kl'), ([8] * 8, 'relu', 'kl')):
        with pytest.raises(NotImplementedError):
            dice_step.make_desc(3, 1, nets(hidden), nets(act), 4, fn)


@pytest.mark.parametrize('tau', [0.5, 0.05])
def test_chi_gradient_closed_form(tau):
    ell = torch.randn(9, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).requires_grad_()
    (torch.softmax(ell / tau, dim=0) * 9 * ell).mean().backward()
    assert float((ell.grad - T.chi_gradient(ell.detach(), tau)).abs().max()) <= 1e-12
