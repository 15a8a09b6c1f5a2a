"""CPU tests of tests/step_twin.py, the float64 statement of one optimiser step the GPU tests of
tests/test_step_oracle_gpu.py compare the 64-row step kernels with.

  * against the REFERENCE: the float64 twin, chained over the recorded permutations, reproduces the per-step losses,
    mean ratios and entropies the unmodified reference logged during `_update()` -- tests/golden/ppolag_epoch.npz (9 steps)
    and the FOCOPS (mask inactive and partially active), CUP (both stages) and P3O goldens (6 steps each) -- and
    agrees with oracle/np_oracle.py's actor_step / critic_step (the reference's own torch calls) at the golden's
    inputs: YAML defaults, a norm clip that bites, a non-zero entropy bonus.  This ties the twin to the real
    reference, not to this project's reading of it;
  * the coverage conditions of step_twin.make_case hold for every case of the GPU table -- and of form_table(), the
    table of tests/test_step_forms_gpu.py, where they include that a scaled first layer does not saturate, that the
    named ragged tails leave the named chunk workgroups empty and that the shapes select the forms they are listed for;
  * the cases of case_table() keep the entries of the measuring stick they had before form_table() joined the file;
  * the ragged tail of a pass is the step of its rows as a minibatch of their own;
  * the measuring stick tests/golden/step_twin_f32_error.json (float32 run against float64 run of the same code, per
    case, network and tensor) reproduces within a factor 2;
  * general networks (step_twin.general_table(), the table of tests/test_general_step_gpu.py): the default cases did
    not move by a bit, the activations are torch.nn's, every case meets its coverage conditions (ReLU kink distance,
    Softplus and Sigmoid saturation counts included), osa_gmlp_plan shows for every case the launch features it is
    named for and for the table as a whole every mechanism and the listed instantiations of gm_gemm_kernel, and
    tests/golden/general_twin_f32_error.json reproduces.

Tolerances against the float32 reference: a logged scalar is a mean over <= 64 float32 terms after ~200-term dot
products: relative error a few 1e-7 of the terms' scale (not of a mean that may cancel), hence rtol 2e-6 with an atol of
2e-6 x the scale of one term (|A| ~ 1, targets ~ 1).  Later steps inherit the earlier ones' parameter differences:
Adam's first steps move every parameter by ~lr whatever its gradient, so the handful of entries whose float32
gradient has another sign than the float64 one differ by 2 lr = 6e-4 -- entries with |g| < 1e-7, whose effect on a loss
is below 1e-10.  The same holds for the clipped gradients compared through np_oracle's optimizer state.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'oracle'), HERE):  # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import np_oracle as O  # noqa: E402
import step_twin as T  # noqa: E402

ERR_FILE = os.path.join(HERE, 'golden', 'step_twin_f32_error.json')
TABLE = T.case_table()
FORM_TABLE = T.form_table()  # the forms beyond one 64-row workgroup per network (tests/test_step_forms_gpu.py)
CASES = dict(TABLE, **{name: e['kw'] for name, e in FORM_TABLE.items()})
RTOL, ATOL = 2e-6, 2e-6
# sha256 of the measuring stick's entries for case_table(), as they stood before form_table() was added to the file
NARROW_E32_SHA256 = '9e8ff14f4dbb9ff74d5aef64304c90645c71e6629dd5eabb2748713761d1da71'


@pytest.fixture(scope='module', autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)  # (one summation order: the float32 figures below are compared with recorded ones)
    yield
    torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------------ reference goldens
def _golden_state(g, prefix='init/'):
    params = {net: {k: g[f'{prefix}{net}/{k}'] for k in T.tensor_shapes(net, 60, 2)} for net in T.NETS}
    zeros = lambda: {net: {k: np.zeros_like(v) for k, v in params[net].items()} for net in T.NETS}  # noqa: E731
    return {'params': params, 'm': zeros(), 'v': zeros(), 't': dict.fromkeys(T.NETS, 0)}


def _ppolag_data(g):
    a_r, a_c, _ = O.buffer_get(g['buffer/adv_r'], g['buffer/adv_c'])
    d = {k: O.env_major(g[f'buffer/{k}']) for k in ('obs', 'act', 'logp', 'target_value_r', 'target_value_c')}
    d.update(adv_r=a_r, adv_c=a_c)
    return d


def _chain(state, data, perms, hp, lam, loss_kind, ext=None, nets=T.NETS, B=64):
    """Passes over `perms` from `state` -> ([per-step results], final state)."""
    res = []
    for perm in perms:
        for s, n in T.minibatches(len(perm), B):
            res.append(T.step(state, T.rows(data, perm[s:s + n]), hp, lam, loss_kind, ext, nets=nets))
            state = T.advance(state, res[-1])
    return res, state


def _close(mine, want, what, scale=1.0):
    mine, want = np.asarray([float(x) for x in mine]), np.asarray(want, np.float64)
    print(what, 'max |diff|', np.abs(mine - want).max(), 'max rel', (np.abs(mine - want) / np.abs(want)).max())
    np.testing.assert_allclose(mine, want, rtol=RTOL, atol=ATOL * scale, err_msg=what)


def test_twin_reproduces_the_reference_ppolag_update(golden):
    g = golden('ppolag_epoch.npz')
    res, final = _chain(_golden_state(g), _ppolag_data(g), g['update/perms'], {}, float(g['update/lambda_after']), 0)
    assert len(res) == 9
    _close([r['actor']['loss'] for r in res], g['update/loss_pi'], 'loss_pi')
    _close([r['reward_critic']['loss'] for r in res], g['update/loss_r'], 'loss_r', scale=4.0)
    _close([r['cost_critic']['loss'] for r in res], g['update/loss_c'], 'loss_c', scale=4.0)
    _close([r['actor']['ratio_mean'] for r in res], g['update/ratio_mean'], 'ratio_mean')
    _close([r['actor']['entropy'] for r in res], g['update/entropy'], 'entropy')
    # parameters after the nine steps: all but the sign-flipped entries of the first steps (see the module docstring)
    for net in T.NETS:
        for k, v in final['params'][net].items():
            d = np.abs(v.numpy() - g[f'post/{net}/{k}'])
            assert np.median(d) < 2e-7 and (d > 5e-6).mean() < 0.01, (net, k, np.median(d), d.max())


ORACLE_CONFIGS = {'defaults': {}, 'norm-clip': dict(max_grad_norm=0.05), 'entropy': dict(entropy_coef=0.02)}


@pytest.mark.parametrize('cfg', sorted(ORACLE_CONFIGS))
def test_twin_agrees_with_np_oracle_steps(golden, cfg):
    """np_oracle.actor_step / critic_step are the reference's own torch calls (float32).  Compared: the losses, the
    CLIPPED gradient read from the optimizer's first moment (exp_avg = (1 - b1) g after one step from zero), and the
    parameters against the twin's Adam formula evaluated on the oracle's own moments."""
    g = golden('ppolag_epoch.npz')
    hp = ORACLE_CONFIGS[cfg]
    lam = 0.37
    data = _ppolag_data(g)
    idx = g['update/perms'][0][:64]
    state = _golden_state(g)
    r = T.step(state, T.rows(data, idx), hp, lam, 0)
    ac = O.ActorCritic(60, 2)
    for net in T.NETS:
        getattr(ac, net).load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state['params'][net].items()})
    t = {k: torch.from_numpy(np.ascontiguousarray(v[idx])) for k, v in data.items()}
    mg = hp.get('max_grad_norm', 40.0)
    loss_r = O.critic_step(ac.reward_critic, ac.reward_critic_optimizer, t['obs'], t['target_value_r'], max_grad_norm=mg)
    loss_c = O.critic_step(ac.cost_critic, ac.cost_critic_optimizer, t['obs'], t['target_value_c'], max_grad_norm=mg)
    loss_pi, ent, ratio = O.actor_step(ac.actor, ac.actor_optimizer, t['obs'], t['act'], t['logp'], t['adv_r'],
                                       t['adv_c'], lam, entropy_coef=hp.get('entropy_coef', 0.0), max_grad_norm=mg)
    _close([r['reward_critic']['loss'], r['cost_critic']['loss'], r['actor']['loss'], r['actor']['entropy'],
            r['actor']['ratio_mean']], [loss_r, loss_c, loss_pi, ent, float(ratio.mean())], cfg, scale=4.0)
    if cfg == 'norm-clip':
        assert all(float(r[net]['coef']) < 0.5 for net in T.NETS)
    for net, opt in (('actor', ac.actor_optimizer), ('reward_critic', ac.reward_critic_optimizer),
                     ('cost_critic', ac.cost_critic_optimizer)):
        for (k, w0), w in zip(state['params'][net].items(), getattr(ac, net).parameters()):
            st = opt.state[w]
            g_ref = st['exp_avg'].double().numpy() / (1.0 - 0.9)
            g_twin = (r[net]['grads'][k] * r[net]['coef']).numpy()
            e = T.rel_l2(g_ref, g_twin)
            print(cfg, net, k, 'clipped gradient rel l2', e)
            assert e <= 16 * T.FLOOR, (net, k, e)  # two float32 evaluations of the same formula: 16 x 2^-22 = 4e-6
            # Adam on the oracle's own moments: half an ulp of p for the final rounding, a dozen float32 roundings of
            # the update term (torch's bias corrections, sqrt, addcdiv)
            ss, ib = T.bias_corrections(3e-4, 0.9, 0.999, 1)
            delta = ss * st['exp_avg'].double() / (torch.sqrt(st['exp_avg_sq'].double()) * ib + 1e-8)
            want = torch.from_numpy(w0.astype(np.float64)) - delta
            bound = np.spacing(np.abs(w0)).astype(np.float64) + 2e-6 * np.abs(delta.numpy())
            assert (np.abs(w.detach().double().numpy() - want.numpy()) <= bound).all(), (net, k)


def _sibling(g, tag):
    state = _golden_state(g)
    data = {k[5:]: v for k, v in g.items() if k.startswith('data/') and k != 'data/discounted_ret'}
    with torch.no_grad():
        p = {k: torch.from_numpy(v.astype(np.float64)) for k, v in state['params']['actor'].items()}
        data['old_mean'] = T._mlp(p, 'mean', torch.from_numpy(data['obs'].astype(np.float64))).numpy()
    data['old_log_std'] = state['params']['actor']['log_std'].astype(np.float64)
    return state, data


@pytest.mark.parametrize('tag,eta', [('focops', 0.02), ('focops_masked', 1e-4)])
def test_twin_reproduces_the_reference_focops_update(golden, tag, eta):
    """focops.py:98-108 with the Lagrangian advantage; the behaviour policy is the actor at the start of the update.
    focops_masked: the trust mask is partially active from the second step on."""
    g = golden(f'sibling_{tag}.npz')
    state, data = _sibling(g, tag)
    ext = dict(kl_coef=1.0, kl_mask_eta=eta, ratio_scale=1.0 / 1.5)
    res, _ = _chain(state, data, g['perms'], {}, float(g['lambda_after']), 1, ext)
    masked = [int((r['actor']['mask'] == 0).sum()) for r in res]
    print(tag, 'rows outside the trust region per step', masked)
    assert (max(masked) > 0) == (tag == 'focops_masked')
    _close([r['actor']['loss'] for r in res], g['log/Loss/Loss_pi'], 'loss_pi')
    _close([r['actor']['entropy'] for r in res], g['log/Train/Entropy'], 'entropy')
    _close([r['actor']['ratio_mean'] for r in res], g['log/Train/PolicyRatio'], 'ratio')
    _close([r['reward_critic']['loss'] for r in res], g['log/Loss/Loss_reward_critic'], 'loss_r', scale=4.0)
    _close([r['cost_critic']['loss'] for r in res], g['log/Loss/Loss_cost_critic'], 'loss_c', scale=4.0)


def test_twin_reproduces_the_reference_p3o_update(golden):
    """p3o.py:76-84, 112-114: PPO's clipped loss on adv_r plus kappa relu(mean(r adv_c) + Jc - limit)."""
    g = golden('sibling_p3o.npz')
    state, data = _sibling(g, 'p3o')
    ext = dict(cost_kappa=2.0, cost_excess=float(g['Jc']) - 1.0)
    res, _ = _chain(state, data, g['perms'], {}, 0.0, 0, ext)
    _close([r['actor']['loss'] for r in res], g['log/Loss/Loss_pi'], 'loss_pi')
    _close([r['actor']['penalty'] for r in res], g['log/Loss/Loss_pi_cost'], 'loss_pi_cost', scale=2.0)
    _close([r['actor']['ratio_mean'] for r in res], g['log/Train/PolicyRatio'], 'ratio')
    assert all(float(r['actor']['penalty']) > 0 for r in res)


def test_twin_reproduces_the_reference_cup_update(golden):
    """cup.py: stage one is PPO on adv_r (two passes, all three networks); stage two, actor only, minimises
    lambda coef r adv_c + KL(pi_theta || pi_stage1) -- here loss_kind 1 on adv = -(lambda coef) adv_c."""
    g = golden('sibling_cup.npz')
    state, data = _sibling(g, 'cup')
    res1, state = _chain(state, data, g['perms'][:2], {}, 0.0, 0)
    _close([r['actor']['loss'] for r in res1], g['log/Loss/Loss_pi'], 'loss_pi')
    _close([r['reward_critic']['loss'] for r in res1], g['log/Loss/Loss_reward_critic'], 'loss_r', scale=4.0)
    coef = (1 - 0.99 * 0.95) / (1 - 0.99)
    lam = float(g['lambda_after'])
    stage2 = dict(data)
    stage2['adv_r'] = (data['adv_c'] * np.float32(-(lam * coef))).astype(np.float32)
    with torch.no_grad():
        p = {k: v.double() for k, v in state['params']['actor'].items()}
        stage2['old_mean'] = T._mlp(p, 'mean', torch.from_numpy(data['obs'].astype(np.float64))).numpy()
        stage2['old_log_std'] = p['log_std'].numpy()
    res2, _ = _chain(state, stage2, g['perms'][2:], {}, 0.0, 1, dict(kl_coef=1.0), nets=('actor',))
    _close([r['actor']['loss'] for r in res2], g['log/Loss/Loss_pi_c'], 'loss_pi_c', scale=0.1)
    _close([r['actor']['ratio_mean'] for r in res2], g['log/Train/SecondStepPolicyRatio'], 'second-step ratio')
    _close([r['actor']['entropy'] for r in res2], g['log/Train/SecondStepEntropy'], 'second-step entropy')


# ------------------------------------------------------------------------------------------------ the table's cases
@pytest.fixture(scope='module')
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = T.make_case(**CASES[name])
        return cache[name]

    return get


def test_table_shapes_are_on_the_narrow_pass():
    """osa_ppo_pass_supported decides (host-side logic of the library): a shape it refuses would leave the table."""
    from omnisafe_amd import _lib

    lib = _lib.load()
    for od, ad in T.SHAPES + T.EXT_SHAPES:
        assert lib.osa_ppo_pass_supported(od, ad, 64) == 1, (od, ad)


def test_form_table_shapes_select_their_forms():
    """The host-side conditions of PPOUpdater.run's selection, per family of form_table(): the chunked and large-batch
    cases sit on shapes of the narrow pass with 64 < B <= 1024 / B >= 2048, the wide cases on shapes it refuses and
    both wide kernels take, with B <= 64.  (That the device then accepts the form is asserted on the GPU.)"""
    from omnisafe_amd import _lib

    lib = _lib.load()
    assert not set(FORM_TABLE) & set(TABLE)
    for name, e in FORM_TABLE.items():
        kw = e['kw']
        od, ad, B = kw['obs_dim'], kw['act_dim'], kw['B']
        assert set(e['paths']) <= set(T.FORMS), name
        narrow = lib.osa_ppo_pass_supported(od, ad, 64) == 1
        if set(e['paths']) & {'wide', 'split', 'split-spread'}:
            assert not narrow and B <= 64 and set(e['paths']) <= {'wide', 'split', 'split-spread'}, name
            assert lib.osa_ppo_wide_pass_supported(od, ad, 64) == 1 and lib.osa_ppo_split_pass_supported(od, ad, 64) == 1
            assert kw['w1_scale'] == (64.0 / od) ** 0.5
        elif set(e['paths']) & {'balanced', 'strided'}:
            assert narrow and B >= 2048 and set(e['paths']) <= {'balanced', 'strided'}, name
        else:
            assert narrow and 64 < B <= 1024 and set(e['paths']) <= {'per-step', 'chunked'}, name
            assert kw.get('ext') is None or e['paths'] == ('per-step',), name


@pytest.mark.parametrize('name', list(CASES))
def test_case_reaches_its_branches(cases, name):
    case = cases(name)
    info = T.check_coverage(case)
    print(name, info)
    if name in FORM_TABLE and 'tail' in FORM_TABLE[name]:
        # the ragged tail the entry names: its rows, and the 64-row chunk workgroups of the chunked pass it leaves empty
        rows, empty = FORM_TABLE[name]['tail']
        n = T.minibatches(case['M'], case['B'])[-1][1]
        assert (n, T.empty_chunks(case['B'], n)) == (rows, empty), (name, n, T.empty_chunks(case['B'], n))


def test_narrow_cases_keep_their_measuring_stick():
    """form_table()'s cases were ADDED to tests/golden/step_twin_f32_error.json: every case of case_table() still maps,
    network by network, to the figures it had (w1_scale = 1 leaves make_case's numbers and streams where they were)."""
    import hashlib

    blob = json.load(open(ERR_FILE))
    old = {name: {net: blob['blocks'][b] for net, b in sorted(blob['cases'][name].items())} for name in TABLE}
    digest = hashlib.sha256(json.dumps([blob['keys'], old], sort_keys=True).encode()).hexdigest()
    assert digest == NARROW_E32_SHA256


def test_ragged_tail_is_a_minibatch_of_its_own(cases):
    """The last step of a pass with M % B != 0 averages over its n = M % B rows: the reward critic's MSE and its
    output-bias gradient 2/n sum(v - target), written out here by hand, not through step()."""
    for name in ('mb-B64-M65-60x2', 'mb-B64-M127-65x17', 'mb-B5-M12-60x2'):
        case = cases(name)
        res, _ = T.run_pass(case)
        state = case['state']
        for r in res[:-1]:
            state = T.advance(state, r)
        s, n = T.minibatches(case['M'], case['B'])[-1]
        assert 0 < n < case['B'] and n == case['M'] % case['B']
        tail = case['perm'][s:]
        v = T._mlp({k: torch.as_tensor(np.asarray(w)).double() for k, w in state['params']['reward_critic'].items()},
                   'critic_0', torch.from_numpy(case['data']['obs'][tail].astype(np.float64)))[:, 0]
        tgt = torch.from_numpy(case['data']['target_value_r'][tail].astype(np.float64))
        last = res[-1]['reward_critic']
        assert abs(float(last['mse']) - float(((v - tgt) ** 2).sum() / n)) < 1e-12
        # (the L2 term adds 2 c b to the bias gradient)
        c, b3 = T._f32(case['hp']['critic_norm_coef']), float(np.asarray(state['params']['reward_critic']['critic_0.4.bias'])[0])
        want = float(2.0 * (v - tgt).sum() / n) + 2.0 * c * b3
        assert abs(float(last['grads']['critic_0.4.bias']) - want) < 1e-12 * max(1.0, abs(want))


def test_f32_measuring_stick_reproduces(cases):
    """tests/golden/step_twin_f32_error.json against a fresh measurement: within a factor 2, on the quantity the GPU
    tests use -- max(e32, 2^-22); below that floor an entry never enters a tolerance.  Held for both recorded figures,
    the worst of ROW_ORDERS row orders (the GPU tests' unit) and the single run with the rows as drawn.
    (`python tests/test_step_twin.py` rewrites the file.)"""
    want = T.load_f32_error(ERR_FILE)
    assert sorted(want[0]) == sorted(CASES)
    for name in CASES:
        got = T.f32_error(cases(name))
        for which, g, w in zip(('worst', 'single'), got, want):
            assert sorted(g) == sorted(w[name]), name
            for net in g:
                assert sorted(g[net]) == sorted(w[name][net]), (name, net)
                for k, e in g[net].items():
                    a, b = max(e, T.FLOOR), max(w[name][net][k], T.FLOOR)
                    assert a <= 2 * b and b <= 2 * a, (which, name, net, k, e, w[name][net][k])


# ------------------------------------------------------------------------------- general networks (general_table())
GENERAL = T.general_table()
GENERAL_ERR_FILE = os.path.join(HERE, 'golden', 'general_twin_f32_error.json')
# inputs and float64 gradients of four default cases as the twin produced them before it learned general networks
DEFAULT_CASES_SHA256 = '4dcc1cbfec348bcfd0853281ba14ad13c3035506defd219228f77664c898c974'
# The instantiations (TM, TN, BK, AT, BT) of gm_gemm_kernel that general_table() launches: 15 of the 24.  The other nine:
#   (64, 64, 16, *)      three: unreachable by shape.  K step 16 needs 256 workgroups of 64 x 64 tiles while the 128-wide
#                        tiles were refused for giving fewer than 128; a 64 x 64 grid has at most twice the workgroups of
#                        the 128 x 64 grid that was refused (OSA_GMLP_DEEP=0 forces it: a once-per-process switch)
#   (64, 128, *, NT/NN)  four: row tiles of 64 mean a minibatch of at most 64 rows on the tiled step, and then 128
#                        workgroups need a layer of 5 400 outputs (inputs, for NN): past the cost limits of the table
#   (128, 64, 16, NT), (128, 64, 16 | 64, NN)   column tiles of 64 with row tiles of 128 on the minibatch's rows:
#                        (128, 64, 64, NN) is in the table (a 64-wide layer under a 512-wide one at 700 rows); K step 16
#                        needs 256 workgroups = 10 900 rows
COVERED_KERNELS = {(64, 64, 64, 0, 0), (64, 64, 64, 0, 1), (64, 64, 64, 1, 1), (64, 128, 16, 1, 1), (64, 128, 64, 1, 1),
                   (128, 64, 16, 1, 1), (128, 64, 64, 0, 0), (128, 64, 64, 0, 1), (128, 64, 64, 1, 1), (128, 128, 16, 0, 0),
                   (128, 128, 16, 0, 1), (128, 128, 16, 1, 1), (128, 128, 64, 0, 0), (128, 128, 64, 0, 1), (128, 128, 64, 1, 1)}
# what the table as a whole must reach, from osa_gmlp_plan
REQUIRED_FEATURES = {'skinny', 'tiled', 'fusedn', 'no-fusedn', 'top-in-fwd:all', 'top-in-fwd:critics', 'loss-fused',
                     'loss-plain', 'tk2', 'S1', 'S2', 'row-split-off', 'rowS4', 'rowS8', 'Si<S', 'TM128', 'TN128',
                     'TM128xTN128', 'BK16', 'BK64', 'NT', 'NN', 'TN'}


@pytest.fixture(scope='module')
def general_cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = T.make_case(**GENERAL[name]['kw'])
        return cache[name]

    return get


def test_default_cases_did_not_move():
    """actor_hidden / critic_hidden / the activations at their defaults: the cases of case_table() and form_table()
    number for number -- parameters, moments, data, permutation, hyper-parameters, float64 gradients."""
    import hashlib

    h = hashlib.sha256()
    for kw in (dict(obs_dim=60, act_dim=2),
               dict(obs_dim=65, act_dim=17, B=48, M=100, norm_clip=(1, 0.5), seeded_moments=True, t0=(3, 5, 7)),
               dict(obs_dim=28, act_dim=8, update_critics=False, loss_kind=1, ext=T.FOCOPS, trust=True),
               dict(obs_dim=376, act_dim=17, w1_scale=(64 / 376) ** 0.5)):
        c = T.make_case(**kw)
        for net in T.NETS:
            for w in ('params', 'm', 'v'):
                for k, a in c['state'][w][net].items():
                    h.update(k.encode())
                    h.update(np.ascontiguousarray(a).tobytes())
        for k in sorted(c['data']):
            h.update(k.encode())
            h.update(np.ascontiguousarray(c['data'][k]).tobytes())
        h.update(c['perm'].tobytes())
        h.update(repr(sorted(c['hp'].items())).encode())
        r = T.case_step(c, c['state'], 0)
        for net in r:
            for g in r[net]['grads'].values():
                h.update(g.numpy().tobytes())
    assert h.hexdigest() == DEFAULT_CASES_SHA256


def test_activations_are_the_reference_modules():
    """step_twin._ACT against torch.nn's modules of the same names (utils/model.py get_activation), float64, on a grid
    that crosses Softplus's threshold of 20 and ReLU's kink."""
    z = torch.linspace(-30.0, 30.0, 2401, dtype=torch.float64)
    mods = dict(tanh=torch.nn.Tanh(), relu=torch.nn.ReLU(), sigmoid=torch.nn.Sigmoid(), softplus=torch.nn.Softplus(),
                identity=torch.nn.Identity())
    assert tuple(mods) == T.ACTIVATIONS
    for kind, m in mods.items():
        assert torch.equal(T._ACT[kind](z), m(z)), kind


@pytest.mark.parametrize('name', list(GENERAL))
def test_general_case_reaches_its_branches(general_cases, name):
    """check_coverage: the clip cells, trust mask, P3O sign and norm-clip conditions of the 64-row table, and the
    conditions on the hidden pre-activations (step_twin.activation_coverage: no ReLU unit at the kink, Softplus above
    20 and below -3, saturated Sigmoid units) -- conditions on the inputs, not tolerances."""
    case = general_cases(name)
    info = T.check_coverage(case)
    print(name, {k: v for k, v in info.items() if k != 'cells'})
    kinds = {T.case_act(case, net) for net in T.case_nets(case) if T.case_hidden(case, net)}
    assert ('relu_margin' in info) == ('relu' in kinds)
    if case.get('z_shift') is not None:
        assert ('softplus' in info) == ('softplus' in kinds) and ('sigmoid' in info) == ('sigmoid' in kinds)
        assert 'softplus' in info or 'sigmoid' in info


@pytest.mark.parametrize('name', list(GENERAL))
def test_general_case_launches_what_it_is_named_for(general_cases, name, monkeypatch):
    """osa_gmlp_plan -- the launchers' own decision functions, walked without a launch -- names every feature the case
    is in the table for.  The once-per-process switches are left alone: every variant is reached by shape."""
    for key, value in GENERAL[name]['env'].items():
        monkeypatch.setenv(key, value)
    case = general_cases(name)
    plan = T.gmlp_plan(case)
    got = T.plan_features(plan)
    print(name, sorted(got))
    assert got >= set(GENERAL[name]['features']), (name, sorted(set(GENERAL[name]['features']) - got))
    assert plan['skinny'] == (case['B'] <= 64 and not GENERAL[name]['env'])
    # modes 1 and 2 never take the Gram-formula norm; every minibatch of the pass stays on the case's step
    for mode in (1, 2):
        assert not T.gmlp_plan(case, mode=mode)['fusedn']
    for _, n in T.minibatches(case['M'], case['B']):
        assert T.gmlp_plan(case, rows=n)['skinny'] == (n <= 64 and not GENERAL[name]['env'])


def test_general_table_reaches_every_mechanism(general_cases):
    """Over the whole table: every feature of the launch plan, the instantiations of gm_gemm_kernel listed above, and
    the shapes the plan does not show (rows, depths, widths, observation rows, activations)."""
    feats, kernels = set(), set()
    for name, e in GENERAL.items():
        if e['env']:
            continue
        plan = T.gmlp_plan(general_cases(name))
        feats |= T.plan_features(plan)
        kernels |= T.plan_kernels(plan)
    assert feats >= REQUIRED_FEATURES, sorted(REQUIRED_FEATURES - feats)
    assert kernels == COVERED_KERNELS, (sorted(kernels - COVERED_KERNELS), sorted(COVERED_KERNELS - kernels))
    cases = [general_cases(name) for name in GENERAL]
    skinny = [c for c in cases if c['B'] <= 64]
    rows = {n for c in skinny for _, n in T.minibatches(c['M'], c['B'])}
    assert rows >= {1, 3, 37, 64}, sorted(rows)
    assert {c['B'] for c in cases} >= {65, 255, 256, 257, 300}
    assert {c['act_dim'] for c in skinny} >= {2, 8, 9, 32, 33}
    assert {c['obs_dim'] for c in skinny} >= {1, 61, 376}
    depths = {len(T.case_hidden(c, net)) for c in skinny for net in T.NETS}
    assert depths >= {0, 1, 2, 3, 7}, depths
    assert any(T.case_hidden(c, 'actor') == [] and T.case_hidden(c, 'reward_critic') != [] for c in skinny)
    widths = {w for c in skinny for net in T.NETS for w in T.case_hidden(c, net)}
    assert widths >= {1, 4, 7, 9, 17, 20, 30, 50, 65, 1040}, sorted(widths)
    for net in ('actor', 'reward_critic'):
        assert {T.case_act(c, net) for c in skinny} == set(T.ACTIVATIONS)
    assert any(T.case_act(c, 'actor') != T.case_act(c, 'reward_critic')
               and T.case_hidden(c, 'actor') != T.case_hidden(c, 'reward_critic') for c in skinny)
    # 1040 only as one thin layer: no weight matrix beyond 1040 x 512
    for c in cases:
        for net in T.NETS:
            sizes = [c['obs_dim']] + T.case_hidden(c, net)
            assert all(a * b <= 1040 * 512 for a, b in zip(sizes, sizes[1:])), (sizes,)
    # the uneven split: 300 rows in two slices of whole K steps
    plan = T.gmlp_plan(general_cases('tl-B300'))
    q = [x for x in plan['launches'] if x['AT']][0]
    kper = -(-(-(-300 // q['splits'])) // q['BK']) * q['BK']
    assert q['splits'] == 2 and 0 < 300 - kper < kper


def test_general_measuring_stick_reproduces(general_cases):
    """tests/golden/general_twin_f32_error.json (tools/step_twin_report.py --general-golden) against a fresh
    measurement, as test_f32_measuring_stick_reproduces holds the 64-row file: within a factor 2 on max(e32, 2^-22)."""
    want = T.load_general_error(GENERAL_ERR_FILE)
    assert sorted(want[0]) == sorted(GENERAL)
    for name in GENERAL:
        got = T.f32_error(general_cases(name))
        for which, g, w in zip(('worst', 'single'), got, want):
            assert sorted(g) == sorted(w[name]), name
            for net in g:
                assert sorted(g[net]) == sorted(w[name][net]), (name, net)
                assert T.out_bias(general_cases(name)) + '/rows' in g[net] or net == 'actor'
                for k, e in g[net].items():
                    a, b = max(e, T.FLOOR), max(w[name][net][k], T.FLOOR)
                    assert a <= 2 * b and b <= 2 * a, (which, name, net, k, e, w[name][net][k])


if __name__ == '__main__':  # writes the measuring stick (`--forms`: keeps case_table()'s entries as recorded, adds form_table()'s)
    torch.set_num_threads(1)
    if '--forms' in sys.argv:
        old = T.load_f32_error(ERR_FILE)
        table = {nm: (old[0][nm], old[1][nm]) for nm in TABLE}
        table.update((nm, T.f32_error(T.make_case(**e['kw']))) for nm, e in FORM_TABLE.items())
        blob = T.pack_f32_error(table)
    else:
        blob = T.pack_f32_error({nm: T.f32_error(T.make_case(**kw)) for nm, kw in CASES.items()})
    with open(ERR_FILE, 'w') as fh:
        fh.write('{"keys": ' + json.dumps(blob['keys']) + ',\n"blocks": [\n'
                 + ',\n'.join(json.dumps(b) for b in blob['blocks']) + '],\n"cases": {\n'
                 + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in blob['cases'].items()) + '}}\n')
    print(ERR_FILE, os.path.getsize(ERR_FILE), 'bytes', len(blob['blocks']), 'blocks')
