"""CPU tests of tests/trust_twin.py, the float64 statement of the trust-region and KL quantities the GPU tests of
tests/test_trust_oracle_gpu.py compare the full-batch kernels with.

  * against what already stands: the twin's fvp / cg / kl agree with oracle/np_oracle.py (the reference's own torch
    calls, float32), and its gradient, loss, product and solution with the numbers the unmodified reference recorded
    in tests/golden/trpolag_actor_update.npz (g, loss_before, Fx, x);
  * the structure of the twin's own product: the log_std block is (2 / D_a + damping) v, and u.Fv = v.Fu;
  * every entry of trust_twin.table() reaches what it is in the table for (trust_twin.check_coverage) and the kernel
    its FVP entries name is the one the solver's own selection logic names;
  * the measuring stick tests/golden/trust_twin_f32_error.json reproduces within a factor 2 on a handful of entries.

Bounds against float32 references.  Two float32 evaluations of one formula differ by a few 1e-7 per tensor (measured:
1e-7 ... 3e-7 for the product): 16 x 2^-22 = 3.8e-6, the bound test_step_twin.py uses for the same situation.  CG
amplifies: float32 iterates sit 1e-7 from the float64 ones up to iteration 5 and 1e-6 ... 1e-4 at iteration 15, so the
short solves are held to 3.8e-6 and the 15-step ones to 1e-3.  The recorded x is the reference's float32 15-step
solution.  A KL of 1e-2 per element is a cancelling sum (var_ratio + t^2 - 1 - log var_ratio): float32 loses 1e-6 of it,
bound 1e-4.
"""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'oracle'), HERE):  # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import np_oracle as O  # noqa: E402
import step_twin as T  # noqa: E402
import trust_twin as W  # noqa: E402

ERR_FILE = os.path.join(HERE, 'golden', 'trust_twin_f32_error.json')
TABLE = W.table()
TIGHT = 16 * T.FLOOR
# re-measured here (the whole table: `python tests/test_trust_twin.py`)
REMEASURED = ('fvp-60x2-M333', 'fvp-33x17-M65', 'fvp-freq2-17x3-M333', 'grad-65x17-M64', 'kl-17x3-M65', 'kl-96x16-M333',
              'eval-60x2-M333', 'cg-60x2-M333', 'cgdone-60x2-M0', 'earlystop-60x2-B64-M130')


@pytest.fixture(scope='module', autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)  # (one summation order: the float32 figures below are compared with recorded ones)
    yield
    torch.set_num_threads(n)


def _oracle_actor(case):
    actor = O.Actor(case['obs_dim'], case['act_dim'])
    actor.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32).copy())
                           for k, v in W.split(case['theta'], case['obs_dim'], case['act_dim']).items()})
    return actor


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize('od,ad,M', [(60, 2, 333), (65, 17, 333)])
def test_twin_agrees_with_np_oracle(od, ad, M):
    case = W.make_case(od, ad, M)
    actor = _oracle_actor(case)
    obs, v, b = (torch.from_numpy(x) for x in (case['data']['obs'], case['v'], case['b']))
    got, want = O.fvp(actor, obs, v, cg_damping=0.1).numpy(), W.fvp(case, case['v'], 0.1).numpy()
    for (k, g), w in zip(W.split(got, od, ad).items(), W.split(want, od, ad).values()):
        print('fvp', k, T.rel_l2(g, w))
        assert T.rel_l2(g, w) <= TIGHT, k
    # the subsample: obs[::3] on both sides
    got = O.fvp(actor, obs[::3], v, cg_damping=0.1).numpy()
    assert T.rel_l2(got, W.fvp(case, case['v'], 0.1, slice(None, None, 3)).numpy()) <= TIGHT
    xs, (_, _, _, done) = W.cg(lambda p: W.fvp(case, p, 0.1), torch.from_numpy(case['b'].astype(np.float64)), 15)
    assert not done
    for steps, bound in ((1, TIGHT), (3, TIGHT), (15, 1e-3)):
        x = O.conjugate_gradients(lambda p: O.fvp(actor, obs, p, cg_damping=0.1), b, num_steps=steps).numpy()
        print('cg', steps, T.rel_l2(x, xs[steps - 1].numpy()))
        assert T.rel_l2(x, xs[steps - 1].numpy()) <= bound, steps
    # KL(old || new), mode 0, at the case's two new parameter vectors
    mean, log_std = W.old_dist(case, torch.float32)
    for kind, th in W.kl_thetas(case).items():
        new = O.Actor(od, ad)
        new.load_state_dict({k: torch.from_numpy(np.asarray(x).copy()) for k, x in W.split(th, od, ad).items()})
        got, want = O.kl_old_new(new, obs, mean, torch.exp(log_std)), float(W.kl(case, th, 0))
        print('kl', kind, got, want)
        assert abs(got - want) <= 1e-4 * want, kind
        assert abs(float(W.kl(case, th, 1)) * ad - want) <= 1e-12 * want  # mode 1 is mode 0 / D_a


def test_twin_reproduces_the_recorded_trpolag_update(golden):
    """g, loss_before, Fx and x as the unmodified reference recorded them (float32), at its own inputs."""
    g = golden('trpolag_actor_update.npz')
    od, ad, M = 60, 2, int(g['data/obs'].shape[0])
    params = {net: {k: g[f'init/{net}/{k}'] for k in T.tensor_shapes(net, od, ad)} for net in T.NETS}
    zeros = lambda: {net: {k: np.zeros_like(v) for k, v in params[net].items()} for net in T.NETS}  # noqa: E731
    case = dict(obs_dim=od, act_dim=ad, M=M, hp=dict(T.DEFAULT_HP), theta=W.flatten(params['actor']),
                state={'params': params, 'm': zeros(), 'v': zeros(), 't': dict.fromkeys(T.NETS, 0)},
                data={k[5:]: v for k, v in g.items() if k.startswith('data/') and k != 'data/discounted_ret'})
    lam = float(g['lambda'])
    r = W.grad(case, lam)
    neg_g = np.concatenate([x.numpy().ravel() for x in r['grads'].values()])
    print('g', T.rel_l2(-neg_g, g['g']), 'loss', float(r['loss']), float(g['loss_before']))
    assert T.rel_l2(-neg_g, g['g']) <= TIGHT
    # the loss is a mean of signed terms of size one: an absolute bound at the terms' scale
    assert abs(float(r['loss']) - float(g['loss_before'])) <= 2e-6
    ev = W.evaluate(case, case['theta'], np.zeros_like(case['theta']), 1.0, lam)
    assert abs(float(ev[0]) - float(g['loss_before'])) <= 2e-6 and float(ev[2]) == 0.0
    assert abs(float(ev[0]) - float(r['loss'])) <= 1e-14
    Fx = W.fvp(case, g['x'], 0.1).numpy()
    print('Fx', T.rel_l2(Fx, g['Fx']))
    assert T.rel_l2(Fx, g['Fx']) <= TIGHT
    xs, _ = W.cg(lambda p: W.fvp(case, p, 0.1), torch.from_numpy(g['g'].astype(np.float64)), 15)
    print('x', T.rel_l2(xs[-1].numpy(), g['x']))
    assert T.rel_l2(xs[-1].numpy(), g['x']) <= 1e-3


# ------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize('od,ad,M,damping', [(60, 2, 333, 0.1), (17, 3, 65, 0.0), (33, 17, 65, 0.1)])
def test_structure_of_the_twins_product(od, ad, M, damping):
    case = W.make_case(od, ad, M)
    u, v = case['dir'], case['v']
    Fu, Fv = W.fvp(case, u, damping).numpy(), W.fvp(case, v, damping).numpy()
    d = T._f32(damping)
    ls = (2.0 / ad + d) * v[:ad].astype(np.float64)  # log_std comes first
    assert np.abs(Fv[:ad] - ls).max() <= 1e-13 * np.abs(ls).max()
    uFv, vFu = float(u.astype(np.float64) @ Fv), float(v.astype(np.float64) @ Fu)
    assert abs(uFv - vFu) <= 1e-12 * abs(uFv) and float(v.astype(np.float64) @ Fv) > 0
    # the log_std block is decoupled from the mean network: a vector on log_std alone has no other image
    e = np.zeros_like(v)
    e[:ad] = v[:ad]
    assert np.abs(W.fvp(case, e, damping).numpy()[ad:]).max() <= 1e-15


def test_cg_step_is_one_iteration_of_cg():
    d, b = W.diag_system(300)
    d64, b64 = torch.from_numpy(d.astype(np.float64)), torch.from_numpy(b.astype(np.float64))
    xs, (r, p, rdotr, done) = W.cg(lambda q: d64 * q, b64, 2)
    x0, r0, p0, rr = np.zeros(300), b64.numpy(), b64.numpy(), float(b64 @ b64)
    for _ in range(2):
        s = W.cg_step(d64.numpy() * p0, x0, r0, p0, rr, 1e-10, 1e-6)
        x0, r0, p0, rr = s['x'], s['r'], s['p'], s['rdotr']
    assert not done and not s['done']
    for a, w in ((x0, xs[-1]), (r0, r), (p0, p)):
        assert np.abs(a - w.numpy()).max() <= 1e-12 * np.abs(w.numpy()).max()
    assert abs(rr - float(rdotr)) <= 1e-13 * rr


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('name', list(TABLE))
def test_entry_reaches_what_it_names(name):
    e = TABLE[name]
    info = W.check_coverage(name, e)
    print(name, {k: v for k, v in info.items() if k != 'kls'} or '')
    assert e['e32'] in TABLE and TABLE[e['e32']]['e32'] == e['e32']
    if e['e32'] != name:  # judged by another entry's figures: the same rows, networks and vectors
        o = TABLE[e['e32']]
        assert all(e[k] == o[k] for k in ('group', 'obs_dim', 'act_dim', 'M')) and 'freq' not in e and 'damping' not in e


def test_fvp_entries_name_the_kernel_the_solver_selects(monkeypatch):
    """The host-side restatement of osa_launch_fvp_fast's conditions (trust_region.fvp_kernel_name, the name behind
    profile_events) selects, for every FVP entry, the kernel the entry is in the table for -- and the fast kernel's
    OT = 2 instantiations, KB 1 ... 5 and KB 3 are all among the entries that run it."""
    from omnisafe_amd.models import Layout
    from omnisafe_amd.trust_region import FVP_FAST, FVP_GENERAL, fvp_kernel_name

    seen = set()
    for name, e in TABLE.items():
        if e['group'] != 'fvp':
            continue
        monkeypatch.setenv('OSA_FVP_FAST', e.get('fast', '1'))
        lay = Layout(e['obs_dim'], e['act_dim'], 64)
        n = len(range(e['M'])[W.fvp_rows(e) or slice(None)])
        got = fvp_kernel_name(types.SimpleNamespace(layout=lay, hidden=64, general=False), n)
        assert got == (FVP_FAST if e['kernel'] == 'fast' else FVP_GENERAL), name
        if e['kernel'] == 'fast':
            seen.add((lay.OUTP // 16, lay.KB))
    assert {kb for _, kb in seen} == {1, 2, 3, 4, 5} and {ot for ot, _ in seen} == {1, 2} and (2, 3) in seen


def test_f32_measuring_stick_reproduces():
    """tests/golden/trust_twin_f32_error.json against a fresh measurement, within a factor 2 on max(e32, 2^-22) (below
    that floor an entry never enters a tolerance) -- both recorded figures, as test_step_twin.py holds its file."""
    want = W.load_f32_error(ERR_FILE)
    assert sorted(want[0]) == sorted(W.measured_entries())
    for name in REMEASURED:
        got = W.f32_error(TABLE[name])
        for which, g, w in zip(('worst', 'single'), got, want):
            assert sorted(g) == sorted(w[name]), name
            for k, e in g.items():
                if k.startswith('residual'):  # (a residual, not an error: no floor)
                    assert e <= 2 * w[name][k] and w[name][k] <= 2 * e, (which, name, k, e, w[name][k])
                    continue
                a, b = max(e, T.FLOOR), max(w[name][k], T.FLOOR)
                assert a <= 2 * b and b <= 2 * a, (which, name, k, e, w[name][k])


if __name__ == '__main__':  # writes the measuring stick
    import time

    torch.set_num_threads(1)
    out = {}
    for nm, ent in W.measured_entries().items():
        t0 = time.time()
        out[nm] = W.f32_error(ent)
        print(f'{nm}: {time.time() - t0:.1f} s', flush=True)
    blob = W.pack_f32_error(out)
    with open(ERR_FILE, 'w') as fh:
        fh.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in blob.items()) + '\n}\n')
    print(ERR_FILE, os.path.getsize(ERR_FILE), 'bytes')
