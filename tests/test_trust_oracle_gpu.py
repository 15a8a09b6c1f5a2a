"""The trust-region and KL kernels -- osa_actor_kl, osa_actor_eval, osa_fvp_kernel + osa_fvp_reduce_kernel,
osa_mb_grad_kernel with loss kind 2, osa_fvp_finish, osa_cg_init / osa_cg_step, osa_vec_dot / osa_vec_lincomb and the
gradient-only mode of osa_ppo_minibatch -- against tests/trust_twin.py, the float64 statement of the same quantities
(the Fisher-vector product there is the reference's double backward, not the kernels' JVP -> VJP).

Driven through the product objects: TrustRegionSolver (begin, fvp, conjugate_gradients, dot, lincomb,
evaluate_candidates, actor_loss_grad), PPOUpdater.snapshot_old_distribution / kl / run; osa_cg_step also through the
library with given vectors.  State goes straight into ac.params (test_step_oracle_gpu.Harness.load).  The cases are
trust_twin.table(); tests/test_trust_twin.py asserts on the CPU that each reaches what it names.

Tolerances.  error <= K max(e32, 2^-22), e32 the quantity's entry in tests/golden/trust_twin_f32_error.json (the
float32 run of the twin against its float64 run, worst of four row orders): relative L2 per reference tensor of Fv and of
the gradient, relative per scalar, rms over rows and dimensions for the snapshot's mean, rel_l2 per CG iterate x_k in
the unit of that k.  K = 16, the project's K (the smallest power of two >= twice the worst measured ratio, 5.59: the KL
of kl-96x16-M1 and the log_std gradient of grad-17x3-M16421; profiles/trust_twin_error.md has every case's ratio).  The
15-step CG solution is also held by its float64 residual |A64 x - b| / |b| <= 1.5 x the float32 twin's at the same k
(measured 1.00; x_15 itself 0.69 of its unit).  Element-wise bounds are derived where they are used.

The unit of the KL and line-search scalars is not e32 alone.  Against e32 alone the kernels' worst ratios were 12.4 (the
KL of eval-60x2-M333 at j = 14, where KL.mean() is 2.2e-4) and 12.3 / 9.8 (the surrogate of eval-65x17-M333 at j = 13 and
of eval-80x32-M333 at j = 8, means of signed terms that cancel to 3 % of their size), identical in every layout of the
rows.  Both are the output-bias situation of DESIGN.md section 3.2: the error of such a mean is the sum of its rows'
forward errors, which do not depend on the order of the rows, so the float32 run shows ONE draw of that sum in all four
orders (3.9e-7 where the typical size is 1.7e-6), and the part of the KL that log_std alone decides is the same number
in every row and does not average at all.  The unit of these scalars is therefore max(e32, rms_rows(x32 - x64) / sqrt M
/ |mean|, the first-order size of the log_std part, 2^-22), the second term from the float32 TWIN's rows
(trust_twin.rows_unit), the third from the twin's log_std vectors (trust_twin.kl_log_std_unit), both recorded in the same
file, with the same K; worst ratios in these units 2.90 (surrogate), 1.89 (KL).  The snapshot says where the rows'
errors come from: the kernels' mean rows are up to 2.6 times as far from float64 as float32 torch's (median 1.06;
osa_tanhf on the hardware exp2 / rcp units against libm).

Structure, after every call: the padding entries of every flat vector the solver returns are exactly 0, and ac.params,
adam_m, adam_v, adam_step keep their bits.  No element, row or case is excluded.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import step_twin as T
import test_step_oracle_gpu as S
import trust_twin as W

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K = 16
F32 = np.float32
U = 2.0 ** -24  # unit roundoff of float32
TABLE = W.table()
E32, E32_SINGLE = W.load_f32_error(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                                                'trust_twin_f32_error.json'))
FIGURES = []  # (case, group, what, measured ratio, bound, ratio against the single-order figure or None)


def names(group):
    return [n for n, e in TABLE.items() if e['group'] == group]


@pytest.fixture(scope='module', autouse=True)
def _figures():
    yield
    dst = os.environ.get('OSA_TRUST_TWIN_FIGURES')
    if dst:
        with open(dst, 'w') as fh:
            json.dump(FIGURES, fh)


def judge(name, what, err, failures, key=None, bound=K):
    """err <= bound x unit for the entry's quantity `key` (default: `what`); records the ratio.  unit = max(e32, 2^-22),
    and for the scalars that carry them the two figures of the module docstring (trust_twin.ROWS, trust_twin.LS)."""
    key = key or what
    e32name = TABLE[name]['e32']
    unit = lambda e: max(e[e32name][key], e[e32name].get(key + W.ROWS, 0.0), e[e32name].get(key + W.LS, 0.0), T.FLOOR)  # noqa: E731
    ratio = err / unit(E32)
    FIGURES.append((name, TABLE[name]['group'], what, float(ratio), float(bound), float(err / unit(E32_SINGLE))))
    if not ratio <= bound:
        failures.append((what, 'error / max(e32, 2^-22)', float(ratio)))


def record(name, what, measured, bound):
    FIGURES.append((name, TABLE[name]['group'] if name in TABLE else 'vector', what, float(measured), float(bound), None))


class Rig(S.Harness):
    """The device networks of one case, loaded with its state (Harness.load / read); no updater of its own."""

    def __init__(self, case):  # pylint: disable=super-init-not-called
        from omnisafe_amd import _lib
        from omnisafe_amd.models import ConstraintActorCritic
        from omnisafe_amd.spaces import Box

        self._lib, self.case = _lib, case
        od, ad = case['obs_dim'], case['act_dim']
        self.ac = ac = ConstraintActorCritic(Box(-np.inf, np.inf, (od,)), Box(-1, 1, (ad,)), S.model_cfgs(), 4, device=DEV)
        self.views = [getattr(ac, net) for net in T.NETS]
        self.index = [v._flat_index.cpu().numpy() for v in self.views]
        self.load(case['state'])
        self.real = torch.zeros(ac.layout.P, dtype=torch.bool, device=DEV)
        self.real[ac.actor._flat_index] = True

    def obs(self, ld=None, offset=0):
        """The case's observations on the device: contiguous rows by default, else a view of row stride `ld` that
        starts `offset` floats into its buffer."""
        x = torch.from_numpy(self.case['data']['obs'])
        M, od = x.shape
        ld = ld or od
        buf = torch.full((offset + M * ld + 4,), 7.0, device=DEV)  # (what lies between the rows is not zero)
        view = buf[offset:offset + M * ld].view(M, ld)[:, :od]
        view.copy_(x)
        assert view.stride(0) == ld and (view.data_ptr() - buf.data_ptr()) == 4 * offset
        return view

    def data(self, **obs_kw):
        d = {k: torch.from_numpy(np.ascontiguousarray(self.case['data'][k])).to(DEV) for k in (
            'act', 'logp', 'target_value_r', 'target_value_c', 'adv_r', 'adv_c')}
        d['obs'] = self.obs(**obs_kw)
        return d

    def pad(self, flat):
        return self.ac.actor.pad(torch.from_numpy(np.asarray(flat, F32)))

    def unpad(self, padded):
        return self.ac.actor.unpad(padded).cpu().numpy()

    def set_theta(self, flat):
        self.ac.actor.set_flat_params(torch.from_numpy(np.asarray(flat, F32)))

    def padding_is_zero(self, vec, what):
        assert torch.isfinite(vec).all(), what
        assert bool((vec[~self.real] == 0).all()), (what, 'padding entries moved')

    def state_bits(self):
        ac = self.ac
        return tuple(t.clone() for t in (ac.params, ac.adam_m, ac.adam_v, ac.adam_step))

    def assert_state_kept(self, bits, what):
        for t, was, which in zip(self.state_bits(), bits, ('params', 'adam_m', 'adam_v', 'adam_step')):
            assert torch.equal(t, was), (what, which, 'changed')


def solver(rig, e=None, **kw):
    from omnisafe_amd.trust_region import TrustRegionSolver

    e = e or {}
    return TrustRegionSolver(rig.ac, cg_iters=15, cg_damping=e.get('damping', W.DAMPING),
                             fvp_sample_freq=e.get('freq', 1), max_blocks=e.get('max_blocks', 256), **kw)


def updater(rig, **kw):
    from omnisafe_amd.update import PPOUpdater

    args = dict(batch_size=64, update_iters=1, target_kl=0.02, kl_early_stop=False)
    args.update(kw)
    return PPOUpdater(rig.ac, **args)


def lam_tensor(lam):
    return torch.tensor([lam], dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------
# Fisher-vector product
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fvp_want(e32name):
    e = TABLE[e32name]
    case = W.entry_case(e)
    return W.fvp(case, case['v'], e.get('damping', W.DAMPING), W.fvp_rows(e)).numpy()


@pytest.mark.parametrize('name', names('fvp'))
def test_fvp_against_the_double_backward(monkeypatch, name):
    """Per reference tensor of Fv; which kernel ran (the solver's own naming of its launch); osa_fvp_finish: the raw
    product leaves the log_std block 0 and the result there is fl32(raw + damping v + (2 / D_a) v) to 2 ulp -- two
    multiply-adds on a zero, each rounding once or twice; the padding of Fv is exactly 0."""
    from omnisafe_amd.trust_region import FVP_FAST, FVP_GENERAL

    e = TABLE[name]
    case, od, ad = W.entry_case(e), e['obs_dim'], e['act_dim']
    monkeypatch.setenv('OSA_FVP_FAST', e.get('fast', '1'))
    rig = Rig(case)
    s = solver(rig, e)
    bits = rig.state_bits()
    obs = rig.obs()
    s.begin(obs)
    freq = e.get('freq', 1)
    n = len(range(e['M'])[W.fvp_rows(e) or slice(None)])
    assert s._fvp_obs.shape[0] == n and s._fvp_obs.stride(0) == freq * od
    s.profile_events = []
    v = rig.pad(case['v'])
    Fv = s.fvp(v)
    torch.cuda.synchronize()
    assert [(ev[0], ev[1]) for ev in s.profile_events] == [(FVP_FAST if e['kernel'] == 'fast' else FVP_GENERAL, n)]
    rig.assert_state_kept(bits, 'begin + fvp')
    rig.padding_is_zero(Fv, 'Fv')
    failures = []
    got, want = W.split(rig.unpad(Fv), od, ad), W.split(fvp_want(e['e32']), od, ad)
    for k in want:
        judge(name, k, T.rel_l2(got[k], want[k]), failures)
    # ---- osa_fvp_finish on the log_std block
    lay = rig.ac.layout
    assert float(s._vecs['raw'][lay.oLS:lay.oLS + lay.OUTP].abs().max()) == 0.0
    d, coef = T._f32(e.get('damping', W.DAMPING)), T._f32(2.0 / ad)
    v_ls = case['v'][:ad].astype(np.float64)
    ulp = float((np.abs(got['log_std'] - (d + coef) * v_ls) / S.ulps((d + coef) * v_ls)).max())
    record(name, 'log_std block [ulp]', ulp, 2.0)
    if not ulp <= 2.0:
        failures.append(('log_std block of Fv, ulp', ulp))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# full-batch gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', names('grad'))
def test_full_batch_gradient(name):
    """TrustRegionSolver.actor_loss_grad (gradient-only mode, loss kind 1): the loss and every tensor of the gradient
    against step_twin.step on all M rows, with lam 0.37 and 0."""
    e = TABLE[name]
    case, od, ad = W.entry_case(e), e['obs_dim'], e['act_dim']
    rig = Rig(case)
    s = solver(rig, e)
    data = rig.data()
    failures = []
    for lam in W.LAMS:
        bits = rig.state_bits()
        loss, g = s.actor_loss_grad(data, 'adv_r', 'adv_c', lam_tensor(lam))
        torch.cuda.synchronize()
        rig.assert_state_kept(bits, 'actor_loss_grad')
        rig.padding_is_zero(g, 'gradient')
        want = W.grad(case, lam)
        got = W.split(rig.unpad(g), od, ad)
        for k, w in want['grads'].items():
            judge(name, f'lam{lam:g}/{k}', T.rel_l2(got[k], w.numpy()), failures)
        judge(name, f'lam{lam:g}/loss', T.rel_l2(float(loss), float(want['loss'])), failures)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# snapshot + KL
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kl_want(e32name):
    case = W.entry_case(TABLE[e32name])
    th = W.kl_thetas(case)
    return W.old_dist(case)[0].numpy(), {(kind, m): float(W.kl(case, th[kind], m)) for kind in th for m in (0, 1)}


@pytest.mark.parametrize('name', names('kl'))
def test_snapshot_and_kl(name):
    """Both snapshots (TrustRegionSolver.begin, PPOUpdater.snapshot_old_distribution) against the twin's mean rows;
    PPOUpdater.kl in both reduce modes at the two new parameter vectors of the case (a step with KL.mean() = 1e-2;
    one that leaves log_std alone, var_ratio = 1 exactly)."""
    e = TABLE[name]
    case, ad = W.entry_case(e), e['act_dim']
    rig = Rig(case)
    s, upd = solver(rig), updater(rig)
    obs = rig.obs(e.get('ld'), e.get('offset', 0))
    mean64, want = kl_want(e['e32'])
    bits = rig.state_bits()
    s.begin(obs)
    upd.snapshot_old_distribution(obs)
    torch.cuda.synchronize()
    rig.assert_state_kept(bits, 'snapshots')
    failures = []
    for who, obj in (('solver', s), ('updater', upd)):
        got = obj._old_mean.cpu().numpy().astype(np.float64)
        assert got.shape == mean64.shape
        judge(name, f'snapshot/{who}', float(np.sqrt(np.mean((got - mean64) ** 2)) / np.sqrt(np.mean(mean64 ** 2))),
              failures, key='snapshot')
        ls = obj._old_log_std.cpu().numpy()
        assert np.array_equal(ls[:ad], case['theta'][:ad]) and (ls[ad:] == 0).all()
    for kind, th in W.kl_thetas(case).items():
        rig.set_theta(th)
        bits = rig.state_bits()
        for mode in (0, 1):
            got = float(upd.kl(obs, mode))
            judge(name, f'{kind}/mode{mode}', T.rel_l2(got, want[(kind, mode)]), failures)
        rig.assert_state_kept(bits, 'kl')
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# the line search's candidates
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eval_want(e32name):
    case = W.entry_case(TABLE[e32name])
    step = W.eval_step(case)
    return {lam: np.array([[float(x) for x in W.evaluate(case, case['theta'], step, f, lam)] for f in W.FRACS])
            for lam in W.LAMS}


@pytest.mark.parametrize('name', names('eval'))
def test_evaluate_candidates(name):
    """All 15 x 4 numbers of the line search (fractions 0.8^j of a step whose KL.mean() crosses 0.01 between j = 3
    and j = 8), with lam 0.37 and 0; the actor's parameters keep their bits."""
    e = TABLE[name]
    case = W.entry_case(e)
    rig = Rig(case)
    s = solver(rig)
    data = rig.data(ld=e.get('ld'), offset=e.get('offset', 0))
    s.begin(data['obs'])
    theta, step = rig.pad(case['theta']), rig.pad(W.eval_step(case))
    assert torch.equal(theta, rig.ac.params[0])
    want = eval_want(e['e32'])
    failures = []
    for lam in W.LAMS:
        bits = rig.state_bits()
        res = s.evaluate_candidates(data, theta, step, W.FRACS, 'adv_r', lam_tensor(lam)).numpy()
        rig.assert_state_kept(bits, 'evaluate_candidates')
        assert res.shape == (15, 4)
        for j in range(15):
            for q, what in enumerate(W.EVAL_WHAT):
                judge(name, f'lam{lam:g}/j{j}/{what}', T.rel_l2(float(res[j, q]), want[lam][j, q]), failures)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# conjugate gradients
# ---------------------------------------------------------------------------------------------------------------------
def cg_launch(lib, n, z, x, r, p, scal, tol, eps):
    from omnisafe_amd import _lib

    _lib.check(lib.osa_cg_step(n, _lib.ptr(z), _lib.ptr(x), _lib.ptr(r), _lib.ptr(p), _lib.ptr(scal), tol, eps,
                               _lib.stream_ptr()), 'osa_cg_step')
    torch.cuda.synchronize()


@pytest.mark.parametrize('big_eps', [False, True])
@pytest.mark.parametrize('od,ad', [(60, 2), (80, 32)])
def test_cg_step_one_iteration(od, ad, big_eps):
    """osa_cg_step on given z, x, r, p, rdotr, element by element against trust_twin.cg_step in float64.

    The kernel's alpha = fl(rdotr / fl(fl32(p.z) + eps)): the dot is accumulated in double (exact products, n 2^-53 of
    rounding: nothing), then three float32 roundings, |alpha_k - alpha| <= 3 u |alpha| to first order (u = 2^-24).
    x' = fl(x + fl(alpha_k p)), or the fused form without the inner rounding: one more u |alpha p| and the final
    rounding,  |x'_k - x'| <= spacing(x') / 2 + c u |alpha p|  with c = 3 + 1 = 4; the test takes c = 5 for the terms of
    second order.  r' = r - alpha_k z: the same with |alpha z|.  mu = fl(fl32(r'.r') / fl(rdotr + eps)) on the kernel's
    OWN r' (the twin is given that r': an element of r' moves r'.r' by more than a rounding): three roundings again,
    p' = fl(r' + fl(mu_k p)): spacing(p') / 2 + 5 u |mu p|.  scal[0] = fl32(r'.r') of that r', 1 ulp.

    big_eps: eps = |p.z| -- alpha is rdotr / (p.z + eps), half of what it is without eps."""
    from omnisafe_amd import _lib
    from omnisafe_amd.models import Layout

    lib = _lib.load(require_gpu=True)
    n = Layout(od, ad, 64).P
    rs = np.random.RandomState(31 + od)
    x, r, p = (rs.randn(n).astype(F32) for _ in range(3))
    z = (rs.uniform(0.5, 1.5, n) * p + 0.1 * rs.randn(n)).astype(F32)
    rdotr = float(F32(r.astype(np.float64) @ r))
    pz = float(p.astype(np.float64) @ z)
    assert pz > 0.25 * float(np.abs(p.astype(np.float64) * z).sum())  # no cancellation in the dot
    eps = float(F32(pz)) if big_eps else 1e-6
    want = W.cg_step(z, x, r, p, rdotr, 1e-10, eps)
    assert not want['done']
    if big_eps:
        assert abs(want['alpha'] * 2 * pz / rdotr - 1) < 1e-6
    dz, dx, dr, dp = (torch.from_numpy(a).to(DEV) for a in (z, x, r, p))
    scal = torch.tensor([rdotr, 0, 0, 0], dtype=torch.float32, device=DEV)
    cg_launch(lib, n, dz, dx, dr, dp, scal, 1e-10, eps)
    gx, gr, gp = (a.cpu().numpy().astype(np.float64) for a in (dx, dr, dp))
    assert torch.equal(dz.cpu(), torch.from_numpy(z))
    want_p = W.cg_step(z, x, r, p, rdotr, 1e-10, eps, r_new=gr)
    tag = f'cg_step-P{n}' + ('-eps' if big_eps else '')
    worst = {}
    for what, got, w, move in (('x', gx, want['x'], want['alpha'] * p), ('r', gr, want['r'], want['alpha'] * z),
                               ('p', gp, want_p['p'], want_p['mu'] * p)):
        bound = 0.5 * np.maximum(S.ulps(w), S.ulps(got)) + 5 * U * np.abs(move.astype(np.float64))
        worst[what] = float((np.abs(got - w) / bound).max())
        record(tag, f"{what}' / bound", worst[what], 1.0)
    s0, s1 = (float(t) for t in scal[:2].cpu())
    ulp = abs(s0 - want_p['new_rdotr']) / float(S.ulps(want_p['new_rdotr']))
    record(tag, 'scal[0] [ulp]', ulp, 1.0)
    assert max(worst.values()) <= 1.0 and ulp <= 1.0 and s1 == 0.0, (worst, ulp, s1)


def test_cg_done_flag_on_a_zero_right_hand_side():
    """b = 0: r.r = 0 is below every tolerance after one step -- the flag is set and x is exactly 0."""
    case = W.make_case(60, 2, 333)
    rig = Rig(case)
    s = solver(rig)
    s.begin(rig.obs())
    x = s.conjugate_gradients(torch.zeros(rig.ac.layout.P, device=DEV), num_steps=1)
    assert float(s._scal[1]) == 1.0 and float(x.abs().max()) == 0.0 and torch.isfinite(s._vecs['p']).all()


def test_cg_done_flag_stops_the_solve():
    """The diagonal system of trust_twin.diag_system, residual_tol = 1e-3 between the twin's |r_1| and |r_2| (a factor
    1.5 and more from both, asserted on the CPU): the flag is clear after one step and set after two, four more
    osa_cg_step launches leave x, r, p and the scalars bit-identical, and x is the twin's x_2."""
    name = 'cgdone-60x2-M0'
    e = TABLE[name]
    rig = Rig(W.entry_case(e))
    s = solver(rig)
    d, b, tol = W.cgdone_system(e)
    dd, bb = rig.pad(d), rig.pad(b)

    def product(p, out=None):
        return out.copy_(dd * p)

    s.fvp = product
    state = {}
    for k in (1, 2, 6):
        x = s.conjugate_gradients(bb, num_steps=k, residual_tol=tol)
        state[k] = [x] + [s._vecs[w].clone() for w in ('x', 'r', 'p')] + [s._scal.clone()]
    assert float(state[1][-1][1]) == 0.0 and float(state[2][-1][1]) == 1.0
    assert all(torch.equal(a, c) for a, c in zip(state[2], state[6]))
    rig.padding_is_zero(state[2][0], 'x')
    d64 = torch.from_numpy(d.astype(np.float64))
    xs, (_, _, _, done) = W.cg(lambda p: d64 * p, torch.from_numpy(b.astype(np.float64)), 6, residual_tol=tol)
    assert done and len(xs) == 2
    failures = []
    judge(name, 'k1', T.rel_l2(rig.unpad(state[1][0]), xs[0].numpy()), failures)
    judge(name, 'k2', T.rel_l2(rig.unpad(state[2][0]), xs[1].numpy()), failures)
    assert not failures, failures


@functools.lru_cache(maxsize=None)
def cg_want(e32name):
    case = W.entry_case(TABLE[e32name])
    return W.cg(lambda p: W.fvp(case, p, W.DAMPING), torch.from_numpy(case['b'].astype(np.float64)), max(W.CG_STEPS))[0]


@pytest.mark.parametrize('name', names('cg'))
def test_cg_solve(name):
    """Fresh solves of 1, 2, 3, 5, 10 and 15 steps on b = 0.1 randn with damping 0.1, each against the twin's x_k in the
    unit of that k; the 15-step solution also by its float64 residual."""
    e = TABLE[name]
    case = W.entry_case(e)
    rig = Rig(case)
    s = solver(rig)
    bits = rig.state_bits()
    s.begin(rig.obs())
    b = rig.pad(case['b'])
    xs = cg_want(e['e32'])
    failures = []
    for k in W.CG_STEPS:
        x = s.conjugate_gradients(b, num_steps=k)
        rig.padding_is_zero(x, f'x_{k}')
        assert float(s._scal[1]) == 0.0
        judge(name, f'k{k}', T.rel_l2(rig.unpad(x), xs[k - 1].numpy()), failures)
    rig.assert_state_kept(bits, 'conjugate_gradients')
    kmax = max(W.CG_STEPS)
    res, unit = W.residual(case, rig.unpad(x), case['b'], W.DAMPING), E32[e['e32']][f'residual{kmax}']
    record(name, f'float64 residual at k = {kmax} / the float32 twin\'s', res / unit, 1.5)
    if not res <= 1.5 * unit:
        failures.append(('float64 residual of x_15', res, unit))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# dot, lincomb
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 1024, 1025, 'P(80x32)'])
def test_dot_and_lincomb(n):
    """dot: the kernel sums exact products in double and rounds once -- 1 ulp of the float32 result against the float64
    dot (half an ulp + the double sum's own n 2^-53).  lincomb: out = fl(fl(a x) + fl(b y)), or with one product fused
    into the add: |err| <= spacing(out) / 2 + u (|a x| + |b y|) -- one ulp of the output where the two terms do not
    cancel; with y = None out = fl(a x) exactly (a x + 0)."""
    from omnisafe_amd.models import Layout

    n = Layout(80, 32, 64).P if n == 'P(80x32)' else n
    rig = Rig(W.make_case(1, 1, 1))
    s = solver(rig)
    rs = np.random.RandomState(n)
    x, y = rs.randn(n).astype(F32), rs.randn(n).astype(F32)
    dx, dy = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    for a, c, w in ((dx, dy, x64 @ y64), (dx, dx, x64 @ x64)):
        got = float(s.dot(a, c))
        ulp = abs(got - w) / float(S.ulps(w))
        record(f'dot-n{n}', 'dot [ulp]', ulp, 1.0)
        assert ulp <= 1.0, (got, w)
    a, b = 0.8 ** 3, -1.7
    a32, b32 = T._f32(a), T._f32(b)
    got = s.lincomb(a, dx, b, dy).cpu().numpy().astype(np.float64)
    want = a32 * x64 + b32 * y64
    bound = 0.5 * np.maximum(S.ulps(want), S.ulps(got)) + U * (np.abs(a32 * x64) + np.abs(b32 * y64))
    worst = float((np.abs(got - want) / bound).max())
    record(f'lincomb-n{n}', 'a x + b y / bound', worst, 1.0)
    assert worst <= 1.0
    got = s.lincomb(a, dx).cpu().numpy()
    assert np.array_equal(got, (a32 * x64).astype(F32))
    out = torch.full((n,), 3.0, device=DEV)
    assert s.lincomb(-1.0, dx, out=out) is out and np.array_equal(out.cpu().numpy(), -x)


# ---------------------------------------------------------------------------------------------------------------------
# PPO's KL early stop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('early_stop', [True, False])
@pytest.mark.parametrize('persistent', [True, False])
def test_kl_early_stop(persistent, early_stop):
    """PPOUpdater(kl_early_stop, update_iters = 4) on 60x2, B = 64, M = 130 with injected permutations and target_kl =
    the geometric mean of the twin's KL after passes 2 and 3 (the KL rises by a factor 1.5 and more per pass: asserted
    on the CPU): run stops after pass 3 -- stop_iter, out['kl'] and the parameters are those after exactly three passes
    (the chain tolerances of test_step_oracle_gpu); without early stop all four passes run."""
    name = 'earlystop-60x2-B64-M130'
    case = W.entry_case(TABLE[name])
    h = S.Harness(case, 'persistent' if persistent else 'per-step')
    hp = case['hp']
    upd = updater(h, batch_size=case['B'], update_iters=W.EARLY_STOP_ITERS, target_kl=case['target_kl'],
                  kl_early_stop=early_stop, clip=hp['clip'], entropy_coef=hp['entropy_coef'],
                  use_critic_norm=bool(hp['use_critic_norm']), critic_norm_coef=hp['critic_norm_coef'],
                  use_max_grad_norm=bool(hp['use_max_grad_norm']), max_grad_norm=hp['max_grad_norm'],
                  loss_kind=case['loss_kind'], persistent=persistent)
    h.load(case['state'])
    before = h.read()
    perms = [torch.from_numpy(p).to(DEV) for p in case['perms']]
    out = upd.run(h.data, h.lam, perms=perms, actor_lr=hp['lr_actor'], critic_lr=hp['lr_critic'])
    torch.cuda.synchronize()
    assert upd.last_path == h.last_path
    passes = 3 if early_stop else W.EARLY_STOP_ITERS
    assert out['stop_iter'] == passes, (out['stop_iter'], out['kl'], case['kls'], case['target_kl'])
    nmb = len(T.minibatches(case['M'], case['B']))
    assert out['steps'] == passes * nmb
    final = h.read()
    S.check_structure(h, before, final, passes * nmb)
    failures = []
    judge(name, f'kl{passes}', T.rel_l2(out['kl'], case['kls'][passes - 1]), failures)
    e32 = {}
    for k, v in E32[name].items():
        if k.startswith('step/'):
            _, net, what = k.split('/', 2)
            e32.setdefault(net, {})[what] = v
    chain = [r for res, _ in case['chain'][:passes] for r in res]
    mark = len(S.FIGURES)
    S.check_final_state(name, upd.last_path, h.nets, chain, e32, final, failures)
    FIGURES.extend((name, 'earlystop', f'{f[1]}: {f[3]} {f[4]}', f[5], f[6], None) for f in S.FIGURES[mark:])
    assert not failures, failures
