"""A plain float64 statement of the trust-region and KL half of the update path -- a module, not a test; built on
tests/step_twin.py (its networks, cases, rel_l2 and FLOOR) and used as step_twin is.

What the full-batch kernels compute (osa_actor_kl, osa_actor_eval, osa_fvp_kernel / osa_mb_grad_kernel with loss kind 2
+ osa_fvp_finish, osa_cg_init / osa_cg_step, the gradient-only mode of osa_ppo_minibatch), written the way the
REFERENCE states each quantity, on CPU torch, nothing of the kernels' schedule or algebra:

  old_dist   p_dist = actor(obs): the mean rows and log_std (policy_gradient.py:357, trpo.py:176)
  kl         kl_divergence(Normal_old, Normal_new) through torch.distributions; reduce mode 0 .sum(-1).mean()
             (policy_gradient.py:383-389), mode 1 .mean() over all M x D_a elements (natural_pg.py:95, trpo.py:113)
  evaluate   one candidate of the line search (trpo.py:93-148, cpo.py:106-180) at theta_old + frac step:
             [-mean(ratio adv), mean(ratio adv_c), KL.mean(), mean(ratio)], adv = (adv_r - lam adv_c) / (1 + lam)
  fvp        natural_pg.py:91-119 literally: the DOUBLE BACKWARD of kl(detached, live).mean(), + damping v.  The kernels
             compute J^T diag(1 / sigma^2) J v / (M D_a) by a JVP and a VJP and add the log_std block 2 / D_a
             analytically: another derivation of the same matrix, so an error of that algebra is not shared
  cg         omnisafe/utils/math.py:86-132 literally, the early break included; every iterate x_k is recorded
  cg_step    one iteration's algebra on given vectors
  grad       the full-batch gradient and loss: step_twin.step on all M rows, the actor only, the unclipped gradient

Every function takes `dtype` (the float32 run of the same code is the measuring stick, not a second reference) and an
optional row `order` (the same rows in another order: the same quantity, another summation order).  Flat vectors are in
the reference's parameter order (log_std first), float32 arrays: what the kernels are given, widened afterwards.

`table()` is the case table of tests/test_trust_oracle_gpu.py; `f32_error` what one float32 evaluation loses on every
quantity of an entry (tests/golden/trust_twin_f32_error.json; `python tests/test_trust_twin.py` rewrites it).
For the scalars that are means over the rows it also records the typical size of the sum of the rows' errors (ROWS)
and, for a KL, the first-order size of the error of its log_std part (LS): rows_unit and kl_log_std_unit say why.
"""
from __future__ import annotations

import functools
import math
from collections import OrderedDict

import numpy as np
import torch

import step_twin as T

F32 = np.float32
DAMPING = 0.1
LAMS = (0.37, 0.0)
FRACS = [0.8 ** j for j in range(15)]  # the line search's own step fractions (trpo.py:93-148: decay 0.8, 15 steps)
CG_STEPS = (1, 2, 3, 5, 10, 15)
TARGET_KL = 0.01
EVAL_WHAT = ('loss', 'cost', 'kl', 'ratio')


# ---------------------------------------------------------------------------------------------------------------------
# flat vectors <-> reference tensors
# ---------------------------------------------------------------------------------------------------------------------
def flatten(d) -> np.ndarray:
    return np.concatenate([np.asarray(x).reshape(-1) for x in d.values()])


def split(vec, obs_dim: int, act_dim: int) -> 'OrderedDict[str, np.ndarray]':
    vec, out, o = np.asarray(vec), OrderedDict(), 0
    for k, s in T.tensor_shapes('actor', obs_dim, act_dim).items():
        n = int(np.prod(s))
        out[k] = vec[o:o + n].reshape(s)
        o += n
    assert o == len(vec)
    return out


def num_params(obs_dim: int, act_dim: int) -> int:
    return sum(int(np.prod(s)) for s in T.tensor_shapes('actor', obs_dim, act_dim).values())


def _t(x, dtype) -> torch.Tensor:
    return x.to(dtype) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(dtype)


def _params(case: dict, theta, dtype, grad: bool = False) -> 'OrderedDict[str, torch.Tensor]':
    flat = _t(case['theta'] if theta is None else theta, dtype)
    p, o = OrderedDict(), 0
    for k, s in T.tensor_shapes('actor', case['obs_dim'], case['act_dim']).items():
        n = int(np.prod(s))
        p[k] = flat[o:o + n].reshape(s).clone().requires_grad_(grad)
        o += n
    return p


def _data(case: dict, key: str, dtype, order=None, rows=None) -> torch.Tensor:
    x = np.asarray(case['data'][key])
    x = x if rows is None else x[rows]
    return _t(x if order is None else x[order], dtype)


def _dist(p: dict, obs: torch.Tensor) -> torch.distributions.Normal:
    return torch.distributions.Normal(T._mlp(p, 'mean', obs), torch.exp(p['log_std']))


# ---------------------------------------------------------------------------------------------------------------------
# the quantities
# ---------------------------------------------------------------------------------------------------------------------
def old_dist(case: dict, dtype=torch.float64, order=None, theta=None) -> tuple:
    """-> (mean rows (M, D_a), log_std (D_a,)) of the actor at `theta` (the case's own parameters by default)."""
    with torch.no_grad():
        p = _params(case, theta, dtype)
        return T._mlp(p, 'mean', _data(case, 'obs', dtype, order)), p['log_std']


def kl(case: dict, theta_new, reduce_mode: int, dtype=torch.float64, order=None, theta_old=None,
       per_row: bool = False) -> torch.Tensor:
    """`per_row`: the rows' terms (their mean is the result)."""
    with torch.no_grad():
        mean, log_std = old_dist(case, dtype, order, theta_old)
        old = torch.distributions.Normal(mean, torch.exp(log_std))
        new = _dist(_params(case, theta_new, dtype), _data(case, 'obs', dtype, order))
        k = torch.distributions.kl_divergence(old, new)
        k = k.sum(-1) if reduce_mode == 0 else k.mean(-1)
        return k if per_row else k.mean()


def evaluate(case: dict, theta_old, step, frac: float, lam: float, dtype=torch.float64, order=None,
             per_row: bool = False) -> list:
    """[loss_pi, loss_cost, KL.mean(), mean ratio] of the actor at theta_old + frac step against the one at theta_old.
    `per_row`: the rows' terms of the four means instead."""
    lam, frac = T._f32(lam), T._f32(frac)
    with torch.no_grad():
        theta_new = _t(theta_old, dtype) + frac * _t(step, dtype)
        obs = _data(case, 'obs', dtype, order)
        mean, log_std = old_dist(case, dtype, order, theta_old)
        old = torch.distributions.Normal(mean, torch.exp(log_std))
        new = _dist(_params(case, theta_new, dtype), obs)
        ratio = torch.exp(new.log_prob(_data(case, 'act', dtype, order)).sum(-1) - _data(case, 'logp', dtype, order))
        adv_c = _data(case, 'adv_c', dtype, order)
        adv = (_data(case, 'adv_r', dtype, order) - lam * adv_c) / (1.0 + lam)
        terms = [-(ratio * adv), ratio * adv_c, torch.distributions.kl_divergence(old, new).mean(-1), ratio]
        return terms if per_row else [x.mean() for x in terms]


def fvp(case: dict, v, damping: float, rows=None, dtype=torch.float64, order=None, theta=None) -> torch.Tensor:
    """NaturalPG._fvp on the rows obs[rows] -> the flat product, damping included."""
    obs = _data(case, 'obs', dtype, order, rows)
    params = _params(case, theta, dtype, grad=True)
    q_dist = _dist(params, obs)
    with torch.no_grad():
        p_dist = _dist(params, obs)
    kl_ = torch.distributions.kl.kl_divergence(p_dist, q_dist).mean()
    grads = torch.autograd.grad(kl_, tuple(params.values()), create_graph=True)
    flat_grad_kl = torch.cat([g.view(-1) for g in grads])
    v = _t(v, dtype)
    kl_p = (flat_grad_kl * v).sum()
    grads = torch.autograd.grad(kl_p, tuple(params.values()), retain_graph=False)
    flat_grad_grad_kl = torch.cat([g.contiguous().view(-1) for g in grads])
    return flat_grad_grad_kl + v * T._f32(damping)


def cg(A, b: torch.Tensor, iters: int, residual_tol: float = 1e-10, eps: float = 1e-6) -> tuple:
    """conjugate_gradients of omnisafe/utils/math.py in b's dtype -> ([x_1 ... x_k], (r, p, rdotr, done))."""
    residual_tol, eps = T._f32(residual_tol), T._f32(eps)
    x = torch.zeros_like(b)
    r = b - A(x)
    p = r.clone()
    rdotr = torch.dot(r, r)
    xs, done = [], False
    for _ in range(iters):
        z = A(p)
        alpha = rdotr / (torch.dot(p, z) + eps)
        x = x + alpha * p
        r = r - alpha * z
        xs.append(x.clone())
        new_rdotr = torch.dot(r, r)
        if torch.sqrt(new_rdotr) < residual_tol:
            done = True
            break
        mu = new_rdotr / (rdotr + eps)
        p = r + mu * p
        rdotr = new_rdotr
    return xs, (r, p, rdotr, done)


def cg_step(z, x, r, p, rdotr: float, residual_tol: float, eps: float, r_new=None) -> dict:
    """One iteration of `cg` on given vectors, float64.  `r_new`: take the second half (new r.r, the test, mu, p')
    from this r' instead of the twin's own -- how a kernel's p' is judged on the kernel's r'."""
    z, x, r, p = (np.asarray(a, np.float64) for a in (z, x, r, p))
    residual_tol, eps = T._f32(residual_tol), T._f32(eps)
    alpha = rdotr / (float(p @ z) + eps)
    out = dict(alpha=alpha, x=x + alpha * p, r=r - alpha * z)
    r1 = out['r'] if r_new is None else np.asarray(r_new, np.float64)
    out['new_rdotr'] = float(r1 @ r1)
    out['done'] = bool(math.sqrt(out['new_rdotr']) < residual_tol)
    out['mu'] = out['new_rdotr'] / (rdotr + eps)
    out['p'] = p if out['done'] else r1 + out['mu'] * p
    out['rdotr'] = rdotr if out['done'] else out['new_rdotr']
    return out


def grad(case: dict, lam: float, dtype=torch.float64, order=None) -> dict:
    """step_twin.step on all M rows, the actor only -> its result (loss, the unclipped grads per tensor)."""
    idx = np.arange(case['M']) if order is None else np.asarray(order)
    hp = dict(case['hp'], entropy_coef=0.0)
    return T.step(case['state'], T.rows(case['data'], idx), hp, lam, 1, None, dtype, ('actor',))['actor']


def residual(case: dict, x, b, damping: float, rows=None) -> float:
    """|A64 x - b| / |b| with A64 the float64 product."""
    x64 = np.asarray(x, np.float64)
    return T.rel_l2(fvp(case, x64, damping, rows).detach().numpy(), np.asarray(b, np.float64))


def diag_system(n: int, seed: int = 7) -> tuple:
    """A diagonal operator whose spectrum is two tight clusters (1 and 3, spread 1e-3): CG's residual falls by three
    orders of magnitude at its second iteration -- a done flag whose iteration no rounding can move.  -> (d, b)."""
    rs = np.random.RandomState(seed)
    d = (np.where(rs.rand(n) < 0.5, 1.0, 3.0) + 1e-3 * rs.uniform(-1, 1, n)).astype(F32)
    return d, rs.randn(n).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_case(obs_dim: int, act_dim: int, M: int) -> dict:
    """step_twin.make_case(loss_kind 1, no entropy bonus, one minibatch of all M rows) + the seeded vectors of the
    trust-region quantities: theta (the actor's parameters, flat), v, b = 0.1 randn, a direction."""
    case = T.make_case(obs_dim, act_dim, B=M, M=M, loss_kind=1, entropy_coef=0.0)
    n = num_params(obs_dim, act_dim)
    rs = np.random.RandomState(52300 + 131 * obs_dim + 17 * act_dim + M)
    case['theta'] = flatten(case['state']['params']['actor']).astype(F32)
    case['v'] = rs.randn(n).astype(F32)
    case['b'] = (0.1 * rs.randn(n)).astype(F32)
    case['dir'] = rs.randn(n).astype(F32)
    return case


def _scaled(case: dict, d: np.ndarray, target: float, frac: float = 1.0) -> np.ndarray:
    """d times the float32 factor at which the twin's KL.mean() of theta + frac s d is `target`.  KL is quadratic in s
    to leading order: a few fixed-point steps; where that does not settle (one row through two tanh layers is not
    quadratic), the first crossing is bracketed by doubling s and bisected."""
    at = lambda s: float(kl(case, (case['theta'] + F32(frac * s) * d).astype(F32), 1))  # noqa: E731
    s = 1e-3
    for _ in range(8):
        s *= math.sqrt(target / at(s))
    if abs(at(s) / target - 1) > 1e-3:
        lo, hi = 0.0, 1e-4
        while at(hi) < target:
            lo, hi = hi, 2 * hi
        for _ in range(30):
            s = 0.5 * (lo + hi)
            lo, hi = (s, hi) if at(s) < target else (lo, s)
        s = hi
    return (F32(s) * d).astype(F32)


def kl_thetas(case: dict) -> dict:
    """The two new parameter vectors of the KL cases: 'full' = theta + a step along the case's direction with twin
    KL.mean() = 1e-2; 'mean' = the same with log_std left alone (var_ratio = 1 exactly)."""
    if 'kl_thetas' not in case:
        d_mean = case['dir'].copy()
        d_mean[:case['act_dim']] = 0.0
        case['kl_thetas'] = {kind: (case['theta'] + _scaled(case, d, TARGET_KL)).astype(F32)
                             for kind, d in (('full', case['dir']), ('mean', d_mean))}
    return case['kl_thetas']


def eval_step(case: dict) -> np.ndarray:
    """The line search's step: along the case's direction, KL.mean() = 0.01 at frac 0.8^5.5 (between j = 5 and 6)."""
    if 'eval_step' not in case:
        case['eval_step'] = _scaled(case, case['dir'], TARGET_KL, 0.8 ** 5.5)
    return case['eval_step']


EARLY_STOP = dict(obs_dim=60, act_dim=2, B=64, M=130, seeded_moments=True, t0=(3, 5, 7), lr_actor=3e-4)
EARLY_STOP_ITERS = 4


@functools.lru_cache(maxsize=None)
def early_stop_case() -> dict:
    """PPO's KL early stop: the step_twin case, four seeded permutations, the float64 chain's state and KL (mode 0)
    after each pass, and target_kl = the geometric mean of the KL after passes 2 and 3."""
    case = T.make_case(**EARLY_STOP)
    rs = np.random.RandomState(9130)
    case['perms'] = [rs.permutation(case['M']).astype(np.int64) for _ in range(EARLY_STOP_ITERS)]
    case['theta'] = flatten(case['state']['params']['actor']).astype(F32)
    case['chain'], case['kls'] = early_stop_chain(case)
    case['target_kl'] = math.sqrt(case['kls'][1] * case['kls'][2])
    return case


def early_stop_chain(case: dict, dtype=torch.float64) -> tuple:
    """-> ([(step results, state) per pass], [KL(old || actor after pass i), mode 0])."""
    state, chain, kls = case['state'], [], []
    for perm in case['perms']:
        res, state = T.run_pass(dict(case, perm=perm), dtype, state)
        chain.append((res, state))
        kls.append(float(kl(case, flatten(state['params']['actor']), 0, dtype)))
    return chain, kls


FVP_SHAPES = [(1, 1), (16, 2), (17, 3), (40, 2), (60, 2), (64, 16), (65, 17), (80, 32)]
KL_SHAPES = [(1, 1), (17, 3), (60, 2), (64, 16), (65, 17), (80, 32), (96, 16)]
KL_ROWS = (1, 63, 64, 65, 333)
BIG = 65601  # 1025 tiles of 64 rows + a tile of one row on a grid capped at 1024 workgroups


def table() -> 'OrderedDict[str, dict]':
    """name -> dict(group, obs_dim, act_dim, M, e32 = the entry of the measuring stick it is judged by, options).
    FVP options: max_blocks, fast ('0': OSA_FVP_FAST=0), freq (fvp_sample_freq), damping, kernel (which one must run)."""
    t = OrderedDict()

    def add(group, tag, od, ad, M, e32=None, **opt):
        name = f'{group}{"-" + tag if tag else ""}-{od}x{ad}-M{M}'
        assert name not in t
        t[name] = dict(group=group, obs_dim=od, act_dim=ad, M=M, e32=e32 or name, **opt)
        return name

    # ---- Fisher-vector product.  The fast kernel holds both parameter blocks in LDS: with act_dim > 16 (OT = 2) that
    # fits up to 48 inputs, so 65x17 and 80x32 run on the general kernel; 33x17 (KB 3) is the OT = 2 case of the fast
    # kernel and 80x3 its KB 5 case.
    for od, ad in FVP_SHAPES + [(33, 17), (80, 3)]:
        for M in (65, 333):
            add('fvp', '', od, ad, M, kernel='general' if (od, ad) in ((65, 17), (80, 32)) else 'fast')
    add('fvp', 'blocks3', 60, 2, 333, e32='fvp-60x2-M333', max_blocks=3, kernel='fast')  # 6 chunks on 3 workgroups
    add('fvp', '', 17, 3, 4908, kernel='fast')  # 77 slabs: the reduce's 64-slab loop, one 8-slab step, a tail of 5
    add('fvp', '', 60, 2, 19201, max_blocks=256, kernel='fast')  # 301 chunks, the last of one row
    add('fvp', '', 96, 16, 333, kernel='general')  # KB 6
    add('fvp', '', 60, 2, 64, kernel='general')  # M <= 64
    add('fvp', '', 60, 2, 37, kernel='general')
    add('fvp', 'fast0', 65, 17, 333, e32='fvp-65x17-M333', fast='0', kernel='general')
    add('fvp', 'fast0', 60, 2, 333, e32='fvp-60x2-M333', fast='0', kernel='general')
    add('fvp', 'freq2', 17, 3, 333, freq=2, kernel='fast')  # row stride 34 floats: the scalar row loader
    add('fvp', 'freq3', 60, 2, 333, freq=3, kernel='fast')  # row stride 180 floats: the float4 row loader
    add('fvp', 'damping0', 60, 2, 333, damping=0.0, kernel='fast')
    # ---- the full-batch gradient (gradient-only mode, loss kind 1)
    for od, ad in ((60, 2), (65, 17)):
        for M in (64, 333):
            add('grad', '', od, ad, M)
    add('grad', '', 17, 3, 16421, max_blocks=256)  # 257 chunks
    # ---- snapshot + KL
    for od, ad in KL_SHAPES:
        for M in KL_ROWS:
            add('kl', '', od, ad, M)
    add('kl', '', 60, 2, BIG)
    # ---- the row loader of the KL and eval kernels: (ld, offset of the first element in its buffer)
    add('kl', 'ld64', 60, 2, 333, e32='kl-60x2-M333', ld=64, offset=0)
    add('kl', 'ld19', 17, 3, 333, e32='kl-17x3-M333', ld=19, offset=0)
    add('kl', 'off1', 60, 2, 333, e32='kl-60x2-M333', ld=60, offset=1)
    # ---- the line search's candidates
    for od, ad, M in ((60, 2, 333), (65, 17, 333), (80, 32, 333), (17, 3, BIG), (17, 3, 333)):
        add('eval', '', od, ad, M)
    add('eval', 'ld64', 60, 2, 333, e32='eval-60x2-M333', ld=64, offset=0)
    add('eval', 'ld19', 17, 3, 333, e32='eval-17x3-M333', ld=19, offset=0)
    add('eval', 'off1', 60, 2, 333, e32='eval-60x2-M333', ld=60, offset=1)
    # ---- conjugate gradients
    for od, ad, M in ((60, 2, 333), (17, 3, 1000), (80, 32, 333)):
        add('cg', '', od, ad, M)
    add('cgdone', '', 60, 2, 0)  # the diagonal system on P(60x2): no rows
    t['earlystop-60x2-B64-M130'] = dict(group='earlystop', obs_dim=60, act_dim=2, M=130, e32='earlystop-60x2-B64-M130')
    return t


def entry_case(e: dict) -> dict:
    if e['group'] == 'earlystop':
        return early_stop_case()
    return make_case(e['obs_dim'], e['act_dim'], e['M'] or 333)


def fvp_rows(e: dict):
    return slice(None, None, e['freq']) if e.get('freq', 1) > 1 else None


def check_coverage(name: str, e: dict) -> dict:
    """Asserts, on the CPU, that the entry reaches what it is in the table for.  Returns what it measured."""
    case, g, M = entry_case(e), e['group'], e['M']
    info = {}
    if g == 'fvp':
        n = len(range(M)[fvp_rows(e) or slice(None)])
        chunks = (n + 63) // 64
        info.update(rows=n, chunks=chunks, last=n - 64 * (chunks - 1))
        if e.get('freq', 1) > 1:
            assert n == (M + e['freq'] - 1) // e['freq'] < M
        if name == 'fvp-blocks3-60x2-M333':
            assert chunks == 6 and e['max_blocks'] == 3
        if name == 'fvp-17x3-M4908':
            assert chunks == 77 == 64 + 8 + 5
        if name == 'fvp-60x2-M19201':
            assert chunks == 301 > e['max_blocks'] and info['last'] == 1
        if M in (65, 333):
            assert info['last'] == (1 if n == 65 else n % 64)
        assert (e['kernel'] == 'general') == (n <= 64 or e['obs_dim'] > 80 or e.get('fast') == '0'
                                              or (e['act_dim'] > 16 and e['obs_dim'] > 48))
    elif g == 'grad':
        for lam in LAMS:
            r = grad(case, lam)
            ratio = r['ratio'].numpy()
            assert (ratio < 0.9).sum() >= M // 8 and (ratio > 1.1).sum() >= M // 8  # the ratio matters to the gradient
            assert float(r['gnorm']) > 0.1
        if M == 16421:
            assert (M + 63) // 64 == 257 > e['max_blocks']
    elif g == 'kl':
        th = kl_thetas(case)
        info['kl'] = {kind: float(kl(case, th[kind], 1)) for kind in th}
        assert all(abs(k / TARGET_KL - 1) < 0.05 for k in info['kl'].values()), info
        assert np.array_equal(th['mean'][:e['act_dim']], case['theta'][:e['act_dim']])
        assert not np.array_equal(th['full'][:e['act_dim']], case['theta'][:e['act_dim']])
        if M == BIG:
            assert (M + 63) // 64 == 1026 and M % 64 == 1
    elif g == 'eval':
        step = eval_step(case)
        kls = [float(evaluate(case, case['theta'], step, f, 0.0)[2]) for f in FRACS]
        cross = [j for j in range(14) if kls[j] > TARGET_KL >= kls[j + 1]]
        info.update(kls=kls, cross=cross)
        assert len(cross) == 1 and 3 <= cross[0] < 8, (cross, kls)
        assert all(a > b for a, b in zip(kls, kls[1:]))
    elif g == 'cg':
        A = lambda p: fvp(case, p, DAMPING)  # noqa: E731
        xs, (_, _, _, done) = cg(A, _t(case['b'], torch.float64), max(CG_STEPS))
        assert len(xs) == max(CG_STEPS) and not done
    elif g == 'cgdone':
        d, b, tol = cgdone_system(e)
        d64 = _t(d, torch.float64)
        rs_ = []
        for k in (1, 2, 3):
            xs, (r, _, _, _) = cg(lambda p: d64 * p, _t(b, torch.float64), k)  # noqa: B023
            rs_.append(float(torch.linalg.norm(r)))
        info['residuals'] = rs_
        assert rs_[0] >= 1.5 * tol and rs_[1] <= tol / 1.5, (rs_, tol)
        xs, (_, _, _, done) = cg(lambda p: d64 * p, _t(b, torch.float64), 6, residual_tol=tol)
        assert done and len(xs) == 2
    elif g == 'earlystop':
        kls = case['kls']
        info['kls'] = kls
        assert all(b >= 1.5 * a for a, b in zip(kls, kls[1:])), kls
        # (the threshold sits a factor sqrt(1.5) or more from the KL on either side of it)
        assert case['target_kl'] / kls[1] >= 1.2 and kls[2] / case['target_kl'] >= 1.2
    return info


CGDONE_TOL = 1e-3


def cgdone_system(e: dict) -> tuple:
    """-> (d, b, residual_tol): the diagonal system with b scaled so that the passed tolerance 1e-3 is the geometric
    mean of the twin's |r_1| and |r_2|."""
    d, b = diag_system(num_params(e['obs_dim'], e['act_dim']))
    d64 = _t(d, torch.float64)
    norms = [float(torch.linalg.norm(cg(lambda p: d64 * p, _t(b, torch.float64), k)[1][0])) for k in (1, 2)]
    b = (b * F32(CGDONE_TOL / math.sqrt(norms[0] * norms[1]))).astype(F32)
    return d, b, CGDONE_TOL


# ---------------------------------------------------------------------------------------------------------------------
# the measuring stick
# ---------------------------------------------------------------------------------------------------------------------
ROWS, LS = '#rows', '#ls'


def rows_unit(x32: torch.Tensor, x64: torch.Tensor) -> float:
    """A mean of n terms whose float32 errors are independent from row to row: the typical size of its error is
    rms_rows(x32 - x64) / sqrt n, here relative to |mean(x64)|.  The errors of the rows' terms come from the forward
    pass and do not depend on the order of the rows, so the float32 run's own error of the mean is ONE draw of that
    sum in every row order (anything between nothing and its full spread) -- step_twin.OUT_BIAS_ROWS, for the scalars
    that are means of cancelling terms (the surrogates) or of small differences of forward values (the KL)."""
    d = x32.to(torch.float64) - x64
    return float(torch.sqrt((d * d).mean()) / math.sqrt(len(d)) / x64.mean().abs())


def kl_log_std_unit(ls_old, ls_new, kl_mean: float) -> float:
    """The part of the KL that log_std alone decides, 0.5 (vr - 1 - log vr) per dimension with vr = exp(2 (ls_old -
    ls_new)), is the SAME number in every row: its float32 error does not average over the rows, and the float32 run
    holds one draw of it whatever the row order.  Its typical size, to first order: vr carries four roundings of
    relative size 2^-24 (two exps, the quotient -- squared, so twice), which vr - log vr damps by |1 - 1 / vr|; the
    log is good to an ulp of its own value.  Root sum of squares over the dimensions, relative to KL.mean()."""
    d = 2.0 * (np.asarray(ls_old, np.float64) - np.asarray(ls_new, np.float64))
    vr = np.exp(d)
    err = np.hypot(np.abs(vr - 1.0) * 4 * 2.0 ** -24, np.spacing(np.abs(d).astype(F32)).astype(np.float64))
    return float(np.sqrt((err ** 2).sum()) / (2 * len(d)) / kl_mean)


def _orders(n: int, seed: int) -> list:
    rs = np.random.RandomState(977 + seed)
    return [None] + [rs.permutation(n) for _ in range(T.ROW_ORDERS - 1)]


def _scalar_err(a, b) -> float:
    return T.rel_l2(float(a), float(b))


def f32_error(e: dict) -> tuple:
    """What the float32 run of the twin loses against its float64 run on every quantity of the entry: relative L2 per
    reference tensor (Fv, gradient), relative per scalar (evaluate, kl, the loss), rms over rows and dimensions of
    mean32 - mean64 against the rms of mean64 for the snapshot, rel_l2(x_k^32, x_k^64) per recorded CG iterate.
    Returns (worst over step_twin.ROW_ORDERS row orders, single = the rows as drawn), as step_twin.f32_error does."""
    case, g = entry_case(e), e['group']
    od, ad = e['obs_dim'], e['act_dim']
    worst, single = {}, {}

    def put(errs, order):
        for dst in (worst,) if order is not None else (worst, single):
            for k, v in errs.items():
                dst[k] = max(dst.get(k, 0.0), v)

    f32 = torch.float32
    if g == 'fvp':
        rows, damping = fvp_rows(e), e.get('damping', DAMPING)
        want = split(fvp(case, case['v'], damping, rows).numpy(), od, ad)
        n = len(range(e['M'])[rows or slice(None)])
        for order in _orders(n, 0):
            got = split(fvp(case, case['v'], damping, rows, f32, order).numpy(), od, ad)
            put({k: T.rel_l2(got[k], want[k]) for k in want}, order)
    elif g == 'grad':
        for lam in LAMS:
            want = grad(case, lam)
            for order in _orders(e['M'], 1):
                got = grad(case, lam, f32, order)
                errs = {f'lam{lam:g}/{k}': T.rel_l2(got['grads'][k].numpy(), w.numpy()) for k, w in want['grads'].items()}
                errs[f'lam{lam:g}/loss'] = _scalar_err(got['loss'], want['loss'])
                put(errs, order)
    elif g == 'kl':
        th = kl_thetas(case)
        mean64 = old_dist(case)[0].numpy()
        want = {(kind, m): kl(case, th[kind], m) for kind in th for m in (0, 1)}
        for order in _orders(e['M'], 2):
            m32 = old_dist(case, f32, order)[0].numpy().astype(np.float64)
            m64 = mean64 if order is None else mean64[order]
            errs = {'snapshot': float(np.sqrt(np.mean((m32 - m64) ** 2)) / np.sqrt(np.mean(m64 ** 2)))}
            for (kind, m), w in want.items():
                errs[f'{kind}/mode{m}'] = _scalar_err(kl(case, th[kind], m, f32, order), w)
                r64 = kl(case, th[kind], m, per_row=True)
                errs[f'{kind}/mode{m}{ROWS}'] = rows_unit(kl(case, th[kind], m, f32, order, per_row=True),
                                                          r64 if order is None else r64[order])
                errs[f'{kind}/mode{m}{LS}'] = kl_log_std_unit(case['theta'][:ad], th[kind][:ad], float(kl(case, th[kind], 1)))
            put(errs, order)
    elif g == 'eval':
        step = eval_step(case)
        for lam in LAMS:
            want = [evaluate(case, case['theta'], step, f, lam, per_row=True) for f in FRACS]
            for order in _orders(e['M'], 3):
                errs = {}
                for j, f in enumerate(FRACS):
                    got = evaluate(case, case['theta'], step, f, lam, f32, order, per_row=True)
                    for q, a, b in zip(EVAL_WHAT, got, want[j]):
                        errs[f'lam{lam:g}/j{j}/{q}'] = _scalar_err(a.mean(), b.mean())
                        errs[f'lam{lam:g}/j{j}/{q}{ROWS}'] = rows_unit(a, b if order is None else b[order])
                    new_ls = case['theta'][:ad].astype(np.float64) + T._f32(f) * step[:ad]
                    errs[f'lam{lam:g}/j{j}/kl{LS}'] = kl_log_std_unit(case['theta'][:ad], new_ls, float(want[j][2].mean()))
                put(errs, order)
    elif g == 'cg':
        kmax = max(CG_STEPS)
        want, _ = cg(lambda p: fvp(case, p, DAMPING), _t(case['b'], torch.float64), kmax)
        for order in _orders(e['M'], 4):
            got, _ = cg(lambda p: fvp(case, p, DAMPING, None, f32, order), _t(case['b'], f32), kmax)  # noqa: B023
            errs = {f'k{k}': T.rel_l2(got[k - 1].numpy(), want[k - 1].numpy()) for k in CG_STEPS}
            errs[f'residual{kmax}'] = residual(case, got[kmax - 1].numpy(), case['b'], DAMPING)
            put(errs, order)
    elif g == 'cgdone':
        d, b, _ = cgdone_system(e)
        want, _ = cg(lambda p: _t(d, torch.float64) * p, _t(b, torch.float64), 2)
        got, _ = cg(lambda p: _t(d, f32) * p, _t(b, f32), 2)
        put({f'k{k}': T.rel_l2(got[k - 1].numpy(), want[k - 1].numpy()) for k in (1, 2)}, None)
    elif g == 'earlystop':
        w, s = T.f32_error(case)
        for src, order in ((w, 0), (s, None)):  # (the step's own figures, flattened: step/<net>/<tensor or scalar>)
            flat = {f'step/{net}/{k}': v for net in src for k, v in src[net].items()}
            if order is None:
                single.update(flat)
            else:
                worst.update(flat)
        _, kls32 = early_stop_chain(case, f32)
        put({f'kl{i + 1}': _scalar_err(kls32[i], case['kls'][i]) for i in range(EARLY_STOP_ITERS)}, None)
    return worst, single


def pack_f32_error(table_: dict) -> dict:
    """{entry: (worst, single)} -> {entry: {quantity: [worst, single]}}, three significant digits."""
    return {name: {k: [float(f'{w[k]:.2e}'), float(f'{s[k]:.2e}')] for k in w} for name, (w, s) in table_.items()}


def load_f32_error(path: str) -> tuple:
    """-> (worst, single), each {entry: {quantity: error}}."""
    import json

    blob = json.load(open(path))
    return ({n: {k: v[0] for k, v in d.items()} for n, d in blob.items()},
            {n: {k: v[1] for k, v in d.items()} for n, d in blob.items()})


def measured_entries() -> 'OrderedDict[str, dict]':
    """The entries that own a block of the measuring stick (the others name one of these as their e32)."""
    return OrderedDict((n, e) for n, e in table().items() if e['e32'] == n)
