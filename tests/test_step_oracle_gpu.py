"""The 64-row optimiser step -- csrc/ppo_pass_body.h through osa_ppo_pass_ext, and its per-step twin osa_mb_grad_kernel
through osa_ppo_minibatch_ext -- against tests/step_twin.py, the float64 statement of the same step, on every branch
of the losses, the norm clip and Adam.  (The bit-pin files test_pass_trim_gpu.py / test_pass_stall_trim_gpu.py prove
that the step did not change; this file says whether it is right.)

Every case of step_twin.case_table() runs on both paths: PPOUpdater(persistent=False) -> 'per-step',
PPOUpdater(persistent=True) -> 'persistent'.  State is written straight into ac.params / adam_m / adam_v / adam_step.

How a step is observed -- never through Adam's division:
  gradient    from ZERO moments one step leaves m' = (1 - b1) g: g_kernel = m' / (1 - b1) is the clipped gradient to
              float32 rounding, for EVERY minibatch of the pass (each launched on its own from the case's initial
              state, the ragged tail included).  With the gradient-norm column of the statistics row the clip factor is
              |g_kernel| / norm and the unclipped gradient g_kernel / factor.  v' must be (1 - b2) g_kernel^2 to 4 ulp
              (moments fed another gradient than the parameters).
  moments     a case with seeded moments takes g_kernel from its zero-moment twin case (same inputs, same kernel,
              and the kernels reproduce themselves bit for bit): m', v' must be the float64 recurrences on g_kernel to
              2 ulp -- of the larger of the result and its operands, the recurrence for m subtracts; the
              (1 - b2) g_kernel^2 of v' as the twin case wrote it (squaring m' / (1 - b1) again costs 2 ulp by itself).
  parameters  p' against the float64 Adam formula on the kernel's OWN m', v' and the case's t: half an ulp of p for the
              final rounding + fewer than ten float32 roundings and two 1-ulp hardware approximations (sqrt, rcp) on
              the update D = p' - p:  |p'_kernel - p'_64| <= spacing(|p|) + 2e-6 |D|.
  bias corr.  the pass writes lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) to columns 10..15 of every step's statistics row:
              the float64 values rounded to float32, 1 ulp -- on the one-step passes and on every step of the chained one.
  chains      seeded moments only (Adam is well conditioned there): per step launch the twin advances in float64 from
              the kernel's state read back before the launch; the persistent pass is compared -- statistics rows of
              every step, final state (parameters element by element) -- with the twin's own float64 chain.

Tolerances.  Per network and reference tensor rel_l2(g_kernel, g_64) <= K_GRAD max(e32, 2^-22) with e32 that tensor's
entry in tests/golden/step_twin_f32_error.json (the float32 run of the twin against its float64 run, worst of four
orders of the minibatch's rows -- step_twin.f32_error says why; the single-order figures are recorded next to them and
profiles/step_twin_error.md states the worst ratios against both); the same form with K_SCALAR for the losses, mean
ratio, entropy, sum p^2, gradient norm, clip factor and penalty.  The kernels are another float32 evaluation of the
formula (MFMA summation order, hardware exp2 / rcp / sqrt): their error is of the order of e32, not equal to it.
K = the smallest power of two >= twice the worst ratio measured on the MI355X over the whole table
(profiles/step_twin_error.md has it per case and tensor):

    K_GRAD   = 16   worst measured ratio 5.01: the reward critic's second hidden bias, mb-B48-M100-65x17, per-step
    K_SCALAR = 16   worst measured ratio 6.62: the reward critic's MSE, mb-B64-M65-60x2

One tensor's unit is not its own e32 alone: a critic's output bias, a single number, 2/n sum_rows (v - target) + the
L2 term.  Where the residuals cancel (sum|x| / |sum x| = 99 in mb-B48-M100-65x17) the kernels miss it by 173 x 2^-22
against an e32 of 21 x 2^-22.  Measured row by row: the float64 sum over the kernel's own
forward values reproduces that figure, the forward values are off by 1.14e-7 rms (float32 torch: 0.84e-7; the
kernels' share is osa_tanhf on the hardware exp2 / rcp units, 4.8e-8 rms per activation against libm's 2.2e-8), and a
sum of 48 such errors is typically 86 x 2^-22 of this gradient -- e32 was a favourable draw.  Its unit is therefore
max(e32, (2 / sqrt n) rms_rows(v32 - v64) / |g_64|, 2^-22), the second term from the float32 TWIN's forward values
(step_twin.OUT_BIAS_ROWS), with the same K_GRAD; worst measured ratio in these units 4.48 (base-1x1; mb-B48-M100-65x17: 1.80).

No element is excluded anywhere.  Structure, in every case: padding entries of params / adam_m / adam_v stay exactly 0,
networks outside the mask keep their bits, adam_step advances by the number of steps for the networks in the mask only.
"""
import ctypes as C
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import step_twin as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K_GRAD, K_SCALAR = 16, 16

TABLE = T.case_table()
PATHS = ('per-step', 'persistent')
# (the cases of step_twin.form_table() too: tests/test_step_forms_gpu.py runs them through the checks of this file)
CASES = dict(TABLE, **{_name: _e['kw'] for _name, _e in T.form_table().items()})
NSTAT = 16
E32, E32_SINGLE = T.load_f32_error(
    os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_twin_f32_error.json'))
F32 = np.float32
OMB1 = float(F32(1) - F32(0.9))  # the kernels' 1.f - beta1, 1.f - beta2
OMB2 = float(F32(1) - F32(0.999))
B1, B2 = float(F32(0.9)), float(F32(0.999))
# statistics columns: (actor, reward critic, cost critic)
COL = {'actor': dict(loss=2, ratio_mean=3, entropy=4, gnorm=7, penalty=10),
       'reward_critic': dict(mse=0, psq=5, gnorm=8), 'cost_critic': dict(mse=1, psq=6, gnorm=9)}
FIGURES = []  # (case, path, kind, net, what, measured, bound): written out when OSA_STEP_TWIN_FIGURES names a file


def record(case, path, kind, net, what, measured, bound, single=None):
    """`single`: the same error in units of the single-order float32 figure (reported, never asserted)."""
    FIGURES.append((case, path, kind, net, what, float(measured), float(bound), None if single is None else float(single)))


def unit(e32, net, what):
    """max(e32, 2^-22) of a tensor or scalar; for a critic's one-element output bias e32 is the larger of the
    tensor's own figure and the typical size of the sum of its rows' forward errors (step_twin.OUT_BIAS_ROWS)."""
    u = max(e32[net][what], T.FLOOR)
    rows = e32[net].get(what + '/rows') if net != 'actor' else None  # (T.OUT_BIAS_ROWS where the critics are [64, 64])
    return u if rows is None else max(u, rows)


def check_bias_columns(h, kind, stats, t_after, failures):
    """The pass's tabulated bias corrections, columns 10..15: float32(lr / (1 - b1^t)), float32(1 / sqrt(1 - b2^t)), 1 ulp."""
    for net in h.nets:
        lr = float(F32(h.case['hp']['lr_actor' if net == 'actor' else 'lr_critic']))
        i = T.NETS.index(net)
        for col, want in zip((10 + 2 * i, 11 + 2 * i), T.bias_corrections(lr, B1, B2, t_after[net])):
            if col == 10 and (h.case['ext'] or {}).get('cost_kappa', 0) > 0:
                continue  # (the penalty's column)
            if not abs(float(stats[col]) - float(F32(want))) <= ulps(want):
                failures.append((kind, net, 'bias-correction column', col, float(stats[col]), want))


@pytest.fixture(scope='module', autouse=True)
def _figures():
    yield
    dst = os.environ.get('OSA_STEP_TWIN_FIGURES')
    if dst:
        with open(dst, 'w') as fh:
            json.dump(FIGURES, fh)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case, its zero-moment twin and their float64 results -- computed once, shared by both paths."""
    torch.set_num_threads(1)
    kw = CASES[name]
    case = T.make_case(**kw)
    zero = T.make_case(**T.zero_moment_twin(kw)) if case['seeded_moments'] else case
    nmb = len(T.minibatches(case['M'], case['B']))
    ref = dict(case=case, zero=zero, first=[T.case_step(zero, zero['state'], k) for k in range(nmb)])
    if case['seeded_moments']:
        ref['chain'] = T.run_pass(case)[0]
    return ref


def model_cfgs(case=None):
    """[64, 64] tanh networks, or those a case of step_twin.general_table() names."""
    ns = types.SimpleNamespace
    case = case or {}
    return ns(actor=ns(hidden_sizes=T.case_hidden(case, 'actor'), activation=T.case_act(case, 'actor'), lr=3e-4),
              critic=ns(hidden_sizes=T.case_hidden(case, 'reward_critic'), activation=T.case_act(case, 'reward_critic'), lr=3e-4),
              weight_initialization_mode='kaiming_uniform', actor_type='gaussian_learning', linear_lr_decay=True)


class Harness:
    """One case on one path: the device networks, the data, the updater.  What depends on the path sits in form()
    and launch_step(); tests/test_step_forms_gpu.py overrides the two for the other forms of the step."""

    def form(self):
        """-> (PPOUpdater's persistent flag, the last_path run() must report, whether the form writes the
        bias-correction columns 10..15, whether a pass is ONE launch -- compared with the twin's float64 chain)."""
        assert self._lib.load(require_gpu=True).osa_ppo_pass_supported(self.case['obs_dim'], self.case['act_dim'], 64) == 1
        persistent = self.path == 'persistent'
        return persistent, self.path, persistent, persistent

    def __init__(self, case, path):
        from omnisafe_amd import _lib
        from omnisafe_amd.models import ConstraintActorCritic, SurrogateExt
        from omnisafe_amd.spaces import Box
        from omnisafe_amd.update import PPOUpdater

        self._lib = _lib
        self.case, self.path = case, path
        od, ad, M = case['obs_dim'], case['act_dim'], case['M']
        persistent, self.last_path, self.bias_columns, self.one_launch = self.form()
        self.ac = ac = ConstraintActorCritic(Box(-np.inf, np.inf, (od,)), Box(-1, 1, (ad,)), model_cfgs(case), 4, device=DEV)
        self.views = [getattr(ac, net) for net in T.NETS]
        self.index = [v._flat_index.cpu().numpy() for v in self.views]
        d = case['data']
        obs = torch.zeros(M, (od + 3) // 4 * 4, device=DEV)  # rows of whole float4s
        obs[:, :od] = torch.from_numpy(d['obs'])
        self.data = {k: torch.from_numpy(np.ascontiguousarray(d[k])).to(DEV) for k in (
            'act', 'logp', 'target_value_r', 'target_value_c', 'adv_r', 'adv_c')}
        self.data['obs'] = obs[:, :od]
        self.perm = torch.from_numpy(case['perm']).to(DEV)
        self.lam = torch.tensor([case['lam']], dtype=torch.float32, device=DEV)
        hp, e = case['hp'], case['ext']
        ext = None if e is None else SurrogateExt(**e)
        self.upd = upd = PPOUpdater(
            ac, batch_size=case['B'], update_iters=1, target_kl=0.02, kl_early_stop=False, clip=hp['clip'],
            entropy_coef=hp['entropy_coef'], use_critic_norm=bool(hp['use_critic_norm']),
            critic_norm_coef=hp['critic_norm_coef'], use_max_grad_norm=bool(hp['use_max_grad_norm']),
            max_grad_norm=hp['max_grad_norm'], use_cost=case['use_cost'], loss_kind=case['loss_kind'],
            update_actor=case['update_actor'], persistent=persistent,
            update_critics=case['update_critics'], ext=ext)
        upd.hp.lr_actor, upd.hp.lr_critic = hp['lr_actor'], hp['lr_critic']
        if ext is not None:  # the PRESCRIBED behaviour policy, not a snapshot of the actor
            upd._old_mean = torch.from_numpy(d['old_mean']).to(DEV).contiguous()
            upd._old_log_std[:ad] = torch.from_numpy(d['old_log_std']).to(DEV)
            upd.snapshot_old_distribution = lambda obs: None
        self.mask = upd._nets_mask()
        self.nets = T.case_nets(case)
        assert [n for i, n in enumerate(T.NETS) if (self.mask >> i) & 1] == list(self.nets)

    # ---- state in, state out
    def load(self, state):
        ac = self.ac
        for i, (net, view) in enumerate(zip(T.NETS, self.views)):
            view.load_state_dict({k: torch.from_numpy(np.asarray(v, F32)) for k, v in state['params'][net].items()})
            for which, blk in (('m', ac.adam_m), ('v', ac.adam_v)):
                flat = torch.cat([torch.from_numpy(np.asarray(v, F32)).reshape(-1) for v in state[which][net].values()])
                blk[i] = view.pad(flat)
        ac.adam_step.copy_(torch.tensor([state['t'][net] for net in T.NETS], dtype=torch.int32))

    def read(self):
        ac = self.ac
        blocks = {'params': ac.params.cpu().numpy(), 'm': ac.adam_m.cpu().numpy(), 'v': ac.adam_v.cpu().numpy()}
        st = {k: {} for k in blocks}
        for i, net in enumerate(T.NETS):
            for which, blk in blocks.items():
                flat, o, d = blk[i][self.index[i]], 0, {}
                for k, s in T.case_shapes(self.case, net).items():
                    n = int(np.prod(s))
                    d[k] = flat[o:o + n].reshape(s).copy()
                    o += n
                st[which][net] = d
        st['t'] = dict(zip(T.NETS, (int(x) for x in ac.adam_step.cpu())))
        st['blocks'] = blocks
        return st

    # ---- launches
    def one_step(self, state, k):
        """Minibatch k of the pass as one launch from `state` -> (state before, state after, statistics row)."""
        self.load(state)
        before = self.read()
        stats = self.launch_step(k)
        return before, self.read(), stats

    def launch_step(self, k):
        """Launches minibatch k on the state the device holds -> its statistics row."""
        upd, lib = self.upd, self._lib
        s, n = T.minibatches(self.case['M'], self.case['B'])[k]
        idx = self.perm[s:s + n]
        stats = torch.zeros(1, NSTAT, device=DEV)
        if self.path == 'per-step':
            upd.minibatch(self.data, idx, n, self.lam, stats[0])
        else:  # a pass of one (possibly ragged) step over these rows
            ext = None
            if upd.ext is not None:
                upd.ext.old_mean, upd.ext.ld_old_mean = upd._old_mean.data_ptr(), upd._old_mean.stride(0)
                upd.ext.old_log_std = upd._old_log_std.data_ptr()
                ext = C.byref(upd.ext)
            lib.check(upd.lib.osa_ppo_pass_ext(
                *upd._operands(self.data, idx, n, self.case['B']), lib.ptr(self.lam), C.byref(upd.hp), upd.loss_kind,
                self.mask, lib.ptr(stats), ext, lib.stream_ptr()), 'osa_ppo_pass_ext')
        torch.cuda.synchronize()
        return stats[0].cpu().numpy()

    def whole_pass(self, state):
        self.load(state)
        before = self.read()
        hp = self.case['hp']
        out = self.upd.run(self.data, self.lam, perms=[self.perm], actor_lr=hp['lr_actor'], critic_lr=hp['lr_critic'])
        torch.cuda.synchronize()
        assert self.upd.last_path == self.last_path, (self.upd.last_path, self.last_path)
        return before, self.read(), out['stats'].cpu().numpy()


def ulps(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)


def f64(d):
    return {k: np.asarray(v, np.float64) for k, v in d.items()}


def check_structure(h, before, after, steps):
    """Padding stays 0, networks outside the mask keep their bits, adam_step advances for the masked networks only."""
    for i, net in enumerate(T.NETS):
        real = np.zeros(after['blocks']['params'].shape[1], bool)
        real[h.index[i]] = True
        for which, blk in after['blocks'].items():
            assert not np.isnan(blk[i]).any(), (net, which)
            assert (blk[i][~real] == 0).all(), (net, which, 'padding moved')
            if net not in h.nets:
                assert np.array_equal(blk[i], before['blocks'][which][i]), (net, which, 'outside the mask')
        assert after['t'][net] == before['t'][net] + (steps if net in h.nets else 0), (net, after['t'], before['t'])


def check_scalars(name, path, kind, r, stats, e32, failures, case=None, e32_single=None):
    """Statistics row against the twin: |x_kernel - x_64| <= K_SCALAR max(e32, 2^-22) |x_64|.
    (`case`, `e32_single`: of a case from another table than this file's -- tests/test_dp_forms_gpu.py.)"""
    case = reference(name)['case'] if case is None else case
    e32_single = E32_SINGLE[name] if e32_single is None else e32_single
    for net, res in r.items():
        for what, col in COL[net].items():
            if what == 'penalty' and not (case['ext'] or {}).get('cost_kappa', 0) > 0:
                continue
            if what == 'psq' and not case['hp']['use_critic_norm']:
                continue  # (nothing reads sum p^2 without the L2 term)
            want = float(res[what])
            err = T.rel_l2(float(stats[col]), want)
            u = unit(e32, net, what)
            record(name, path, kind + '/scalar', net, what, err / u, K_SCALAR, err / unit(e32_single, net, what))
            if not err <= K_SCALAR * u:
                failures.append((kind, net, what, float(stats[col]), want, err / u))


def check_adam(name, path, kind, h, before, after, failures):
    """p' against the float64 Adam formula on the kernel's own m', v' and t: spacing(|p|) + 2e-6 |D|."""
    hp = h.case['hp']
    for net in h.nets:
        lr = float(F32(hp['lr_actor' if net == 'actor' else 'lr_critic']))
        ss, ib = T.bias_corrections(lr, B1, B2, after['t'][net])
        worst = 0.0
        for k in after['params'][net]:
            p, m1, v1 = (np.asarray(x[net][k], np.float64) for x in (before['params'], after['m'], after['v']))
            delta = ss * m1 / (np.sqrt(v1) * ib + float(F32(1e-8)))
            err = np.abs(np.asarray(after['params'][net][k], np.float64) - (p - delta))
            bound = ulps(p) + 2e-6 * np.abs(delta)
            worst = max(worst, float((err / bound).max()))
        record(name, path, kind + '/adam', net, 'p residual / bound', worst, 1.0)
        if not worst <= 1.0:
            failures.append((kind, net, 'parameter residual / (spacing + 2e-6 |D|)', worst))


def kernel_gradient(h, after, stats, net):
    """From a step that started at zero moments: (clipped gradient per tensor, clip factor, unclipped gradient)."""
    g = {k: np.asarray(v, np.float64) / OMB1 for k, v in after['m'][net].items()}
    norm = np.sqrt(sum((x * x).sum() for x in g.values()))
    factor = norm / float(stats[COL[net]['gnorm']])
    return g, factor, {k: x / factor for k, x in g.items()}


def check_second_moment(name, path, kind, net, g, v_after, failures):
    """v' of a step from zero moments against (1 - b2) g_kernel^2: 4 ulp."""
    worst = 0.0
    for t, x in g.items():
        want = OMB2 * x * x
        worst = max(worst, float((np.abs(v_after[t] - want) / ulps(want)).max()))
    record(name, path, kind + '/moments', net, "v' - (1 - b2) g^2 [ulp]", worst, 4.0)
    if not worst <= 4.0:
        failures.append((kind, net, "v' against (1 - b2) g_kernel^2, ulp", worst))


def check_step_moments(name, path, kind, net, tol, after, r, failures):
    """m', v' of one step against the twin's step from the same state, per tensor within `tol` (state_tolerances)."""
    for t in tol:
        em = np.linalg.norm(after['m'][net][t] - r[net]['m'][t].numpy())
        ev = np.linalg.norm(after['v'][net][t] - r[net]['v'][t].numpy())
        record(name, path, kind + '/state', net, t + " m'", em / tol[t][0], 1.0)
        record(name, path, kind + '/state', net, t + " v'", ev / tol[t][1], 1.0)
        if not (em <= tol[t][0] and ev <= tol[t][1]):
            failures.append((kind, net, t, 'moments / tolerance', em / tol[t][0], ev / tol[t][1]))


def check_first_step(name, path, h, ref, k, failures):
    """Minibatch k from the zero-moment state: gradient, clip factor, v', statistics, Adam, bias-correction columns."""
    zero, r = ref['zero'], ref['first'][k]
    before, after, stats = h.one_step(zero['state'], k)
    check_structure(h, before, after, 1)
    e32 = E32[name]
    kind = f'step{k}'
    check_scalars(name, path, kind, r, stats, e32, failures)
    grads = {}
    for net in h.nets:
        g, factor, raw = kernel_gradient(h, after, stats, net)
        grads[net] = g
        for t, want in r[net]['grads'].items():
            err = T.rel_l2(raw[t], want.numpy())
            u = unit(e32, net, t)
            record(name, path, kind + '/grad', net, t, err / u, K_GRAD, err / unit(E32_SINGLE[name], net, t))
            if not err <= K_GRAD * u:
                failures.append((kind, net, t, 'gradient rel l2 / max(e32, 2^-22)', err / u))
        err = T.rel_l2(factor, float(r[net]['coef']))
        u = unit(e32, net, 'gnorm')
        record(name, path, kind + '/scalar', net, 'clip factor', err / u, K_SCALAR, err / unit(E32_SINGLE[name], net, 'gnorm'))
        if not err <= K_SCALAR * u:
            failures.append((kind, net, 'clip factor', factor, float(r[net]['coef']), err / u))
        check_second_moment(name, path, kind, net, g, after['v'][net], failures)
    if h.bias_columns:
        check_bias_columns(h, kind, stats, after['t'], failures)
    check_adam(name, path, kind, h, before, after, failures)
    return grads, {net: after['v'][net] for net in h.nets}


def check_seeded_step(name, path, h, ref, g_kernel, gsq_kernel, failures):
    """The first minibatch from SEEDED moments: m', v' are the float64 recurrences on the zero-moment twin's gradient.
    The (1 - b2) g^2 term of v' is taken as the zero-moment twin wrote it to ITS v' (which check_first_step holds to
    (1 - b2) g_kernel^2 within 4 ulp): squaring g_kernel = m' / (1 - b1) here would add up to 2 ulp of its own."""
    case = ref['case']
    before, after, stats = h.one_step(case['state'], 0)
    check_structure(h, before, after, 1)
    for net in h.nets:
        wm = wv = 0.0
        for t, g in g_kernel[net].items():
            m, v = np.asarray(before['m'][net][t], np.float64), np.asarray(before['v'][net][t], np.float64)
            want_m, want_v = m + (g - m) * OMB1, B2 * v + np.asarray(gsq_kernel[net][t], np.float64)
            scale = np.maximum(np.abs(want_m), OMB1 * (np.abs(g) + np.abs(m)))
            wm = max(wm, float((np.abs(after['m'][net][t] - want_m) / ulps(scale)).max()))
            wv = max(wv, float((np.abs(after['v'][net][t] - want_v) / ulps(want_v)).max()))
        record(name, path, 'seeded/moments', net, "m' recurrence [ulp]", wm, 2.0)
        record(name, path, 'seeded/moments', net, "v' recurrence [ulp]", wv, 2.0)
        if not (wm <= 2.0 and wv <= 2.0):
            failures.append(('seeded', net, "m', v' against the recurrences on g_kernel, ulp", wm, wv))
    check_adam(name, path, 'seeded', h, before, after, failures)


def state_tolerances(r, e32, net):
    """Per tensor: how far m', v' of ONE float32 step may sit (in L2) from the float64 step taken from the same state,
    given gradients within K_GRAD max(e32, 2^-22) and a clip factor within K_SCALAR max(e32, 2^-22):
      |dm| <= (1 - b1) |dg| + 2^-23 |m'|,   |dv| <= (1 - b2) |dg| max|2.5 g| + 2^-22 |v'|   (g the clipped gradient)."""
    coef = float(r[net]['coef'])
    ec = K_SCALAR * max(e32[net]['gnorm'], T.FLOOR) if coef < 1.0 else 0.0
    out = {}
    for t, g in r[net]['grads'].items():
        g = g.numpy() * coef
        dg = (K_GRAD * unit(e32, net, t) + ec) * np.linalg.norm(g)
        out[t] = (OMB1 * dg + 2.0 ** -23 * np.linalg.norm(r[net]['m'][t].numpy()),
                  OMB2 * dg * 2.5 * np.abs(g).max() + 2.0 ** -22 * np.linalg.norm(r[net]['v'][t].numpy()))
    return out


def check_chain(name, path, h, ref, failures):
    """Seeded moments, the whole pass.  per-step: every launch against the twin advanced from the kernel's own state
    before it, then the pass through PPOUpdater.run (same launches: same bits).  persistent: one launch, statistics
    rows and final state against the twin's float64 chain."""
    case, e32 = ref['case'], E32[name]
    nmb = len(T.minibatches(case['M'], case['B']))
    if not h.one_launch:
        state = case['state']
        for k in range(nmb):
            before, after, stats = h.one_step(state, k)
            r = T.case_step(case, {w: before[w] for w in ('params', 'm', 'v', 't')}, k)
            check_scalars(name, path, f'chain{k}', r, stats, e32, failures)
            for net in h.nets:
                check_step_moments(name, path, f'chain{k}', net, state_tolerances(r, e32, net), after, r, failures)
            check_adam(name, path, f'chain{k}', h, before, after, failures)
            state = {w: after[w] for w in ('params', 'm', 'v', 't')}
        before, final, stats = h.whole_pass(case['state'])
        check_structure(h, before, final, nmb)
        for which in ('params', 'm', 'v'):
            assert np.array_equal(final['blocks'][which], after['blocks'][which]), (which, 'run() against its launches')
        return
    before, final, stats = h.whole_pass(case['state'])
    check_structure(h, before, final, nmb)
    chain = ref['chain']
    for k, r in enumerate(chain):  # the statistics row of EVERY step, bias-correction columns included
        check_scalars(name, path, f'chain{k}', r, stats[k], e32, failures)
        check_bias_columns(h, f'chain{k}', stats[k], {net: before['t'][net] + k + 1 for net in h.nets}, failures)
    check_final_state(name, path, h.nets, chain, e32, final, failures)


def check_final_state(name, path, nets, chain, e32, final, failures, tolerances=None):
    """The state a chain of float32 steps leaves against the twin's float64 chain of the same steps.
    (`tolerances`: state_tolerances' counterpart for the steps of another twin -- tests/test_dp_forms_gpu.py.)"""
    tolerances = state_tolerances if tolerances is None else tolerances
    for net in nets:
        # the steps' tolerances add up (a step inherits b1 of the previous first moment's error); a parameter inherits,
        # ELEMENT BY ELEMENT, ss dm / den + |D| dv / (2 v') of its step's moments on top of the Adam bound (dm, dv: the
        # tensor's L2 tolerances, which bound every element's error), so an entry with a tiny second moment loosens
        # its own bound and no other
        tm, tv, tp = {}, {}, {}
        for r in chain:
            tol = tolerances(r, e32, net)
            for t in tol:
                tm[t] = tm.get(t, 0.0) + tol[t][0]
                tv[t] = tv.get(t, 0.0) + tol[t][1]
                v1, m1 = r[net]['v'][t].numpy(), r[net]['m'][t].numpy()
                den = np.sqrt(v1) * r[net]['inv_bc2_sqrt'] + 1e-8
                delta = r[net]['step_size'] * m1 / den
                tp[t] = tp.get(t, 0.0) + (ulps(r[net]['p'][t].numpy()) + 2e-6 * np.abs(delta)
                                          + r[net]['step_size'] * tm[t] / den + np.abs(delta) * 0.5 * tv[t] / v1)
        last = chain[-1][net]
        for t in tm:
            for which, want, tol in (('m', last['m'][t], tm[t]), ('v', last['v'][t], tv[t])):
                err = np.linalg.norm(final[which][net][t] - want.numpy())
                record(name, path, 'pass/state', net, f'{t} {which}', err / tol, 1.0)
                if not err <= tol:
                    failures.append(('pass', net, t, which, 'final state / tolerance', err / tol))
            worst = float((np.abs(final['params'][net][t] - last['p'][t].numpy()) / tp[t]).max())
            record(name, path, 'pass/state', net, f'{t} params (per element)', worst, 1.0)
            if not worst <= 1.0:
                failures.append(('pass', net, t, 'params', 'final state / per-element tolerance', worst))


def check_case(name, path, h):
    """Every check of this file on one case and one harness."""
    ref = reference(name)
    case = ref['case']
    failures = []
    nmb = len(T.minibatches(case['M'], case['B']))
    grads0 = None
    for k in range(nmb):
        g = check_first_step(name, path, h, ref, k, failures)
        if k == 0:
            grads0, gsq0 = g
    if case['seeded_moments']:
        check_seeded_step(name, path, h, ref, grads0, gsq0, failures)
        check_chain(name, path, h, ref, failures)
    else:  # the pass as the updater runs it: the path, the step counters, the padding, the networks outside the mask
        before, final, stats = h.whole_pass(case['state'])
        check_structure(h, before, final, nmb)
        assert np.isfinite(stats).all()
        if any(net in h.nets for net in T.NETS):
            moved = [net for net in h.nets if not np.array_equal(
                final['blocks']['params'][T.NETS.index(net)], before['blocks']['params'][T.NETS.index(net)])]
            assert moved == list(h.nets)
    assert not failures, failures


@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('name', list(TABLE))
def test_step_against_the_float64_twin(name, path):
    check_case(name, path, Harness(reference(name)['case'], path))
