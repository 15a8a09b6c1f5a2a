"""A plain float64 statement of ONE optimiser step of PolicyGradient._update -- a module, not a test (as
tests/rollout_twin.py and tests/nav_twin.py are for the rollout side).

What the 64-row step kernels (csrc/ppo_pass_body.h through osa_ppo_pass(_ext), the per-step kernel of
csrc/mlp_kernels.hip through osa_ppo_minibatch(_ext)) compute, written as the obvious formula on CPU torch with
autograd for the backward, nothing of the kernels' schedule:

  networks   three tanh MLPs obs -> 64 -> 64 -> {act_dim | 1 | 1}; the actor is Normal(mean(obs), exp(log_std)) with a
             state-independent log_std (reference: models/actor/gaussian_learning_actor.py, models/critic/v_critic.py)
  actor      _update_actor (algorithms/on_policy/base/policy_gradient.py:514-524) on the surrogate advantage
             (adv_r - lam adv_c) / (1 + lam) (naive_lagrange/ppo_lag.py:101-102);
             loss_kind 0: -mean(min(r A, clamp(r, 1 - clip, 1 + clip) A)) (base/ppo.py:66-78),
             loss_kind 1: -mean(r A) (policy_gradient.py:574-578);  - entropy_coef Normal.entropy().mean()
  extension  osa_surrogate_ext: KL(pi_theta || pi_old) per sample, the trust mask 1[KL <= eta] with the reference's
             (B, 1) x (B,) broadcast (first_order/focops.py:103-108: the surrogate term sees the minibatch MEAN of the
             mask), ratio_scale, and P3O's kappa relu(mean(r adv_c) + excess) (penalty_function/p3o.py:76-84)
  critics    _update_reward_critic / _update_cost_critic (policy_gradient.py:428-445, 468-485): mse_loss
             + critic_norm_coef sum(p^2) when use_critic_norm
  clip       clip_grad_norm_ per network: the norm over THAT network's gradient, L2 term included; factor
             min(1, max_grad_norm / (norm + 1e-6))
  Adam       torch.optim.Adam's update for given m, v and step count t (the count AFTER the step):
             m' = b1 m + (1 - b1) g,  v' = b2 v + (1 - b2) g^2,  p' = p - lr / (1 - b1^t) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
  ragged     a last minibatch of n < B rows is a minibatch of n rows: every mean is over n

`step(..., dtype=torch.float32)` runs the identical code in float32.  That run is the measuring stick of the GPU
tests' tolerances (what ONE other float32 evaluation of the same formula loses), not a second reference.

`make_case` builds seeded inputs (numpy.random.RandomState streams only) and arranges that every branch of the losses
carries rows; `check_coverage` asserts it on the CPU so that no case can pass vacuously.  Every float32 input --
parameters, moments, data, hyper-parameters, the multiplier -- is rounded to float32 first and widened afterwards: the
twin and the kernels see the same numbers.

`case_table()` is the table of the 64-row step (tests/test_step_oracle_gpu.py); `form_table()` that of the other forms
of the same step -- several blocks + slab reduce, the chunked, wide and split passes, the large-batch partial
gradients (tests/test_step_forms_gpu.py).  The twin itself is the same for all: a step of n rows is a step of n rows.
`dp_step` (end of the file) states the data-parallel step of W ranks on top of `step` -- clip per rank, average, one
Adam step -- and `dp_table()` is the table of its forms (tests/test_dp_twin.py, tests/test_dp_forms_gpu.py).

General networks.  A case may carry `actor_hidden` / `critic_hidden` (0 to 7 hidden widths; None: [64, 64]) and
`actor_act` / `critic_act` (ACTIVATIONS: tanh, relu, sigmoid, softplus, identity -- computed as the reference's torch
modules do, utils/model.py get_activation, never through the output as the kernels take their derivatives).  With the
defaults every number of the cases above is what it was.  `general_table()` is the table of the layer-wise path
(csrc/general_mlp.hip + csrc/skinny_mlp.h; tests/test_general_step_gpu.py): per mechanism of that path the smallest
shape that reaches it, named by the features `plan_features` reads from osa_gmlp_plan, the launchers' own decisions.
Of the 24 instantiations (TM, TN, BK, form) of gm_gemm_kernel the table launches 15:
    64 x 64 x 64 NT NN TN;  128 x 128 x 64 NT NN TN;  128 x 128 x 16 NT NN TN;  128 x 64 x 64 NT NN TN;
    128 x 64 x 16 TN;  64 x 128 x 64 TN;  64 x 128 x 16 TN
and no shape under the table's cost limits reaches the other nine (tests/test_step_twin.py COVERED_KERNELS says why):
    64 x 64 x 16 in all three forms (K step 16 needs 256 workgroups, which a launch that was refused 128-wide tiles for
    having fewer than 128 of them cannot have);  64 x 128 NT / NN at either K step (a minibatch of at most 64 rows on
    the tiled step with a layer of 5 400 columns);  128 x 64 x 16 NT and NN (10 900 rows).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch

H = 64
NETS = ('actor', 'reward_critic', 'cost_critic')
F32 = np.float32


ACTIVATIONS = ('tanh', 'relu', 'sigmoid', 'softplus', 'identity')  # the OSA_ACT_* kinds, in the order of their codes


def tensor_shapes(net: str, obs_dim: int, act_dim: int, hidden=None) -> 'OrderedDict[str, tuple]':
    """The reference's named_parameters of one network, in its order (log_std first: a module's own parameters come
    before its sub-modules').  `hidden`: the widths of its hidden layers (utils/model.py build_mlp_network: Linear
    layers at the Sequential's indices 0, 2, 4, ...); None: [64, 64]."""
    out = act_dim if net == 'actor' else 1
    pre = 'mean' if net == 'actor' else 'critic_0'
    sizes = [obs_dim] + [int(h) for h in ((H, H) if hidden is None else hidden)] + [out]
    sh = OrderedDict()
    if net == 'actor':
        sh['log_std'] = (act_dim,)
    for j in range(len(sizes) - 1):
        sh[f'{pre}.{2 * j}.weight'] = (sizes[j + 1], sizes[j])
        sh[f'{pre}.{2 * j}.bias'] = (sizes[j + 1],)
    return sh


def case_hidden(case: dict, net: str) -> list:
    """The hidden widths of one network of a case ([64, 64] where the case does not say)."""
    h = case.get('actor_hidden' if net == 'actor' else 'critic_hidden')
    return [H, H] if h is None else list(h)


def case_act(case: dict, net: str) -> str:
    return case.get('actor_act' if net == 'actor' else 'critic_act', 'tanh')


def case_shapes(case: dict, net: str) -> 'OrderedDict[str, tuple]':
    return tensor_shapes(net, case['obs_dim'], case['act_dim'], case_hidden(case, net))


def out_bias(case: dict) -> str:
    """The name of the critics' output bias."""
    return f"critic_0.{2 * len(case_hidden(case, 'reward_critic'))}.bias"


def _f32(x) -> float:
    """A hyper-parameter as the kernels receive it: rounded to float32, then widened."""
    return float(F32(x))


# the hidden activations as the reference's torch modules compute them (utils/model.py get_activation: nn.Tanh,
# nn.ReLU, nn.Sigmoid, nn.Softplus with its defaults beta = 1, threshold = 20, nn.Identity)
_ACT = {'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid,
        'softplus': torch.nn.functional.softplus, 'identity': lambda z: z}


def _mlp(p: dict, pre: str, x: torch.Tensor, act: str = 'tanh', pre_acts: list | None = None) -> torch.Tensor:
    """Linear layers {pre}.0, {pre}.2, ... with `act` between them and none after the last.  `pre_acts`: a list that
    receives the hidden layers' pre-activations."""
    n = sum(1 for k in p if k.startswith(pre + '.') and k.endswith('.weight'))
    h = x
    for j in range(n - 1):
        z = h @ p[f'{pre}.{2 * j}.weight'].T + p[f'{pre}.{2 * j}.bias']
        if pre_acts is not None:
            pre_acts.append(z)
        h = _ACT[act](z)
    return h @ p[f'{pre}.{2 * (n - 1)}.weight'].T + p[f'{pre}.{2 * (n - 1)}.bias']


DEFAULT_HP = dict(clip=0.2, entropy_coef=0.0, critic_norm_coef=0.001, max_grad_norm=40.0, lr_actor=3e-4, lr_critic=3e-4,
                  beta1=0.9, beta2=0.999, adam_eps=1e-8, use_critic_norm=1, use_max_grad_norm=1)


def bias_corrections(lr: float, b1: float, b2: float, t: int) -> tuple:
    """Adam's two bias-correction factors at step count t, float64: lr / (1 - b1^t) and 1 / sqrt(1 - b2^t)."""
    return lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)


def adam(p, m, v, g, lr: float, b1: float, b2: float, eps: float, t: int):
    """torch.optim.Adam (amsgrad off, no weight decay) for one tensor; t = the step count after this step."""
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    step_size, inv_bc2_sqrt = bias_corrections(lr, b1, b2, t)
    return p - step_size * m1 / (torch.sqrt(v1) * inv_bc2_sqrt + eps), m1, v1


def step(state: dict, batch: dict, hp: dict, lam: float, loss_kind: int, ext: dict | None = None,
         dtype=torch.float64, nets=NETS, acts: dict | None = None) -> dict:
    """One optimiser step of the networks in `nets` on the rows of `batch`.

    state   {'params' | 'm' | 'v': {net: {tensor name: array}}, 't': {net: steps taken so far}}
    batch   obs (n, D), act (n, A), logp, target_value_r, target_value_c, adv_r, adv_c (n,); with an extension that
            looks at the behaviour policy also old_mean (n, A) and old_log_std (A,)
    hp      the fields of osa_ppo_hparams (DEFAULT_HP for what is missing)
    ext     None or the scalar fields of osa_surrogate_ext
    acts    {net: hidden activation}, tanh for what is missing (the depth and widths are those of state['params'])

    Returns {net: {...}} with the losses, (actor) mean ratio / entropy / penalty, sum p^2, the UNCLIPPED gradient per
    reference tensor, its norm, the clip factor, p', m', v', the new step count and the two bias-correction factors;
    the actor's entry also carries the per-row ratio, surrogate advantage, KL and mask (for coverage checks)."""
    hp = dict(DEFAULT_HP, **hp)
    f = {k: _f32(hp[k]) for k in ('clip', 'entropy_coef', 'critic_norm_coef', 'max_grad_norm', 'lr_actor',
                                  'lr_critic', 'beta1', 'beta2', 'adam_eps')}
    lam = _f32(lam)
    as_t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    b = {k: as_t(v) for k, v in batch.items()}
    out = {}
    for net in nets:
        p = OrderedDict((k, as_t(v).clone().requires_grad_(True)) for k, v in state['params'][net].items())
        r = {}
        act = (acts or {}).get(net, 'tanh')
        zs = []  # the hidden layers' pre-activations (coverage checks)
        if net == 'actor':
            dist = torch.distributions.Normal(_mlp(p, 'mean', b['obs'], act, zs), torch.exp(p['log_std']))
            logp_ = dist.log_prob(b['act']).sum(-1)
            ratio = torch.exp(logp_ - b['logp'])
            adv = (b['adv_r'] - lam * b['adv_c']) / (1.0 + lam)
            if loss_kind == 0:
                surr = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - f['clip'], 1.0 + f['clip']) * adv)
            else:
                surr = -(ratio * adv)
            penalty = torch.zeros((), dtype=dtype)
            kl = torch.zeros(len(ratio), 1, dtype=dtype)
            mask = torch.ones(len(ratio), 1, dtype=dtype)
            if ext is None:
                loss = surr.mean()
            else:
                e = {k: _f32(ext.get(k, d)) for k, d in (('kl_coef', 0.0), ('kl_mask_eta', -1.0), ('ratio_scale', 1.0),
                                                         ('cost_kappa', 0.0), ('cost_excess', 0.0))}
                if e['kl_coef'] != 0.0 or e['kl_mask_eta'] >= 0.0:
                    old = torch.distributions.Normal(b['old_mean'], torch.exp(b['old_log_std']))
                    kl = torch.distributions.kl_divergence(dist, old).sum(-1, keepdim=True)
                if e['kl_mask_eta'] >= 0.0:
                    mask = (kl.detach() <= e['kl_mask_eta']).to(dtype)
                # (n, 1) KL and mask against the (n,) surrogate: an (n, n) matrix, as the reference forms it
                loss = ((e['kl_coef'] * kl + e['ratio_scale'] * surr) * mask).mean()
                if e['cost_kappa'] > 0.0:
                    penalty = e['cost_kappa'] * torch.relu((ratio * b['adv_c']).mean() + e['cost_excess'])
            entropy = dist.entropy().mean()
            loss = loss - f['entropy_coef'] * entropy
            total = loss + penalty
            r.update(loss=loss.detach(), ratio_mean=ratio.mean().detach(), entropy=entropy.detach(),
                     penalty=penalty.detach(), ratio=ratio.detach(), adv=adv.detach(), kl=kl.detach()[:, 0],
                     mask=mask[:, 0], cost_surrogate=(ratio * b['adv_c']).mean().detach())
            lr = f['lr_actor']
        else:
            v = torch.squeeze(_mlp(p, 'critic_0', b['obs'], act, zs), -1)
            mse = torch.nn.functional.mse_loss(v, b['target_value_r' if net == 'reward_critic' else 'target_value_c'])
            total = mse
            if hp['use_critic_norm']:
                for w in p.values():
                    total = total + w.pow(2).sum() * f['critic_norm_coef']
            r.update(loss=total.detach(), mse=mse.detach(), value=v.detach())
            lr = f['lr_critic']
        grads = torch.autograd.grad(total, list(p.values()))
        gnorm = torch.sqrt(sum((g * g).sum() for g in grads))
        coef = torch.clamp(f['max_grad_norm'] / (gnorm + 1e-6), max=1.0) if hp['use_max_grad_norm'] else torch.ones(
            (), dtype=dtype)
        t = int(state['t'][net]) + 1
        new_p, new_m, new_v = OrderedDict(), OrderedDict(), OrderedDict()
        for (k, w), g in zip(p.items(), grads):
            new_p[k], new_m[k], new_v[k] = adam(w.detach(), as_t(state['m'][net][k]), as_t(state['v'][net][k]), g * coef,
                                                lr, f['beta1'], f['beta2'], f['adam_eps'], t)
        ss, ib = bias_corrections(lr, f['beta1'], f['beta2'], t)
        r.update(psq=sum(w.detach().pow(2).sum() for w in p.values()), grads=OrderedDict(zip(p.keys(), grads)),
                 gnorm=gnorm, coef=coef, p=new_p, m=new_m, v=new_v, t=t, step_size=ss, inv_bc2_sqrt=ib,
                 pre_acts=[z.detach() for z in zs])
        out[net] = r
    return out


def advance(state: dict, res: dict) -> dict:
    """The state after the step whose result is `res` (networks outside `res` keep theirs)."""
    new = {k: dict(state[k]) for k in ('params', 'm', 'v', 't')}
    for net, r in res.items():
        new['params'][net], new['m'][net], new['v'][net], new['t'][net] = r['p'], r['m'], r['v'], r['t']
    return new


def minibatches(M: int, B: int) -> list:
    return [(s, min(B, M - s)) for s in range(0, M, B)]


def rows(data: dict, idx) -> dict:
    """The rows `idx` of the per-sample arrays (old_log_std is per dimension)."""
    return {k: (v if k == 'old_log_std' else np.asarray(v)[np.asarray(idx)]) for k, v in data.items()}


def case_nets(case: dict) -> tuple:
    """The networks a case updates: PPOUpdater's nets mask."""
    nets = ('actor',) if case['update_actor'] else ()
    if case['update_critics']:
        nets += ('reward_critic', 'cost_critic') if case['use_cost'] else ('reward_critic',)
    return nets


def case_acts(case: dict) -> dict:
    return {net: case_act(case, net) for net in NETS}


def case_step(case: dict, state: dict, k: int, dtype=torch.float64, order=None) -> dict:
    """Minibatch k of the case's pass, taken from `state` (`order`: its rows in another order -- the same step)."""
    s, n = minibatches(case['M'], case['B'])[k]
    idx = case['perm'][s:s + n]
    return step(state, rows(case['data'], idx if order is None else idx[order]), case['hp'], case['lam'],
                case['loss_kind'], case['ext'], dtype, case_nets(case), case_acts(case))


def run_pass(case: dict, dtype=torch.float64, state: dict | None = None) -> tuple:
    """The whole pass: ceil(M / B) dependent steps over the case's permutation -> ([step results], final state)."""
    state = case['state'] if state is None else state
    res = []
    for k in range(len(minibatches(case['M'], case['B']))):
        res.append(case_step(case, state, k, dtype))
        state = advance(state, res[-1])
    return res, state


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs with arranged branch coverage
# ---------------------------------------------------------------------------------------------------------------------
# log-ratios of the issue's probe at clip 0.2: two per range (below, inside, above); other clips scale the same picture
def log_ratios(clip: float) -> np.ndarray:
    if abs(clip - 0.2) < 1e-9:
        return np.array([-0.5, -0.35, -0.1, 0.1, 0.35, 0.5])
    return np.log([(1 - clip) * 0.75, (1 - clip) * 0.9, 1 - clip / 2, 1 + clip / 2, (1 + clip) * 1.15, (1 + clip) * 1.35])


def _zero_like_state(shapes: dict) -> dict:
    return {net: OrderedDict((k, np.zeros(s, F32)) for k, s in sh.items()) for net, sh in shapes.items()}


def make_case(obs_dim: int, act_dim: int, B: int = 64, M: int = 100, *, loss_kind: int = 0, clip: float = 0.2,
              lam: float = 0.37, entropy_coef: float = 0.01, use_critic_norm: int = 1, critic_norm_coef: float = 0.001,
              norm_clip=None, use_max_grad_norm: int = 1, use_cost: bool = True, update_actor: bool = True,
              update_critics: bool = True, seeded_moments: bool = False, t0=(0, 0, 0), lr_actor: float = 3e-4,
              lr_critic: float = 3e-4, ext: dict | None = None, trust: bool = False, p3o: str | None = None,
              w1_scale: float = 1.0, target_c_scale: float = 5.0, actor_hidden=None, critic_hidden=None,
              actor_act: str = 'tanh', critic_act: str = 'tanh', fan_scale: bool = False, z_shift=None,
              seed: int = 0) -> dict:
    """One case of the GPU table.

    norm_clip  None: max_grad_norm = 1000 bites nowhere (the clip code runs, its factor is 1);  (net index | 'all', factor): max_grad_norm = factor x the
               twin's float64 gradient norm of that network on the first minibatch ('all': of the smallest of the three)
    trust      prescribe old_mean / old_log_std so that the per-sample KL sits at 0.4 eta or 2 eta (ext['kl_mask_eta'])
    p3o        'active' / 'inactive': cost_excess puts mean(r adv_c) + excess of every minibatch at >= +0.05 / <= -0.05
    w1_scale   multiplies every network's first-layer weight AFTER it is drawn (no random stream moves).  Weights from
               U(-0.2, 0.2) on D inputs give first-layer pre-activations of rms 0.115 sqrt(D): 2.2 at D = 376 with 23 %
               of the units at |tanh| > 0.99, which damps exactly the first-layer gradients the wide kernels exist
               for; the wide cases pass sqrt(64 / D) (rms 0.92, under 1 % saturated; check_coverage asserts <= 2 %)
    target_c_scale  spread of the cost critic's targets.  Its gradient is a mean of n signed residuals and shrinks like
               1 / sqrt n: at n = 2085 the default 5 leaves its norm at 1.63 next to the actor's 1.54, and a clip factor
               taken from the wrong network would pass; the large-batch cases pass 20 (norm about 6, as at 64 rows)
    actor_hidden, critic_hidden   hidden widths, 0 to 7 of them (None: [64, 64]);  actor_act, critic_act: one of
               ACTIVATIONS.  The defaults are the cases of case_table() / form_table(), number for number.
    fan_scale  multiplies every weight matrix of more than 64 inputs by sqrt(64 / inputs) after it is drawn (what
               w1_scale does for the first layer alone): a 1040-wide layer feeds the next one pre-activations of the
               same size as a 64-wide one
    z_shift    (scale, offset): the first-layer weights x scale and the first-layer biases + offset, after they are
               drawn -- places the first-layer pre-activations where an activation's branches are (softplus above
               its threshold of 20 and far below 0, sigmoid near 1)
    seed       added to the seed of the case's random streams (a ReLU case whose draw puts a pre-activation at the
               kink takes another one: check_coverage asserts the distance)
    """
    rs = np.random.RandomState(20240 + 131 * obs_dim + 17 * act_dim + 7 * B + M + seed)
    arch = dict(actor_hidden=None if actor_hidden is None else [int(h) for h in actor_hidden],
                critic_hidden=None if critic_hidden is None else [int(h) for h in critic_hidden],
                actor_act=actor_act, critic_act=critic_act, obs_dim=obs_dim, act_dim=act_dim)
    assert actor_act in ACTIVATIONS and critic_act in ACTIVATIONS
    assert all(len(case_hidden(arch, net)) <= 7 for net in NETS)
    acts = case_acts(arch)
    shapes = {net: case_shapes(arch, net) for net in NETS}
    params = {net: OrderedDict((k, rs.uniform(-0.2, 0.2, s).astype(F32)) for k, s in sh.items())
              for net, sh in shapes.items()}
    params['actor']['log_std'] = np.linspace(-0.5, 0.3, act_dim).astype(F32)
    if w1_scale != 1.0:
        for net in NETS:
            k = ('mean' if net == 'actor' else 'critic_0') + '.0.weight'
            params[net][k] = (params[net][k] * F32(w1_scale)).astype(F32)
    if fan_scale:
        for net in NETS:
            for k, w in params[net].items():
                if w.ndim == 2 and w.shape[1] > 64:
                    params[net][k] = (w * F32(math.sqrt(64.0 / w.shape[1]))).astype(F32)
    if z_shift is not None:
        for net in NETS:
            pre = 'mean' if net == 'actor' else 'critic_0'
            if len(case_hidden(arch, net)) > 0:
                params[net][pre + '.0.weight'] = (params[net][pre + '.0.weight'] * F32(z_shift[0])).astype(F32)
                params[net][pre + '.0.bias'] = (params[net][pre + '.0.bias'] + F32(z_shift[1])).astype(F32)
    m, v = _zero_like_state(shapes), _zero_like_state(shapes)
    # (the streams are drawn whether used or not: a case and its zero-moment twin share every other number)
    for net in NETS:
        for k, s in shapes[net].items():
            mm = (1e-3 * rs.randn(*s)).astype(F32)
            vv = (1e-5 * rs.uniform(0.1, 1.0, s)).astype(F32)
            if seeded_moments:
                m[net][k], v[net][k] = mm, vv
    state = {'params': params, 'm': m, 'v': v, 't': dict(zip(NETS, (int(t) for t in t0)))}
    perm = rs.permutation(M).astype(np.int64)
    data = dict(obs=rs.randn(M, obs_dim).astype(F32), act=(0.5 * rs.randn(M, act_dim)).astype(F32),
                target_value_r=(0.1 * rs.randn(M)).astype(F32), target_value_c=(target_c_scale * rs.randn(M)).astype(F32),
                adv_r=rs.randn(M).astype(F32), adv_c=rs.randn(M).astype(F32))
    # The three gradient norms are kept well apart (about 0.2 : 1.5 : 7), so that a clip factor taken from another
    # network's norm is a visible error and the reward critic's L2 term can dominate its norm: the reward critic's
    # targets sit close to its own float64 values, the advantages are scaled (below, by a power of two) until the
    # actor's norm is near 1.5, the cost critic's targets are wide.
    obs64 = torch.from_numpy(data['obs'].astype(np.float64))
    with torch.no_grad():
        vr = _mlp({k: torch.from_numpy(w.astype(np.float64)) for k, w in params['reward_critic'].items()}, 'critic_0', obs64,
                  acts['reward_critic'])
    data['target_value_r'] = (vr[:, 0].numpy() + data['target_value_r']).astype(F32)
    # ---- clip cells: position k of the permutation gets cell k mod 6 = (range, sign of A); the two log-ratios of a
    # range alternate from one group of six to the next
    lam32 = _f32(lam)
    pos = np.empty(M, np.int64)
    pos[perm] = np.arange(M)  # position of row i in the pass
    cell = pos % 6
    want_pos = cell % 2 == 0
    A = (data['adv_r'].astype(np.float64) - lam32 * data['adv_c']) / (1 + lam32)
    flip = (A > 0) != want_pos
    data['adv_r'][flip] *= -1
    data['adv_c'][flip] *= -1
    lr_tab = log_ratios(clip)
    delta = lr_tab[2 * (cell // 2) + (pos // 6) % 2]
    with torch.no_grad():
        p64 = {k: torch.from_numpy(w.astype(np.float64)) for k, w in params['actor'].items()}
        mean = _mlp(p64, 'mean', torch.from_numpy(data['obs'].astype(np.float64)), acts['actor'])
        dist = torch.distributions.Normal(mean, torch.exp(p64['log_std']))
        logp_new = dist.log_prob(torch.from_numpy(data['act'].astype(np.float64))).sum(-1).numpy()
    data['logp'] = (logp_new - delta).astype(F32)
    hp = dict(clip=clip, entropy_coef=entropy_coef, critic_norm_coef=critic_norm_coef, max_grad_norm=1000.0,
              lr_actor=lr_actor, lr_critic=lr_critic, beta1=0.9, beta2=0.999, adam_eps=1e-8,
              use_critic_norm=int(use_critic_norm), use_max_grad_norm=int(use_max_grad_norm))
    ext = None if ext is None else dict(ext)
    if ext is not None:
        # the behaviour policy: old_log_std a little wider than log_std, old_mean at a prescribed KL from the mean
        old_ls = (params['actor']['log_std'].astype(np.float64) + 0.05).astype(F32)
        data['old_log_std'] = old_ls
        s0, s1 = np.exp(old_ls.astype(np.float64)), np.exp(params['actor']['log_std'].astype(np.float64))
        floor = float(np.sum(np.log(s0 / s1) + s1 ** 2 / (2 * s0 ** 2) - 0.5))  # KL at equal means
        if trust:
            eta = _f32(ext['kl_mask_eta'])
            assert 0.4 * eta > floor, (floor, eta)
            inside = rs.permutation(M) % 2 == 0
            target = np.where(inside, 0.4 * eta, 2.0 * eta)
        else:
            rs.permutation(M)
            target = floor + 0.05 + 0.1 * (pos % 3)
        sign = np.where(rs.rand(M, act_dim) < 0.5, -1.0, 1.0)
        dmu = sign * s0[None, :] * np.sqrt(2 * (target - floor) / act_dim)[:, None]
        data['old_mean'] = (mean.numpy() + dmu).astype(F32)
    case = dict(obs_dim=obs_dim, act_dim=act_dim, B=B, M=M, state=state, data=data, perm=perm, hp=hp, lam=lam32,
                loss_kind=loss_kind, ext=ext, use_cost=bool(use_cost), update_actor=bool(update_actor),
                update_critics=bool(update_critics), seeded_moments=bool(seeded_moments), trust=bool(trust), p3o=p3o,
                norm_clip=norm_clip, w1_scale=float(w1_scale))
    if (actor_hidden, critic_hidden, actor_act, critic_act) != (None, None, 'tanh', 'tanh'):
        case.update(arch, z_shift=z_shift)
    if update_actor:
        g0 = float(case_step(dict(case, update_critics=False, ext=None), state, 0)['actor']['gnorm'])
        scale = F32(2.0 ** round(math.log2(1.5 / g0)))
        data['adv_r'] *= scale
        data['adv_c'] *= scale
    if p3o is not None:
        # mean(r adv_c) of every minibatch at the case's initial parameters, then an excess clear of all of them
        ext['cost_excess'] = 0.0
        cs = [float(case_step(case, state, k)['actor']['cost_surrogate']) for k in range(len(minibatches(M, B)))]
        ext['cost_excess'] = _f32(-min(cs) + 0.5 if p3o == 'active' else -max(cs) - 0.5)
    if norm_clip is not None:
        which, factor = norm_clip
        all_nets = dict(case, update_actor=True, update_critics=True, use_cost=True)
        r0 = case_step(all_nets, state, 0)
        norms = [float(r0[net]['gnorm']) for net in NETS]
        hp['max_grad_norm'] = _f32(factor * (min(norms) if which == 'all' else norms[which]))
        case['norms0'] = norms
    return case


def check_coverage(case: dict) -> dict:
    """Asserts that the case reaches the branches it is in the table for -- on the float64 chain of its pass, so for
    every minibatch at the parameters that minibatch meets.  Returns what it counted."""
    res, _ = run_pass(case)
    clip = _f32(case['hp']['clip'])
    seen = set()
    info = {'cells': [], 'edge': np.inf}
    for k, r in enumerate(res):
        if 'actor' not in r:
            continue
        a = r['actor']
        ratio, adv = a['ratio'].numpy(), a['adv'].numpy()
        n = len(ratio)
        edge = np.minimum(np.abs(ratio - (1 - clip)), np.abs(ratio - (1 + clip))).min()
        info['edge'] = min(info['edge'], float(edge))
        assert edge >= 1e-3, (k, edge)  # float32 and float64 take the same branch
        assert np.abs(adv).min() > 0
        rng = np.where(ratio < 1 - clip, 0, np.where(ratio > 1 + clip, 2, 1))
        cells = {(int(g), bool(s)) for g, s in zip(rng, adv > 0)}
        info['cells'].append(len(cells))
        seen |= cells
        # six cells wherever six rows exist; a shorter minibatch (B = 5, a tail of one or two rows) cannot hold six
        # and must put every row into a cell of its own
        assert len(cells) == min(n, 6), (k, n, sorted(cells))
        if case['trust']:
            eta = _f32(case['ext']['kl_mask_eta'])
            kl = a['kl'].numpy()
            assert np.abs(kl - eta).min() >= 0.01 * eta, (k, np.abs(kl - eta).min())
            if n >= 8:
                inside = int((kl <= eta).sum())
                assert inside >= n / 4 and n - inside >= n / 4, (k, inside, n)
            info.setdefault('inside', []).append(int((kl <= eta).sum()))
        if case['p3o'] is not None:
            val = float(a['cost_surrogate']) + _f32(case['ext']['cost_excess'])
            assert (val >= 0.05) if case['p3o'] == 'active' else (val <= -0.05), (k, val)
            assert (float(a['penalty']) > 0) == (case['p3o'] == 'active')
            info.setdefault('penalty_arg', []).append(val)
    if case['update_actor']:
        assert len(seen) == 6, sorted(seen)  # over the pass every cell is reached, whatever the minibatch size
    if case['norm_clip'] is not None:
        which, factor = case['norm_clip']
        mg, norms = _f32(case['hp']['max_grad_norm']), case['norms0']
        for i, net in enumerate(NETS):
            own = which == 'all' or i == which
            if own and which != 'all':
                assert abs(mg / norms[i] - factor) < 1e-6
            elif not own:  # the other networks: far from the threshold, on whichever side
                assert not (1 / 1.5 < mg / norms[i] < 1.5), (net, mg, norms)
        r0 = res[0]
        active = [net for net in r0 if float(r0[net]['coef']) < 1.0]
        info['clipped'] = active
        if factor < 1.0:
            assert (set(active) == set(r0)) if which == 'all' else (NETS[which] in active or NETS[which] not in r0)
    elif case['hp']['use_max_grad_norm']:
        assert all(float(r[net]['coef']) == 1.0 for r in res for net in r)
    if case.get('w1_scale', 1.0) != 1.0:
        info['saturated'] = first_layer_saturation(case)
        assert max(info['saturated'].values()) <= 0.02, info['saturated']
    info.update(activation_coverage(case))
    return info


def activation_coverage(case: dict) -> dict:
    """Conditions on the hidden pre-activations of every minibatch of the case at its initial state (where the GPU
    tests take the gradient), per network the case updates:
      relu      no pre-activation of any hidden layer sits at the kink: min |z64| >= 64 max |z32 - z64|, both from
                the twin's own float32 and float64 runs -- float32 and float64 (and the kernels, whose forward error
                is of the size of the float32 run's) take the same side everywhere;
      softplus  (a case with z_shift) first-layer pre-activations above 20, torch's linear branch, exist, and at
                least a quarter lie below -3, where the output h = log1p(exp z) is small and a derivative taken
                through it as 1 - exp(-h) cancels;
      sigmoid   (a case with z_shift) at least 5 % of the first-layer units have h > 0.99."""
    info = {}
    nets = case_nets(case)
    kinds = {net: case_act(case, net) for net in nets if len(case_hidden(case, net)) > 0}
    probe = case.get('z_shift') is not None
    if not ('relu' in kinds.values() or (probe and {'softplus', 'sigmoid'} & set(kinds.values()))):
        return info
    for k in range(len(minibatches(case['M'], case['B']))):
        r64 = case_step(case, case['state'], k)
        r32 = case_step(case, case['state'], k, torch.float32) if 'relu' in kinds.values() else None
        for net, kind in kinds.items():
            z64 = [z.numpy() for z in r64[net]['pre_acts']]
            if kind == 'relu':
                for l, z in enumerate(z64):
                    lo = float(np.abs(z).min())
                    d = float(np.abs(r32[net]['pre_acts'][l].numpy().astype(np.float64) - z).max())
                    assert lo >= 64.0 * d, (net, k, l, lo, d)
                    info['relu_margin'] = min(info.get('relu_margin', np.inf), lo / max(d, 1e-300))
            elif probe and kind == 'softplus':
                c = info.setdefault('softplus', {}).setdefault(net, [0, 0, 0])
                c[0] += int((z64[0] > 20.0).sum())
                c[1] += int((z64[0] < -3.0).sum())
                c[2] += z64[0].size
            elif probe and kind == 'sigmoid':
                c = info.setdefault('sigmoid', {}).setdefault(net, [0, 0])
                c[0] += int((1.0 / (1.0 + np.exp(-z64[0])) > 0.99).sum())
                c[1] += z64[0].size
    for net, (above, below, n) in info.get('softplus', {}).items():
        assert above >= 1 and 4 * below >= n, (net, above, below, n)
    for net, (sat, n) in info.get('sigmoid', {}).items():
        assert 20 * sat >= n, (net, sat, n)
    return info


def first_layer_saturation(case: dict) -> dict:
    """Per network: the share of first-layer units (over all rows of the case, at its initial parameters) with
    |tanh| > 0.99 -- units whose derivative, and with it the first-layer gradient, has all but vanished."""
    obs = torch.from_numpy(case['data']['obs'].astype(np.float64))
    out = {}
    for net in NETS:
        pre = 'mean' if net == 'actor' else 'critic_0'
        p = {k: torch.from_numpy(np.asarray(w, np.float64)) for k, w in case['state']['params'][net].items()}
        h = torch.tanh(obs @ p[f'{pre}.0.weight'].T + p[f'{pre}.0.bias'])
        out[net] = float((h.abs() > 0.99).double().mean())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the table of the GPU tests (tests/test_step_oracle_gpu.py) and of the float32 measuring stick
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (16, 2), (17, 3), (60, 2), (64, 16), (65, 17), (80, 32), (96, 16)]
VARIANT_SHAPES = [(60, 2), (65, 17)]
EXT_SHAPES = [(60, 2), (28, 8)]
BATCHES = [(64, 64), (64, 65), (64, 127), (32, 80), (48, 100), (5, 12)]  # (B, M)
FOCOPS = dict(kl_coef=1.0, kl_mask_eta=0.5, ratio_scale=1.0 / 1.5)


def case_table() -> 'OrderedDict[str, dict]':
    """name -> make_case keyword arguments.  Every entry changes ONE thing from the base configuration (loss_kind 0,
    clip 0.2, lam 0.37, entropy_coef 0.01, critic L2 on at 0.001, norm clip inactive, B 64, M 100)."""
    t = OrderedDict()
    for od, ad in SHAPES:
        t[f'base-{od}x{ad}'] = dict(obs_dim=od, act_dim=ad)
    for od, ad in VARIANT_SHAPES:
        s = f'{od}x{ad}'
        kw = dict(obs_dim=od, act_dim=ad)
        for B, M in BATCHES:
            t[f'mb-B{B}-M{M}-{s}'] = dict(kw, B=B, M=M)
        for net in range(3):
            for fac in (0.5, 0.999, 1.001, 2.0):
                t[f'normclip-{NETS[net]}-{fac}-{s}'] = dict(kw, norm_clip=(net, fac))
        t[f'normclip-all-{s}'] = dict(kw, norm_clip=('all', 0.5))
        t[f'normclip-off-{s}'] = dict(kw, use_max_grad_norm=0)
        t[f'l2-off-{s}'] = dict(kw, use_critic_norm=0)
        t[f'l2-0.05-{s}'] = dict(kw, critic_norm_coef=0.05)
        # (with the L2 term dominating the critics' norms, a norm taken before the term would not clip)
        t[f'l2-0.05-clipped-{s}'] = dict(kw, critic_norm_coef=0.05, norm_clip=(1, 0.5))
        t[f'entropy-0-{s}'] = dict(kw, entropy_coef=0.0)
        t[f'entropy-0.05-{s}'] = dict(kw, entropy_coef=0.05)
        t[f'losskind1-{s}'] = dict(kw, loss_kind=1)
        t[f'lam-0-{s}'] = dict(kw, lam=0.0)
        t[f'lam-50-{s}'] = dict(kw, lam=50.0)
        t[f'nocost-{s}'] = dict(kw, use_cost=False)
        t[f'actor-off-{s}'] = dict(kw, update_actor=False)
        t[f'critics-off-{s}'] = dict(kw, update_critics=False)
        t[f'clip-0.05-{s}'] = dict(kw, clip=0.05)
        t[f'clip-0.4-{s}'] = dict(kw, clip=0.4)
        t[f'seeded-{s}'] = dict(kw, seeded_moments=True, t0=(3, 5, 7))
        for t0 in (0, 9, 999, 250000):
            t[f't0-{t0}-{s}'] = dict(kw, seeded_moments=True, t0=(t0, t0, t0))
        t[f'lr-{s}'] = dict(kw, lr_actor=3e-4, lr_critic=1e-3, seeded_moments=True, t0=(3, 5, 7))
    for od, ad in EXT_SHAPES:
        s = f'{od}x{ad}'
        kw = dict(obs_dim=od, act_dim=ad, update_critics=False)
        t[f'focops-mask-{s}'] = dict(kw, loss_kind=1, ext=FOCOPS, trust=True)
        t[f'focops-nomask-{s}'] = dict(kw, loss_kind=1, ext=dict(FOCOPS, kl_mask_eta=-1.0))
        t[f'cup-{s}'] = dict(kw, loss_kind=1, ext=dict(kl_coef=1.0), entropy_coef=0.0)
        t[f'p3o-active-{s}'] = dict(kw, ext=dict(cost_kappa=2.0), p3o='active')
        t[f'p3o-inactive-{s}'] = dict(kw, ext=dict(cost_kappa=2.0), p3o='inactive')
    return t


# ---------------------------------------------------------------------------------------------------------------------
# the second table: the forms of the step beyond one 64-row workgroup per network (tests/test_step_forms_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
# form -> how PPOUpdater is brought to it and what it reports: persistent flag, environment, PPOUpdater.last_path
FORMS = OrderedDict([
    ('per-step', dict(persistent=False, env={}, last_path='per-step')),  # osa_mb_grad_kernel on several blocks + slab reduce
    ('chunked', dict(persistent=True, env={}, last_path='persistent-chunked')),
    ('wide', dict(persistent=True, env={'OSA_WIDE_SPLIT': '0'}, last_path='persistent-wide')),
    ('split', dict(persistent=True, env={}, last_path='persistent-wide-split')),  # local placement, the default
    ('split-spread', dict(persistent=True, env={'OSA_WIDE_SPLIT': 'spread'}, last_path='persistent-wide-split')),
    ('balanced', dict(persistent=False, env={}, last_path='per-step')),  # B >= 2048: osa_ppo_part_kernel
    ('strided', dict(persistent=False, env={'OSA_LARGE_BATCH_BALANCED': '0'}, last_path='per-step')),
])
CHUNK_SHAPES = [(60, 2), (65, 17)]
# (B, M, rows of the tail minibatch, 64-row chunks of the B-row step that the tail leaves EMPTY)
CHUNK_BATCHES = [(65, 130, 65, 0), (128, 300, 44, 1), (129, 129, 129, 0), (200, 500, 100, 2), (192, 256, 64, 2)]
WIDE_SHAPES = [(97, 3), (90, 17), (192, 2), (193, 5), (375, 17), (376, 17), (512, 32)]
WIDE_BATCHES = [(40, 100), (64, 65), (5, 12)]  # on 376x17
LARGE_TARGET_C = 20.0
LARGE = [(60, 2, 2048, 2048), (60, 2, 2085, 2085), (60, 2, 2048, 2048 + 37), (72, 17, 6000, 6000), (16, 1, 2048, 2048)]
# the variants run on ONE shape per family, on the family's first form; SECOND_FORM also on its second
FORM_VARIANT_SHAPES = [(dict(obs_dim=65, act_dim=17, B=128, M=300), ('chunked', 'per-step')),
                       (dict(obs_dim=376, act_dim=17, B=64, M=100), ('split', 'wide')),
                       (dict(obs_dim=60, act_dim=2, B=2085, M=2085), ('balanced', 'strided'))]
SECOND_FORM = ('losskind1', 'critics-off', 'l2-0.05-clipped', 'seeded')


def form_variants() -> 'OrderedDict[str, dict]':
    v = OrderedDict()
    v['losskind1'] = dict(loss_kind=1)
    v['lam-0'] = dict(lam=0.0)
    v['lam-50'] = dict(lam=50.0)
    v['nocost'] = dict(use_cost=False)
    v['actor-off'] = dict(update_actor=False)  # (large batch: the masks move the balanced task boundaries)
    v['critics-off'] = dict(update_critics=False)
    v['l2-off'] = dict(use_critic_norm=0)
    v['l2-0.05'] = dict(critic_norm_coef=0.05)
    v['l2-0.05-clipped'] = dict(critic_norm_coef=0.05, norm_clip=(1, 0.5))
    v['entropy-0'] = dict(entropy_coef=0.0)
    v['clip-0.05'] = dict(clip=0.05)
    for net in range(3):
        for fac in (0.5, 0.999, 1.001):
            v[f'normclip-{NETS[net]}-{fac}'] = dict(norm_clip=(net, fac))
    v['normclip-all'] = dict(norm_clip=('all', 0.5))
    v['normclip-off'] = dict(use_max_grad_norm=0)
    v['seeded'] = dict(seeded_moments=True, t0=(3, 5, 7))
    v['t0-0'] = dict(seeded_moments=True, t0=(0, 0, 0))
    v['t0-250000'] = dict(seeded_moments=True, t0=(250000, 250000, 250000))
    v['lr'] = dict(lr_actor=3e-4, lr_critic=1e-3, seeded_moments=True, t0=(3, 5, 7))
    return v


def form_name(tag: str, kw: dict) -> str:
    return f"{tag}-{kw['obs_dim']}x{kw['act_dim']}-B{kw['B']}-M{kw['M']}"


def wide_kw(od: int, ad: int, B: int = 64, M: int = 100) -> dict:
    """A case of the wide family: first-layer weights scaled so that the layer does not saturate (make_case)."""
    return dict(obs_dim=od, act_dim=ad, B=B, M=M, w1_scale=math.sqrt(64.0 / od))


def form_table() -> 'OrderedDict[str, dict]':
    """name -> dict(kw = make_case keyword arguments, paths = the FORMS the case runs on[, tail = (rows, empty chunks)]).
    As in case_table() an entry changes ONE thing from its family's base configuration; names end in the shape and
    -B<batch>-M<rows>, which no name of case_table() does."""
    t = OrderedDict()

    def add(tag, kw, paths, **more):
        name = form_name(tag, kw)
        assert name not in t
        t[name] = dict(kw=kw, paths=tuple(paths), **more)

    # ---- 64 < B <= 1024 on a shape of the narrow pass: cooperating chunk workgroups / several blocks + slab reduce
    for od, ad in CHUNK_SHAPES:
        for B, M, tail, empty in CHUNK_BATCHES:
            add('base', dict(obs_dim=od, act_dim=ad, B=B, M=M), ('per-step', 'chunked'), tail=(tail, empty))
    add('base', dict(obs_dim=60, act_dim=2, B=1024, M=1025), ('per-step', 'chunked'), tail=(1, 15))  # the upper end
    # ---- B <= 64 on shapes the narrow pass cannot hold
    for od, ad in WIDE_SHAPES:
        add('base', wide_kw(od, ad), ('wide', 'split') + (('split-spread',) if (od, ad) == (376, 17) else ()))
    for B, M in WIDE_BATCHES:
        add('base', wide_kw(376, 17, B, M), ('wide', 'split'))
    # ---- B >= 2048: partial gradients of one minibatch over the whole device
    for od, ad, B, M in LARGE:
        add('base', dict(obs_dim=od, act_dim=ad, B=B, M=M, target_c_scale=LARGE_TARGET_C), ('balanced', 'strided'))
    # ---- the loss / clip / Adam variants on one shape per family
    for base, forms in FORM_VARIANT_SHAPES:
        kw0 = (wide_kw(base['obs_dim'], base['act_dim'], base['B'], base['M']) if base['obs_dim'] > 96
               else dict(base, target_c_scale=LARGE_TARGET_C) if base['B'] >= 2048 else base)
        for tag, change in form_variants().items():
            add(tag, dict(kw0, **change), forms if tag in SECOND_FORM else forms[:1])
    # ---- an extended surrogate above 64 rows: legal on the per-step kernels only, without mask or penalty
    add('cup', dict(obs_dim=60, act_dim=2, B=128, M=300, update_critics=False, loss_kind=1, ext=dict(kl_coef=1.0),
                    entropy_coef=0.0), ('per-step',))
    return t


# ---------------------------------------------------------------------------------------------------------------------
# the third table: general networks -- the layer-wise path of csrc/general_mlp.hip + csrc/skinny_mlp.h
# (tests/test_general_step_gpu.py).  Every shape is the smallest that reaches the mechanism the case is named for;
# tests/test_step_twin.py asserts from osa_gmlp_plan that it does.
# ---------------------------------------------------------------------------------------------------------------------
GENERAL_BASE = dict(obs_dim=20, act_dim=3, B=37, M=70, actor_hidden=[30, 7], critic_hidden=[50, 1, 9])
GENERAL_SMALL = dict(obs_dim=20, act_dim=3, B=37, M=70, actor_hidden=[24, 12], critic_hidden=[24, 12])
GENERAL_TILED = dict(obs_dim=20, act_dim=3, actor_hidden=[24, 12], critic_hidden=[12, 24])


def general_table() -> 'OrderedDict[str, dict]':
    """name -> dict(kw = make_case keyword arguments, env = environment of the run, features = what osa_gmlp_plan
    must report for the case: the vocabulary of tests/test_step_twin.py plan_features)."""
    t = OrderedDict()

    def add(name, features, env=None, **kw):
        assert name not in t
        t[name] = dict(kw=kw, env=dict(env or {}), features=tuple(features))

    base, small = GENERAL_BASE, GENERAL_SMALL
    fused = ('skinny', 'fusedn', 'top-in-fwd:all', 'loss-fused')
    # ---- skinny step (B <= 64): rows 1, 3, 37, 64; the ways the top layer fuses
    add('sk-a2-rows1', fused, **dict(small, obs_dim=1, act_dim=2, B=1, M=6))
    add('sk-a8-one-hidden-rows64', fused, obs_dim=61, act_dim=8, B=64, M=65, actor_hidden=[64], critic_hidden=[64])
    add('sk-a9-odd-widths-rows3', ('skinny', 'fusedn', 'top-in-fwd:critics', 'loss-fused'), **dict(base, act_dim=9, B=3, M=9))
    add('sk-a32-h65', ('skinny', 'fusedn', 'top-in-fwd:critics', 'loss-fused', 'tk2'),
        **dict(base, act_dim=32, actor_hidden=[65, 65], critic_hidden=[17, 65]))
    add('sk-a33-plain-loss', ('skinny', 'no-fusedn', 'loss-plain'), **dict(base, act_dim=33, actor_hidden=[20], critic_hidden=[20]))
    add('sk-a33-normclip-all', ('skinny', 'no-fusedn', 'loss-plain'),
        **dict(base, act_dim=33, actor_hidden=[20], critic_hidden=[20], norm_clip=('all', 0.5)))
    add('sk-nohidden-actor', ('skinny', 'no-fusedn', 'loss-fused'), **dict(base, actor_hidden=[], critic_hidden=[20]))
    add('sk-nohidden-all', ('skinny', 'no-fusedn', 'loss-fused'), **dict(base, actor_hidden=[], critic_hidden=[]))
    add('sk-seven-layers', fused, **dict(base, actor_hidden=[16, 12, 10, 9, 8, 6, 5], critic_hidden=[16, 12, 10, 9, 8, 6, 5]))
    add('sk-k1040', fused, **dict(base, obs_dim=376, M=43, actor_hidden=[1040, 20], critic_hidden=[1040, 20], fan_scale=True))
    add('sk-k4-k20', fused, **dict(base, actor_hidden=[4, 20], critic_hidden=[20, 4]))
    # (a fused top layer below a layer of more than 1024 columns: more than 64 partial slabs, summed by the loop of
    # gs_top_kernel and not by its register path)
    add('sk-top1040', fused, **dict(base, actor_hidden=[20, 1040], critic_hidden=[20, 1040], fan_scale=True))
    # ---- the loss, clip and mask variants on the base networks ([30, 7] / [50, 1, 9]: no width a multiple of 4)
    add('sk-base', fused, **base)
    add('sk-l2-off', fused, **dict(base, use_critic_norm=0))
    add('sk-l2-0.05', fused, **dict(base, critic_norm_coef=0.05))
    add('sk-l2-0.05-clipped', fused, **dict(base, critic_norm_coef=0.05, norm_clip=(1, 0.5)))
    for net in range(3):
        add(f'sk-normclip-{NETS[net]}', fused, **dict(base, norm_clip=(net, 0.5)))
    add('sk-normclip-off', fused, **dict(base, use_max_grad_norm=0))
    add('sk-entropy-0.05', fused, **dict(base, entropy_coef=0.05))
    add('sk-actor-off', fused, **dict(base, update_actor=False))
    add('sk-critics-off', fused, **dict(base, update_critics=False))
    add('sk-nocost', fused, **dict(base, use_cost=False))
    add('sk-losskind1', fused, **dict(base, loss_kind=1))
    ext = dict(base, update_critics=False)
    add('sk-focops-mask', fused, **dict(ext, loss_kind=1, ext=FOCOPS, trust=True))
    add('sk-p3o-active', fused, **dict(ext, ext=dict(cost_kappa=2.0), p3o='active'))
    add('sk-p3o-inactive', fused, **dict(ext, ext=dict(cost_kappa=2.0), p3o='inactive'))
    add('sk-seeded', fused, **dict(base, seeded_moments=True, t0=(3, 5, 7)))
    # ---- activations: one case each, and actor and critics of different depth and kind
    add('sk-mixed-relu-softplus', fused, **dict(base, actor_act='relu', critic_act='softplus'))
    for kind in ACTIVATIONS:
        shift = {'softplus': (16.0, -5.0), 'sigmoid': (8.0, 1.0)}.get(kind)
        add(f'sk-act-{kind}', fused, **dict(small, actor_act=kind, critic_act=kind, z_shift=shift))
    # ---- tiled step (B > 64, or B = 64 with the skinny kernels switched off)
    tiled = GENERAL_TILED
    add('tl-skinny-off-B64', ('tiled', 'S1'), env={'OSA_GMLP_SKINNY': '0'}, **dict(tiled, B=64, M=64))
    add('tl-B65', ('tiled', 'S1', 'row-split-off'), **dict(tiled, B=65, M=65))
    add('tl-B255', ('tiled', 'S1'), **dict(tiled, B=255, M=255))
    add('tl-B256', ('tiled', 'S2'), **dict(tiled, B=256, M=256))
    add('tl-B257', ('tiled', 'S2', 'row-split-off'), **dict(tiled, B=257, M=257))
    add('tl-B300', ('tiled', 'S2'), **dict(tiled, B=300, M=300))
    add('tl-B130-tail', ('tiled', 'S1'), **dict(tiled, B=130, M=200, seeded_moments=True, t0=(3, 5, 7)))
    add('tl-normclip-all', ('tiled',), **dict(tiled, B=130, M=130, norm_clip=('all', 0.5)))
    add('tl-losskind1-sigmoid', ('tiled',), **dict(tiled, B=130, M=130, loss_kind=1, actor_act='sigmoid', critic_act='softplus'))
    add('tl-focops-mask-B200', ('tiled',), **dict(tiled, B=200, M=200, update_critics=False, loss_kind=1, ext=FOCOPS, trust=True))
    add('tl-rowsplit-512', ('tiled', 'rowS4'), **dict(tiled, B=65, M=65, actor_hidden=[512, 16], critic_hidden=[16, 512], fan_scale=True))
    add('tl-rowsplit-mixed', ('tiled', 'rowS4', 'Si<S'),
        **dict(tiled, B=65, M=65, actor_hidden=[512, 16], critic_hidden=[130, 16], fan_scale=True))
    add('tl-rowsplit-1040', ('tiled', 'rowS8'), **dict(tiled, B=65, M=65, actor_hidden=[1040, 8], critic_hidden=[1040, 8], fan_scale=True))
    add('tl-ragged-64-65-129', ('tiled', 'NT', 'NN', 'TN'),
        **dict(tiled, obs_dim=63, B=130, M=130, actor_hidden=[64, 65, 129], critic_hidden=[64, 65, 129], fan_scale=True))
    # ---- the instantiations of gm_gemm_kernel beyond 64 x 64 x 64, by the launcher's arithmetic on workgroup counts
    # (gm_pick_tile: 128-wide tiles where they still give 128 workgroups, K step 16 from 256 workgroups)
    h512 = dict(tiled, actor_hidden=[512, 512], critic_hidden=[512, 512], fan_scale=True)
    add('tl-h512-B384', ('tiled', 'S3', 'k128x128x64TN', 'TM128xTN128', 'BK64'), **dict(h512, B=384, M=384))
    add('tl-h512-B700', ('tiled', 'S5', 'k128x128x16TN', 'k128x64x64NT', 'k128x64x64NN', 'BK16', 'TM128'), **dict(h512, B=700, M=700))
    thin = dict(tiled, actor_hidden=[1040, 64], critic_hidden=[1040, 64], fan_scale=True)
    add('tl-h1040x64-B640', ('tiled', 'k64x128x64TN', 'k128x64x64TN', 'k128x128x64NN', 'k128x128x64NT', 'TN128'),
        **dict(thin, B=640, M=640))
    add('tl-h1040x64-B1280', ('tiled', 'k64x128x16TN', 'k128x64x16TN', 'k128x128x16NN', 'k128x128x16NT'),
        **dict(thin, B=1280, M=1280, target_c_scale=LARGE_TARGET_C))
    return t


def empty_chunks(B: int, n: int) -> int:
    """64-row chunks of a B-row step that a minibatch of n rows leaves without a row (chunk c holds rows 64 c ...)."""
    return (B + 63) // 64 - (n + 63) // 64


def zero_moment_twin(kwargs: dict) -> dict:
    """The same case from zero moments: same inputs, same kernel -- where the clipped gradient is m' / (1 - b1)."""
    return dict(kwargs, seeded_moments=False)


# ---------------------------------------------------------------------------------------------------------------------
# the measuring stick: what one float32 evaluation of the same formula loses against float64
# ---------------------------------------------------------------------------------------------------------------------
SCALARS = {'actor': ('loss', 'ratio_mean', 'entropy', 'gnorm', 'penalty'), 'reward_critic': ('mse', 'psq', 'gnorm'),
           'cost_critic': ('mse', 'psq', 'gnorm')}
FLOOR = 2.0 ** -22
# A critic's output-bias gradient is ONE number, 2/n sum_rows (v - target) (+ the L2 term): where the residuals
# cancel, what a float32 evaluation loses on it is the sum of its n forward-value errors over a small result, and the
# tensor's own e32 is one draw of that sum (it can come out at a fifth of its typical size).  OUT_BIAS_ROWS records
# the typical size instead, from the float32 run's forward values: a sum of n independent errors of their rms,
# (2 / sqrt n) rms_rows(v32 - v64) / |g_64|.  The GPU tests take the larger of the two as this tensor's unit.
OUT_BIAS, OUT_BIAS_ROWS = 'critic_0.4.bias', 'critic_0.4.bias/rows'


def rel_l2(a, b) -> float:
    """|a - b|_2 / |b|_2 in float64 (0 when both vanish)."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    den = np.linalg.norm(b)
    num = np.linalg.norm(a - b)
    return 0.0 if num == 0.0 else float(num / den) if den > 0 else np.inf


ROW_ORDERS = 4


def f32_error(case: dict) -> tuple:
    """Per network: relative L2 error of the float32 run against the float64 run of every minibatch of the case taken
    from its INITIAL state -- per reference tensor of the unclipped gradient and per scalar.  Returns (worst, single).

    `single` is the float32 run with the rows as drawn, worst over the minibatches.  The rounding error of a sum
    depends on the order of its terms, and a one-element tensor (an output bias: a sum over the rows of signed
    residuals) or a scalar shows ONE draw of it per evaluation -- anything between nothing and its full spread.  As a
    unit of measurement one draw is arbitrary there, so the float32 run is repeated with the minibatch's rows in
    ROW_ORDERS orders (as drawn, and seeded shuffles of it: the same step, another summation order) and `worst` is
    the worst over the orders and the minibatches.  That is the unit of the GPU tests; a tensor of many elements
    averages the draws by itself and the choice matters little there.  Both are recorded, and
    profiles/step_twin_error.md states the kernels' worst ratios against both."""
    worst, single = {}, {}
    for k, (_, n) in enumerate(minibatches(case['M'], case['B'])):
        r64 = case_step(case, case['state'], k)
        rs = np.random.RandomState(977 + k)
        for order in [None] + [rs.permutation(n) for _ in range(ROW_ORDERS - 1)]:
            r32 = case_step(case, case['state'], k, torch.float32, order)
            for net in r64:
                errs = {name: rel_l2(r32[net]['grads'][name].numpy(), g.numpy()) for name, g in r64[net]['grads'].items()}
                errs.update((sc, rel_l2(float(r32[net][sc]), float(r64[net][sc]))) for sc in SCALARS[net])
                if net != 'actor':
                    v64 = r64[net]['value'].numpy() if order is None else r64[net]['value'].numpy()[order]
                    rms = float(np.sqrt(np.mean((r32[net]['value'].numpy().astype(np.float64) - v64) ** 2)))
                    ob = out_bias(case)  # (OUT_BIAS wherever the critics have two hidden layers)
                    errs[ob + '/rows'] = 2.0 / math.sqrt(n) * rms / abs(float(r64[net]['grads'][ob]))
                for dst in (worst,) if order is not None else (worst, single):
                    o = dst.setdefault(net, {})
                    for name, e in errs.items():
                        o[name] = max(o.get(name, 0.0), e)
    return worst, single


def pack_f32_error(table: dict) -> dict:
    """{case: (worst, single)} -> the layout of tests/golden/step_twin_f32_error.json: every distinct per-network
    block once (cases that share a network's inputs share its figures), as [worst..., single...] in the order of
    `keys`; `cases` maps case and network to a block."""
    keys, blocks, index, cases = {}, [], {}, {}
    for name, (worst, single) in table.items():
        cases[name] = {}
        for net in worst:
            keys.setdefault(net, list(worst[net]))
            assert list(worst[net]) == keys[net] == list(single[net])
            blk = (net,) + tuple(float(f'{d[k]:.2e}') for d in (worst[net], single[net]) for k in keys[net])
            if blk not in index:
                index[blk] = len(blocks)
                blocks.append(list(blk[1:]))
            cases[name][net] = index[blk]
    return {'keys': keys, 'blocks': blocks, 'cases': cases}


def load_f32_error(path: str) -> tuple:
    """-> (worst, single), each {case: {network: {tensor or scalar: error}}}."""
    import json

    blob = json.load(open(path))
    worst, single = {}, {}
    for name, nets in blob['cases'].items():
        worst[name], single[name] = {}, {}
        for net, b in nets.items():
            ks, row = blob['keys'][net], blob['blocks'][b]
            worst[name][net] = dict(zip(ks, row[:len(ks)]))
            single[name][net] = dict(zip(ks, row[len(ks):]))
    return worst, single


def pack_general_error(table: dict) -> dict:
    """{case: (worst, single)} -> the layout of tests/golden/general_twin_f32_error.json: per case and network
    {tensor or scalar: [worst, single]} (the networks of general_table() differ from case to case: no shared keys)."""
    return {'cases': {name: {net: {k: [float(f'{worst[net][k]:.2e}'), float(f'{single[net][k]:.2e}')] for k in worst[net]}
                             for net in worst} for name, (worst, single) in table.items()}}


def load_general_error(path: str) -> tuple:
    """-> (worst, single), each {case: {network: {tensor or scalar: error}}}, as load_f32_error."""
    import json

    blob = json.load(open(path))['cases']
    return tuple({name: {net: {k: v[i] for k, v in d.items()} for net, d in nets.items()} for name, nets in blob.items()}
                 for i in (0, 1))


# ---------------------------------------------------------------------------------------------------------------------
# the launch plan of a case on the layer-wise path: osa_gmlp_plan, host only
# ---------------------------------------------------------------------------------------------------------------------
PLAN_HEAD, PLAN_LAUNCH = 59, 15  # OSA_GMLP_PLAN_HEAD, OSA_GMLP_PLAN_LAUNCH (include/omnisafe_amd.h)


def gmlp_desc(case: dict):
    """The osa_gmlp_desc of a case's networks."""
    from omnisafe_amd.models import ACTIVATIONS as CODES, GmlpDesc

    d = GmlpDesc()
    d.obs_dim, d.act_dim = case['obs_dim'], case['act_dim']
    for i, net in enumerate(NETS):
        widths = case_hidden(case, net) + [case['act_dim'] if net == 'actor' else 1]
        d.n_layers[i] = len(widths)
        for l, w in enumerate(widths):
            d.width[i][l] = w
        d.activation[i] = CODES[case_act(case, net)]
    return d


def gmlp_plan(case: dict, rows: int | None = None, mode: int = 0) -> dict:
    """What osa_gmlp_minibatch_ext will launch for a minibatch of `rows` rows (the case's B) of the case, in THIS
    process and its environment."""
    import ctypes as C

    from omnisafe_amd import _lib
    from omnisafe_amd.models import HParams

    lib = _lib.load()
    hp = HParams()
    hp.use_cost = int(case['use_cost'])
    hp.use_critic_norm = int(case['hp']['use_critic_norm'])
    mask = sum(1 << NETS.index(net) for net in case_nets(case))
    out = (C.c_int * 4096)()
    desc = gmlp_desc(case)
    _lib.check(lib.osa_gmlp_plan(C.byref(desc), int(case['B'] if rows is None else rows), int(case['loss_kind']), mode,
                                 mask, C.byref(hp), out, len(out)), 'osa_gmlp_plan')
    r = list(out[:out[0]])
    grid = lambda o: [r[o + 8 * i:o + 8 * i + 8] for i in range(3)]  # noqa: E731
    plan = dict(skinny=bool(r[1]), fusedn=bool(r[2]), top_in_fwd=[bool(x) for x in r[3:6]],
                loss_fused=[bool(x) for x in r[6:9]], sk_maxT1=r[9], sk_tk=grid(10), S=grid(34), mask=mask, launches=[])
    assert len(r) == PLAN_HEAD + PLAN_LAUNCH * r[PLAN_HEAD - 1]
    for i in range(r[PLAN_HEAD - 1]):
        q = r[PLAN_HEAD + PLAN_LAUNCH * i:PLAN_HEAD + PLAN_LAUNCH * (i + 1)]
        plan['launches'].append(dict(TM=q[0], TN=q[1], BK=q[2], AT=q[3], BT=q[4], splits=q[5], rowS=q[6], nprob=q[7],
                                     Si=q[8:8 + q[7]], psplits=q[11:11 + q[7]], xcd=q[14]))
    return plan


def plan_features(plan: dict) -> set:
    """The vocabulary of general_table()'s `features`."""
    f = {'skinny' if plan['skinny'] else 'tiled'}
    active = [i for i in range(3) if (plan['mask'] >> i) & 1]
    if plan['skinny']:
        f.add('fusedn' if plan['fusedn'] else 'no-fusedn')
        fwd = [plan['top_in_fwd'][i] for i in active]
        if all(fwd):
            f.add('top-in-fwd:all')
        elif 0 in active and not plan['top_in_fwd'][0] and any(fwd):
            f.add('top-in-fwd:critics')
        f.add('loss-fused' if all(plan['loss_fused'][i] for i in active) else 'loss-plain')
        if any(tk == 2 for i in active for tk in plan['sk_tk'][i]):
            f.add('tk2')
        return f
    f.add(f"S{max(s for i in active for s in plan['S'][i])}")
    if not any(q['rowS'] for q in plan['launches']):
        f.add('row-split-off')
    for q in plan['launches']:
        form = {(0, 0): 'NT', (0, 1): 'NN', (1, 1): 'TN'}[(q['AT'], q['BT'])]
        f.add(form)
        f.add(f"k{q['TM']}x{q['TN']}x{q['BK']}{form}")
        f.add(f"BK{q['BK']}")
        if q['rowS']:
            f.add(f"rowS{q['rowS']}")
            if min(q['Si']) < q['rowS']:
                f.add('Si<S')
        if q['TM'] == 128:
            f.add('TM128xTN128' if q['TN'] == 128 else 'TM128')
        elif q['TN'] == 128:
            f.add('TN128')
    return f


def plan_kernels(plan: dict) -> set:
    """The instantiations (TM, TN, BK, AT, BT) of gm_gemm_kernel a step of this plan launches."""
    return {(q['TM'], q['TN'], q['BK'], q['AT'], q['BT']) for q in plan['launches']}


# ---------------------------------------------------------------------------------------------------------------------
# data parallelism: the step of W ranks (tests/test_dp_twin.py on the CPU, tests/test_dp_forms_gpu.py on the device)
# ---------------------------------------------------------------------------------------------------------------------
# What makes W ranks different from one minibatch of W n rows (reference: every rank runs _update on ITS rows,
# algorithms/on_policy/base/policy_gradient.py:428-445 / 468-485 / 514-524; clip_grad_norm_ comes BEFORE
# distributed.avg_grads, policy_gradient.py:437-443; avg_grads is all_reduce(SUM) / world_size, utils/distributed.py:167-198):
#
#   gradient   for rank r = 0 .. W - 1 the gradient g_r of the rank's loss on ITS n rows -- every mean over n, the critics'
#              L2 term once per rank -- exactly step()'s `grads`; its norm gives coef_r = min(1, max_grad_norm / (|g_r| + 1e-6))
#   average    g = (1 / W) sum_r coef_r g_r, summed in rank order
#   update     ONE Adam step on g (adam(), the step count advances by one whatever W)
#   chunked    a rank whose minibatch is spread over 64-row chunk workgroups: g_r is the SUM of its chunks' shares (each
#              scaled by 1 / n, the L2 and entropy terms from chunk 0 alone), THEN its norm, THEN the rank's factor
#              (csrc/ppo_pass_body.h, `chunk_norm`) -- the same formula: a mean over n rows is a mean over n rows
#   statistics every logged scalar is the mean over the ranks of the rank's own value (what Logger.get_stats averages):
#              loss, mean ratio, entropy, sum p^2, the UNCLIPPED gradient norm |g_r|, MSE.  osa_dp_apply_kernel writes them
#              to columns 0..9 and nothing to columns 10..15; the cooperative forms (osa_ppo_dp_pass_placed,
#              osa_ppo_dp_chunked_pass -- whose chunk-0 leader forms the rank's loss and ratio as the sum of its chunks'
#              shares and takes sum p^2 and the entropy from chunk 0 -- and osa_ppo_split_dp_pass) write the same ten
#              columns and, per step of the launch, Adam's bias corrections float32(lr / (1 - b1^t)), float32(1 / sqrt(1 - b2^t))
#              to columns 10 + 2 net, 11 + 2 net, as the single-rank passes do.
#   layout     a case is make_case's data for W M rows; rank r owns rows r M .. r M + M - 1 and minibatch k of rank r is
#              perm[r, k B:(k + 1) B] + r M (PPOUpdater.run_pass_replicated).  Extended surrogates have no DP form.


def dp_step(state: dict, batches: list, hp: dict, lam: float, loss_kind: int, dtype=torch.float64, nets=NETS,
            acts: dict | None = None) -> dict:
    """One data-parallel optimiser step: `batches` holds the W ranks' minibatches (rank order).

    Returns {net: {...}}: `g` the averaged clipped gradient per reference tensor, p' / m' / v' / t / step_size /
    inv_bc2_sqrt of the ONE Adam step on it, every scalar of SCALARS (and the critics' `loss`) as the mean over the ranks,
    `coefs` / `gnorms` the ranks' factors and unclipped norms, `ranks` the W results of step()."""
    W = len(batches)
    ranks = [step(state, b, hp, lam, loss_kind, None, dtype, nets, acts) for b in batches]
    full = dict(DEFAULT_HP, **hp)
    f = {k: _f32(full[k]) for k in ('lr_actor', 'lr_critic', 'beta1', 'beta2', 'adam_eps')}
    as_t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    out = {}
    for net in nets:
        g = OrderedDict()
        for k in ranks[0][net]['grads']:
            acc = None
            for r in ranks:
                term = r[net]['grads'][k] * r[net]['coef']
                acc = term if acc is None else acc + term
            g[k] = acc / W
        lr = f['lr_actor' if net == 'actor' else 'lr_critic']
        t = int(state['t'][net]) + 1
        new_p, new_m, new_v = OrderedDict(), OrderedDict(), OrderedDict()
        for k, gk in g.items():
            new_p[k], new_m[k], new_v[k] = adam(as_t(state['params'][net][k]), as_t(state['m'][net][k]),
                                                as_t(state['v'][net][k]), gk, lr, f['beta1'], f['beta2'], f['adam_eps'], t)
        ss, ib = bias_corrections(lr, f['beta1'], f['beta2'], t)
        res = dict(g=g, p=new_p, m=new_m, v=new_v, t=t, step_size=ss, inv_bc2_sqrt=ib, ranks=[r[net] for r in ranks],
                   coefs=[float(r[net]['coef']) for r in ranks], gnorms=[float(r[net]['gnorm']) for r in ranks])
        for sc in SCALARS[net] + (() if net == 'actor' else ('loss',)):
            acc = None
            for r in ranks:
                acc = r[net][sc] if acc is None else acc + r[net][sc]
            res[sc] = acc / W
        out[net] = res
    return out


def dp_minibatch(case: dict, k: int, orders=None) -> list:
    """The W ranks' row indices of minibatch k (`orders`: per rank another order of its rows -- the same step)."""
    s, n = minibatches(case['M'], case['B'])[k]
    idx = [case['perm'][r, s:s + n] + r * case['M'] for r in range(case['W'])]
    return idx if orders is None else [i[o] for i, o in zip(idx, orders)]


def dp_case_step(case: dict, state: dict, k: int, dtype=torch.float64, orders=None) -> dict:
    """Minibatch k of the case's data-parallel pass, taken from `state`."""
    return dp_step(state, [rows(case['data'], i) for i in dp_minibatch(case, k, orders)], case['hp'], case['lam'],
                   case['loss_kind'], dtype, case_nets(case), case_acts(case))


def dp_run_pass(case: dict, dtype=torch.float64, state: dict | None = None) -> tuple:
    """The whole data-parallel pass: ceil(M / B) dependent steps -> ([step results], final state)."""
    state = case['state'] if state is None else state
    res = []
    for k in range(len(minibatches(case['M'], case['B']))):
        res.append(dp_case_step(case, state, k, dtype))
        state = advance(state, res[-1])
    return res, state


def make_dp_case(obs_dim: int, act_dim: int, W: int, B: int, M: int, *, norm_clip=None, **kw) -> dict:
    """A data-parallel case: make_case's inputs for W M rows (every stream of make_case as it is), laid out rank by rank.

    layout     position j of rank r's pass takes the row make_case put at position r M + j of ITS pass, so a minibatch of
               a rank is a run of consecutive positions and holds the six clip cells as make_case arranged them; inside
               the rank's M rows the rows sit in a seeded random order (`perm`, (W, M), drawn from a stream of its own)
    ranks      rank r's targets and advantages are multiplied by float32(1 + r / W) after everything is drawn: the
               ranks' gradient norms differ by tens of percent, so a factor taken from another rank, from the mean of
               the ranks or from the averaged gradient is a visible error (tests/test_dp_twin.py computes each)
    norm_clip  None: max_grad_norm = 1000 bites on no rank;  ('straddle', net): the geometric mean of the two middle
               per-rank float64 norms of that network on the first minibatch -- half the ranks clip, half do not (an
               odd world has a middle pair on either side of its median rank: the pair that lies further apart);
               ('all', 0.5): half the smallest norm of any rank and network on the first minibatch -- every rank clips
    """
    assert kw.get('ext') is None and W >= 1
    case = make_case(obs_dim, act_dim, B, W * M, norm_clip=None, **kw)
    rs = np.random.RandomState(770077 + 131 * obs_dim + 17 * act_dim + 7 * B + M + 1009 * W + kw.get('seed', 0))
    perm = np.stack([rs.permutation(M) for _ in range(W)]).astype(np.int64)
    src = np.empty(W * M, np.int64)
    for r in range(W):
        src[r * M + perm[r]] = case['perm'][r * M:(r + 1) * M]
    data = {k: np.ascontiguousarray(np.asarray(v)[src]) for k, v in case['data'].items()}
    for r in range(W):
        fac = F32(1.0 + r / W)
        for k in ('target_value_r', 'target_value_c', 'adv_r', 'adv_c'):
            data[k][r * M:(r + 1) * M] *= fac
    case.update(W=int(W), M=int(M), perm=perm, data=data, norm_clip=norm_clip)
    if norm_clip is not None:
        which, arg = norm_clip
        r0 = dp_case_step(dict(case, update_actor=True, update_critics=True, use_cost=True), case['state'], 0)
        if which == 'straddle':
            assert W >= 2
            norms = sorted(r0[arg]['gnorms'])
            # (an odd world has two middle pairs, below and above the median rank: the one with the wider gap)
            lo, hi = max(((norms[i], norms[i + 1]) for i in {(W - 2) // 2, (W - 1) // 2}), key=lambda p: p[1] / p[0])
            case['hp']['max_grad_norm'] = _f32(math.sqrt(lo * hi))
        else:
            assert which == 'all'
            case['hp']['max_grad_norm'] = _f32(arg * min(min(r0[net]['gnorms']) for net in NETS))
        case['norms0'] = {net: r0[net]['gnorms'] for net in NETS}
    return case


def dp_check_coverage(case: dict) -> dict:
    """Asserts that the case reaches what it is in the table for.  At the case's INITIAL state, where the GPU tests take
    every minibatch's gradient: every rank's every minibatch holds its clip cells with every ratio at least 1e-3 from
    the clip edges (float32 and float64 take the same branch), as check_coverage asks of a single rank; a case with
    seeded moments, whose float64 CHAIN the GPU tests compare, meets the same along the chain.  A case without
    norm_clip clips on no rank anywhere.  A clipped case, on its first minibatch (the one max_grad_norm was placed
    on; a tail of a few rows has norms of its own, and tests/test_dp_twin.py holds every minibatch to the
    right-from-wrong condition instead):
      ('straddle', net)  at least one rank of that network with coef <= 0.95 and at least one with norm <= 0.95 max_grad_norm
      ('all', .)         every rank of every network the case updates has coef < 1."""
    clip = _f32(case['hp']['clip'])
    info = {'edge': np.inf, 'coefs': []}
    seen = set()
    nmb = len(minibatches(case['M'], case['B']))
    first = [dp_case_step(case, case['state'], k) for k in range(nmb)]
    chain = dp_run_pass(case)[0]
    for k, r in enumerate(first + (chain if case['seeded_moments'] else [])):
        if 'actor' in r:
            for a in r['actor']['ranks']:
                ratio, adv = a['ratio'].numpy(), a['adv'].numpy()
                edge = np.minimum(np.abs(ratio - (1 - clip)), np.abs(ratio - (1 + clip))).min()
                info['edge'] = min(info['edge'], float(edge))
                assert edge >= 1e-3 and np.abs(adv).min() > 0, (k, edge)
                rng = np.where(ratio < 1 - clip, 0, np.where(ratio > 1 + clip, 2, 1))
                cells = {(int(g), bool(s)) for g, s in zip(rng, adv > 0)}
                assert len(cells) == min(len(ratio), 6), (k, sorted(cells))
                seen |= cells
    if case['update_actor']:
        assert len(seen) == 6, sorted(seen)
    mg = _f32(case['hp']['max_grad_norm'])
    if case['norm_clip'] is None:
        if case['hp']['use_max_grad_norm']:
            assert all(c == 1.0 for r in chain + first for net in r for c in r[net]['coefs'])
    else:
        which, arg = case['norm_clip']
        for k, r in enumerate(first):
            for net in r:
                info['coefs'].append((k, net, [round(c, 3) for c in r[net]['coefs']]))
        for net, r in first[0].items():
            if which == 'all':
                assert all(c < 1.0 for c in r['coefs']), (net, r['coefs'])
            elif net == arg:
                assert min(r['coefs']) <= 0.95 and min(r['gnorms']) <= 0.95 * mg, (net, r['coefs'], r['gnorms'], mg)
    if case.get('w1_scale', 1.0) != 1.0:
        info['saturated'] = first_layer_saturation(case)
        assert max(info['saturated'].values()) <= 0.02, info['saturated']
    return info


def dp_wrong_statements(case: dict, k: int, state: dict | None = None) -> dict:
    """{what: {net: {tensor: gradient}}}: statements of minibatch k's averaged gradient that are NOT the data-parallel
    step, in float64, next to 'right' -- what a kernel would compute that
      clip-after-average   averaged the unclipped gradients and clipped the average by its own norm
      mean-factor          applied the mean of the ranks' factors to every rank
      next-rank-factor     applied rank (r + 1 mod W)'s factor to rank r
      sum                  summed the clipped gradients without dividing by W
      tail-over-B          (a minibatch of n < B rows) divided the ranks' row sums by B: the data term of every rank's
                           gradient (everything but the critics' L2 term 2 c p) x n / B, norms and factors from that."""
    state = case['state'] if state is None else state
    r = dp_case_step(case, state, k)
    hp = dict(DEFAULT_HP, **case['hp'])
    mg, use = _f32(hp['max_grad_norm']), bool(hp['use_max_grad_norm'])
    W, (_, n) = case['W'], minibatches(case['M'], case['B'])[k]

    def factor(norm):
        return min(1.0, mg / (float(norm) + 1e-6)) if use else 1.0

    def norm_of(g):
        return math.sqrt(sum(float((x * x).sum()) for x in g.values()))

    out = {w: {} for w in ('right', 'clip-after-average', 'mean-factor', 'next-rank-factor', 'sum')}
    if n < case['B']:
        out['tail-over-B'] = {}
    for net, res in r.items():
        gr = [rk['grads'] for rk in res['ranks']]
        c = res['coefs']
        avg = lambda coefs, grads=gr: OrderedDict((t, sum(cf * g[t] for cf, g in zip(coefs, grads)) / W) for t in grads[0])  # noqa: E731
        out['right'][net] = res['g']
        plain = avg([1.0] * W)
        fa = factor(norm_of(plain))
        out['clip-after-average'][net] = OrderedDict((t, fa * x) for t, x in plain.items())
        out['mean-factor'][net] = avg([sum(c) / W] * W)
        out['next-rank-factor'][net] = avg([c[(i + 1) % W] for i in range(W)])
        out['sum'][net] = OrderedDict((t, W * x) for t, x in res['g'].items())
        if n < case['B']:
            l2 = (2.0 * _f32(hp['critic_norm_coef'])) if (net != 'actor' and hp['use_critic_norm']) else 0.0
            p = state['params'][net]
            wrong = []
            for g in gr:
                reg = {t: l2 * torch.as_tensor(np.asarray(p[t], np.float64)) for t in g}
                wrong.append(OrderedDict((t, (g[t] - reg[t]) * (n / case['B']) + reg[t]) for t in g))
            out['tail-over-B'][net] = avg([factor(norm_of(g)) for g in wrong], wrong)
    return out


def dp_state_tolerances(r: dict, units: dict, net: str, k_grad: float) -> dict:
    """state_tolerances of tests/test_step_oracle_gpu.py for a data-parallel step.  There the clipped gradient is the
    unclipped one times ONE factor, both observed, and the factor's own tolerance (`ec`) is added to the gradient's.
    Here the ranks' factors are not observable -- the kernels publish the rank-averaged norm alone -- and they are
    INSIDE g = (1 / W) sum_r coef_r g_r, the quantity whose float32 error `units` measures (dp_f32_error) and the GPU
    test bounds by k_grad units; so dg = k_grad unit |g| with no second term:
      |dm| <= (1 - b1) dg + 2^-23 |m'|,   |dv| <= (1 - b2) dg max|2.5 g| + 2^-22 |v'|."""
    omb1, omb2 = float(F32(1) - F32(0.9)), float(F32(1) - F32(0.999))
    out = {}
    for t, g in r[net]['g'].items():
        g = g.numpy()
        dg = k_grad * units[t] * np.linalg.norm(g)
        out[t] = (omb1 * dg + 2.0 ** -23 * np.linalg.norm(r[net]['m'][t].numpy()),
                  omb2 * dg * 2.5 * np.abs(g).max() + 2.0 ** -22 * np.linalg.norm(r[net]['v'][t].numpy()))
    return out


def dp_f32_error(case: dict) -> tuple:
    """f32_error for a data-parallel case: the float32 run of dp_case_step against its float64 run on every minibatch
    from the case's INITIAL state -- per reference tensor of the AVERAGED CLIPPED gradient g (the quantity the device
    shows; the ranks' factors are inside it) and per rank-mean scalar -- worst of ROW_ORDERS orders of the rows, permuted
    within each rank (`worst`), and with the rows as drawn (`single`).

    The critics' one-element output bias gets the second unit of OUT_BIAS_ROWS, stated for W ranks: its gradient is
    (1 / W) sum_r coef_r (2 / n) sum_rows (v - target) (+ L2), W n independent forward errors of rms_r each, typically
    (1 / W) sqrt(sum_r (coef_r (2 / sqrt n) rms_r)^2) / |g_64| -- from the float32 TWIN's forward values."""
    worst, single = {}, {}
    W = case['W']
    for k, (_, n) in enumerate(minibatches(case['M'], case['B'])):
        r64 = dp_case_step(case, case['state'], k)
        rs = np.random.RandomState(977 + k)
        for orders in [None] + [[rs.permutation(n) for _ in range(W)] for _ in range(ROW_ORDERS - 1)]:
            r32 = dp_case_step(case, case['state'], k, torch.float32, orders)
            for net in r64:
                errs = {name: rel_l2(r32[net]['g'][name].numpy(), g.numpy()) for name, g in r64[net]['g'].items()}
                errs.update((sc, rel_l2(float(r32[net][sc]), float(r64[net][sc]))) for sc in SCALARS[net])
                if net != 'actor':
                    ob, acc = out_bias(case), 0.0
                    for i in range(W):
                        v64 = r64[net]['ranks'][i]['value'].numpy()
                        v64 = v64 if orders is None else v64[orders[i]]
                        rms = float(np.sqrt(np.mean((r32[net]['ranks'][i]['value'].numpy().astype(np.float64) - v64) ** 2)))
                        acc += (r64[net]['coefs'][i] * 2.0 / math.sqrt(n) * rms) ** 2
                    errs[ob + '/rows'] = math.sqrt(acc) / W / abs(float(r64[net]['g'][ob]))
                for dst in (worst,) if orders is not None else (worst, single):
                    o = dst.setdefault(net, {})
                    for name, e in errs.items():
                        o[name] = max(o.get(name, 0.0), e)
    return worst, single


# form -> how PPOUpdater.run_pass_replicated is brought to it (coop / use_graph arguments, environment, the wide
# switch _repl_wide) and what PPOUpdater._dp must report afterwards
DP_FORMS = OrderedDict([
    ('dp-steps', dict(coop=False, graph=False, env={})),  # osa_ppo_dp_step + osa_dp_apply_kernel, osa_ppo_dp_end_pass
    ('dp-steps-graph', dict(coop=False, graph=True, env={})),  # the same launches: warm pass, capture, replay
    ('dp-coop', dict(coop=True, env={'OSA_DP_XCH': 'local'}, chunked=False, local=True)),  # osa_ppo_dp_pass_placed
    ('dp-coop-uncached', dict(coop=True, env={'OSA_DP_XCH': 'uncached'}, chunked=False, local=False)),
    ('dp-coop-walk', dict(coop=True, env={'OSA_CHUNKED_PASS': '0'}, chunked=False, local=True)),  # B > 64, one workgroup per rank
    ('dp-chunked', dict(coop=True, env={}, chunked=True, local=True)),  # osa_ppo_dp_chunked_pass
    ('dp-split', dict(wide=True, env={'OSA_WIDE_DP': 'place'}, place=True)),  # osa_ppo_split_dp_pass
    ('dp-split-spread', dict(wide=True, env={'OSA_WIDE_DP': 'spread'}, place=False)),
])
DP_ENV_KEYS = ('OSA_DP_XCH', 'OSA_CHUNKED_PASS', 'OSA_WIDE_DP', 'OSA_WIDE_SPLIT', 'OSA_DEBUG_PLACEMENT', 'OSA_DP_PLAIN_LAUNCH')
# (obs, act, W, B, M per rank): the smallest shapes at which each mechanism is at work
DP_NARROW = [(60, 2, 2, 64, 65),    # a tail of one row on every rank
             (60, 2, 3, 48, 100),   # B no multiple of 16, an odd world, a tail of 4
             (65, 17, 8, 64, 100),  # two output tiles, an observation width that is no multiple of 4; one rank per XCC
             (1, 1, 1, 5, 12),      # a world of one
             (60, 2, 11, 64, 64),   # more ranks than XCCs, an odd count
             (60, 2, 16, 64, 64)]
DP_CHUNK = [(60, 2, 2, 65, 130),    # a second chunk of one row
            (65, 17, 3, 128, 300),  # a tail of 44 rows: one empty chunk on every rank
            (60, 2, 8, 200, 500),   # two empty chunks; 8 x 4 = 32 peers, the local-placement limit
            (27, 8, 16, 128, 128)]  # 16 ranks, the chunked form's limit
DP_WIDE = [(376, 17, 2, 64, 65), (376, 17, 8, 40, 100), (97, 3, 3, 64, 100), (193, 5, 5, 5, 12)]
# the variants: one shape per family on the family's cooperative form (narrow: also on the stepwise form)
DP_VARIANT_SHAPES = [((65, 17, 8, 64, 100), ('dp-coop', 'dp-steps')), ((65, 17, 3, 128, 300), ('dp-chunked',)),
                     ((376, 17, 2, 64, 65), ('dp-split',))]


def dp_variants() -> 'OrderedDict[str, dict]':
    v = OrderedDict()
    v['losskind1'] = dict(loss_kind=1)
    v['lam-0'] = dict(lam=0.0)
    v['nocost'] = dict(use_cost=False)
    v['actor-off'] = dict(update_actor=False)
    v['critics-off'] = dict(update_critics=False)
    v['l2-off'] = dict(use_critic_norm=0)
    v['l2-0.05'] = dict(critic_norm_coef=0.05)
    for net in NETS:
        v[f'straddle-{net}'] = dict(norm_clip=('straddle', net))
    v['normclip-all'] = dict(norm_clip=('all', 0.5))
    v['normclip-off'] = dict(use_max_grad_norm=0)
    v['seeded'] = dict(seeded_moments=True, t0=(3, 5, 7))
    v['t0-250000'] = dict(seeded_moments=True, t0=(250000, 250000, 250000))
    v['lr'] = dict(lr_actor=3e-4, lr_critic=1e-3, seeded_moments=True, t0=(3, 5, 7))
    return v


def dp_kw(od: int, ad: int, W: int, B: int, M: int) -> dict:
    kw = dict(obs_dim=od, act_dim=ad, W=W, B=B, M=M)
    return dict(kw, w1_scale=math.sqrt(64.0 / od)) if od > 96 else kw  # (the wide family: wide_kw)


def dp_name(tag: str, kw: dict) -> str:
    return f"{tag}-{kw['obs_dim']}x{kw['act_dim']}-W{kw['W']}-B{kw['B']}-M{kw['M']}"


def dp_table() -> 'OrderedDict[str, dict]':
    """name -> dict(kw = make_dp_case keyword arguments, forms = the DP_FORMS the case runs on[, tail = (rows, empty
    chunks)]); names end in the shape and -W<ranks>-B<batch>-M<rows per rank>, which no name of the other tables does."""
    t = OrderedDict()

    def add(tag, kw, forms, **more):
        name = dp_name(tag, kw)
        assert name not in t
        t[name] = dict(kw=kw, forms=tuple(forms), **more)

    for i, shape in enumerate(DP_NARROW):
        forms = ('dp-steps', 'dp-coop') + (('dp-steps-graph',) if i in (0, 2) else ()) + (
            ('dp-coop-uncached',) if i in (0, 4, 5) else ())
        add('base', dp_kw(*shape), forms)
    for i, shape in enumerate(DP_CHUNK):
        _, _, _, B, M = shape
        n = minibatches(M, B)[-1][1]
        add('base', dp_kw(*shape), ('dp-coop-walk', 'dp-chunked') + (('dp-steps',) if i == 1 else ()),
            tail=(n, empty_chunks(B, n)))
    for shape in DP_WIDE:
        add('base', dp_kw(*shape), ('dp-split',) + (('dp-split-spread',) if shape[:3] in ((376, 17, 8), (376, 17, 2)) else ()))
    for shape, forms in DP_VARIANT_SHAPES:
        for tag, change in dp_variants().items():
            add(tag, dict(dp_kw(*shape), **change), forms)
    # ---- seeded moments at worlds that are no power of two, on the other families' forms: 1 / W is then no exact
    # factor, and the average must reach both moments as ONE float32 number (DP_VARIANT_SHAPES has W = 3 on the
    # chunked form alone)
    seeded = dp_variants()['seeded']
    add('seeded', dict(dp_kw(60, 2, 3, 48, 100), **seeded), ('dp-steps', 'dp-coop'))
    add('seeded', dict(dp_kw(60, 2, 11, 64, 64), **seeded), ('dp-coop', 'dp-coop-uncached'))
    add('seeded', dict(dp_kw(97, 3, 3, 64, 100), **seeded), ('dp-split', 'dp-split-spread'))
    walk = dp_name('seeded', dp_kw(65, 17, 3, 128, 300))
    t[walk] = dict(t[walk], forms=t[walk]['forms'] + ('dp-coop-walk',))
    return t
