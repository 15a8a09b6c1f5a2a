"""The device side of off-policy TD3 / DDPG (csrc/td3_kernels.hip): the deterministic ``MLPActor`` and the ``QCritic``
blocks with the reference's state-dict names, their targets and Adam moments, the replay ring, the draws, acting and
the gradient step.

``Td3Actor`` is what the trainer and the players of a saved policy share: the actor block, its state dict and ``act``.
``Td3Step`` adds the critics, the ring, the device step counter and ``run(n)``, which enqueues n gradient steps on the
current stream with no host synchronisation; ``stats`` holds the per-step scalars ``[nslots][NSTAT]`` until the caller
reads them.  Draws come from ``draw(seed, first_step, n)`` (Philox on the device, indices below the ring's fill count
at that moment) or are injected with ``set_draws`` (tests).  ``OSA_TD3_ROUTE=layer|fused`` chooses how the step's
forward runs: one tile-GEMM launch per layer, or one launch of the row-resident kernel.

``Td3LagStep`` is the step of DDPGLag, TD3Lag, DDPGPID and TD3PID: the cost critic in the actor loss with the
multiplier read on the device, ``update_multiplier`` (one launch per update round) and, with ``cost_normalize``, the
cost normaliser inside ``store``.  ``OSA_TD3_LAG_DACT=stacked|gemm`` chooses layer 0 of the critics' data gradient.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .bcq_step import _get, _index, _set
from .crr_step import _init_mlp
from .models import ACTIVATIONS, GMLP_MAX_LAYERS

STAT_KEYS = ('Loss/Loss_reward_critic', 'Value/reward_critic', 'Loss/Loss_pi', 'Loss/Loss_cost_critic',
             'Value/cost_critic')  # columns 0 .. 4 of a statistics row
ROUTES = {'layer': 0, 'fused': 1}  # OSA_TD3_ROUTE_*
DEFAULT_ROUTE = 'layer'            # the faster one at the YAML shape: 285 v 369 us per step
MAX_ACT_DIM = 32


class Td3Desc(C.Structure):
    """ctypes mirror of ``osa_td3_desc``."""

    _fields_ = [('obs_dim', C.c_int), ('act_dim', C.c_int), ('n_hidden', C.c_int * 2),
                ('hidden', (C.c_int * GMLP_MAX_LAYERS) * 2), ('activation', C.c_int * 2), ('batch', C.c_int),
                ('num_critics', C.c_int), ('use_cost', C.c_int)]


class Td3HParams(C.Structure):
    """ctypes mirror of ``osa_td3_hparams``."""

    _fields_ = [('gamma', C.c_float), ('polyak', C.c_float), ('one_minus_polyak', C.c_float),
                ('policy_noise', C.c_float), ('policy_noise_clip', C.c_float), ('target_actor', C.c_int),
                ('policy_delay', C.c_int), ('lr_actor', C.c_float), ('lr_critic', C.c_float), ('beta1', C.c_double),
                ('beta2', C.c_double), ('adam_eps', C.c_double), ('max_grad_norm', C.c_float),
                ('critic_norm_coeff', C.c_float), ('route', C.c_int)]


class Td3State(C.Structure):
    """ctypes mirror of ``osa_td3_state``."""

    _fields_ = [(n, C.c_void_p) for n in ('actor', 'actor_m', 'actor_v', 'actor_t', 'critic', 'critic_m', 'critic_v',
                                           'critic_t', 'adam_step', 'step')]


class Td3Ring(C.Structure):
    """ctypes mirror of ``osa_td3_ring``."""

    _fields_ = [(n, C.c_void_p) for n in ('obs', 'act', 'reward', 'cost', 'done', 'next_obs', 'pos')] + [
        ('size', C.c_long), ('ld_obs', C.c_int), ('ld_act', C.c_int)]


class Td3DrawBuffers(C.Structure):
    """ctypes mirror of ``osa_td3_draw_buffers``."""

    _fields_ = [('idx', C.c_void_p), ('eps', C.c_void_p), ('nslots', C.c_int)]


def make_desc(obs_dim: int, act_dim: int, actor_hidden, critic_hidden, actor_act: str, critic_act: str, batch: int = 1,
              num_critics: int = 2, use_cost: bool = False) -> Td3Desc:
    """The description of a TD3 (``num_critics`` 2) or DDPG (1) problem; NotImplementedError, before any GPU is
    touched, for an activation outside the five, a network without a hidden layer or with more than
    GMLP_MAX_LAYERS - 1, a width outside 1 .. 4096 and act_dim outside 1 .. 32."""
    a_h, c_h = [int(h) for h in actor_hidden], [int(h) for h in critic_hidden]
    for name in (actor_act, critic_act):
        if name not in ACTIVATIONS:
            raise NotImplementedError(f'activation {name!r}: one of {list(ACTIVATIONS)}')
    if (any(h < 1 or h > 4096 for h in a_h + c_h) or min(len(a_h), len(c_h)) < 1
            or max(len(a_h), len(c_h)) + 1 > GMLP_MAX_LAYERS):
        raise NotImplementedError(f'hidden_sizes {a_h}/{c_h}: 1 .. {GMLP_MAX_LAYERS - 1} hidden layers of width 1 .. 4096')
    if not 1 <= int(act_dim) <= MAX_ACT_DIM:
        raise NotImplementedError(f'act_dim {act_dim}: the action head takes 1 .. {MAX_ACT_DIM} action dimensions')
    if int(num_critics) not in (1, 2):
        raise NotImplementedError(f'num_critics {num_critics}: 1 (DDPG) or 2 (TD3)')
    d = Td3Desc()
    d.obs_dim, d.act_dim = int(obs_dim), int(act_dim)
    for net, sizes in enumerate((a_h, c_h)):
        d.n_hidden[net] = len(sizes)
        for l, w in enumerate(sizes):
            d.hidden[net][l] = w
    d.activation[0], d.activation[1] = ACTIVATIONS[actor_act], ACTIVATIONS[critic_act]
    d.batch, d.num_critics, d.use_cost = int(batch), int(num_critics), int(bool(use_cost))
    return d


def _hidden(desc: Td3Desc, net: int) -> list[int]:
    return [int(desc.hidden[net][l]) for l in range(desc.n_hidden[net])]


class Td3Layout:
    """Offsets of the reference's tensors inside the padded blocks (osa_td3_layout).  Host only."""

    def __init__(self, desc, entry: str = 'osa_td3_layout', actor_out: int | None = None) -> None:
        """``entry`` / ``actor_out``: the layout function and the actor's top width of another description with the
        same ``out`` format (sac_step: osa_sac_layout, 2 act_dim)."""
        out = (C.c_int * (4 + 2 * GMLP_MAX_LAYERS * 3))()
        _lib.check(getattr(_lib.load(), entry)(C.byref(desc), out), entry)
        self.Pa, self.Pc, self.nstat = (int(x) for x in out[:3])
        D, A = int(desc.obs_dim), int(desc.act_dim)
        self.num_critics = int(getattr(desc, 'num_critics', 2))
        self._layers = []
        k = 4
        for sizes in ([D] + _hidden(desc, 0) + [actor_out or A], [D + A] + _hidden(desc, 1) + [1]):
            rows = []
            for l in range(GMLP_MAX_LAYERS):
                oW, ob, ld = int(out[k]), int(out[k + 1]), int(out[k + 2])
                k += 3
                if oW >= 0:
                    rows.append((oW, ob, ld, sizes[l + 1], sizes[l]))
            self._layers.append(rows)

    def tensors(self, net: int = 0, prefix: str = 'net') -> list[tuple[str, tuple[int, ...], np.ndarray]]:
        """``(name, shape, offsets)`` of the actor (net 0: ``net.0.weight, ...`` as ``MLPActor.state_dict()`` names
        them) or of one critic (net 1, prefix ``critic_j.0`` as ``QCritic.state_dict()`` does)."""
        items = []
        for j, (oW, ob, ld, n_out, n_in) in enumerate(self._layers[net]):
            ix = (oW + np.arange(n_out)[:, None] * ld + np.arange(n_in)[None, :]).reshape(-1)
            items.append((f'{prefix}.{2 * j}.weight', (n_out, n_in), ix))
            items.append((f'{prefix}.{2 * j}.bias', (n_out,), ob + np.arange(n_out)))
        return items

    def critic_tensors(self, n: int) -> list:
        """The tensors of a ``QCritic`` of n networks, block by block."""
        return [self.tensors(1, f'critic_{c}.0') for c in range(n)]


def route_of(desc: Td3Desc, name: str | None = None) -> int:
    """The forward's route: ``name`` or ``OSA_TD3_ROUTE`` where given -- ``fused`` on a shape the kernel does not take
    is an OsaError, not another kernel -- else the default where it is supported and ``layer`` where not."""
    name = os.environ.get('OSA_TD3_ROUTE', '') if name is None else name
    if name not in ('', 'layer', 'fused'):
        raise ValueError(f'OSA_TD3_ROUTE={name!r}: layer or fused')
    route = ROUTES[name or DEFAULT_ROUTE]
    if route == ROUTES['fused'] and not _lib.load().osa_td3_chain_supported(C.byref(desc)):
        if name:
            raise _lib.OsaError('OSA_TD3_ROUTE=fused: a hidden width above 256 or an observation too wide for the '
                                'forward kernel\'s LDS')
        route = ROUTES['layer']
    return route


class Td3Actor:
    """``MLPActor``: the actor block, its state dict and ``act``."""

    def __init__(self, desc, device, layout: Td3Layout | None = None) -> None:
        """``layout``: the layout of another description with the same block format (sac_step.SacLayout)."""
        self._lib = _lib.load(require_gpu=True)
        self.desc, self.device = desc, torch.device(device)
        self.layout = lay = layout or Td3Layout(desc)
        self.D, self.A, self.B = int(desc.obs_dim), int(desc.act_dim), int(desc.batch)
        self.f32 = dict(dtype=torch.float32, device=self.device)
        self.actor = torch.zeros(lay.Pa, **self.f32)
        self._ix = {'actor': _index(lay.tensors(), self.device)}

    def state_dict(self, which: str = 'actor'):
        """The keys, order and shapes of ``MLPActor.state_dict()`` (of the parameters; ``actor_m`` / ``actor_v`` /
        ``actor_t``: an Adam moment, the target)."""
        return _get(getattr(self, which), self._ix['actor'])

    def load_state_dict(self, sd, which: str = 'actor') -> None:
        _set(getattr(self, which), self._ix['actor'], sd)

    def act(self, obs: torch.Tensor, noise: float = 0.0, random: bool = False, seed: int = 0, offset: int = 0,
            out: torch.Tensor | None = None) -> torch.Tensor:
        """``MLPActor.predict`` of the rows of ``obs``: the tanh-headed forward, plus ``noise`` times a normal clamped
        to [-1, 1] (``noise`` 0: deterministic); ``random``: a uniform draw over the action box instead
        (``use_rand_action``).  Draws: Philox(seed, offset, element) on the device."""
        n = int(obs.shape[0])
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] == self.D \
            and obs.stride(1) == 1
        if out is None:
            out = torch.empty(n, self.A, **self.f32)
        p = _lib.ptr
        _lib.check(self._lib.osa_td3_act(C.byref(self.desc), p(self.actor), p(obs), obs.stride(0), n, int(bool(random)),
                                         float(noise), int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), p(out),
                                         out.stride(0), _lib.stream_ptr()), 'osa_td3_act')
        return out


class Td3Step(Td3Actor):  # pylint: disable=too-many-instance-attributes
    def __init__(self, desc: Td3Desc, *, size: int, gamma: float, polyak: float, lr_actor: float, lr_critic: float,
                 nslots: int, policy_noise: float = 0.0, policy_noise_clip: float = 0.0, policy_delay: int = 1,
                 target_actor: bool | None = None, max_grad_norm: float | None = None, critic_norm_coeff: float = 0.0,
                 route: str | None = None, device='cuda:0') -> None:
        self.route = route_of(desc, route)
        super().__init__(desc, device)
        self._init_training_state(size, nslots, int(desc.num_critics), 3)
        f32, B, A = self.f32, self.B, self.A
        self.eps = torch.zeros(self.nslots, B, A, **f32)
        self.ws_floats = int(self._lib.osa_td3_ws_floats(C.byref(desc)))
        self.ws = torch.zeros(self.ws_floats, **f32)
        self.hp = Td3HParams(gamma=gamma, polyak=polyak, one_minus_polyak=1.0 - polyak, policy_noise=policy_noise,
                             policy_noise_clip=policy_noise_clip,
                             target_actor=int(self.nq == 2 if target_actor is None else target_actor),
                             policy_delay=int(policy_delay), lr_actor=lr_actor, lr_critic=lr_critic, beta1=0.9,
                             beta2=0.999, adam_eps=1e-8, max_grad_norm=float(max_grad_norm or 0.0),
                             critic_norm_coeff=float(critic_norm_coeff), route=self.route)
        p = _lib.ptr
        self._state = Td3State(p(self.actor), p(self.actor_m), p(self.actor_v), p(self.actor_t), p(self.critic),
                               p(self.critic_m), p(self.critic_v), p(self.critic_t), p(self.adam_step), p(self.step))
        self._draws = Td3DrawBuffers(p(self.idx), p(self.eps), self.nslots)

    def _init_training_state(self, size: int, nslots: int, nq: int, n_adam: int) -> None:
        """What every off-policy step built on the actor block holds (``SacStep`` too): the Adam moments and targets,
        the critic blocks with their state-dict indices, the counters, the statistics rows, the index draws and the
        replay ring that ``store`` writes."""
        self.nslots, self.size = int(nslots), int(size)
        assert self.nslots >= 1 and self.size >= 1
        lay, f32, B, D, A = self.layout, self.f32, self.B, self.D, self.A
        self.nq, self.use_cost = int(nq), bool(self.desc.use_cost)
        nc = self.nq + int(self.use_cost)
        self.actor_m, self.actor_v, self.actor_t = (torch.zeros_like(self.actor) for _ in range(3))
        self.critic, self.critic_m, self.critic_v, self.critic_t = (torch.zeros(nc, lay.Pc, **f32) for _ in range(4))
        self.adam_step = torch.zeros(n_adam, dtype=torch.int32, device=self.device)
        self.step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.update_count = 0  # the host's mirror of ``step``: which steps update the actor
        self.stats = torch.zeros(self.nslots, lay.nstat, **f32)
        self.idx = torch.zeros(self.nslots, B, dtype=torch.int64, device=self.device)
        self.ring = {'obs': torch.zeros(self.size, D, **f32), 'act': torch.zeros(self.size, A, **f32),
                     'reward': torch.zeros(self.size, **f32), 'cost': torch.zeros(self.size, **f32),
                     'done': torch.zeros(self.size, **f32), 'next_obs': torch.zeros(self.size, D, **f32)}
        self.pos = torch.zeros(2, dtype=torch.int64, device=self.device)  # write position, rows filled
        p, r = _lib.ptr, self.ring
        self._ring = Td3Ring(p(r['obs']), p(r['act']), p(r['reward']), p(r['cost']), p(r['done']), p(r['next_obs']),
                             p(self.pos), self.size, D, A)
        self._ix['reward'] = [_index(t, self.device) for t in lay.critic_tensors(self.nq)]
        self._ix['cost'] = [_index(t, self.device) for t in lay.critic_tensors(1)]

    # ------------------------------------------------------------------ state dicts
    def _critic_blocks(self, name: str, which: str):
        block = getattr(self, which)
        return list(block[:self.nq]) if name == 'reward' else [block[self.nq]]

    def critic_state_dict(self, name: str = 'reward', which: str = 'critic'):
        """``QCritic.state_dict()`` of the reward critic (``critic_0.0.0.weight, ..., critic_1.0.0.weight, ...``) or of
        the one-network cost critic; ``which``: ``critic``, ``critic_m``, ``critic_v`` or ``critic_t``."""
        sd = OrderedDict()
        for blk, ix in zip(self._critic_blocks(name, which), self._ix[name]):
            sd.update(_get(blk, ix))
        return sd

    def load_critic_state_dict(self, sd, name: str = 'reward', which: str = 'critic') -> None:
        for blk, ix in zip(self._critic_blocks(name, which), self._ix[name]):
            _set(blk, ix, sd)

    def init_parameters(self, mode: str = 'kaiming_uniform') -> None:
        """The reference's initial weights for the current torch seed, in its construction order: the actor, the
        reward critics, the cost critic (actor_q_critic.py:70-100, constraint_actor_q_critic.py:70-78; the cost critic
        is drawn with or without ``use_cost``, as the reference builds it either way); targets are copies."""
        D, A = self.D, self.A
        sd = OrderedDict()
        for j, (w, b) in enumerate(_init_mlp([D] + _hidden(self.desc, 0) + [A], mode)):
            sd[f'net.{2 * j}.weight'], sd[f'net.{2 * j}.bias'] = w, b
        self.load_state_dict(sd)
        for name, n in (('reward', self.nq), ('cost', 1)):
            sd = OrderedDict()
            for c in range(n):
                for j, (w, b) in enumerate(_init_mlp([D + A] + _hidden(self.desc, 1) + [1], mode)):
                    sd[f'critic_{c}.0.{2 * j}.weight'], sd[f'critic_{c}.0.{2 * j}.bias'] = w, b
            if name == 'reward' or self.use_cost:
                self.load_critic_state_dict(sd, name)
        self.actor_t.copy_(self.actor)
        self.critic_t.copy_(self.critic)

    # ------------------------------------------------------------------ ring
    def store(self, obs, act, reward, cost, terminated, truncated, next_obs, final_obs=None, final_mask=None,
              episodes: tuple | None = None) -> None:
        """``n`` transitions into the ring at the device-held write position (one launch; ``done`` = ``terminated``).
        ``final_obs`` / ``final_mask``: rows whose mask byte is set store ``final_obs`` as their ``next_obs``.
        ``episodes = (acc [n][3], out [cap][3], count [1])``: running and finished returns, costs, lengths."""
        n = int(obs.shape[0])
        p = _lib.ptr
        acc, out, count = episodes or (None, None, None)
        _lib.check(self._lib.osa_td3_store(
            C.byref(self._ring), n, self.D, self.A, p(obs), obs.stride(0), p(act), act.stride(0), p(reward), p(cost),
            p(terminated), p(truncated), p(next_obs), next_obs.stride(0), p(final_obs),
            final_obs.stride(0) if final_obs is not None else 0, p(final_mask), p(acc), p(out),
            int(out.shape[0]) if out is not None else 0, p(count), _lib.stream_ptr()), 'osa_td3_store')

    # ------------------------------------------------------------------ draws
    def draw(self, seed: int, first_step: int, nsteps: int = 1) -> None:
        """The device draws of steps first_step .. first_step + nsteps - 1 into their slots; the indices are uniform
        over the rows the ring holds when the launch runs."""
        assert 1 <= nsteps <= self.nslots
        p = _lib.ptr
        _lib.check(self._lib.osa_td3_draws(C.byref(self.desc), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_step),
                                           int(nsteps), self.nslots, C.byref(self._ring), p(self.idx), p(self.eps),
                                           _lib.stream_ptr()), 'osa_td3_draws')

    def set_draws(self, first_step: int, idx, eps) -> None:
        """Inject the draws of consecutive steps (leading dimension = steps) into their slots."""
        idx = torch.as_tensor(idx, dtype=torch.int64)
        n = idx.shape[0]
        assert 1 <= n <= self.nslots
        if int(idx.min()) < 0 or int(idx.max()) >= self.size:
            raise ValueError(f'indices outside [0, {self.size})')
        slots = (torch.arange(n) + int(first_step)) % self.nslots
        self.idx[slots] = idx.reshape(n, self.B).to(self.device)
        self.eps[slots] = torch.as_tensor(eps).reshape(n, self.B, self.A).to(**self.f32)

    # ------------------------------------------------------------------ the step
    def run(self, nsteps: int = 1) -> None:
        """Enqueue ``nsteps`` gradient steps on the current stream (ddpg.py:382-400 each)."""
        _lib.check(self._lib.osa_td3_step(
            C.byref(self.desc), C.byref(self.hp), C.byref(self._state), C.byref(self._ring), C.byref(self._draws),
            _lib.ptr(self.stats), _lib.ptr(self.ws), self.ws_floats, self.update_count, int(nsteps),
            _lib.stream_ptr()), 'osa_td3_step')
        self.update_count += int(nsteps)


# ---------------------------------------------------------------------- TD3Lag / DDPGLag / TD3PID / DDPGPID
LAG_STAT_KEYS = STAT_KEYS + ('Metrics/LagrangeMultiplier',)  # column 5: OSA_TD3_LAG_COL
DACTS = {'gemm': 0, 'stacked': 1}  # OSA_TD3_LAG_DACT_*
DEFAULT_DACT = 'stacked'           # the faster one at the YAML shape: 326 v 332 us per step
DACT_MAX_WIDTH = 1024              # OSA_TD3_LAG_DACT_MAXW


class Td3Lag(C.Structure):
    """ctypes mirror of ``osa_td3_lag``."""

    _fields_ = [('multiplier', C.c_void_p), ('adam', C.c_void_p), ('count', C.c_void_p), ('pid', C.c_void_p),
                ('mode', C.c_int), ('dact', C.c_int), ('window_lens', C.c_int), ('pid_d_delay', C.c_int),
                ('sum_norm', C.c_int), ('diff_norm', C.c_int), ('cost_limit', C.c_double), ('lambda_lr', C.c_double),
                ('upper_bound', C.c_double), ('kp', C.c_double), ('ki', C.c_double), ('kd', C.c_double),
                ('alpha_p', C.c_double), ('alpha_d', C.c_double), ('penalty_max', C.c_double)]


def dact_of(desc: Td3Desc, name: str | None = None) -> int:
    """How layer 0's data gradient of the constrained actor step runs: ``name`` or ``OSA_TD3_LAG_DACT`` where given --
    ``gemm`` above a first critic width of DACT_MAX_WIDTH is an OsaError, not another kernel -- else the default where
    it is supported and ``stacked`` where not."""
    name = os.environ.get('OSA_TD3_LAG_DACT', '') if name is None else name
    if name not in ('', *DACTS):
        raise ValueError(f'OSA_TD3_LAG_DACT={name!r}: gemm or stacked')
    dact = DACTS[name or DEFAULT_DACT]
    if dact == DACTS['gemm'] and int(desc.hidden[1][0]) > DACT_MAX_WIDTH:
        if name:
            raise _lib.OsaError(f'OSA_TD3_LAG_DACT=gemm: a first critic layer wider than {DACT_MAX_WIDTH}')
        dact = DACTS['stacked']
    return dact


def check_lagrange_cfgs(lagrange_cfgs: dict) -> str:
    """``'pid'`` or ``'adam'`` for a ``lagrange_cfgs`` block; NotImplementedError, before any GPU is touched, for a
    ``lambda_optimizer`` other than Adam (the device step restates torch.optim.Adam on the scalar)."""
    if 'pid_kp' in lagrange_cfgs:
        return 'pid'
    if lagrange_cfgs.get('lambda_optimizer', 'Adam') != 'Adam':
        raise NotImplementedError(f"lambda_optimizer {lagrange_cfgs['lambda_optimizer']!r}: the device multiplier "
                                  "takes 'Adam' only")
    return 'adam'


class Td3LagStep(Td3Step):  # pylint: disable=too-many-instance-attributes
    """``Td3Step`` with the cost critic in the actor loss (ddpg_lag.py:73-100), the multiplier on the device
    (``multiplier``, float32 [1]; ``update_multiplier`` is lagrange.py / pid_lagrange.py as one launch) and, with
    ``cost_normalize``, ``CostNormalize`` inside the store launch (``cost_normalizer``: mean, sumsq, count as doubles).
    ``OSA_TD3_LAG_DACT=gemm|stacked`` chooses layer 0 of the critics' data gradient."""

    def __init__(self, desc: Td3Desc, *, lagrange_cfgs: dict, window_lens: int, cost_normalize: bool = False,
                 dact: str | None = None, **kw) -> None:
        mode = check_lagrange_cfgs(lagrange_cfgs)
        if not desc.use_cost:
            raise ValueError('the constrained step needs the cost critic: use_cost')
        self.dact = dact_of(desc, dact)
        super().__init__(desc, **kw)
        g, dev = dict(lagrange_cfgs), self.device
        self.ws_floats = int(self._lib.osa_td3_lag_ws_floats(C.byref(desc)))
        self.ws = torch.zeros(self.ws_floats, **self.f32)
        init = float(g['lagrangian_multiplier_init'])
        # lagrange.py:71-75: max(init, 0); pid_lagrange.py:77-83: the penalty starts at 0, the integral at init
        self.initial_multiplier = 0.0 if mode == 'pid' else max(init, 0.0)
        self.multiplier = torch.full((1,), self.initial_multiplier, **self.f32)
        self.lag_adam = torch.zeros(2, **self.f32)
        self.lag_count = torch.zeros(1, dtype=torch.int32, device=dev)
        depth = int(g.get('pid_d_delay', 1))
        self.lag_pid = torch.zeros(3 + depth, dtype=torch.float64, device=dev)
        self.lag_pid[0] = init
        self.cost_normalizer = torch.zeros(3, dtype=torch.float64, device=dev) if cost_normalize else None
        bound = g.get('lagrangian_upper_bound')
        p = _lib.ptr
        self._lag = Td3Lag(p(self.multiplier), p(self.lag_adam), p(self.lag_count), p(self.lag_pid),
                           int(mode == 'pid'), self.dact, int(window_lens), depth, int(bool(g.get('sum_norm', False))),
                           int(bool(g.get('diff_norm', False))), float(g['cost_limit']), float(g.get('lambda_lr', 0.0)),
                           -1.0 if bound is None else float(bound), float(g.get('pid_kp', 0.0)),
                           float(g.get('pid_ki', 0.0)), float(g.get('pid_kd', 0.0)),
                           float(g.get('pid_delta_p_ema_alpha', 0.0)), float(g.get('pid_delta_d_ema_alpha', 0.0)),
                           float(g.get('penalty_max', 0.0)))

    def head_dz(self) -> torch.Tensor:
        """The actor head's dz of the last actor step, padded: a view ``[batch][act_dim rounded up to 4]`` of the
        workspace (intact after the step while the actor has one hidden layer: a deeper backward reuses it)."""
        off, lda = int(self._lib.osa_td3_lag_dz_offset(C.byref(self.desc))), (self.A + 3) // 4 * 4
        return self.ws[off:off + self.B * lda].view(self.B, lda)

    def state_dict(self, which: str = 'actor'):
        """``Td3Step.state_dict``; with ``cost_normalize`` the actor's carries the normaliser's running moments
        ``[mean, sumsq, count]`` under ``cost_normalizer``.  The multiplier and its optimiser state are not saved."""
        sd = super().state_dict(which)
        if which == 'actor' and self.cost_normalizer is not None:
            sd['cost_normalizer'] = self.cost_normalizer.clone()
        return sd

    def load_state_dict(self, sd, which: str = 'actor') -> None:
        super().load_state_dict(sd, which)
        if which == 'actor' and self.cost_normalizer is not None and 'cost_normalizer' in sd:
            self.cost_normalizer.copy_(torch.as_tensor(sd['cost_normalizer'], dtype=torch.float64))

    def store(self, obs, act, reward, cost, terminated, truncated, next_obs, final_obs=None, final_mask=None,
              episodes: tuple | None = None) -> None:
        """``Td3Step.store``; with ``cost_normalize`` the ring takes the normalised cost, the episodes the raw one."""
        if self.cost_normalizer is None:
            return super().store(obs, act, reward, cost, terminated, truncated, next_obs, final_obs, final_mask,
                                 episodes)
        n = int(obs.shape[0])
        p = _lib.ptr
        acc, out, count = episodes or (None, None, None)
        _lib.check(self._lib.osa_td3_store_cn(
            C.byref(self._ring), n, self.D, self.A, p(obs), obs.stride(0), p(act), act.stride(0), p(reward), p(cost),
            p(terminated), p(truncated), p(next_obs), next_obs.stride(0), p(final_obs),
            final_obs.stride(0) if final_obs is not None else 0, p(final_mask), p(acc), p(out),
            int(out.shape[0]) if out is not None else 0, p(count), p(self.cost_normalizer), _lib.stream_ptr()),
            'osa_td3_store_cn')
        return None

    def update_multiplier(self, carry, ncarry: int, episodes: tuple, update: bool = True) -> None:
        """One launch after an update round: the multiplier's step on the mean cost of the last ``window_lens``
        episodes of ``carry[:ncarry]`` and the running epoch's ``episodes`` (``update`` False: none), and the
        multiplier into column 5 of the round's last statistics row."""
        _, out, count = episodes
        p = _lib.ptr
        _lib.check(self._lib.osa_td3_multiplier_update(
            C.byref(self._lag), p(carry), int(ncarry), p(out), int(out.shape[0]), p(count), int(bool(update)),
            p(self.stats), p(self.step), self.nslots, _lib.stream_ptr()), 'osa_td3_multiplier_update')

    def run(self, nsteps: int = 1) -> None:
        """Enqueue ``nsteps`` gradient steps on the current stream (ddpg.py:382-400 with ddpg_lag.py:73-100)."""
        _lib.check(self._lib.osa_td3_lag_step(
            C.byref(self.desc), C.byref(self.hp), C.byref(self._state), C.byref(self._lag), C.byref(self._ring),
            C.byref(self._draws), _lib.ptr(self.stats), _lib.ptr(self.ws), self.ws_floats, self.update_count,
            int(nsteps), _lib.stream_ptr()), 'osa_td3_lag_step')
        self.update_count += int(nsteps)


__all__ = ['Td3Desc', 'Td3HParams', 'Td3Layout', 'Td3Actor', 'Td3Step', 'Td3Lag', 'Td3LagStep', 'STAT_KEYS',
           'LAG_STAT_KEYS', 'make_desc', 'route_of', 'dact_of', 'check_lagrange_cfgs']
