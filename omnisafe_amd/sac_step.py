"""The device side of off-policy SAC (csrc/sac_kernels.hip): the tanh-squashed ``GaussianSACActor`` and the two-network
``QCritic`` blocks with the reference's state-dict names, their targets and Adam moments, the temperature, the draws,
acting and the gradient step.  The replay ring, its store launch and the critics' state dicts are td3_step's.

``SacActor`` is what the trainer and the players of a saved policy share: the actor block, its state dict and ``act``.
``SacStep`` adds the critics, the ring, ``log_alpha`` with its moments and ``run(n)``, which enqueues n gradient steps
on the current stream with no host synchronisation.  Every step reads three normal draws ``[B][A]`` -- target, actor,
temperature -- from ``draw(seed, first_step, n)`` or ``set_draws`` (tests).  ``OSA_SAC_HEAD=layer|fused`` chooses how
the Gaussian head runs: the top layer's tile GEMM with a row kernel, or one fused launch each way.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import OrderedDict

import torch

from . import _lib
from .bcq_step import _get
from .crr_step import _init_mlp
from .models import GMLP_MAX_LAYERS
from .td3_step import MAX_ACT_DIM, Td3Actor, Td3Layout, Td3Step, _hidden
from .td3_step import make_desc as _td3_make_desc

STAT_KEYS = ('Loss/Loss_reward_critic', 'Value/reward_critic', 'Loss/Loss_pi', 'Loss/Loss_cost_critic',
             'Value/cost_critic', 'Value/alpha', 'Loss/alpha_loss')  # columns 0 .. 6 of a statistics row
HEADS = {'layer': 0, 'fused': 1}  # OSA_SAC_HEAD_*
DEFAULT_HEAD = 'layer'            # the faster one at the YAML shape: 289 v 313 us per step
ACT_SAMPLE, ACT_UNIFORM, ACT_MEAN = 0, 1, 2  # osa_sac_act's modes


class SacDesc(C.Structure):
    """ctypes mirror of ``osa_sac_desc``."""

    _fields_ = [('obs_dim', C.c_int), ('act_dim', C.c_int), ('n_hidden', C.c_int * 2),
                ('hidden', (C.c_int * GMLP_MAX_LAYERS) * 2), ('activation', C.c_int * 2), ('batch', C.c_int),
                ('use_cost', C.c_int)]


class SacHParams(C.Structure):
    """ctypes mirror of ``osa_sac_hparams``."""

    _fields_ = [('gamma', C.c_float), ('polyak', C.c_float), ('one_minus_polyak', C.c_float), ('auto_alpha', C.c_int),
                ('target_entropy', C.c_float), ('policy_delay', C.c_int), ('lr_actor', C.c_float),
                ('lr_critic', C.c_float), ('lr_alpha', C.c_float), ('beta1', C.c_double), ('beta2', C.c_double),
                ('adam_eps', C.c_double), ('max_grad_norm', C.c_float), ('critic_norm_coeff', C.c_float),
                ('head', C.c_int)]


class SacState(C.Structure):
    """ctypes mirror of ``osa_sac_state``."""

    _fields_ = [(n, C.c_void_p) for n in ('actor', 'actor_m', 'actor_v', 'actor_t', 'critic', 'critic_m', 'critic_v',
                                           'critic_t', 'adam_step', 'step', 'log_alpha')]


class SacDrawBuffers(C.Structure):
    """ctypes mirror of ``osa_sac_draw_buffers``."""

    _fields_ = [('idx', C.c_void_p), ('eps', C.c_void_p), ('nslots', C.c_int)]


def make_desc(obs_dim: int, act_dim: int, actor_hidden, critic_hidden, actor_act: str, critic_act: str, batch: int = 1,
              num_critics: int = 2, use_cost: bool = False) -> SacDesc:
    """The description of a SAC problem; NotImplementedError, before any GPU is touched, for what
    ``td3_step.make_desc`` refuses and for ``num_critics`` other than 2 (sac.py takes the min over a pair)."""
    if int(num_critics) != 2:
        raise NotImplementedError(f'num_critics {num_critics}: SAC takes the minimum over 2 reward critics')
    t = _td3_make_desc(obs_dim, act_dim, actor_hidden, critic_hidden, actor_act, critic_act, batch, 2, use_cost)
    d = SacDesc()
    for name, _ in SacDesc._fields_:  # pylint: disable=protected-access
        setattr(d, name, getattr(t, name))
    return d


def head_of(desc: SacDesc, name: str | None = None) -> int:
    """The head's route: ``name`` or ``OSA_SAC_HEAD`` where given -- ``fused`` on a shape the kernels do not take is an
    OsaError, not another kernel -- else the default where it is supported and ``layer`` where not."""
    name = os.environ.get('OSA_SAC_HEAD', '') if name is None else name
    if name not in ('', 'layer', 'fused'):
        raise ValueError(f'OSA_SAC_HEAD={name!r}: layer or fused')
    head = HEADS[name or DEFAULT_HEAD]
    if head == HEADS['fused'] and not _lib.load().osa_sac_head_supported(C.byref(desc)):
        if name:
            raise _lib.OsaError('OSA_SAC_HEAD=fused: the actor\'s last hidden width or the batch is above what the '
                                'fused head kernels take (osa_sac_head_supported)')
        head = HEADS['layer']
    return head


class SacLayout(Td3Layout):
    """Offsets of the reference's tensors inside the padded blocks (osa_sac_layout): the actor's top layer is
    ``(2 act_dim, hidden)``.  Host only."""

    def __init__(self, desc: SacDesc) -> None:
        super().__init__(desc, 'osa_sac_layout', 2 * int(desc.act_dim))


class SacActor(Td3Actor):
    """``GaussianSACActor``: the actor block, its state dict and ``act``."""

    def __init__(self, desc: SacDesc, device) -> None:
        # (named, not super(): in SacStep's order of bases Td3Step comes next, whose constructor builds TD3's state)
        Td3Actor.__init__(self, desc, device, SacLayout(desc))

    def state_dict(self, which: str = 'actor'):
        """The keys, order and shapes of ``GaussianSACActor.state_dict()``: its ``_log2`` buffer, then ``net.*``."""
        sd = OrderedDict(_log2=torch.log(torch.tensor(2.0)).to(self.device))
        sd.update(_get(getattr(self, which), self._ix['actor']))
        return sd

    def act(self, obs: torch.Tensor, mode: int = ACT_SAMPLE, seed: int = 0, offset: int = 0,
            out: torch.Tensor | None = None) -> torch.Tensor:  # pylint: disable=arguments-differ
        """``GaussianSACActor.predict`` of the rows of ``obs``: ``tanh(mu + sigma eps)`` (ACT_SAMPLE), ``tanh mu``
        (ACT_MEAN) or a uniform draw over the action box (ACT_UNIFORM: ``use_rand_action``).  Draws: Philox(seed,
        offset, element) on the device."""
        n = int(obs.shape[0])
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] == self.D \
            and obs.stride(1) == 1
        if out is None:
            out = torch.empty(n, self.A, **self.f32)
        p = _lib.ptr
        _lib.check(self._lib.osa_sac_act(C.byref(self.desc), p(self.actor), p(obs), obs.stride(0), n, int(mode),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), p(out), out.stride(0),
                                         _lib.stream_ptr()), 'osa_sac_act')
        return out


class SacStep(SacActor, Td3Step):  # pylint: disable=too-many-instance-attributes
    """The SAC trainer's device state.  The ring (``store``), the critics' state dicts and the state they read
    (``Td3Step._init_training_state``) are ``Td3Step``'s; its constructor, which builds TD3's own draws, workspace and
    hyperparameters, is not called."""

    def __init__(self, desc: SacDesc, *, size: int, gamma: float, polyak: float, lr_actor: float, lr_critic: float,
                 nslots: int, alpha: float = 0.2, auto_alpha: bool = False, policy_delay: int = 1,
                 max_grad_norm: float | None = None, critic_norm_coeff: float = 0.0, head: str | None = None,
                 device='cuda:0') -> None:  # pylint: disable=super-init-not-called
        if not alpha > 0:
            raise ValueError(f'alpha {alpha}: the temperature is positive')
        self.head = head_of(desc, head)
        SacActor.__init__(self, desc, device)
        self._init_training_state(size, nslots, 2, 4)
        f32, B, A, self.auto_alpha = self.f32, self.B, self.A, bool(auto_alpha)
        # log alpha and its Adam moments: sac.py:67-80 starts auto_alpha at 0 and a fixed temperature at log(alpha)
        self.log_alpha = torch.tensor([0.0 if auto_alpha else math.log(alpha), 0.0, 0.0], **f32)
        self.eps = torch.zeros(self.nslots, 3, B, A, **f32)
        self.ws_floats = int(self._lib.osa_sac_ws_floats(C.byref(desc)))
        self.ws = torch.zeros(self.ws_floats, **f32)
        self.hp = SacHParams(gamma=gamma, polyak=polyak, one_minus_polyak=1.0 - polyak, auto_alpha=int(self.auto_alpha),
                             target_entropy=-float(A), policy_delay=int(policy_delay), lr_actor=lr_actor,
                             lr_critic=lr_critic, lr_alpha=lr_critic, beta1=0.9, beta2=0.999, adam_eps=1e-8,
                             max_grad_norm=float(max_grad_norm or 0.0), critic_norm_coeff=float(critic_norm_coeff),
                             head=self.head)
        p = _lib.ptr
        self._state = SacState(p(self.actor), p(self.actor_m), p(self.actor_v), p(self.actor_t), p(self.critic),
                               p(self.critic_m), p(self.critic_v), p(self.critic_t), p(self.adam_step), p(self.step),
                               p(self.log_alpha))
        self._draws = SacDrawBuffers(p(self.idx), p(self.eps), self.nslots)

    def init_parameters(self, mode: str = 'kaiming_uniform') -> None:
        """The reference's initial weights for the current torch seed, in its construction order: the actor (its top
        layer ``2 act_dim`` wide), the reward critics, the cost critic; targets are copies."""
        D, A = self.D, self.A
        sd = OrderedDict()
        for j, (w, b) in enumerate(_init_mlp([D] + _hidden(self.desc, 0) + [2 * A], mode)):
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

    def draw(self, seed: int, first_step: int, nsteps: int = 1) -> None:
        """The device draws of steps first_step .. first_step + nsteps - 1 into their slots."""
        assert 1 <= nsteps <= self.nslots
        p = _lib.ptr
        _lib.check(self._lib.osa_sac_draws(C.byref(self.desc), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_step),
                                           int(nsteps), self.nslots, C.byref(self._ring), p(self.idx), p(self.eps),
                                           _lib.stream_ptr()), 'osa_sac_draws')

    def set_draws(self, first_step: int, idx, eps) -> None:
        """Inject the draws of consecutive steps: ``idx [steps][B]``, ``eps [steps][3][B][A]``."""
        idx = torch.as_tensor(idx, dtype=torch.int64)
        n = idx.shape[0]
        assert 1 <= n <= self.nslots
        if int(idx.min()) < 0 or int(idx.max()) >= self.size:
            raise ValueError(f'indices outside [0, {self.size})')
        slots = (torch.arange(n) + int(first_step)) % self.nslots
        self.idx[slots] = idx.reshape(n, self.B).to(self.device)
        self.eps[slots] = torch.as_tensor(eps).reshape(n, 3, self.B, self.A).to(**self.f32)

    def run(self, nsteps: int = 1) -> None:
        """Enqueue ``nsteps`` gradient steps on the current stream (ddpg.py:382-400 with sac.py:93-207 each)."""
        _lib.check(self._lib.osa_sac_step(
            C.byref(self.desc), C.byref(self.hp), C.byref(self._state), C.byref(self._ring), C.byref(self._draws),
            _lib.ptr(self.stats), _lib.ptr(self.ws), self.ws_floats, self.update_count, int(nsteps),
            _lib.stream_ptr()), 'osa_sac_step')
        self.update_count += int(nsteps)


__all__ = ['SacDesc', 'SacHParams', 'SacLayout', 'SacActor', 'SacStep', 'STAT_KEYS', 'MAX_ACT_DIM', 'HEADS',
           'DEFAULT_HEAD', 'ACT_SAMPLE', 'ACT_UNIFORM', 'ACT_MEAN', 'make_desc', 'head_of']
