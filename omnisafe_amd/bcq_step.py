"""The device side of offline BCQ / BCQ-Lag (csrc/bcq_kernels.hip): the PerturbationActor of
models/actor/perturbation_actor.py:27-101 (a VAE block and a perturbation block) with the reference's state-dict names,
one or two critic pairs with targets in CRR's layout, the dataset on the device, the draws, the train step and
``predict`` for the players.

``BcqActor`` is what the trainer and the players of a saved policy share: the two actor blocks, ``phi``, the state dict
and ``predict``.  ``BcqStep`` adds the critics, the Adam moments, the multiplier, the device step counter and
``run(n)``, which enqueues n train steps on the current stream with no host synchronisation; ``stats`` holds the
per-step scalars ``[nslots][NSTAT]`` until the caller reads them.  Draws come from ``draw(seed, first_step, n)``
(Philox on the device) or are injected with ``set_draws`` (tests).  ``OSA_BCQ_CHAIN=layer|fused`` chooses how the
target chain and ``predict`` run: one tile-GEMM launch per layer, or one launch of the row-resident chain kernel.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, vae_step
from .crr_step import CrrData, FIELDS, _init_mlp, load_dataset
from .models import ACTIVATIONS, GMLP_MAX_LAYERS

STAT_KEYS = ('Loss/Loss_vae', 'Loss/Loss_recon', 'Loss/Loss_kl', 'Loss/Loss_reward_critic', 'Qr/data_Qr',
             'Qr/target_Qr', 'Loss/Loss_cost_critic', 'Qc/data_Qc', 'Qc/target_Qc', 'Loss/Loss_actor', 'Qr/current_Qr',
             'Qc/current_Qc', 'Metrics/LagrangeMultiplier')  # columns 0 .. 12 of a statistics row
BCQ_STATS = (0, 1, 2, 3, 4, 5, 9, 10)
ROUTES = {'layer': 0, 'fused': 1}  # OSA_BCQ_ROUTE_*
DEFAULT_ROUTE = 'layer'            # the faster one at the YAML shape, by 2 - 8 % of the chain
MAX_ACT_DIM = 32


class BcqDesc(C.Structure):
    """ctypes mirror of ``osa_bcq_desc``."""

    _fields_ = [('obs_dim', C.c_int), ('act_dim', C.c_int), ('n_hidden', C.c_int * 2),
                ('hidden', (C.c_int * GMLP_MAX_LAYERS) * 2), ('activation', C.c_int * 2), ('batch', C.c_int),
                ('samples', C.c_int), ('pairs', C.c_int)]


class BcqHParams(C.Structure):
    """ctypes mirror of ``osa_bcq_hparams``."""

    _fields_ = [('gamma', C.c_float), ('cost_gamma', C.c_float), ('polyak', C.c_float), ('one_minus_polyak', C.c_float),
                ('phi', C.c_float), ('min_weight', C.c_float), ('one_minus_min_weight', C.c_float),
                ('lr_actor', C.c_float), ('lr_critic', C.c_float), ('beta1', C.c_double), ('beta2', C.c_double),
                ('adam_eps', C.c_double), ('cost_limit', C.c_float), ('lambda_lr', C.c_float),
                ('lagrange_open', C.c_int), ('route', C.c_int), ('vae_route', C.c_int)]


class BcqState(C.Structure):
    """ctypes mirror of ``osa_bcq_state``."""

    _fields_ = [(n, C.c_void_p) for n in ('vae', 'vae_m', 'vae_v', 'pert', 'pert_m', 'pert_v', 'critic', 'critic_m',
                                           'critic_v', 'target', 'adam_step', 'lagrange', 'step', 'vae_stats')]


class BcqDrawBuffers(C.Structure):
    """ctypes mirror of ``osa_bcq_draw_buffers``."""

    _fields_ = [(n, C.c_void_p) for n in ('idx', 'z_r', 'z_c', 'eps', 'z_a')] + [('nslots', C.c_int)]


def make_desc(obs_dim: int, act_dim: int, actor_hidden, critic_hidden, actor_act: str, critic_act: str, batch: int = 1,
              samples: int = 1, pairs: int = 1) -> BcqDesc:
    """The description of a BCQ / BCQ-Lag problem; NotImplementedError, before any GPU is touched, for an activation
    outside the five, a network without a hidden layer or with more than GMLP_MAX_LAYERS - 1, and act_dim > 32."""
    a_h, c_h = [int(h) for h in actor_hidden], [int(h) for h in critic_hidden]
    for name in (actor_act, critic_act):
        if name not in ACTIVATIONS:
            raise NotImplementedError(f'activation {name!r}: one of {list(ACTIVATIONS)}')
    if (any(h < 1 or h > 4096 for h in a_h + c_h) or min(len(a_h), len(c_h)) < 1
            or max(len(a_h), len(c_h)) + 1 > GMLP_MAX_LAYERS):
        raise NotImplementedError(f'hidden_sizes {a_h}/{c_h}: 1 .. {GMLP_MAX_LAYERS - 1} hidden layers of width 1 .. 4096')
    if not 1 <= int(act_dim) <= MAX_ACT_DIM:
        raise NotImplementedError(f'act_dim {act_dim}: the VAE heads take 1 .. {MAX_ACT_DIM} action dimensions')
    d = BcqDesc()
    d.obs_dim, d.act_dim = int(obs_dim), int(act_dim)
    for net, sizes in enumerate((a_h, c_h)):
        d.n_hidden[net] = len(sizes)
        for l, w in enumerate(sizes):
            d.hidden[net][l] = w
    d.activation[0], d.activation[1] = ACTIVATIONS[actor_act], ACTIVATIONS[critic_act]
    d.batch, d.samples, d.pairs = int(batch), int(samples), int(pairs)
    return d


def _hidden(desc: BcqDesc, net: int) -> list[int]:
    return [int(desc.hidden[net][l]) for l in range(desc.n_hidden[net])]


def vae_desc_of(desc: BcqDesc) -> vae_step.VaeDesc:
    """The VAE inside the actor: ``actor.hidden_sizes`` and its activation (perturbation_actor.py:57)."""
    d = vae_step.VaeDesc()
    d.obs_dim, d.act_dim, d.n_hidden = desc.obs_dim, desc.act_dim, desc.n_hidden[0]
    for l in range(desc.n_hidden[0]):
        d.hidden[l] = desc.hidden[0][l]
    d.activation, d.batch = desc.activation[0], desc.batch
    return d


class BcqLayout:
    """Offsets of the reference's tensors inside the padded blocks (osa_bcq_layout, osa_vae_layout).  Host only."""

    def __init__(self, desc: BcqDesc) -> None:
        out = (C.c_int * (6 + 2 * GMLP_MAX_LAYERS * 3))()
        _lib.check(_lib.load().osa_bcq_layout(C.byref(desc), out), 'osa_bcq_layout')
        self.Pe, self.Pd, self.Pp, self.Pc, self.nstat = (int(x) for x in out[:5])
        self.vae = vae_step.VaeLayout(vae_desc_of(desc))
        assert (self.vae.Pe, self.vae.Pd) == (self.Pe, self.Pd)
        D, A = int(desc.obs_dim), int(desc.act_dim)
        self._layers = []
        k = 6
        for sizes in ([D + A] + _hidden(desc, 0) + [A], [D + A] + _hidden(desc, 1) + [1]):
            rows = []
            for l in range(GMLP_MAX_LAYERS):
                oW, ob, ld = int(out[k]), int(out[k + 1]), int(out[k + 2])
                k += 3
                if oW >= 0:
                    rows.append((oW, ob, ld, sizes[l + 1], sizes[l]))
            self._layers.append(rows)

    def tensors(self, net: int, prefix: str) -> list[tuple[str, tuple[int, ...], np.ndarray]]:
        """``(name, shape, offsets)`` of the perturbation network (net 0: ``perturbation.0.weight, ...``) or of a
        critic of a pair (net 1: prefix ``critic_j.0``)."""
        items = []
        for j, (oW, ob, ld, n_out, n_in) in enumerate(self._layers[net]):
            ix = (oW + np.arange(n_out)[:, None] * ld + np.arange(n_in)[None, :]).reshape(-1)
            items.append((f'{prefix}.{2 * j}.weight', (n_out, n_in), ix))
            items.append((f'{prefix}.{2 * j}.bias', (n_out,), ob + np.arange(n_out)))
        return items

    def actor_tensors(self) -> dict[str, list]:
        """The actor's tensors per block, named as ``PerturbationActor.state_dict()`` names them behind ``_phi``:
        ``vae.*`` as ``VaeLayout.tensors()`` has them, then ``perturbation.*``."""
        return {'vae': [(f'vae.{n}', s, ix) for n, s, ix in self.vae.tensors()],
                'pert': self.tensors(0, 'perturbation')}

    def real_mask(self, net: int) -> np.ndarray:
        """True where a block holds a parameter, False in its padding."""
        mask = np.zeros(self.Pp if net == 0 else self.Pc, bool)
        for _, _, ix in self.tensors(net, 'x'):
            mask[ix] = True
        return mask


def route_of(desc: BcqDesc, name: str | None = None) -> int:
    """The chain's route: ``name`` or ``OSA_BCQ_CHAIN`` where given -- ``fused`` on a shape the kernel does not take is
    an OsaError, not another kernel -- else the default where it is supported and ``layer`` where not."""
    name = os.environ.get('OSA_BCQ_CHAIN', '') if name is None else name
    if name not in ('', 'layer', 'fused'):
        raise ValueError(f'OSA_BCQ_CHAIN={name!r}: layer or fused')
    route = ROUTES[name or DEFAULT_ROUTE]
    if route == ROUTES['fused'] and not _lib.load().osa_bcq_chain_supported(C.byref(desc)):
        if name:
            raise _lib.OsaError('OSA_BCQ_CHAIN=fused: a hidden width above 256 or an observation too wide for the '
                                'chain kernel\'s LDS')
        route = ROUTES['layer']
    return route


def _index(items, device):
    return items, torch.from_numpy(np.concatenate([ix for _, _, ix in items])).to(device)


def _get(block: torch.Tensor, index) -> 'OrderedDict[str, torch.Tensor]':
    items, flat_ix = index
    flat = block[flat_ix]
    sd, i = OrderedDict(), 0
    for name, shape, ix in items:
        sd[name] = flat[i:i + len(ix)].reshape(shape).clone()
        i += len(ix)
    return sd


def _set(block: torch.Tensor, index, sd) -> None:
    """Either name of a VAE tensor is taken (``vae.encoder.0.weight`` or ``vae._encoder.0.weight``)."""
    items, flat_ix = index
    parts = []
    for name, shape, _ in items:
        key = name if name in sd else name.replace('._', '.')
        t = torch.as_tensor(sd[key], dtype=torch.float32)
        assert tuple(t.shape) == tuple(shape), (name, tuple(t.shape), shape)
        parts.append(t.reshape(-1))
    block[flat_ix] = torch.cat(parts).to(block.device)


class BcqActor:
    """``PerturbationActor``: the VAE block, the perturbation block and ``phi``."""

    def __init__(self, desc: BcqDesc, device, phi: float = 0.05, route: str | None = None) -> None:
        self.route = route_of(desc, route)
        self._lib = _lib.load(require_gpu=True)
        self.desc, self.device = desc, torch.device(device)
        self.phi = float(np.float32(phi))  # (the reference keeps it as a float32 tensor: perturbation_actor.py:64-74)
        self.layout = lay = BcqLayout(desc)
        self.D, self.A, self.B, self.S = int(desc.obs_dim), int(desc.act_dim), int(desc.batch), int(desc.samples)
        self.pairs = int(desc.pairs)
        self.f32 = dict(dtype=torch.float32, device=self.device)
        self.vae, self.pert = torch.zeros(lay.Pe + lay.Pd, **self.f32), torch.zeros(lay.Pp, **self.f32)
        self._ix = {k: _index(items, self.device) for k, items in lay.actor_tensors().items()}
        self._pred_ws: torch.Tensor | None = None

    def state_dict(self, which: str = ''):
        """The keys, order and shapes of the reference's ``PerturbationActor.state_dict()``: ``_phi``, ``vae.*``,
        ``perturbation.*`` (of the parameters, or of an Adam moment: ``which='_m'`` / ``'_v'``)."""
        sd = OrderedDict(_phi=torch.tensor(self.phi, device=self.device))
        sd.update(_get(getattr(self, 'vae' + which), self._ix['vae']))
        sd.update(_get(getattr(self, 'pert' + which), self._ix['pert']))
        return sd

    def load_state_dict(self, sd, which: str = '') -> None:
        if '_phi' in sd and not which:
            self.phi = float(sd['_phi'])
        _set(getattr(self, 'vae' + which), self._ix['vae'], sd)
        _set(getattr(self, 'pert' + which), self._ix['pert'], sd)

    def predict(self, obs: torch.Tensor, z: torch.Tensor | None = None, seed: int = 0, offset: int = 0) -> torch.Tensor:
        """``PerturbationActor.predict`` (perturbation_actor.py:76-90) of the rows of ``obs``; ``z=None`` draws the
        latent on the device from Philox(seed, offset, element)."""
        obs = obs.to(self.device, torch.float32)
        n = int(obs.shape[0])
        assert obs.dim() == 2 and obs.shape[1] == self.D and obs.stride(1) == 1 and n >= 1
        if z is not None:
            z = z.to(self.device, torch.float32)
            assert z.shape == (n, 2 * self.A) and z.stride(1) == 1
        need = int(self._lib.osa_bcq_predict_ws_floats(C.byref(self.desc), n))
        if self._pred_ws is None or self._pred_ws.numel() < need:
            self._pred_ws = torch.zeros(need, **self.f32)
        out = torch.empty(n, self.A, **self.f32)
        p = _lib.ptr
        _lib.check(self._lib.osa_bcq_predict(
            C.byref(self.desc), self.route, self.phi, self.vae.data_ptr() + 4 * self.layout.Pe, p(self.pert), p(obs),
            obs.stride(0), p(z), z.stride(0) if z is not None else 0, n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset),
            p(out), out.stride(0), p(self._pred_ws), self._pred_ws.numel(), _lib.stream_ptr()), 'osa_bcq_predict')
        return out


class BcqStep(BcqActor):  # pylint: disable=too-many-instance-attributes
    def __init__(self, desc: BcqDesc, data: dict[str, torch.Tensor] | None, *, gamma: float, polyak: float, phi: float,
                 minimum_weighting: float, lr_actor: float, lr_critic: float, nslots: int, cost_gamma: float = 0.99,
                 cost_limit: float = 0.0, lambda_lr: float = 0.0, lambda_init: float = 0.0, route: str | None = None,
                 device='cuda:0') -> None:
        super().__init__(desc, device, phi, route)
        self.nslots = int(nslots)
        assert self.nslots >= 1
        lay, nq, f32, B, S, A2 = self.layout, 2 * self.pairs, self.f32, self.B, self.S, 2 * self.A
        self.vae_m, self.vae_v = torch.zeros_like(self.vae), torch.zeros_like(self.vae)
        self.pert_m, self.pert_v = torch.zeros_like(self.pert), torch.zeros_like(self.pert)
        self.critic, self.critic_m, self.critic_v, self.target = (torch.zeros(nq, lay.Pc, **f32) for _ in range(4))
        self.adam_step = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.lagrange = torch.tensor([max(float(lambda_init), 0.0), 0.0, 0.0, 0.0], **f32)
        self.steps = torch.zeros(2, dtype=torch.int64, device=self.device)  # [1]: the VAE launches' copy
        self.step = self.steps[:1]
        self.stats = torch.zeros(self.nslots, lay.nstat, **f32)
        self.vae_stats = torch.zeros(self.nslots, lay.vae.nstat, **f32)
        self.idx = torch.zeros(self.nslots, B, dtype=torch.int64, device=self.device)
        self.z_r = torch.zeros(self.nslots, B * S, A2, **f32)
        self.z_c = torch.zeros(self.nslots, B * S, A2, **f32) if self.pairs == 2 else None
        self.eps, self.z_a = torch.zeros(self.nslots, B, A2, **f32), torch.zeros(self.nslots, B, A2, **f32)
        self.ws_floats = int(self._lib.osa_bcq_ws_floats(C.byref(desc)))
        self.ws = torch.zeros(self.ws_floats, **f32)
        self.data, self.n_rows, self._data = None, 0, None
        skinny = bool(self._lib.osa_vae_skinny_supported(C.byref(vae_desc_of(desc))))
        self.hp = BcqHParams(gamma=gamma, cost_gamma=cost_gamma, polyak=polyak, one_minus_polyak=1.0 - polyak, phi=phi,
                             min_weight=minimum_weighting, one_minus_min_weight=1.0 - minimum_weighting,
                             lr_actor=lr_actor, lr_critic=lr_critic, beta1=0.9, beta2=0.999, adam_eps=1e-8,
                             cost_limit=cost_limit, lambda_lr=lambda_lr, lagrange_open=0, route=self.route,
                             vae_route=vae_step.ROUTES['skinny' if skinny else 'tile'])
        p = _lib.ptr
        self._state = BcqState(p(self.vae), p(self.vae_m), p(self.vae_v), p(self.pert), p(self.pert_m), p(self.pert_v),
                               p(self.critic), p(self.critic_m), p(self.critic_v), p(self.target), p(self.adam_step),
                               p(self.lagrange), p(self.steps), p(self.vae_stats))
        self._draws = BcqDrawBuffers(p(self.idx), p(self.z_r), p(self.z_c), p(self.eps), p(self.z_a), self.nslots)
        for c in range(2):
            self._ix[c] = _index(lay.tensors(1, f'critic_{c}.0'), self.device)
        if data is not None:
            self.set_data(data)

    def set_data(self, data: dict[str, torch.Tensor]) -> None:
        """The dataset (load_dataset's six device tensors); read by every step, never written or copied."""
        p = _lib.ptr
        for k in FIELDS:
            t = data[k]
            assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1, k
        self.data = data
        self.n_rows = int(data['obs'].shape[0])
        self._data = CrrData(p(data['obs']), p(data['action']), p(data['reward']), p(data['cost']), p(data['next_obs']),
                             p(data['done']), data['obs'].stride(0), data['action'].stride(0),
                             data['next_obs'].stride(0), self.n_rows)

    # ------------------------------------------------------------------ state dicts
    def critic_state_dict(self, pair: int, which: str = 'critic'):
        """``critic_0.0.0.weight, ..., critic_1.0.0.weight, ...`` of pair 0 (reward) or 1 (cost)."""
        sd = OrderedDict()
        for c in range(2):
            sd.update(_get(getattr(self, which)[2 * pair + c], self._ix[c]))
        return sd

    def load_critic_state_dict(self, pair: int, sd, which: str = 'critic') -> None:
        for c in range(2):
            _set(getattr(self, which)[2 * pair + c], self._ix[c], sd)

    def init_parameters(self, mode: str = 'kaiming_uniform') -> None:
        """The reference's initial weights for the current torch seed, in its construction order: the VAE, the
        perturbation network, the reward pair, (BCQ-Lag) the cost pair (bcq.py:78-120, bcq_lag.py:64-87); targets
        are copies."""
        D, A = self.D, self.A
        sd = OrderedDict((f'vae.{k}', v) for k, v in vae_step.initial_state_dict(vae_desc_of(self.desc), mode).items())
        for j, (w, b) in enumerate(_init_mlp([D + A] + _hidden(self.desc, 0) + [A], mode)):
            sd[f'perturbation.{2 * j}.weight'], sd[f'perturbation.{2 * j}.bias'] = w, b
        self.load_state_dict(sd)
        for pair in range(self.pairs):
            sd = OrderedDict()
            for c in range(2):
                for j, (w, b) in enumerate(_init_mlp([D + A] + _hidden(self.desc, 1) + [1], mode)):
                    sd[f'critic_{c}.0.{2 * j}.weight'], sd[f'critic_{c}.0.{2 * j}.bias'] = w, b
            self.load_critic_state_dict(pair, sd)
        self.target.copy_(self.critic)

    # ------------------------------------------------------------------ draws
    def draw(self, seed: int, first_step: int, nsteps: int) -> None:
        """The device draws of steps first_step .. first_step + nsteps - 1 into their slots."""
        assert 1 <= nsteps <= self.nslots
        p = _lib.ptr
        _lib.check(self._lib.osa_bcq_draws(
            C.byref(self.desc), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_step), int(nsteps), self.nslots, self.n_rows,
            p(self.idx), p(self.z_r), p(self.z_c), p(self.eps), p(self.z_a), _lib.stream_ptr()), 'osa_bcq_draws')

    def set_draws(self, first_step: int, idx, z_r, eps, z_a, z_c=None) -> None:
        """Inject the draws of consecutive steps (leading dimension = steps) into their slots."""
        idx = torch.as_tensor(idx, dtype=torch.int64)
        n = idx.shape[0]
        assert 1 <= n <= self.nslots
        if int(idx.min()) < 0 or int(idx.max()) >= self.n_rows:
            raise ValueError(f'indices outside [0, {self.n_rows})')
        slots = (torch.arange(n) + int(first_step)) % self.nslots
        self.idx[slots] = idx.reshape(n, self.B).to(self.device)
        for name, src in (('z_r', z_r), ('eps', eps), ('z_a', z_a)) + ((('z_c', z_c),) if self.pairs == 2 else ()):
            dst = getattr(self, name)
            dst[slots] = torch.as_tensor(src).reshape(n, *dst.shape[1:]).to(**self.f32)

    # ------------------------------------------------------------------ the step
    def run(self, nsteps: int = 1, lagrange_open: bool = False) -> None:
        """Enqueue ``nsteps`` train steps on the current stream (bcq.py:122-213 / bcq_lag.py:91-193 each)."""
        assert self._data is not None, 'set_data() first'
        self.hp.lagrange_open, self.hp.phi = int(bool(lagrange_open)), self.phi
        _lib.check(self._lib.osa_bcq_step(
            C.byref(self.desc), C.byref(self.hp), C.byref(self._state), C.byref(self._data), C.byref(self._draws),
            _lib.ptr(self.stats), _lib.ptr(self.ws), self.ws_floats, int(nsteps), _lib.stream_ptr()), 'osa_bcq_step')

    def target_q(self, pair: int, z: torch.Tensor) -> torch.Tensor:
        """The target chain's values ``[B S]`` of pair 0 (reward) or 1 (cost) over the current slot's rows of
        ``next_obs`` with the latents ``z [B S][2 A]``: what the TD target takes its max over."""
        assert self._data is not None, 'set_data() first'
        z = z.to(**self.f32).contiguous()
        assert z.shape == (self.B * self.S, 2 * self.A)
        out = torch.empty(self.B * self.S, **self.f32)
        self.hp.phi = self.phi
        _lib.check(self._lib.osa_bcq_target_q(
            C.byref(self.desc), C.byref(self.hp), C.byref(self._state), C.byref(self._data), _lib.ptr(self.idx),
            self.nslots, int(pair), _lib.ptr(z), _lib.ptr(out), _lib.ptr(self.ws), self.ws_floats, _lib.stream_ptr()),
            'osa_bcq_target_q')
        return out


__all__ = ['BcqDesc', 'BcqHParams', 'BcqLayout', 'BcqActor', 'BcqStep', 'STAT_KEYS', 'BCQ_STATS', 'make_desc',
           'load_dataset', 'route_of']
