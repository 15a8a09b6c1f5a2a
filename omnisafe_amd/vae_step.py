"""The device side of offline VAE-BC (csrc/vae_kernels.hip): the conditional VAE of models/actor/vae_actor.py:43-138 as
one padded parameter block with the reference's state-dict names, the dataset on the device, the draws, the train step
and ``decode`` for the players.

``VaeStep`` owns the joint block ``[Pe + Pd]`` (encoder, then decoder), its Adam moments and the device step counter.
``run(n)`` enqueues n train steps on the current stream with no host synchronisation; ``stats`` holds the per-step
scalars ``[nslots][NSTAT]`` until the caller reads them.  Draws come from ``draw(seed, first_step, n)`` (Philox on the
device) or are injected with ``set_draws`` (tests).  ``OSA_VAE_GEMM=tile|skinny`` chooses the kernel of the body layers
(every layer but a network's first): the 64 x 64 tile GEMM of the general networks or the skinny-batch kernel.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .crr_step import CrrData, _init_mlp, load_dataset
from .models import ACTIVATIONS, GMLP_MAX_LAYERS

STAT_KEYS = ('Loss/Loss_vae', 'Loss/Loss_recon', 'Loss/Loss_kl')  # columns 0 .. 2 of a statistics row
ROUTES = {'tile': 0, 'skinny': 1}  # OSA_VAE_ROUTE_*
DEFAULT_ROUTE = 'skinny'           # the faster one at the YAML shape
MAX_ACT_DIM = 32


class VaeDesc(C.Structure):
    """ctypes mirror of ``osa_vae_desc``."""

    _fields_ = [('obs_dim', C.c_int), ('act_dim', C.c_int), ('n_hidden', C.c_int),
                ('hidden', C.c_int * GMLP_MAX_LAYERS), ('activation', C.c_int), ('batch', C.c_int)]


class VaeHParams(C.Structure):
    """ctypes mirror of ``osa_vae_hparams``."""

    _fields_ = [('lr', C.c_float), ('route', C.c_int), ('beta1', C.c_double), ('beta2', C.c_double),
                ('adam_eps', C.c_double)]


class VaeState(C.Structure):
    """ctypes mirror of ``osa_vae_state``."""

    _fields_ = [(n, C.c_void_p) for n in ('params', 'm', 'v', 'adam_step', 'step')]


class VaeDrawBuffers(C.Structure):
    """ctypes mirror of ``osa_vae_draw_buffers``."""

    _fields_ = [('idx', C.c_void_p), ('eps', C.c_void_p), ('nslots', C.c_int)]


def make_desc(obs_dim: int, act_dim: int, hidden_sizes, activation: str, batch: int) -> VaeDesc:
    """The description of a VAE; NotImplementedError, before any GPU is touched, for an activation outside the five, a
    network without a hidden layer or with more than GMLP_MAX_LAYERS - 1, a width below 1 and act_dim > 32."""
    hidden = [int(h) for h in hidden_sizes]
    if activation not in ACTIVATIONS:
        raise NotImplementedError(f'activation {activation!r}: one of {list(ACTIVATIONS)}')
    if any(h < 1 or h > 4096 for h in hidden) or not 1 <= len(hidden) <= GMLP_MAX_LAYERS - 1:
        raise NotImplementedError(f'hidden_sizes {hidden}: 1 .. {GMLP_MAX_LAYERS - 1} hidden layers of width 1 .. 4096')
    if not 1 <= int(act_dim) <= MAX_ACT_DIM:
        raise NotImplementedError(f'act_dim {act_dim}: the VAE heads take 1 .. {MAX_ACT_DIM} action dimensions')
    d = VaeDesc()
    d.obs_dim, d.act_dim, d.n_hidden = int(obs_dim), int(act_dim), len(hidden)
    for l, w in enumerate(hidden):
        d.hidden[l] = w
    d.activation, d.batch = ACTIVATIONS[activation], int(batch)
    return d


def _sizes(desc: VaeDesc):
    D, A = int(desc.obs_dim), int(desc.act_dim)
    hidden = [int(desc.hidden[l]) for l in range(desc.n_hidden)]
    return [D + A] + hidden + [4 * A], [D + 2 * A] + hidden + [A]


class VaeLayout:
    """Offsets of the reference's tensors inside the joint block (osa_vae_layout).  Host only."""

    def __init__(self, desc: VaeDesc) -> None:
        out = (C.c_int * (4 + 2 * GMLP_MAX_LAYERS * 3))()
        _lib.check(_lib.load().osa_vae_layout(C.byref(desc), out), 'osa_vae_layout')
        self.Pe, self.Pd, self.nstat = int(out[0]), int(out[1]), int(out[2])
        self.P = self.Pe + self.Pd
        self._layers = []
        k = 4
        for net, sizes in enumerate(_sizes(desc)):
            rows = []
            for l in range(GMLP_MAX_LAYERS):
                oW, ob, ld = int(out[k]), int(out[k + 1]), int(out[k + 2])
                k += 3
                if oW >= 0:
                    base = net * self.Pe
                    rows.append((base + oW, base + ob, ld, sizes[l + 1], sizes[l]))
            self._layers.append(rows)

    def tensors(self) -> list[tuple[str, tuple[int, ...], np.ndarray]]:
        """``(name, shape, offsets)`` in the order of the reference's ``VAE.state_dict()``: the module registers each
        network twice (vae_actor.py:55-66: the attributes ``_encoder`` / ``_decoder``, then ``add_module``), so the
        keys are ``_encoder.*, _decoder.*, encoder.*, decoder.*``."""
        items = []
        for prefix in ('_', ''):
            for net, name in enumerate(('encoder', 'decoder')):
                for j, (oW, ob, ld, n_out, n_in) in enumerate(self._layers[net]):
                    ix = (oW + np.arange(n_out)[:, None] * ld + np.arange(n_in)[None, :]).reshape(-1)
                    items.append((f'{prefix}{name}.{2 * j}.weight', (n_out, n_in), ix))
                    items.append((f'{prefix}{name}.{2 * j}.bias', (n_out,), ob + np.arange(n_out)))
        return items

    def real_mask(self) -> np.ndarray:
        """True where the block holds a parameter, False in its padding."""
        mask = np.zeros(self.P, bool)
        for _, _, ix in self.tensors():
            mask[ix] = True
        return mask


def initial_state_dict(desc: VaeDesc, mode: str = 'kaiming_uniform'):
    """The reference's initial weights for the current torch seed: encoder, then decoder (vae_actor.py:55-64)."""
    sd = OrderedDict()
    for name, sizes in zip(('encoder', 'decoder'), _sizes(desc)):
        for j, (w, b) in enumerate(_init_mlp(sizes, mode)):
            sd[f'{name}.{2 * j}.weight'], sd[f'{name}.{2 * j}.bias'] = w, b
    return sd


def route_of(name: str | None = None) -> int:
    name = os.environ.get('OSA_VAE_GEMM', '') if name is None else name
    if name not in ('', 'tile', 'skinny'):
        raise ValueError(f'OSA_VAE_GEMM={name!r}: tile or skinny')
    return ROUTES[name or DEFAULT_ROUTE]


class VaeDecoder:
    """``decode`` of a VAE block: what the trainer and the players of a saved VAE-BC policy share."""

    def __init__(self, desc: VaeDesc, device, route: str | None = None) -> None:
        self._lib = _lib.load(require_gpu=True)
        self.desc, self.device = desc, torch.device(device)
        self.layout = VaeLayout(desc)
        self.D, self.A, self.B = int(desc.obs_dim), int(desc.act_dim), int(desc.batch)
        forced = route if route is not None else os.environ.get('OSA_VAE_GEMM', '')
        self.route = route_of(forced)
        if self.route == ROUTES['skinny'] and not self._lib.osa_vae_skinny_supported(C.byref(desc)):
            if forced:  # asked for by name: a shape it does not take is an error, not another kernel
                raise _lib.OsaError(f'OSA_VAE_GEMM=skinny: batch {self.B} is above the skinny kernel\'s 512 rows')
            self.route = ROUTES['tile']
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.layout.P, **f32)
        items = self.layout.tensors()
        self._items = items
        self._flat_ix = torch.from_numpy(np.concatenate([ix for _, _, ix in items])).to(self.device)
        self._dec_ws: torch.Tensor | None = None

    # ------------------------------------------------------------------ state dicts
    def _get(self, block: torch.Tensor) -> 'OrderedDict[str, torch.Tensor]':
        flat = block[self._flat_ix]
        sd, i = OrderedDict(), 0
        for name, shape, ix in self._items:
            sd[name] = flat[i:i + len(ix)].reshape(shape).clone()
            i += len(ix)
        return sd

    def _set(self, block: torch.Tensor, sd) -> None:
        """Either name of a tensor is taken (``encoder.0.weight`` or ``_encoder.0.weight``)."""
        parts = []
        for name, shape, _ in self._items:
            key = name if name in sd else name.lstrip('_')
            t = torch.as_tensor(sd[key], dtype=torch.float32)
            assert tuple(t.shape) == tuple(shape), (name, tuple(t.shape), shape)
            parts.append(t.reshape(-1))
        block[self._flat_ix] = torch.cat(parts).to(self.device)

    def state_dict(self, which: str = 'params'):
        """The keys, order and shapes of the reference's ``VAE.state_dict()`` (of the parameters, or of an Adam moment:
        ``which='m'`` / ``'v'``)."""
        return self._get(getattr(self, which))

    def load_state_dict(self, sd, which: str = 'params') -> None:
        self._set(getattr(self, which), sd)

    # ------------------------------------------------------------------ decode
    def decode(self, obs: torch.Tensor, z: torch.Tensor | None = None, seed: int = 0, offset: int = 0) -> torch.Tensor:
        """``VAE.decode`` (vae_actor.py:83-98) of the rows of ``obs``; ``z=None`` draws the latent on the device from
        Philox(seed, offset, element)."""
        obs = obs.to(self.device, torch.float32)
        n = int(obs.shape[0])
        assert obs.dim() == 2 and obs.shape[1] == self.D and obs.stride(1) == 1 and n >= 1
        if z is not None:
            z = z.to(self.device, torch.float32)
            assert z.shape == (n, 2 * self.A) and z.stride(1) == 1
        need = int(self._lib.osa_vae_decode_ws_floats(C.byref(self.desc), n))
        if self._dec_ws is None or self._dec_ws.numel() < need:
            self._dec_ws = torch.zeros(need, dtype=torch.float32, device=self.device)
        out = torch.empty(n, self.A, dtype=torch.float32, device=self.device)
        p = _lib.ptr
        _lib.check(self._lib.osa_vae_decode(
            C.byref(self.desc), self.route, self.params.data_ptr() + 4 * self.layout.Pe, p(obs), obs.stride(0), p(z),
            z.stride(0) if z is not None else 0, n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), p(out), out.stride(0),
            p(self._dec_ws), self._dec_ws.numel(), _lib.stream_ptr()), 'osa_vae_decode')
        return out


class VaeStep(VaeDecoder):  # pylint: disable=too-many-instance-attributes
    def __init__(self, desc: VaeDesc, data: dict[str, torch.Tensor] | None, *, lr: float, nslots: int,
                 route: str | None = None, device='cuda:0') -> None:
        super().__init__(desc, device, route)
        self.nslots = int(nslots)
        assert self.nslots >= 1
        f32 = dict(dtype=torch.float32, device=self.device)
        lay = self.layout
        self.m, self.v = torch.zeros(lay.P, **f32), torch.zeros(lay.P, **f32)
        self.adam_step = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.stats = torch.zeros(self.nslots, lay.nstat, **f32)
        self.idx = torch.zeros(self.nslots, self.B, dtype=torch.int64, device=self.device)
        self.eps = torch.zeros(self.nslots, self.B, 2 * self.A, **f32)
        self.ws_floats = int(self._lib.osa_vae_ws_floats(C.byref(desc)))
        self.ws = torch.zeros(self.ws_floats, **f32)
        self.data, self.n_rows, self._data = None, 0, None
        self.hp = VaeHParams(lr=lr, route=self.route, beta1=0.9, beta2=0.999, adam_eps=1e-8)
        p = _lib.ptr
        self._state = VaeState(p(self.params), p(self.m), p(self.v), p(self.adam_step), p(self.step))
        self._draws = VaeDrawBuffers(p(self.idx), p(self.eps), self.nslots)
        if data is not None:
            self.set_data(data)

    def set_data(self, data: dict[str, torch.Tensor]) -> None:
        """The dataset (load_dataset's device tensors; ``obs`` and ``action`` are read); never written or copied."""
        for k in ('obs', 'action'):
            t = data[k]
            assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1, k
        self.data = data
        self.n_rows = int(data['obs'].shape[0])
        p = _lib.ptr
        self._data = CrrData(obs=p(data['obs']), act=p(data['action']), ld_obs=data['obs'].stride(0),
                             ld_act=data['action'].stride(0), n_rows=self.n_rows)

    def init_parameters(self, mode: str = 'kaiming_uniform') -> None:
        """The reference's initial weights for the current torch seed."""
        self.load_state_dict(initial_state_dict(self.desc, mode))

    @property
    def moment1(self) -> torch.Tensor:
        """Adam's first moment, the joint block (padding included)."""
        return self.m

    @property
    def moment2(self) -> torch.Tensor:
        return self.v

    # ------------------------------------------------------------------ draws
    def draw(self, seed: int, first_step: int, nsteps: int) -> None:
        """The device draws of steps first_step .. first_step + nsteps - 1 into their slots."""
        assert 1 <= nsteps <= self.nslots
        _lib.check(self._lib.osa_vae_draws(
            C.byref(self.desc), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_step), int(nsteps), self.nslots, self.n_rows,
            _lib.ptr(self.idx), _lib.ptr(self.eps), _lib.stream_ptr()), 'osa_vae_draws')

    def set_draws(self, first_step: int, idx, eps) -> None:
        """Inject the draws of consecutive steps (leading dimension = steps) into their slots."""
        idx = torch.as_tensor(idx, dtype=torch.int64)
        n = idx.shape[0]
        assert 1 <= n <= self.nslots
        if int(idx.min()) < 0 or int(idx.max()) >= self.n_rows:
            raise ValueError(f'indices outside [0, {self.n_rows})')
        slots = (torch.arange(n) + int(first_step)) % self.nslots
        self.idx[slots] = idx.reshape(n, self.B).to(self.device)
        self.eps[slots] = torch.as_tensor(eps).reshape(n, self.B, 2 * self.A).to(self.device, torch.float32)

    # ------------------------------------------------------------------ the step
    def run(self, nsteps: int = 1) -> None:
        """Enqueue ``nsteps`` train steps on the current stream (vae_bc.py:79-97 each)."""
        assert self._data is not None, 'set_data() first'
        _lib.check(self._lib.osa_vae_step(
            C.byref(self.desc), C.byref(self.hp), C.byref(self._state), C.byref(self._data), C.byref(self._draws),
            _lib.ptr(self.stats), _lib.ptr(self.ws), self.ws_floats, int(nsteps), _lib.stream_ptr()), 'osa_vae_step')


__all__ = ['VaeDesc', 'VaeHParams', 'VaeLayout', 'VaeDecoder', 'VaeStep', 'STAT_KEYS', 'make_desc', 'load_dataset',
           'initial_state_dict', 'route_of']
