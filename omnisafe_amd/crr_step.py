"""The device side of offline CRR / CCRR (csrc/crr_kernels.hip): parameter blocks with the reference's state-dict names,
the dataset on the device, the draws and the train step.

``CrrStep`` owns an actor block ``[Pa]``, ``2 * pairs`` critic blocks ``[Pc]`` with a target copy each, their Adam
moments, the multiplier's state and the device step counter.  ``run(n)`` enqueues n train steps on the current stream
with no host synchronisation; ``stats`` holds the per-step scalars ``[nslots][NSTAT]`` until the caller reads them.
Draws come from ``draw(first_step, n)`` (Philox on the device) or are injected with ``set_draws`` (tests).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .models import ACTIVATIONS, GMLP_MAX_LAYERS

FIELDS = ('obs', 'action', 'reward', 'cost', 'next_obs', 'done')
STAT_KEYS = ('Loss/Loss_reward_critic', 'Qr/data_Qr', 'Qr/target_Qr', 'Loss/Loss_cost_critic', 'Qc/data_Qc',
             'Qc/target_Qc', 'Loss/Loss_actor', 'Qr/current_Qr', 'Qc/current_Qc', 'Train/PolicyStd',
             'Metrics/LagrangeMultiplier')  # columns 0 .. 10 of a statistics row (include/omnisafe_amd.h)
CRR_STATS = (0, 1, 2, 6, 7, 9)


class CrrDesc(C.Structure):
    """ctypes mirror of ``osa_crr_desc``."""

    _fields_ = [('obs_dim', C.c_int), ('act_dim', C.c_int), ('n_layers', C.c_int * 2),
                ('width', (C.c_int * GMLP_MAX_LAYERS) * 2), ('activation', C.c_int * 2), ('batch', C.c_int),
                ('samples', C.c_int), ('pairs', C.c_int)]


class CrrHParams(C.Structure):
    """ctypes mirror of ``osa_crr_hparams``."""

    _fields_ = [('gamma', C.c_float), ('beta', C.c_float), ('polyak', C.c_float), ('one_minus_polyak', C.c_float),
                ('lr_actor', C.c_float), ('lr_critic', C.c_float), ('beta1', C.c_double), ('beta2', C.c_double),
                ('adam_eps', C.c_double), ('cost_limit', C.c_float), ('lambda_lr', C.c_float),
                ('lagrange_open', C.c_int), ('reference_wiring', C.c_int)]


class CrrState(C.Structure):
    """ctypes mirror of ``osa_crr_state``."""

    _fields_ = [(n, C.c_void_p) for n in ('actor', 'actor_m', 'actor_v', 'critic', 'critic_m', 'critic_v', 'target',
                                           'adam_step', 'lagrange', 'step')]


class CrrData(C.Structure):
    """ctypes mirror of ``osa_crr_data``."""

    _fields_ = [(n, C.c_void_p) for n in ('obs', 'act', 'reward', 'cost', 'next_obs', 'done')] + [
        ('ld_obs', C.c_int), ('ld_act', C.c_int), ('ld_next', C.c_int), ('n_rows', C.c_long)]


class CrrDrawBuffers(C.Structure):
    """ctypes mirror of ``osa_crr_draw_buffers``."""

    _fields_ = [('idx', C.c_void_p), ('eps_next', C.c_void_p), ('eps_next_c', C.c_void_p), ('eps_samp', C.c_void_p),
                ('nslots', C.c_int)]


def make_desc(obs_dim: int, act_dim: int, actor_hidden, critic_hidden, actor_act: str, critic_act: str, batch: int,
              samples: int, pairs: int) -> CrrDesc:
    """The description of a CRR / CCRR problem; NotImplementedError for what ConstraintActorCritic refuses too, and for
    a network without a hidden layer."""
    a_h, c_h = [int(h) for h in actor_hidden], [int(h) for h in critic_hidden]
    for name in (actor_act, critic_act):
        if name not in ACTIVATIONS:
            raise NotImplementedError(f'activation {name!r}: one of {list(ACTIVATIONS)}')
    if (any(h < 1 for h in a_h + c_h) or min(len(a_h), len(c_h)) < 1
            or max(len(a_h), len(c_h)) + 1 > GMLP_MAX_LAYERS):
        raise NotImplementedError(f'hidden_sizes {a_h}/{c_h}: 1 .. {GMLP_MAX_LAYERS - 1} hidden layers of width >= 1')
    d = CrrDesc()
    d.obs_dim, d.act_dim = int(obs_dim), int(act_dim)
    for net, sizes in enumerate((a_h + [d.act_dim], c_h + [1])):
        d.n_layers[net] = len(sizes)
        for l, w in enumerate(sizes):
            d.width[net][l] = w
    d.activation[0], d.activation[1] = ACTIVATIONS[actor_act], ACTIVATIONS[critic_act]
    d.batch, d.samples, d.pairs = int(batch), int(samples), int(pairs)
    return d


class CrrLayout:
    """Offsets of the reference's tensors inside the padded blocks (osa_crr_layout).  Host only."""

    def __init__(self, desc: CrrDesc) -> None:
        out = (C.c_int * (4 + 2 * GMLP_MAX_LAYERS * 3))()
        _lib.check(_lib.load().osa_crr_layout(C.byref(desc), out), 'osa_crr_layout')
        self.Pa, self.Pc, self.oLS, self.nstat = (int(x) for x in out[:4])
        self.obs_dim, self.act_dim = int(desc.obs_dim), int(desc.act_dim)
        ins = (self.obs_dim, self.obs_dim + self.act_dim)
        self._layers = []
        k = 4
        for net in range(2):
            rows, prev = [], ins[net]
            for l in range(GMLP_MAX_LAYERS):
                oW, ob, ld = int(out[k]), int(out[k + 1]), int(out[k + 2])
                k += 3
                if oW >= 0:
                    rows.append((oW, ob, ld, int(desc.width[net][l]), prev))
                    prev = int(desc.width[net][l])
            self._layers.append(rows)

    def tensors(self, net: int, prefix: str | None = None) -> list[tuple[str, tuple[int, ...], np.ndarray]]:
        """``(name, shape, offsets)`` in the reference's state-dict order: the actor ``log_std, mean.0.weight, ...``;
        a critic of a pair ``<prefix>.0.weight, ...`` with prefix ``critic_j.0``."""
        items = []
        if net == 0:
            prefix = 'mean'
            items.append(('log_std', (self.act_dim,), self.oLS + np.arange(self.act_dim)))
        for j, (oW, ob, ld, n_out, n_in) in enumerate(self._layers[net]):
            ix = (oW + np.arange(n_out)[:, None] * ld + np.arange(n_in)[None, :]).reshape(-1)
            items.append((f'{prefix}.{2 * j}.weight', (n_out, n_in), ix))
            items.append((f'{prefix}.{2 * j}.bias', (n_out,), ob + np.arange(n_out)))
        return items

    def real_mask(self, net: int) -> np.ndarray:
        """True where a block holds a parameter, False in its padding."""
        mask = np.zeros(self.Pa if net == 0 else self.Pc, bool)
        for _, _, ix in self.tensors(net, 'x'):
            mask[ix] = True
        return mask


def _init_mlp(sizes, mode: str):
    """utils/model.py:25-45, 103-111: nn.Linear default-initialised, then the chosen initialiser on the weight."""
    out = []
    for j in range(len(sizes) - 1):
        lin = torch.nn.Linear(sizes[j], sizes[j + 1])
        if mode == 'kaiming_uniform':
            torch.nn.init.kaiming_uniform_(lin.weight, a=math.sqrt(5))
        elif mode == 'xavier_normal':
            torch.nn.init.xavier_normal_(lin.weight)
        elif mode in ('glorot', 'xavier_uniform'):
            torch.nn.init.xavier_uniform_(lin.weight)
        elif mode == 'orthogonal':
            torch.nn.init.orthogonal_(lin.weight, gain=math.sqrt(2))
        else:
            raise TypeError(f'Invalid initialization function: {mode}')
        out.append((lin.weight.detach().clone(), lin.bias.detach().clone()))
    return out


def initial_state_dicts(desc: CrrDesc, mode: str = 'kaiming_uniform'):
    """``(actor, [pair, ...])`` state dicts with the reference's initial weights for the current torch seed:
    construction order actor, reward critic pair, then (CCRR) cost critic pair (crr.py:71-112, c_crr.py:64-89)."""
    D, A = int(desc.obs_dim), int(desc.act_dim)
    a_sizes = [D] + [int(desc.width[0][l]) for l in range(desc.n_layers[0])]
    c_sizes = [D + A] + [int(desc.width[1][l]) for l in range(desc.n_layers[1])]
    actor = OrderedDict(log_std=torch.zeros(A))
    for j, (w, b) in enumerate(_init_mlp(a_sizes, mode)):
        actor[f'mean.{2 * j}.weight'], actor[f'mean.{2 * j}.bias'] = w, b
    pairs = []
    for _ in range(int(desc.pairs)):
        sd = OrderedDict()
        for c in range(2):
            for j, (w, b) in enumerate(_init_mlp(c_sizes, mode)):
                sd[f'critic_{c}.0.{2 * j}.weight'], sd[f'critic_{c}.0.{2 * j}.bias'] = w, b
        pairs.append(sd)
    return actor, pairs


def load_dataset(source, obs_dim: int, act_dim: int, device) -> dict[str, torch.Tensor]:
    """The six fields as contiguous float32 device tensors.  ``source``: the path of an ``.npz`` file the collector
    wrote, or an ``OfflineDataCollector`` whose ``data`` is on the device already.  A missing file (or a name that is
    no file: nothing is ever downloaded) is the FileNotFoundError of its ``open``; a missing field a KeyError naming
    it; rows that do not fit the env a ValueError."""
    if hasattr(source, 'data') and not isinstance(source, (str, os.PathLike)):
        raw = source.data
        if not raw:
            raise ValueError('the collector holds no data yet: call collect() first')
    else:
        with open(os.fspath(source), 'rb') as f:  # FileNotFoundError for a dataset name or a missing path
            npz = np.load(f)
            raw = {}
            for k in FIELDS:
                if k not in npz.files:
                    raise KeyError(k)
                raw[k] = npz[k]
    data = {}
    for k in FIELDS:
        if k not in raw:
            raise KeyError(k)
        data[k] = torch.as_tensor(raw[k]).to(device=device, dtype=torch.float32).contiguous()
    n = data['obs'].shape[0]
    want = {'obs': obs_dim, 'action': act_dim, 'reward': 1, 'cost': 1, 'next_obs': obs_dim, 'done': 1}
    for k, w in want.items():
        t = data[k]
        if t.dim() == 1 and w == 1:
            t = data[k] = t.reshape(-1, 1)
        if t.dim() != 2 or t.shape[0] != n or t.shape[1] != w or n < 1:
            raise ValueError(f'dataset field {k!r} has shape {tuple(t.shape)}; the env needs ({n}, {w})')
    return data


class CrrStep:  # pylint: disable=too-many-instance-attributes
    def __init__(self, desc: CrrDesc, data: dict[str, torch.Tensor], *, gamma: float, beta: float, polyak: float,
                 lr_actor: float, lr_critic: float, nslots: int, cost_limit: float = 0.0, lambda_lr: float = 0.0,
                 lambda_init: float = 0.0, wiring: str | None = None, device='cuda:0') -> None:
        self._lib = _lib.load(require_gpu=True)
        self.desc, self.device = desc, torch.device(device)
        self.layout = CrrLayout(desc)
        self.B, self.S, self.A, self.D = int(desc.batch), int(desc.samples), int(desc.act_dim), int(desc.obs_dim)
        self.pairs = int(desc.pairs)
        self.nslots = int(nslots)
        assert self.nslots >= 1
        wiring = os.environ.get('OSA_CCRR_WIRING', 'intended') if wiring is None else wiring
        if wiring not in ('intended', 'reference'):
            raise ValueError(f'OSA_CCRR_WIRING={wiring!r}: intended or reference')
        self.wiring = wiring
        f32 = dict(dtype=torch.float32, device=self.device)
        lay, nq = self.layout, 2 * self.pairs
        self.actor, self.actor_m, self.actor_v = (torch.zeros(lay.Pa, **f32) for _ in range(3))
        self.critic, self.critic_m, self.critic_v, self.target = (torch.zeros(nq, lay.Pc, **f32) for _ in range(4))
        self.adam_step = torch.zeros(1 + self.pairs, dtype=torch.int32, device=self.device)
        self.lagrange = torch.tensor([max(float(lambda_init), 0.0), 0.0, 0.0, 0.0], **f32)
        self.step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.stats = torch.zeros(self.nslots, lay.nstat, **f32)
        self.idx = torch.zeros(self.nslots, self.B, dtype=torch.int64, device=self.device)
        self.eps_next = torch.zeros(self.nslots, self.B, self.A, **f32)
        self.eps_next_c = torch.zeros(self.nslots, self.B, self.A, **f32) if self.pairs == 2 else None
        self.eps_samp = torch.zeros(self.nslots, self.B * self.S, self.A, **f32)
        self.ws_floats = int(self._lib.osa_crr_ws_floats(C.byref(desc)))
        self.ws = torch.zeros(self.ws_floats, **f32)
        self.data, self.n_rows, self._data = None, 0, None
        self.hp = CrrHParams(gamma=gamma, beta=beta, polyak=polyak, one_minus_polyak=1.0 - polyak, lr_actor=lr_actor,
                             lr_critic=lr_critic, beta1=0.9, beta2=0.999, adam_eps=1e-8, cost_limit=cost_limit,
                             lambda_lr=lambda_lr, lagrange_open=0, reference_wiring=int(wiring == 'reference'))
        p = _lib.ptr
        self._state = CrrState(p(self.actor), p(self.actor_m), p(self.actor_v), p(self.critic), p(self.critic_m),
                               p(self.critic_v), p(self.target), p(self.adam_step), p(self.lagrange), p(self.step))
        if data is not None:
            self.set_data(data)
        self._draws = CrrDrawBuffers(p(self.idx), p(self.eps_next), p(self.eps_next_c), p(self.eps_samp), self.nslots)
        self._index = {}
        for net in range(2):
            for c in range(2):
                key = (net, c)
                items = lay.tensors(net, f'critic_{c}.0')
                self._index[key] = (items, torch.from_numpy(np.concatenate([ix for _, _, ix in items])).to(self.device))

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
    def _get(self, block: torch.Tensor, key) -> 'OrderedDict[str, torch.Tensor]':
        items, flat_ix = self._index[key]
        flat = block[flat_ix]
        sd, i = OrderedDict(), 0
        for name, shape, ix in items:
            sd[name] = flat[i:i + len(ix)].reshape(shape).clone()
            i += len(ix)
        return sd

    def _set(self, block: torch.Tensor, key, sd) -> None:
        items, flat_ix = self._index[key]
        parts = []
        for name, shape, _ in items:
            t = torch.as_tensor(sd[name], dtype=torch.float32)
            assert tuple(t.shape) == tuple(shape), (name, tuple(t.shape), shape)
            parts.append(t.reshape(-1))
        block[flat_ix] = torch.cat(parts).to(self.device)

    def actor_state_dict(self, which: str = 'actor'):
        """``log_std, mean.0.weight, mean.0.bias, mean.2. ...`` of the actor (or of its Adam moments)."""
        return self._get(getattr(self, which), (0, 0))

    def load_actor_state_dict(self, sd, which: str = 'actor') -> None:
        self._set(getattr(self, which), (0, 0), sd)

    def critic_state_dict(self, pair: int, which: str = 'critic'):
        """``critic_0.0.0.weight, ..., critic_1.0.0.weight, ...`` of pair 0 (reward) or 1 (cost)."""
        sd = OrderedDict()
        for c in range(2):
            sd.update(self._get(getattr(self, which)[2 * pair + c], (1, c)))
        return sd

    def load_critic_state_dict(self, pair: int, sd, which: str = 'critic') -> None:
        for c in range(2):
            self._set(getattr(self, which)[2 * pair + c], (1, c), sd)

    def init_parameters(self, mode: str = 'kaiming_uniform') -> None:
        """The reference's initial weights for the current torch seed; targets are copies."""
        actor, pairs = initial_state_dicts(self.desc, mode)
        self.load_actor_state_dict(actor)
        for p, sd in enumerate(pairs):
            self.load_critic_state_dict(p, sd)
        self.target.copy_(self.critic)

    # ------------------------------------------------------------------ draws
    def draw(self, seed: int, first_step: int, nsteps: int) -> None:
        """The device draws of steps first_step .. first_step + nsteps - 1 into their slots."""
        assert 1 <= nsteps <= self.nslots
        _lib.check(self._lib.osa_crr_draws(
            C.byref(self.desc), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_step), int(nsteps), self.nslots, self.n_rows,
            _lib.ptr(self.idx), _lib.ptr(self.eps_next), _lib.ptr(self.eps_next_c), _lib.ptr(self.eps_samp),
            _lib.stream_ptr()), 'osa_crr_draws')

    def set_draws(self, first_step: int, idx, eps_next, eps_samp, eps_next_c=None) -> None:
        """Inject the draws of consecutive steps (leading dimension = steps) into their slots."""
        idx = torch.as_tensor(idx, dtype=torch.int64)
        n = idx.shape[0]
        assert 1 <= n <= self.nslots
        if int(idx.min()) < 0 or int(idx.max()) >= self.n_rows:
            raise ValueError(f'indices outside [0, {self.n_rows})')
        slots = (torch.arange(n) + int(first_step)) % self.nslots
        f32 = dict(dtype=torch.float32, device=self.device)
        self.idx[slots] = idx.reshape(n, self.B).to(self.device)
        self.eps_next[slots] = torch.as_tensor(eps_next).reshape(n, self.B, self.A).to(**f32)
        self.eps_samp[slots] = torch.as_tensor(eps_samp).reshape(n, self.B * self.S, self.A).to(**f32)
        if self.pairs == 2:
            self.eps_next_c[slots] = torch.as_tensor(eps_next_c).reshape(n, self.B, self.A).to(**f32)

    # ------------------------------------------------------------------ the step
    def run(self, nsteps: int = 1, lagrange_open: bool = False) -> None:
        """Enqueue ``nsteps`` train steps on the current stream (crr.py:114-200 / c_crr.py:91-206 each)."""
        assert self._data is not None, 'set_data() first'
        self.hp.lagrange_open = int(bool(lagrange_open))
        _lib.check(self._lib.osa_crr_step(
            C.byref(self.desc), C.byref(self.hp), C.byref(self._state), C.byref(self._data), C.byref(self._draws),
            _lib.ptr(self.stats), _lib.ptr(self.ws), self.ws_floats, int(nsteps), _lib.stream_ptr()), 'osa_crr_step')

    @property
    def policy_std(self) -> float:
        return float(torch.exp(self.actor[self.layout.oLS:self.layout.oLS + self.A]).mean())


__all__ = ['CrrDesc', 'CrrHParams', 'CrrLayout', 'CrrStep', 'STAT_KEYS', 'CRR_STATS', 'make_desc', 'load_dataset',
           'initial_state_dicts']
