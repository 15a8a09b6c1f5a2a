"""The device side of offline COptiDICE (csrc/dice_kernels.hip): the ``nu`` and ``chi`` networks of
models/offline/dice.py:27-87 and a ``GaussianLearningActor`` with the reference's state-dict names, the multipliers
``lambda`` and ``tau``, the dataset with its ``init_obs`` on the device, the draws and the train step.

``DiceStep`` owns the three parameter blocks with their Adam moments, the multipliers' state and the device step
counter.  ``run(n)`` enqueues n train steps on the current stream with no host synchronisation; ``stats`` holds the
per-step scalars ``[nslots][NSTAT]`` until the caller reads them.  Draws (row indices only) come from
``draw(seed, first_step, n)`` or are injected with ``set_draws`` (tests).  ``OSA_DICE_ROUTE=list|single`` chooses between
one launch per layer depth and one launch per problem (the timing comparison).
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .crr_step import FIELDS, _init_mlp, load_dataset
from .models import ACTIVATIONS, GMLP_MAX_LAYERS

STAT_KEYS = ('Loss/Loss_Nu', 'Loss/Loss_Chi', 'Loss/Loss_Lamb', 'Loss/Loss_Tau', 'Train/CostUB', 'Train/KL_divergence',
             'Train/tau', 'Train/lagrange_multiplier', 'Loss/Loss_actor', 'Train/PolicyStd')  # columns 0 .. 9
FN_TYPES = {'kl': 0, 'softchi': 1, 'chisquare': 2}  # OSA_DICE_FN_*
ROUTES = {'list': 0, 'single': 1}                   # OSA_DICE_ROUTE_*
NETS = ('nu', 'chi', 'actor')
DATA_FIELDS = FIELDS + ('init_obs',)


class DiceDesc(C.Structure):
    """ctypes mirror of ``osa_dice_desc``."""

    _fields_ = [('obs_dim', C.c_int), ('act_dim', C.c_int), ('n_hidden', C.c_int * 3),
                ('hidden', (C.c_int * GMLP_MAX_LAYERS) * 3), ('activation', C.c_int * 3), ('batch', C.c_int),
                ('fn_type', C.c_int)]


class DiceHParams(C.Structure):
    """ctypes mirror of ``osa_dice_hparams``."""

    _fields_ = [(n, C.c_float) for n in ('gamma', 'alpha', 'cost_limit', 'cost_ub_eps', 'lr_nu', 'lr_chi', 'lr_actor',
                                         'lr_lamb', 'lr_tau')] + [
        ('beta1', C.c_double), ('beta2', C.c_double), ('adam_eps', C.c_double), ('route', C.c_int)]


class DiceState(C.Structure):
    """ctypes mirror of ``osa_dice_state``."""

    _fields_ = [(n, C.c_void_p) for n in ('nu', 'nu_m', 'nu_v', 'chi', 'chi_m', 'chi_v', 'actor', 'actor_m', 'actor_v',
                                           'adam_step', 'mult', 'step')]


class DiceData(C.Structure):
    """ctypes mirror of ``osa_dice_data``."""

    _fields_ = [(n, C.c_void_p) for n in ('obs', 'act', 'reward', 'cost', 'next_obs', 'done', 'init_obs')] + [
        ('ld_obs', C.c_int), ('ld_act', C.c_int), ('ld_next', C.c_int), ('ld_init', C.c_int), ('n_rows', C.c_long)]


class DiceDrawBuffers(C.Structure):
    """ctypes mirror of ``osa_dice_draw_buffers``."""

    _fields_ = [('idx', C.c_void_p), ('nslots', C.c_int)]


def make_desc(obs_dim: int, act_dim: int, hidden: dict, activation: dict, batch: int, fn_type: str) -> DiceDesc:
    """The description of a COptiDICE problem; ``hidden`` and ``activation`` are keyed ``nu``, ``chi``, ``actor``.
    NotImplementedError, before any GPU is touched, for an unknown ``fn_type`` or activation and for a network without a
    hidden layer or with more than GMLP_MAX_LAYERS - 1."""
    if fn_type not in FN_TYPES:
        raise NotImplementedError(f'fn_type {fn_type!r}: one of {list(FN_TYPES)}')
    d = DiceDesc()
    d.obs_dim, d.act_dim, d.batch, d.fn_type = int(obs_dim), int(act_dim), int(batch), FN_TYPES[fn_type]
    for k, net in enumerate(NETS):
        sizes = [int(h) for h in hidden[net]]
        if activation[net] not in ACTIVATIONS:
            raise NotImplementedError(f'activation {activation[net]!r}: one of {list(ACTIVATIONS)}')
        if not 1 <= len(sizes) <= GMLP_MAX_LAYERS - 1 or any(h < 1 or h > 4096 for h in sizes):
            raise NotImplementedError(f'{net}.hidden_sizes {sizes}: 1 .. {GMLP_MAX_LAYERS - 1} hidden layers of width '
                                      '1 .. 4096')
        d.n_hidden[k] = len(sizes)
        for l, w in enumerate(sizes):
            d.hidden[k][l] = w
        d.activation[k] = ACTIVATIONS[activation[net]]
    return d


def _sizes(desc: DiceDesc, k: int) -> list[int]:
    return ([int(desc.obs_dim)] + [int(desc.hidden[k][l]) for l in range(desc.n_hidden[k])]
            + [int(desc.act_dim) if k == 2 else 1])


class DiceLayout:
    """Offsets of the reference's tensors inside the padded blocks (osa_dice_layout).  Host only: a batch above
    ``max_batch`` is refused here, before any launch."""

    def __init__(self, desc: DiceDesc) -> None:
        out = (C.c_int * (6 + 3 * GMLP_MAX_LAYERS * 3))()
        _lib.check(_lib.load().osa_dice_layout(C.byref(desc), out), 'osa_dice_layout')
        self.P = tuple(int(x) for x in out[:3])
        self.oLS, self.nstat, self.max_batch = int(out[3]), int(out[4]), int(out[5])
        self.act_dim = int(desc.act_dim)
        self._layers, k = [], 6
        for net in range(3):
            sizes, rows = _sizes(desc, net), []
            for l in range(GMLP_MAX_LAYERS):
                oW, ob, ld = int(out[k]), int(out[k + 1]), int(out[k + 2])
                k += 3
                if oW >= 0:
                    rows.append((oW, ob, ld, sizes[l + 1], sizes[l]))
            self._layers.append(rows)

    def tensors(self, net: int) -> list[tuple[str, tuple[int, ...], np.ndarray]]:
        """``(name, shape, offsets)`` in the reference's state-dict order: ``net.0.weight, ...`` of an ObsEncoder (net 0,
        1), ``log_std, mean.0.weight, ...`` of the actor (net 2)."""
        items, prefix = [], 'mean' if net == 2 else 'net'
        if net == 2:
            items.append(('log_std', (self.act_dim,), self.oLS + np.arange(self.act_dim)))
        for j, (oW, ob, ld, n_out, n_in) in enumerate(self._layers[net]):
            ix = (oW + np.arange(n_out)[:, None] * ld + np.arange(n_in)[None, :]).reshape(-1)
            items.append((f'{prefix}.{2 * j}.weight', (n_out, n_in), ix))
            items.append((f'{prefix}.{2 * j}.bias', (n_out,), ob + np.arange(n_out)))
        return items

    def real_mask(self, net: int) -> np.ndarray:
        """True where a block holds a parameter, False in its padding."""
        mask = np.zeros(self.P[net], bool)
        for _, _, ix in self.tensors(net):
            mask[ix] = True
        return mask


def episode_starts(obs: np.ndarray, next_obs: np.ndarray, done: np.ndarray) -> np.ndarray:
    """True where row i starts an episode: ``i == 0``, or ``done[i - 1] == 1``, or ``obs[i] != next_obs[i - 1]`` anywhere
    in the row.  Holds for files of ``OfflineDataCollector``: lanes are contiguous and each lane starts with a reset."""
    n = obs.shape[0]
    start = np.ones(n, bool)
    if n > 1:
        start[1:] = (np.asarray(done).reshape(n)[:-1] == 1) | (obs[1:] != next_obs[:-1]).any(axis=1)
    return start


def load_init_obs(source, data: dict[str, torch.Tensor]) -> torch.Tensor:
    """``init_obs`` for ``data`` (load_dataset's tensors): the field of the ``.npz`` file ``source`` where it carries one
    (what dataset.py:329-335 requires), else derived on the host -- every row gets the ``obs`` of its episode's first row
    (``episode_starts``)."""
    obs = data['obs']
    if isinstance(source, (str, os.PathLike)):
        with open(os.fspath(source), 'rb') as f:
            npz = np.load(f)
            if 'init_obs' in npz.files:
                init = torch.as_tensor(npz['init_obs']).to(device=obs.device, dtype=torch.float32).contiguous()
                if init.shape != obs.shape:
                    raise ValueError(f"dataset field 'init_obs' has shape {tuple(init.shape)}; obs has {tuple(obs.shape)}")
                return init
    start = episode_starts(obs.cpu().numpy(), data['next_obs'].cpu().numpy(), data['done'].cpu().numpy())
    first = np.maximum.accumulate(np.where(start, np.arange(len(start)), 0))
    return obs[torch.from_numpy(first).to(obs.device)].contiguous()


def route_of(name: str | None = None) -> int:
    name = os.environ.get('OSA_DICE_ROUTE', '') if name is None else name
    if name not in ('', *ROUTES):
        raise ValueError(f'OSA_DICE_ROUTE={name!r}: list or single')
    return ROUTES[name or 'list']


class DiceStep:  # pylint: disable=too-many-instance-attributes
    def __init__(self, desc: DiceDesc, data: dict[str, torch.Tensor] | None, *, gamma: float, alpha: float,
                 cost_limit: float, cost_ub_eps: float, lr_nu: float, lr_chi: float, lr_actor: float, lr_lamb: float,
                 lr_tau: float, lamb_init: float, tau_init: float, nslots: int, route: str | None = None,
                 device='cuda:0') -> None:
        self.route = route_of(route)
        self.layout = lay = DiceLayout(desc)  # (refuses the description before any GPU is touched)
        self._lib = _lib.load(require_gpu=True)
        self.desc, self.device = desc, torch.device(device)
        self.D, self.A, self.B = int(desc.obs_dim), int(desc.act_dim), int(desc.batch)
        self.nslots = int(nslots)
        assert self.nslots >= 1
        self.f32 = f32 = dict(dtype=torch.float32, device=self.device)
        for k, net in enumerate(NETS):
            for which in ('', '_m', '_v'):
                setattr(self, net + which, torch.zeros(lay.P[k], **f32))
        self.adam_step = torch.zeros(2, dtype=torch.int32, device=self.device)
        # coptidice.py:140-160: lambda = clamp(init, 0, 1e3), tau = init + 1e-6, both float32
        lam0 = float(torch.clamp(torch.tensor(lamb_init, dtype=torch.float32), 0, 1e3))
        tau0 = float(torch.tensor(tau_init, dtype=torch.float32) + 1e-6)
        self.mult = torch.tensor([lam0, 0, 0, 0, tau0, 0, 0, 0], **f32)
        self.step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.stats = torch.zeros(self.nslots, lay.nstat, **f32)
        self.idx = torch.zeros(self.nslots, self.B, dtype=torch.int64, device=self.device)
        self.ws_floats = int(self._lib.osa_dice_ws_floats(C.byref(desc)))
        self.ws = torch.zeros(self.ws_floats, **f32)
        self.data, self.n_rows, self._data = None, 0, None
        self.hp = DiceHParams(gamma=gamma, alpha=alpha, cost_limit=cost_limit, cost_ub_eps=cost_ub_eps, lr_nu=lr_nu,
                              lr_chi=lr_chi, lr_actor=lr_actor, lr_lamb=lr_lamb, lr_tau=lr_tau, beta1=0.9, beta2=0.999,
                              adam_eps=1e-8, route=self.route)
        p = _lib.ptr
        self._state = DiceState(*(p(getattr(self, net + which)) for net in NETS for which in ('', '_m', '_v')),
                                p(self.adam_step), p(self.mult), p(self.step))
        self._draws = DiceDrawBuffers(p(self.idx), self.nslots)
        self._ix = []
        for k in range(3):
            items = lay.tensors(k)
            self._ix.append((items, torch.from_numpy(np.concatenate([ix for _, _, ix in items])).to(self.device)))
        if data is not None:
            self.set_data(data)

    def set_data(self, data: dict[str, torch.Tensor]) -> None:
        """The dataset (load_dataset's six device tensors and ``init_obs``); read by every step, never written."""
        p = _lib.ptr
        for k in DATA_FIELDS:
            t = data[k]
            assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1, k
        assert data['init_obs'].shape == data['obs'].shape
        self.data = data
        self.n_rows = int(data['obs'].shape[0])
        self._data = DiceData(p(data['obs']), p(data['action']), p(data['reward']), p(data['cost']), p(data['next_obs']),
                              p(data['done']), p(data['init_obs']), data['obs'].stride(0), data['action'].stride(0),
                              data['next_obs'].stride(0), data['init_obs'].stride(0), self.n_rows)

    # ------------------------------------------------------------------ state dicts
    def state_dict(self, net: str = 'actor', which: str = ''):
        """``net.0.weight, ...`` of ``nu`` / ``chi``, ``log_std, mean.0.weight, ...`` of the actor (of the parameters, or
        of an Adam moment: ``which='_m'`` / ``'_v'``)."""
        items, flat_ix = self._ix[NETS.index(net)]
        flat = getattr(self, net + which)[flat_ix]
        sd, i = OrderedDict(), 0
        for name, shape, ix in items:
            sd[name] = flat[i:i + len(ix)].reshape(shape).clone()
            i += len(ix)
        return sd

    def load_state_dict(self, sd, net: str = 'actor', which: str = '') -> None:
        items, flat_ix = self._ix[NETS.index(net)]
        parts = []
        for name, shape, _ in items:
            t = torch.as_tensor(sd[name], dtype=torch.float32)
            assert tuple(t.shape) == tuple(shape), (name, tuple(t.shape), shape)
            parts.append(t.reshape(-1))
        getattr(self, net + which)[flat_ix] = torch.cat(parts).to(self.device)

    def actor_state_dict(self):
        return self.state_dict('actor')

    def init_parameters(self, mode: str = 'kaiming_uniform') -> None:
        """The reference's initial weights for the current torch seed, in its construction order: the actor, nu, chi
        (coptidice.py:93-138)."""
        for k in (2, 0, 1):
            prefix = 'mean' if k == 2 else 'net'
            sd = OrderedDict(log_std=torch.zeros(self.A)) if k == 2 else OrderedDict()
            for j, (w, b) in enumerate(_init_mlp(_sizes(self.desc, k), mode)):
                sd[f'{prefix}.{2 * j}.weight'], sd[f'{prefix}.{2 * j}.bias'] = w, b
            self.load_state_dict(sd, NETS[k])

    # ------------------------------------------------------------------ draws
    def draw(self, seed: int, first_step: int, nsteps: int) -> None:
        """The device draws of steps first_step .. first_step + nsteps - 1 into their slots."""
        assert 1 <= nsteps <= self.nslots
        _lib.check(self._lib.osa_dice_draws(
            C.byref(self.desc), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_step), int(nsteps), self.nslots, self.n_rows,
            _lib.ptr(self.idx), _lib.stream_ptr()), 'osa_dice_draws')

    def set_draws(self, first_step: int, idx) -> None:
        """Inject the row indices of consecutive steps (leading dimension = steps) into their slots."""
        idx = torch.as_tensor(idx, dtype=torch.int64)
        n = idx.shape[0]
        assert 1 <= n <= self.nslots
        if int(idx.min()) < 0 or int(idx.max()) >= self.n_rows:
            raise ValueError(f'indices outside [0, {self.n_rows})')
        slots = (torch.arange(n) + int(first_step)) % self.nslots
        self.idx[slots] = idx.reshape(n, self.B).to(self.device)

    # ------------------------------------------------------------------ the step
    def run(self, nsteps: int = 1, lagrange_open: bool = False) -> None:  # pylint: disable=unused-argument
        """Enqueue ``nsteps`` train steps on the current stream (coptidice.py:162-275 each)."""
        assert self._data is not None, 'set_data() first'
        _lib.check(self._lib.osa_dice_step(
            C.byref(self.desc), C.byref(self.hp), C.byref(self._state), C.byref(self._data), C.byref(self._draws),
            _lib.ptr(self.stats), _lib.ptr(self.ws), self.ws_floats, int(nsteps), _lib.stream_ptr()), 'osa_dice_step')

    def values(self, obs: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """``nu(obs)`` and ``chi(obs)`` of at most ``3 B`` plain rows."""
        obs = obs.to(**self.f32)
        n = int(obs.shape[0])
        assert obs.dim() == 2 and obs.shape[1] == self.D and obs.stride(1) == 1 and 1 <= n <= 3 * self.B
        nu, chi = torch.empty(n, **self.f32), torch.empty(n, **self.f32)
        p = _lib.ptr
        _lib.check(self._lib.osa_dice_values(
            C.byref(self.desc), self.route, p(self.nu), p(self.chi), p(obs), obs.stride(0), n, p(nu), p(chi), p(self.ws),
            self.ws_floats, _lib.stream_ptr()), 'osa_dice_values')
        return nu, chi

    @property
    def lamb(self) -> float:
        return float(self.mult[0])

    @property
    def tau(self) -> float:
        return float(self.mult[4])


__all__ = ['DiceDesc', 'DiceHParams', 'DiceLayout', 'DiceStep', 'STAT_KEYS', 'FN_TYPES', 'make_desc', 'load_dataset',
           'load_init_obs', 'episode_starts']
