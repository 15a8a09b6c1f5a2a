"""HBM-resident ConstraintActorCritic.

Mirror of omnisafe/models/actor_critic/constraint_actor_critic.py:57-109 (+ actor_critic.py:60-136,
models/actor/gaussian_learning_actor.py:29-139, models/critic/v_critic.py:40-92): a Gaussian MLP
policy with state-independent log_std, a reward critic and a cost critic, each with an Adam optimiser,
and a LinearLR/ConstantLR schedule on the actor.  Instead of three torch modules the three networks
are three padded float32 blocks in ONE device tensor ``params[3][P]`` (layout: osa_mlp_layout), with
Adam moments and gradients in tensors of the same shape; every forward / backward / optimiser step is
a HIP kernel of libomnisafe_amd.  ``state_dict()`` of each network reproduces the reference's
parameter names, shapes and order, so checkpoints (``torch_save/epoch-N.pt`` key ``pi``) stay loadable
by the reference's Evaluator.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .spaces import is_box

# activation codes of the C ABI (csrc/mlp_device.h OSA_ACT_*)
ACTIVATIONS = {'tanh': 0, 'relu': 1, 'sigmoid': 2, 'softplus': 3, 'identity': 4}
ACTOR, REWARD_CRITIC, COST_CRITIC = 0, 1, 2


class HParams(C.Structure):
    """ctypes mirror of ``osa_ppo_hparams`` (include/omnisafe_amd.h)."""

    _fields_ = [('clip', C.c_float), ('entropy_coef', C.c_float), ('critic_norm_coef', C.c_float),
                ('max_grad_norm', C.c_float), ('lr_actor', C.c_float), ('lr_critic', C.c_float),
                ('beta1', C.c_float), ('beta2', C.c_float), ('adam_eps', C.c_float),
                ('use_critic_norm', C.c_int), ('use_max_grad_norm', C.c_int), ('use_cost', C.c_int),
                ('lr_device', C.c_void_p)]


class SurrogateExt(C.Structure):
    """ctypes mirror of ``osa_surrogate_ext`` (include/omnisafe_amd.h): FOCOPS / CUP / P3O actor losses."""

    _fields_ = [('old_mean', C.c_void_p), ('ld_old_mean', C.c_int), ('old_log_std', C.c_void_p),
                ('kl_coef', C.c_float), ('kl_mask_eta', C.c_float), ('ratio_scale', C.c_float),
                ('cost_kappa', C.c_float), ('cost_excess', C.c_float)]

    def __init__(self, kl_coef: float = 0.0, kl_mask_eta: float = -1.0, ratio_scale: float = 1.0,
                 cost_kappa: float = 0.0, cost_excess: float = 0.0) -> None:
        super().__init__(None, 0, None, kl_coef, kl_mask_eta, ratio_scale, cost_kappa, cost_excess)


class PassMember(C.Structure):
    """ctypes mirror of ``osa_pass_member`` (include/omnisafe_amd.h): one agent's pass in osa_ppo_pass_group."""

    _fields_ = [('params', C.c_void_p), ('adam_m', C.c_void_p), ('adam_v', C.c_void_p), ('adam_step', C.c_void_p),
                ('obs', C.c_void_p), ('ld_obs', C.c_int), ('act', C.c_void_p), ('ld_act', C.c_int),
                ('logp', C.c_void_p), ('target_value_r', C.c_void_p), ('target_value_c', C.c_void_p),
                ('adv_r', C.c_void_p), ('adv_c', C.c_void_p), ('perm', C.c_void_p), ('M', C.c_long), ('B', C.c_int),
                ('lagrange', C.c_void_p), ('hp', HParams), ('loss_kind', C.c_int), ('nets_mask', C.c_int),
                ('step_stats', C.c_void_p), ('has_ext', C.c_int), ('ext', SurrogateExt)]


class Layout:
    """Padded parameter block of one network + index maps to the reference tensor order."""

    def __init__(self, obs_dim: int, act_dim: int, hidden: int):
        lib = _lib.load()
        out = (C.c_int * 12)()
        _lib.check(lib.osa_mlp_layout(obs_dim, act_dim, hidden, out), 'osa_mlp_layout')
        (self.INP, self.OUTP, self.oW1, self.ob1, self.oW2, self.ob2, self.oW3, self.ob3, self.oLS,
         self.P, self.H, self.KB) = list(out)
        self.obs_dim, self.act_dim = obs_dim, act_dim

    def tensors(self, net: int) -> list[tuple[str, tuple[int, ...], np.ndarray]]:
        """(name, shape, padded offsets) in the reference's ``named_parameters`` order: the actor
        yields log_std first (its own Parameter precedes sub-modules), then mean.{0,2,4}.{weight,bias};
        critics yield critic_0.{0,2,4}.{weight,bias}."""
        H, D_o = self.H, self.obs_dim
        out_dim = self.act_dim if net == ACTOR else 1
        prefix = 'mean' if net == ACTOR else 'critic_0'

        def mat(off, rows, cols, ld):
            return (off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]).reshape(-1)

        items = []
        if net == ACTOR:
            items.append(('log_std', (self.act_dim,), self.oLS + np.arange(self.act_dim)))
        items += [
            (f'{prefix}.0.weight', (H, D_o), mat(self.oW1, H, D_o, self.INP)),
            (f'{prefix}.0.bias', (H,), self.ob1 + np.arange(H)),
            (f'{prefix}.2.weight', (H, H), mat(self.oW2, H, H, H)),
            (f'{prefix}.2.bias', (H,), self.ob2 + np.arange(H)),
            (f'{prefix}.4.weight', (out_dim, H), mat(self.oW3, out_dim, H, H)),
            (f'{prefix}.4.bias', (out_dim,), self.ob3 + np.arange(out_dim)),
        ]
        return items


GMLP_MAX_LAYERS = 8


class GmlpDesc(C.Structure):
    """ctypes mirror of ``osa_gmlp_desc`` (include/omnisafe_amd.h): the shapes of a GENERAL actor-critic."""

    _fields_ = [('obs_dim', C.c_int), ('act_dim', C.c_int), ('n_layers', C.c_int * 3),
                ('width', (C.c_int * GMLP_MAX_LAYERS) * 3), ('activation', C.c_int * 3)]


class GeneralLayout:
    """Parameter blocks of general networks (any hidden_sizes; csrc/general_mlp.hip): same interface as Layout."""

    def __init__(self, desc: GmlpDesc, sizes: list[list[int]]):
        lib = _lib.load()
        out = (C.c_int * (2 + 3 * GMLP_MAX_LAYERS * 3))()
        _lib.check(lib.osa_gmlp_layout(C.byref(desc), out), 'osa_gmlp_layout')
        self.P, self.oLS = int(out[0]), int(out[1])
        self.obs_dim, self.act_dim = int(desc.obs_dim), int(desc.act_dim)
        self.OUTP = (self.act_dim + 3) // 4 * 4
        self._layers = []  # per network: [(oW, ob, ld, out, in)]
        k = 2
        for net in range(3):
            rows = []
            for l in range(GMLP_MAX_LAYERS):
                oW, ob, ld = int(out[k]), int(out[k + 1]), int(out[k + 2])
                k += 3
                if oW >= 0:
                    rows.append((oW, ob, ld, sizes[net][l + 1], sizes[net][l]))
            self._layers.append(rows)

    def tensors(self, net: int) -> list[tuple[str, tuple[int, ...], np.ndarray]]:
        """Reference `named_parameters` order (utils/model.py:103-111: Linear layers at Sequential indices 0, 2, 4 ...)."""
        prefix = 'mean' if net == ACTOR else 'critic_0'
        items = []
        if net == ACTOR:
            items.append(('log_std', (self.act_dim,), self.oLS + np.arange(self.act_dim)))
        for j, (oW, ob, ld, n_out, n_in) in enumerate(self._layers[net]):
            ix = (oW + np.arange(n_out)[:, None] * ld + np.arange(n_in)[None, :]).reshape(-1)
            items.append((f'{prefix}.{2 * j}.weight', (n_out, n_in), ix))
            items.append((f'{prefix}.{2 * j}.bias', (n_out,), ob + np.arange(n_out)))
        return items


class NetView:
    """One network of the actor-critic: reference-shaped access to its padded parameter block."""

    def __init__(self, owner: 'ConstraintActorCritic', net: int):
        self._o, self._net = owner, net
        items = owner.layout.tensors(net)
        self._items = items
        self._flat_index = torch.from_numpy(np.concatenate([ix for _, _, ix in items])).to(owner.device)

    @property
    def num_params(self) -> int:
        return int(self._flat_index.numel())

    def _block(self, which: str = 'params') -> torch.Tensor:
        return getattr(self._o, which)[self._net]

    def flat_params(self) -> torch.Tensor:
        """get_flat_params_from (omnisafe/utils/tools.py:35-65): reference-ordered flat vector."""
        return self._block('params')[self._flat_index]

    def flat_grads(self) -> torch.Tensor:
        """get_flat_gradients_from (tools.py:68-91)."""
        return self._block('grads')[self._flat_index]

    def set_flat_params(self, vals: torch.Tensor) -> None:
        """set_param_values_to_model (tools.py:94-129)."""
        assert vals.numel() == self.num_params
        self._block('params')[self._flat_index] = vals.to(self._o.device, torch.float32)

    def pad(self, flat_ref: torch.Tensor) -> torch.Tensor:
        """Reference-ordered flat vector -> padded block vector (zeros in the padding)."""
        out = torch.zeros(self._o.layout.P, dtype=torch.float32, device=self._o.device)
        out[self._flat_index] = flat_ref.to(self._o.device, torch.float32)
        return out

    def unpad(self, padded: torch.Tensor) -> torch.Tensor:
        return padded[self._flat_index]

    def state_dict(self) -> 'OrderedDict[str, torch.Tensor]':
        flat = self.flat_params()
        sd, i = OrderedDict(), 0
        for name, shape, ix in self._items:
            sd[name] = flat[i:i + len(ix)].reshape(shape).clone()
            i += len(ix)
        return sd

    def load_state_dict(self, sd) -> None:
        parts = []
        for name, shape, _ in self._items:
            t = torch.as_tensor(sd[name], dtype=torch.float32)
            assert tuple(t.shape) == tuple(shape), (name, tuple(t.shape), shape)
            parts.append(t.reshape(-1))
        self.set_flat_params(torch.cat(parts))

    def parameters(self):
        return list(self.state_dict().values())

    @property
    def std(self) -> float:
        """GaussianLearningActor.std (gaussian_learning_actor.py:131-134)."""
        assert self._net == ACTOR
        lay = self._o.layout
        return float(torch.exp(self._block()[lay.oLS:lay.oLS + lay.act_dim]).mean())

    @std.setter
    def std(self, std: float) -> None:
        """gaussian_learning_actor.py:136-139: log_std.fill_(log(std)), float32 like the reference."""
        assert self._net == ACTOR
        self.log_std.fill_(float(torch.log(torch.tensor(std))))

    @property
    def log_std(self) -> torch.Tensor:
        lay = self._o.layout
        return self._block()[lay.oLS:lay.oLS + lay.act_dim]


class _ActorSchedule:
    """LinearLR(start_factor=1, end_factor=0, total_iters=epochs) / ConstantLR(factor=1)
    (actor_critic.py:99-113), closed form."""

    def __init__(self, base_lr: float, epochs: int, linear: bool):
        self.base_lr, self.epochs, self.linear, self.k = base_lr, max(int(epochs), 1), linear, 0

    def step(self) -> None:
        self.k += 1

    def get_last_lr(self) -> list[float]:
        if not self.linear:
            return [self.base_lr]
        return [self.base_lr * (1.0 - min(self.k, self.epochs) / self.epochs)]


class ConstraintActorCritic:  # pylint: disable=too-many-instance-attributes
    """``ConstraintActorCritic(obs_space, act_space, model_cfgs, epochs)`` on the device.

    ``model_cfgs`` needs: actor.hidden_sizes/activation/lr, critic.hidden_sizes/activation/lr,
    weight_initialization_mode, actor_type, linear_lr_decay (attribute access, like the reference's
    Config)."""

    def __init__(self, obs_space, act_space, model_cfgs, epochs: int, device='cuda:0') -> None:
        if not is_box(obs_space) or not is_box(act_space):
            raise NotImplementedError  # models/base.py:66-74
        self.device = torch.device(device)
        self.obs_dim, self.act_dim = int(obs_space.shape[0]), int(act_space.shape[0])
        a_h, c_h = [int(h) for h in model_cfgs.actor.hidden_sizes], [int(h) for h in model_cfgs.critic.hidden_sizes]
        # hidden activation (utils/model.py:47-70: identity / relu / sigmoid / softplus / tanh)
        for act_name in (model_cfgs.actor.activation, model_cfgs.critic.activation):
            if act_name not in ACTIVATIONS:
                raise NotImplementedError(f'activation {act_name!r}: one of {list(ACTIVATIONS)}')
        if getattr(model_cfgs, 'actor_type', 'gaussian_learning') != 'gaussian_learning':
            raise NotImplementedError('only actor_type gaussian_learning is on the accelerated path')
        if any(h < 1 for h in a_h + c_h) or max(len(a_h), len(c_h)) + 1 > GMLP_MAX_LAYERS:
            raise NotImplementedError(f'hidden_sizes {a_h}/{c_h}: 0 .. {GMLP_MAX_LAYERS - 1} hidden layers of width >= 1')
        self.activation = model_cfgs.actor.activation
        self.hidden_sizes = (a_h, c_h)
        # Two kernel families behind one interface:
        #   FUSED    [H, H] with H in 32, 64, 128, 256, one activation for actor and critics -- a network fits a compute
        #            unit (mlp_kernels.hip; H = 64 with tanh, every on-policy YAML default, also runs the persistent
        #            passes); the activation code rides in bits 16-19 of the `hidden` word of the C ABI
        #   GENERAL  everything else utils/model.py:73-111 builds (any depth / widths, actor != critics, e.g. the
        #            1024 x 1024 networks of docs/source/start/efficiency.rst:15-23): layer-wise on the float32-MFMA GEMM
        #            of general_mlp.hip, shapes in an osa_gmlp_desc.  OSA_FORCE_GENERAL_MLP=1 sends fused-family shapes
        #            there too (how the tests pin the general path to the reference goldens)
        fused_ok = (a_h == c_h and len(a_h) == 2 and a_h[0] == a_h[1] and a_h[0] in (32, 64, 128, 256)
                    and model_cfgs.actor.activation == model_cfgs.critic.activation)
        import os as _os

        self.general = (not fused_ok) or _os.environ.get('OSA_FORCE_GENERAL_MLP', '0') == '1'
        self.width = int(a_h[0]) if a_h else 0
        self._lib = _lib.load(require_gpu=True)  # (after the configuration checks: those need no GPU)
        if self.general:
            self.hidden = 0  # (no fused kernel takes this network: every osa_*_supported(..., hidden = 0) says no)
            sizes = [[self.obs_dim] + a_h + [self.act_dim], [self.obs_dim] + c_h + [1], [self.obs_dim] + c_h + [1]]
            d = GmlpDesc()
            d.obs_dim, d.act_dim = self.obs_dim, self.act_dim
            acts = (model_cfgs.actor.activation, model_cfgs.critic.activation, model_cfgs.critic.activation)
            for net in range(3):
                d.n_layers[net] = len(sizes[net]) - 1
                for l, w in enumerate(sizes[net][1:]):
                    d.width[net][l] = w
                d.activation[net] = ACTIVATIONS[acts[net]]
            self.desc = d
            self.layout = GeneralLayout(d, sizes)
            self._gws: torch.Tensor | None = None
            self._gfin = torch.zeros(24, dtype=torch.float32, device=self.device)
        else:
            self.hidden = self.width | (ACTIVATIONS[self.activation] << 16)  # what the C ABI calls `hidden`
            self.layout = Layout(self.obs_dim, self.act_dim, self.hidden)
        P = self.layout.P
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(3, P, **f32)
        self.adam_m = torch.zeros(3, P, **f32)
        self.adam_v = torch.zeros(3, P, **f32)
        self.grads = torch.zeros(3, P, **f32)
        self.adam_step = torch.zeros(3, dtype=torch.int32, device=self.device)
        self.actor = NetView(self, ACTOR)
        self.reward_critic = NetView(self, REWARD_CRITIC)
        self.cost_critic = NetView(self, COST_CRITIC)
        self._init_parameters(getattr(model_cfgs, 'weight_initialization_mode', 'kaiming_uniform'))
        self.actor_lr = model_cfgs.actor.lr
        self.critic_lr = model_cfgs.critic.lr
        if self.actor_lr is not None:
            self.actor_scheduler = _ActorSchedule(float(self.actor_lr), epochs,
                                                  bool(getattr(model_cfgs, 'linear_lr_decay', True)))
        self._rng_offset = 0  # host part of the Philox stream position (by value); see commit_rng
        self._rng_base = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.seed = 0

    # ------------------------------------------------------------------ init
    def _init_parameters(self, mode: str) -> None:
        """Same construction order and initialisers as the reference so that an identical torch seed
        yields identical initial weights: actor mean layers, reward critic, cost critic; each
        nn.Linear default-initialised then kaiming_uniform_(a=sqrt(5)) on the weight
        (omnisafe/utils/model.py:25-45,103-111).  Runs once on the host (plumbing, not hot path)."""
        def mlp_state(sizes, prefix):
            sd = OrderedDict()
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
                sd[f'{prefix}.{2 * j}.weight'] = lin.weight.detach()
                sd[f'{prefix}.{2 * j}.bias'] = lin.bias.detach()
            return sd

        a_h, c_h = self.hidden_sizes
        sd = mlp_state([self.obs_dim] + a_h + [self.act_dim], 'mean')
        sd['log_std'] = torch.zeros(self.act_dim)
        self.actor.load_state_dict(sd)
        self.reward_critic.load_state_dict(mlp_state([self.obs_dim] + c_h + [1], 'critic_0'))
        self.cost_critic.load_state_dict(mlp_state([self.obs_dim] + c_h + [1], 'critic_0'))

    # ------------------------------------------------------------------ general networks: scratch
    def gmlp_ws(self, rows: int) -> tuple[torch.Tensor, int]:
        """Scratch of the layer-wise path for a call over `rows` rows (grow-only; the library carves it up by `rows`)."""
        need = int(self._lib.osa_gmlp_ws_floats(C.byref(self.desc), int(rows)))
        assert need > 0
        if self._gws is None or self._gws.numel() < need:
            self._gws = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._gws, int(self._gws.numel())

    # ------------------------------------------------------------------ rollout step
    def step(self, obs: torch.Tensor, deterministic: bool = False, eps: torch.Tensor | None = None,
             out: dict | None = None, nets_mask: int = 7):
        """constraint_actor_critic.py:84-109: ``(act, value_r, value_c, logp)`` for a batch (N, D_o) or a
        single row (D_o,).  ``eps`` injects the standard-normal noise (tests); ``out`` may provide
        pre-allocated destination tensors (e.g. rows of the rollout buffer)."""
        single = obs.dim() == 1
        x = obs.reshape(-1, self.obs_dim).to(self.device, torch.float32)
        if not x.is_contiguous():
            x = x.contiguous()
        N = x.shape[0]
        o = out or {}
        f32 = dict(dtype=torch.float32, device=self.device)
        act = o.get('act') if 'act' in o else torch.empty(N, self.act_dim, **f32)
        v_r = o.get('value_r') if 'value_r' in o else torch.empty(N, **f32)
        v_c = o.get('value_c') if 'value_c' in o else torch.empty(N, **f32)
        logp = o.get('logp') if 'logp' in o else torch.empty(N, **f32)
        e = None
        if eps is not None:
            e = eps.reshape(N, self.act_dim).to(self.device, torch.float32).contiguous()
        self._rng_offset += 1
        sc = o.get('scale')  # (act_env rows, old_min, old_max, min_action, max_action): ActionScale in the same launch
        if self.general:
            ws, nws = self.gmlp_ws(N)
            _lib.check(self._lib.osa_gmlp_policy_step(
                C.byref(self.desc), _lib.ptr(self.params), _lib.ptr(x), x.stride(0), N, _lib.ptr(e), self.seed,
                self._rng_offset, _lib.ptr(self._rng_base), int(deterministic), nets_mask, _lib.ptr(act), self.act_dim,
                _lib.ptr(v_r), _lib.ptr(v_c), _lib.ptr(logp), None, 0,
                _lib.ptr(sc[0]) if sc else None, sc[0].stride(0) if sc else 0, _lib.ptr(sc[1]) if sc else None,
                _lib.ptr(sc[2]) if sc else None, float(sc[3]) if sc else 0.0, float(sc[4]) if sc else 1.0,
                _lib.ptr(ws), nws, _lib.stream_ptr()), 'osa_gmlp_policy_step')
            if single:
                return act[0], v_r[0], v_c[0], logp[0]
            return act, v_r, v_c, logp
        _lib.check(self._lib.osa_policy_step_scaled(
            self.obs_dim, self.act_dim, self.hidden, _lib.ptr(self.params), _lib.ptr(x), x.stride(0), N,
            _lib.ptr(e), self.seed, self._rng_offset, _lib.ptr(self._rng_base), int(deterministic), nets_mask,
            _lib.ptr(act),
            self.act_dim, _lib.ptr(v_r), _lib.ptr(v_c), _lib.ptr(logp), None, 0,
            _lib.ptr(sc[0]) if sc else None, sc[0].stride(0) if sc else 0, _lib.ptr(sc[1]) if sc else None,
            _lib.ptr(sc[2]) if sc else None, float(sc[3]) if sc else 0.0, float(sc[4]) if sc else 1.0,
            _lib.stream_ptr()), 'osa_policy_step_scaled')
        if single:
            return act[0], v_r[0], v_c[0], logp[0]
        return act, v_r, v_c, logp

    def commit_rng(self) -> None:
        """Fold the host part of the noise stream position into the device part (end of an epoch; a plain
        tensor add, so it is capturable: see OnPolicyAdapter's rollout graph)."""
        self._rng_base += self._rng_offset
        self._rng_offset = 0

    def __call__(self, obs: torch.Tensor, deterministic: bool = False):
        """nn.Module.forward of the reference (actor_critic.py:141-155) = step."""
        return self.step(obs, deterministic=deterministic)

    def set_annealing(self, epochs: list[int], std: list[float]) -> None:
        """actor_critic.py:157-171: piecewise-linear schedule of the exploration std over the epochs
        (omnisafe/utils/schedule.py:37-82: outside the end points the last value applies)."""
        idxes = list(epochs)
        assert idxes == sorted(idxes)
        self._std_endpoints = list(zip(epochs, std))
        self._std_outside = std[-1]

    def annealing(self, epoch: int) -> None:
        """actor_critic.py:173-183."""
        value = self._std_outside
        for (left_t, left), (right_t, right) in zip(self._std_endpoints[:-1], self._std_endpoints[1:]):
            if left_t <= epoch < right_t:
                alpha = float(epoch - left_t) / (right_t - left_t)
                value = left + alpha * (right - left)
                break
        self.actor.std = value

    def values(self, obs: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """Critic values only (bootstrap V(s) at truncation / epoch end)."""
        _, v_r, v_c, _ = self.step(obs, deterministic=True, nets_mask=6)
        return v_r, v_c

    def set_seed(self, seed: int) -> None:
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF

    # ------------------------------------------------------------------ distributed
    def sync_params(self) -> None:
        """distributed.sync_params (omnisafe/utils/distributed.py:201-228): broadcast rank 0's
        parameters -- one message for all three networks."""
        from . import distributed as dist

        dist.broadcast_(self.params, src=0)
