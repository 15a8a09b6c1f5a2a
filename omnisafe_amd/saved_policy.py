"""What the players of a saved policy (``Evaluator``, ``OfflineDataCollector``) both know: the device env classes, the
checkpoint this package's logger writes (``config.json``, ``torch_save/<model_name>`` with keys ``pi`` and, with
``obs_normalize``, ``obs_normalizer``), the ActionScale bounds, the policy's slice of the players' C arguments and the
choice between the persistent and the per-step path."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import _lib
from . import envs as envs_mod
from .config import (BC_DEFAULTS, BCQ_DEFAULTS, DICE_DEFAULTS, OFFPOLICY_DEFAULTS, OFFPOLICY_LAG_DEFAULTS, SAC_DEFAULTS,
                     Config)
from .models import ConstraintActorCritic
from .normalizer import Normalizer
from .spaces import Box

DEVICE_ENVS = tuple(envs_mod.DeviceVectorEnv.__subclasses__())


def device_env_class(env_id: str):
    """The class of a device env id -- a built-in family or one of register_device_env -- or None: what decides whether
    a player knows the env's dimensions without building it, may play it in the persistent kernel, lets its own
    horizon end the episodes and can ask it for its state rows."""
    cls = envs_mod.ENV_REGISTRY.get(env_id)
    return cls if cls in DEVICE_ENVS else envs_mod.CUSTOM_ENV_REGISTRY.get(env_id)


def load_checkpoint(save_dir: str, model_name: str):
    """``(dict_cfgs, cfgs, state)`` of a run directory; a missing file is the FileNotFoundError of its ``open``."""
    with open(os.path.join(save_dir, 'config.json'), encoding='utf-8') as f:
        dict_cfgs = json.load(f)
    cfgs = Config.dict2config(dict_cfgs)
    return dict_cfgs, cfgs, torch.load(os.path.join(save_dir, 'torch_save', model_name), weights_only=False)


class VaePolicy:
    """The actor of a VAE-BC run for the per-step players: ``VAE.predict`` (models/actor/vae_actor.py:121-138) is
    ``decode(obs)`` with a fresh standard-normal latent, so the policy is stochastic by construction and
    ``deterministic`` is ignored.  The latent of call k is drawn on the device from Philox(seed, k, element)
    (osa_vae_decode).  ``general`` keeps it off the persistent players, whose kernels hold a Gaussian actor."""

    general = True

    def __init__(self, cfgs, state, obs_dim: int, act_dim: int, device, seed: int) -> None:
        from .vae_step import VaeDecoder, make_desc

        m = cfgs.model_cfgs
        self._dec = VaeDecoder(make_desc(obs_dim, act_dim, m.hidden_sizes, m.activation, 1), device)
        self._dec.load_state_dict(state['pi'])
        self._seed, self._calls, self._act_dim = int(seed), 0, int(act_dim)

    def _act(self, obs: torch.Tensor) -> torch.Tensor:
        return self._dec.decode(obs, None, seed=self._seed, offset=self._calls)

    def step(self, obs: torch.Tensor, deterministic: bool = False, nets_mask: int = 1, out: dict | None = None):
        act = self._act(obs)
        self._calls += 1
        if out and 'scale' in out:  # ActionScale, as the Gaussian actors' step fuses it
            dst, lo, hi, min_a, max_a = out['scale']
            n, A = act.shape[0], self._act_dim
            _lib.check(_lib.load().osa_action_scale(_lib.ptr(act), act.stride(0), _lib.ptr(dst), dst.stride(0), n, A,
                                                    _lib.ptr(lo), _lib.ptr(hi), min_a, max_a, _lib.stream_ptr()),
                       'osa_action_scale')
        return (act,)


class BcqPolicy(VaePolicy):
    """The actor of a BCQ / BCQ-Lag run for the per-step players: ``PerturbationActor.predict``
    (models/actor/perturbation_actor.py:76-90), the VAE's decode of a fresh latent perturbed by at most ``phi`` --
    osa_bcq_predict, one launch of the fused chain kernel where it takes the shape."""

    def __init__(self, cfgs, state, obs_dim: int, act_dim: int, device, seed: int) -> None:  # pylint: disable=super-init-not-called
        from .bcq_step import BcqActor, make_desc

        m = cfgs.model_cfgs
        self._dec = BcqActor(make_desc(obs_dim, act_dim, m.actor.hidden_sizes, m.critic.hidden_sizes, m.actor.activation,
                                       m.critic.activation), device, phi=float(cfgs.algo_cfgs.phi))
        self._dec.load_state_dict(state['pi'])
        self._seed, self._calls, self._act_dim = int(seed), 0, int(act_dim)

    def _act(self, obs: torch.Tensor) -> torch.Tensor:
        return self._dec.predict(obs, None, seed=self._seed, offset=self._calls)


class MlpPolicy(VaePolicy):
    """The deterministic actor of a DDPG / TD3 run for the per-step players: ``MLPActor.predict(deterministic=True)``,
    the tanh-headed forward (osa_td3_act).  Its ``pi`` state dict holds ``net.*`` keys and no ``log_std``, so the
    persistent players, whose kernels hold a Gaussian actor's block, do not take it: ``general``."""

    def __init__(self, cfgs, state, obs_dim: int, act_dim: int, device, seed: int) -> None:  # pylint: disable=super-init-not-called
        from .td3_step import Td3Actor, make_desc

        m = cfgs.model_cfgs
        self._dec = Td3Actor(make_desc(obs_dim, act_dim, m.actor.hidden_sizes, m.critic.hidden_sizes,
                                       m.actor.activation, m.critic.activation), device)
        self._dec.load_state_dict(state['pi'])
        self._seed, self._calls, self._act_dim = int(seed), 0, int(act_dim)

    def _act(self, obs: torch.Tensor) -> torch.Tensor:
        return self._dec.act(obs.contiguous())


class SacPolicy(VaePolicy):
    """The Gaussian actor of a SAC run for the per-step players: ``GaussianSACActor.predict(deterministic=True)``,
    ``tanh mu`` (osa_sac_act).  Its ``pi`` state dict holds a ``(2 act_dim, hidden)`` top layer and no ``log_std``
    parameter: ``general``, like ``MlpPolicy``."""

    def __init__(self, cfgs, state, obs_dim: int, act_dim: int, device, seed: int) -> None:  # pylint: disable=super-init-not-called
        from .sac_step import SacActor, make_desc

        m = cfgs.model_cfgs
        self._dec = SacActor(make_desc(obs_dim, act_dim, m.actor.hidden_sizes, m.critic.hidden_sizes,
                                       m.actor.activation, m.critic.activation), device)
        self._dec.load_state_dict(state['pi'])
        self._seed, self._calls, self._act_dim = int(seed), 0, int(act_dim)

    def _act(self, obs: torch.Tensor) -> torch.Tensor:
        from .sac_step import ACT_MEAN

        return self._dec.act(obs.contiguous(), mode=ACT_MEAN)


class _ActorOnly:
    """The ``model_cfgs`` of a COptiDICE run as ``ConstraintActorCritic`` reads them: the critics, which no player
    evaluates, take the actor's shape."""

    def __init__(self, model_cfgs) -> None:
        self._m = model_cfgs

    def __getattr__(self, key):
        return self._m.actor if key == 'critic' else getattr(self._m, key)


def build_policy(cfgs, state, obs_dim: int, act_dim: int, device, extra_inputs: int = 0, seed: int = 0):
    """``(actor, normalizer)`` of a checkpoint (evaluator.py:174-177, 250-303); ``extra_inputs``: policy input columns
    behind the observation (the Saute / Simmer safety column); ``normalizer`` is None without ``obs_normalize``.  A
    VAE-BC run gives a ``VaePolicy``, a BCQ / BCQ-Lag run a ``BcqPolicy``, whose latent draws are seeded by ``seed``; a
    DDPG / TD3 run, constrained or not, gives an ``MlpPolicy`` (the cost normaliser is not needed to play)."""
    if str(getattr(cfgs, 'algo', '')) in BC_DEFAULTS:
        return VaePolicy(cfgs, state, obs_dim, act_dim, device, seed), None
    if str(getattr(cfgs, 'algo', '')) in BCQ_DEFAULTS:
        return BcqPolicy(cfgs, state, obs_dim, act_dim, device, seed), None
    if str(getattr(cfgs, 'algo', '')) in (*OFFPOLICY_DEFAULTS, *OFFPOLICY_LAG_DEFAULTS):
        return MlpPolicy(cfgs, state, obs_dim, act_dim, device, seed), None
    if str(getattr(cfgs, 'algo', '')) in SAC_DEFAULTS:
        return SacPolicy(cfgs, state, obs_dim, act_dim, device, seed), None
    model_cfgs = cfgs.model_cfgs
    if str(getattr(cfgs, 'algo', '')) in DICE_DEFAULTS:  # (a Gaussian actor and no critic: the players read the actor)
        model_cfgs = _ActorOnly(model_cfgs)
    actor = ConstraintActorCritic(Box(-np.inf, np.inf, (obs_dim + extra_inputs,)), Box(-1.0, 1.0, (act_dim,)),
                                  model_cfgs, epochs=1, device=device)
    actor.actor.load_state_dict(state['pi'])
    normalizer = None
    if getattr(cfgs.algo_cfgs, 'obs_normalize', False):  # (absent in an offline run: that family has no normaliser)
        normalizer = Normalizer((obs_dim,), clip=5, device=device)
        normalizer.load_state_dict(state['obs_normalizer'])
    return actor, normalizer


def scale_bounds(env, device) -> tuple[torch.Tensor, torch.Tensor]:
    f32 = dict(dtype=torch.float32, device=device)
    lo = torch.as_tensor(env.action_space.low, **f32).reshape(-1).contiguous()
    hi = torch.as_tensor(env.action_space.high, **f32).reshape(-1).contiguous()
    return lo, hi


def policy_args(actor, normalizer, obs_dim: int, act_dim: int, lo, hi) -> tuple:
    """The 12 consecutive arguments ``obs_dim .. max_action`` of osa_eval_episodes and osa_collect_episodes."""
    nm = normalizer
    return (obs_dim, act_dim, actor.hidden, _lib.ptr(actor.params), _lib.ptr(nm._mean) if nm else None,
            _lib.ptr(nm._std) if nm else None, _lib.ptr(nm._count) if nm else None,
            float(nm._clip_value) if nm else 0.0, _lib.ptr(lo), _lib.ptr(hi), -1.0, 1.0)


def choose_path(var: str, ok: bool, why_not: str) -> str:
    """'persistent' or 'per-step': the persistent path where it can take the case (``ok``), unless the environment
    variable ``var`` forces one; forcing the persistent path on a case it cannot take raises OsaError."""
    want = os.environ.get(var, '')
    if want not in ('', 'per-step', 'persistent'):
        raise ValueError(f'{var}={want!r}: per-step or persistent')
    if want == 'persistent' and not ok:
        raise _lib.OsaError(f'{var}=persistent: {why_not}')
    return 'persistent' if (ok if want == '' else want == 'persistent') else 'per-step'
