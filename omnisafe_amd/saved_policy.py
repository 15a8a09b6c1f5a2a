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
from .config import Config
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


def build_policy(cfgs, state, obs_dim: int, act_dim: int, device, extra_inputs: int = 0):
    """``(actor, normalizer)`` of a checkpoint (evaluator.py:174-177, 250-303); ``extra_inputs``: policy input columns
    behind the observation (the Saute / Simmer safety column); ``normalizer`` is None without ``obs_normalize``."""
    actor = ConstraintActorCritic(Box(-np.inf, np.inf, (obs_dim + extra_inputs,)), Box(-1.0, 1.0, (act_dim,)),
                                  cfgs.model_cfgs, epochs=1, device=device)
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
