"""Environment plug-in boundary (mirror of the part of omnisafe/envs/core.py:37-182,300-421 that the
on-policy adapter touches) and the device-resident synthetic vector CMDP.

An environment handed to :class:`omnisafe_amd.adapter.OnPolicyAdapter` must provide, like a reference
``CMDP``: ``num_envs``, ``observation_space``, ``action_space`` (Box), ``reset(seed=None, options=None)
-> (obs, info)``, ``step(action) -> (obs, reward, cost, terminated, truncated, info)`` returning DEVICE
tensors with gymnasium's vector auto-reset convention (``info['final_observation']`` +
``info['_final_observation']`` on steps where some env finished: envs/wrapper.py:232-238),
``set_seed``, ``close``, ``need_auto_reset_wrapper`` / ``need_time_limit_wrapper`` (must be False here).

Safety-Gymnasium (MuJoCo, CPU, third-party: not in the reference repository, not installed) is outside
this package; ``Synth*`` ids give fixed-shape stand-ins with the observation/action dimensions of the
BASELINE configs.
"""
from __future__ import annotations

from typing import Any, Callable

import numpy as np
import torch

from . import _lib
from .spaces import Box

SYNTH_DIMS = {
    'SynthPointGoal1-v0': (60, 2),     # SafetyPointGoal1-v0 (dims verified from the reference's
                                       # tests/saved_source PPO checkpoint: SURVEY.md section 8)
    'SynthCarGoal1-v0': (72, 2),       # SafetyCarGoal1-v0
    'SynthAnt-v0': (27, 8),            # SafetyAntVelocity-v1
    'SynthHumanoid-v0': (376, 17),     # SafetyHumanoidVelocity-v1
    'SynthTiny-v0': (6, 2),
}

ENV_REGISTRY: dict[str, Callable[..., Any]] = {}
# the ids of register_device_env, in a registry of their own: ENV_REGISTRY is the closed list of the built-in ids
CUSTOM_ENV_REGISTRY: dict[str, type] = {}


def env_register(cls):
    """Class decorator keyed by ``cls._support_envs`` (envs/core.py:300-360)."""
    for env_id in cls._support_envs:
        ENV_REGISTRY[env_id] = cls
    return cls


def support_envs() -> list[str]:
    return sorted(ENV_REGISTRY)


def make(env_id: str, num_envs: int = 1, device='cuda:0', **env_cfgs):
    """envs/core.py:389-421.  Ids of this package are device-resident envs; any other id is looked up in the
    caller's ``omnisafe`` env registry (Safety-Gymnasium, user classes under ``@env_register``), built on the
    host and driven through :class:`omnisafe_amd.host_env.HostEnvBridge` (one D2H / H2D pair per vector step)."""
    if env_id in ENV_REGISTRY:
        return ENV_REGISTRY[env_id](env_id, num_envs=num_envs, device=device, **env_cfgs)
    if env_id in CUSTOM_ENV_REGISTRY:
        return CUSTOM_ENV_REGISTRY[env_id](env_id, num_envs=num_envs, device=device, **env_cfgs)
    from .host_env import make_reference_env

    env = make_reference_env(env_id, num_envs=num_envs, device=device, **env_cfgs)
    if env is None:
        raise KeyError(f'{env_id} is registered neither with omnisafe_amd (known: {support_envs()}) nor with an '
                       'importable omnisafe (omnisafe.envs.core.support_envs())')
    return env


class DeviceEnvProtocol:  # pylint: disable=too-many-instance-attributes
    """Host side of a vector CMDP that lives entirely in HBM: one launch of the subclass's entry point per ``reset``
    / ``step`` on buffers allocated once.  Observations are double-buffered (the caller may still hold the previous
    one); all envs reset together, so the truncating steps are known on the host and ``info['final_observation']`` /
    ``info['_final_observation']`` appear on exactly those (a class with ``terminates``: on every step from the
    ``horizon``-th after a reset on, see ``step``).  Philox stream position = ``_t_base`` (device) + ``_t``
    (host, passed by value); ``commit()`` folds the host part into the device part: a captured hipGraph of an epoch
    replays with the same by-value positions 0..T while the device part advances, so every epoch still draws fresh
    numbers.

    Two classes derive from it: :class:`DeviceVectorEnv`, whose direct subclasses are the built-in families of
    libomnisafe_amd.so, and :class:`CustomDeviceEnv`, the envs of ``register_device_env`` with a library each.

    A subclass states class-level facts only: ``entry_point``, ``levels`` (id -> level, empty without levels),
    ``obs_act_dims``, ``state_width`` (floats per row of ``state``; 0: no state matrix), ``default_horizon``, and for
    the evaluator ``eval_kind_base`` (OSA_EVAL_ENV_* of level 0) and ``trace_state_floats`` (leading state floats in a
    trace record)."""

    entry_point: str
    eval_entry_point = 'osa_eval_episodes'
    collect_entry_point = 'osa_collect_episodes'  # (OfflineDataCollector's persistent path; env_kind as eval_kind)
    takes_level = False  # the entry point takes a level even while `levels` is empty (a custom class without ids)
    render_state = True  # whether a rasteriser knows the state row (csrc/render_kernels.hip, or a description's draw())
    levels: dict[str, int] = {}
    obs_act_dims = (60, 2)
    state_width = 0
    default_horizon = 1000
    eval_kind_base = 0
    trace_state_floats = 0
    need_auto_reset_wrapper = False
    need_time_limit_wrapper = False
    need_evaluation = False
    graph_safe = True  # every step is a fixed sequence of launches on device tensors (no host-side data flow)
    terminates = False  # whether an env ends episodes of its own (a custom description with terminal()); see step()
    _cost_p = 0.0

    @classmethod
    def dims(cls, env_id: str) -> tuple[int, int]:
        """(obs_dim, act_dim) of a registered id; needs neither the library nor a GPU."""
        return cls.obs_act_dims

    @classmethod
    def eval_kind(cls, env_id: str) -> int:
        """env_kind of osa_eval_episodes."""
        return cls.eval_kind_base + cls.levels.get(env_id, 0)

    @classmethod
    def render_kind(cls, env_id: str):
        """What ``render.rasterise`` takes in the place of its ``env_kind`` to draw a state row of this id."""
        return cls.eval_kind(env_id)

    @classmethod
    def library(cls):
        """The library that exports ``entry_point``, ``eval_entry_point`` and ``collect_entry_point``, its prototypes
        declared."""
        return _lib.load(require_gpu=True)

    def __init__(self, env_id: str, num_envs: int = 1, device='cuda:0', horizon: int | None = None,
                 seed: int = 0, **_unused) -> None:
        self._lib = self.library()
        self._step_fn = getattr(self._lib, self.entry_point)
        self._env_id = env_id
        self._level = self.levels.get(env_id, 0)
        self._num_envs = int(num_envs)
        self._device = torch.device(device)
        self._obs_dim, self._act_dim = self.dims(env_id)
        self._horizon = int(self.default_horizon if horizon is None else horizon)
        self._observation_space = Box(-np.inf, np.inf, (self._obs_dim,))
        self._action_space = Box(-1.0, 1.0, (self._act_dim,))
        self._seed = int(seed)
        self._t = 0
        self._since_reset = 0
        self._flip = 0
        N, dev = self._num_envs, self._device
        f32 = dict(dtype=torch.float32, device=dev)
        self._t_base = torch.zeros(1, dtype=torch.int64, device=dev)
        if self.state_width:
            self.state = torch.zeros(N, self.state_width, **f32)
        self._steps = torch.zeros(N, dtype=torch.int32, device=dev)
        self._obs = [torch.empty(N, self._obs_dim, **f32) for _ in range(2)]
        self._final = torch.zeros(N, self._obs_dim, **f32)
        self._reward, self._cost = torch.empty(N, **f32), torch.empty(N, **f32)
        self._term = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._trunc = torch.zeros(N, dtype=torch.uint8, device=dev)

    num_envs = property(lambda self: self._num_envs)
    observation_space = property(lambda self: self._observation_space)
    action_space = property(lambda self: self._action_space)
    max_episode_steps = property(lambda self: self._horizon)
    level = property(lambda self: self._level)

    def set_seed(self, seed: int) -> None:
        self._seed = int(seed)

    def _middle_args(self, action) -> tuple:
        """The entry point's arguments between ``horizon`` and ``obs``: [level,] state, steps, action, ld_action."""
        ld_a = 0
        if action is not None:
            assert action.dtype == torch.float32 and action.shape == (self._num_envs, self._act_dim) \
                and action.stride(1) == 1
            ld_a = action.stride(0)
        mid = (_lib.ptr(self.state), _lib.ptr(self._steps), _lib.ptr(action), ld_a)
        return (self._level, *mid) if (self.levels or self.takes_level) else mid

    def _launch(self, middle: tuple, reset_only: int) -> torch.Tensor:
        self._flip ^= 1
        obs = self._obs[self._flip]
        _lib.check(self._step_fn(
            self._seed & 0xFFFFFFFFFFFFFFFF, self._t, _lib.ptr(self._t_base), self._num_envs, self._obs_dim,
            self._horizon, *middle, _lib.ptr(obs), self._obs_dim, _lib.ptr(self._reward), _lib.ptr(self._cost),
            _lib.ptr(self._term), _lib.ptr(self._trunc), _lib.ptr(self._final), self._obs_dim, reset_only,
            *self._param_args(), _lib.stream_ptr()), self.entry_point)
        self._t += 1
        return obs

    def _param_args(self) -> tuple:
        """What the entry point takes between ``reset_only`` and the stream: nothing, but for a custom class with
        runtime parameters (range, par, ld_par)."""
        return ()

    def player_param_args(self, rows: int) -> tuple[tuple, torch.Tensor | None]:
        """What ``eval_entry_point`` / ``collect_entry_point`` take in front of the stream, and the (rows, P) tensor the
        player leaves parameter rows in: ``((), None)`` but for a custom class with runtime parameters."""
        return (), None

    def _render_kind(self, lane: int):
        return self.render_kind(self._env_id)

    def reset(self, seed: int | None = None, options: dict | None = None):
        if seed is not None:
            self.set_seed(seed)
        obs = self._launch(self._middle_args(None), 1)
        self._since_reset = 0
        return obs, {}

    def step(self, action: torch.Tensor):
        obs = self._launch(self._middle_args(action), 0)
        self._since_reset += 1
        info: dict[str, Any] = {}
        if self.terminates:
            # Episodes end per env, so which steps truncate is known to the device alone.  No env can truncate earlier
            # than `horizon` steps after the common reset: from there on every step hands out the final observations
            # under the device's `truncated` mask (often all zeros), and none before -- still a function of
            # host-known numbers only, so the captured rollout graph keeps replaying.
            have_final = self._since_reset >= self._horizon
        else:
            have_final = self._since_reset % self._horizon == 0  # every env truncates on this step
        if have_final:
            info['final_observation'] = self._final
            info['_final_observation'] = self._trunc
        return obs, self._reward, self._cost, self._term, self._trunc, info

    def commit(self) -> None:
        """Fold the host part of the stream position into the device part (end of an epoch; capturable)."""
        self._t_base += self._t
        self._t = 0

    def render(self, lane: int = 0, width: int = 256, height: int = 256, camera_name: str = 'fixed') -> np.ndarray:
        """The current state of env ``lane`` as an (height, width, 3) uint8 picture: osa_render_episode with one frame
        and no trail (2 x 2 sub-samples; the picture is specified in include/omnisafe_amd.h)."""
        if not self.state_width:
            raise NotImplementedError(f'{type(self).__name__} has no state to draw')
        from . import render as render_mod

        if not 0 <= lane < self._num_envs:
            raise IndexError(f'lane {lane} of {self._num_envs} envs')
        frame = render_mod.rasterise(self._render_kind(lane), self.state, lane * self.state_width,
                                     self.state_width, 0, 1, 0, None, render_mod.camera_index(camera_name),
                                     width, height, 2)
        return frame[0].cpu().numpy()

    def close(self) -> None:
        return None


class DeviceVectorEnv(DeviceEnvProtocol):
    """The built-in families: every DIRECT subclass is one family of libomnisafe_amd.so (csrc/env_device.h), which the
    evaluator and the plugin enumerate through ``__subclasses__()``.  An env of the user's own is no subclass of this
    class: ``register_device_env`` derives it from :class:`CustomDeviceEnv`."""


@env_register
class SynthVectorEnv(DeviceVectorEnv):
    """Zero-cost synthetic vector CMDP living entirely in HBM (osa_synth_env_step)."""

    _support_envs = list(SYNTH_DIMS)
    entry_point = 'osa_synth_env_step'

    def __init__(self, env_id: str, num_envs: int = 1, device='cuda:0', horizon: int = 1000,
                 cost_p: float = 0.05, seed: int = 0, **_unused) -> None:
        super().__init__(env_id, num_envs, device, horizon, seed)
        self._cost_p = float(cost_p)

    @classmethod
    def dims(cls, env_id: str) -> tuple[int, int]:
        return SYNTH_DIMS[env_id]

    def _middle_args(self, action) -> tuple:  # noise: the action is not read
        return self._cost_p, _lib.ptr(self._steps)


@env_register
class ReachVectorEnv(DeviceVectorEnv):
    """Learnable synthetic vector CMDP in HBM (osa_reach_env_step): a point reaches resampled goals
    (reward = progress, +1 per goal) past a hazard disc (cost 1 inside).  Observation/action dims of
    SafetyPointGoal1 (60 / 2).  Used for learning-curve comparisons against the reference, which trains
    on the CPU twin of this env kept with the test harness under oracle/."""

    _support_envs = ['SynthReach-v0']
    entry_point = 'osa_reach_env_step'
    state_width = 8  # p, goal, hazard, pad
    default_horizon = 50
    eval_kind_base = 1
    trace_state_floats = 6


NAV_LEVELS = {'SynthNavGoal0-v0': 0, 'SynthNavGoal1-v0': 1, 'SynthNavGoal2-v0': 2}


@env_register
class NavGoalVectorEnv(DeviceVectorEnv):
    """Lidar navigation vector CMDP in HBM (osa_nav_env_step), with the structure of the Safety-Gymnasium Goal
    tasks: a point robot with heading and inertia drives to resampled goals (reward = progress, +1 per goal)
    between hazard discs (cost 1 inside) and vases (cost on level 2), which it sees only through three egocentric
    16-bin lidars.  Levels 0 / 1 / 2: 0 / 8 / 10 hazards, 0 / 1 / 10 vases.  Observation/action dims of
    SafetyPointGoal (60 / 2).  ``state`` is the (N, 64) state matrix laid out as include/omnisafe_amd.h states."""

    _support_envs = list(NAV_LEVELS)
    entry_point = 'osa_nav_env_step'
    levels = NAV_LEVELS
    state_width = trace_state_floats = 64
    eval_kind_base = 16


CIRCLE_LEVELS = {'SynthNavCircle0-v0': 0, 'SynthNavCircle1-v0': 1, 'SynthNavCircle2-v0': 2}


@env_register
class NavCircleVectorEnv(DeviceVectorEnv):
    """Circle-running vector CMDP in HBM (osa_circle_env_step), with the structure of the Safety-Gymnasium Circle
    tasks: the point robot of SynthNavGoal is paid for running round the origin on the circle of radius 1
    (reward = tangential progress, damped away from the circle) and charged for leaving a corridor narrower than the
    circle, so the unconstrained optimum is infeasible.  Levels 0 / 1 / 2: no cost / walls at |x| = 0.75 / walls at
    |x| = 0.75 and |y| = 0.75; the walls are not observed.  Observation/action dims 28 / 2: the sensor columns of
    SynthNavGoal and a 16-bin lidar of the circle's centre.  ``state`` is the (N, 8) state matrix laid out as
    include/omnisafe_amd.h states."""

    _support_envs = list(CIRCLE_LEVELS)
    entry_point = 'osa_circle_env_step'
    levels = CIRCLE_LEVELS
    obs_act_dims = (28, 2)
    state_width = trace_state_floats = 8
    default_horizon = 500
    eval_kind_base = 32


CAR_GOAL_LEVELS = {'SynthNavCarGoal0-v0': 0, 'SynthNavCarGoal1-v0': 1, 'SynthNavCarGoal2-v0': 2}


@env_register
class NavCarGoalVectorEnv(DeviceVectorEnv):
    """SynthNavGoal driven by the Car (osa_car_goal_env_step), with the structure of the Safety-Gymnasium CarGoal
    tasks: the two actions command the left and the right wheel, whose speeds lag the commands; the forward speed is
    the wheels' mean and the turn rate their difference.  Goal, hazards, vases, reward, costs and levels are
    SynthNavGoal's, and so is the reset: the same seed gives the same arena as ``SynthNavGoal<level>-v0``.
    Observation/action dims of SafetyCarGoal (72 / 2): 24 sensor columns (f, f - f_prev, t, heading, wheel speeds,
    t - t_prev, zeros) and the three 16-bin lidars.  ``state`` is the (N, 64) state matrix laid out as
    include/omnisafe_amd.h states."""

    _support_envs = list(CAR_GOAL_LEVELS)
    entry_point = 'osa_car_goal_env_step'
    levels = CAR_GOAL_LEVELS
    obs_act_dims = (72, 2)
    state_width = trace_state_floats = 64
    eval_kind_base = 48


CAR_CIRCLE_LEVELS = {'SynthNavCarCircle0-v0': 0, 'SynthNavCarCircle1-v0': 1, 'SynthNavCarCircle2-v0': 2}


@env_register
class NavCarCircleVectorEnv(DeviceVectorEnv):
    """SynthNavCircle driven by the Car (osa_car_circle_env_step), with the structure of the Safety-Gymnasium
    CarCircle tasks: the two actions command the left and the right wheel (see :class:`NavCarGoalVectorEnv`); reward,
    corridor cost, levels and reset are SynthNavCircle's (the same seed gives the same start).  Observation/action
    dims 40 / 2: the Car's 24 sensor columns and a 16-bin lidar of the circle's centre.  ``state`` is the (N, 12)
    state matrix laid out as include/omnisafe_amd.h states."""

    _support_envs = list(CAR_CIRCLE_LEVELS)
    entry_point = 'osa_car_circle_env_step'
    levels = CAR_CIRCLE_LEVELS
    obs_act_dims = (40, 2)
    state_width = trace_state_floats = 12
    default_horizon = 500
    eval_kind_base = 64


# ----------------------------------------------------------------------------------------------------------------
# Device envs of the user's own: a description struct in a header of theirs (include/omnisafe_amd_env.h), compiled with
# the generic per-step kernel and the evaluation kernel into a library of its own (build.build_custom_env).
# ----------------------------------------------------------------------------------------------------------------
class CustomDeviceEnv(DeviceEnvProtocol):
    """A device env whose kernels live in a library of its own.  ``register_device_env`` makes one subclass per
    description; its dimensions are what the compiled library reports (osa_custom_env_info), and so is ``terminates``:
    whether the description has a ``terminal()`` member and ends episodes per env.  ``eval_kind`` is the level: the
    first argument of the library's osa_custom_eval_episodes.  ``draws`` (and with it ``render_state``) is what
    osa_custom_render_info reports: whether the description has a ``draw()`` member, which the library's generic scene
    rasteriser (csrc/scene_render.h) turns into ``render()`` and ``Evaluator.render`` for the class.  ``lds_row``
    (osa_custom_row_info) is the row kind: True for a description with ``LDS_ROW = true``, whose state row (up to 256
    floats) holds objects that the kernels keep in LDS and whose per-step kernel is the generic row kernel
    (csrc/env_frame.h: osa_custom_row_env_kernel); nothing else about the class differs.

    A description with ``PARAMS`` has runtime parameters: ``param_names`` / ``param_defaults`` are the library's
    (empty tuples otherwise), ``make(env_id, ..., wind=0.3, band=(0.4, 0.8))`` -- or the same keys in ``env_cfgs`` --
    fixes a parameter (a number) or gives the range each env draws it from at every reset (a pair); see
    :func:`param_ranges`.  On the env, ``params`` is the (N, P) device tensor of the envs' current rows, ``param_ranges``
    the (2, P) device tensor of the ranges, which the kernels read through its pointer, and ``set_param`` rewrites a
    range in place."""

    entry_point = 'osa_custom_env_step'
    eval_entry_point = 'osa_custom_eval_episodes'
    collect_entry_point = 'osa_custom_collect_episodes'
    takes_level = True
    graph_safe = True
    render_state = False  # (a state row the rasteriser has never heard of, unless the description draws it)
    draws = False
    lds_row = False
    draw_max = 0  # OSA_DRAW_MAX of the library: the primitives a scene holds
    draw_view = (0.0, 0.0)  # DRAW_VIEW, DRAW_TRACK
    header: str
    struct: str
    lib_path: str
    lanes = 32
    max_level = 0
    param_names: tuple = ()
    param_defaults: tuple = ()
    _support_envs: list[str] = []
    _cdll = None

    def __init__(self, env_id: str, num_envs: int = 1, device='cuda:0', horizon: int | None = None,
                 seed: int = 0, **env_cfgs) -> None:
        ranges = param_ranges(type(self), env_cfgs)  # (refuses before anything is allocated)
        super().__init__(env_id, num_envs, device, horizon, seed)
        if self.param_names:
            self.param_ranges = torch.from_numpy(ranges).to(self._device)
            self.params = torch.zeros(self._num_envs, len(self.param_names), dtype=torch.float32, device=self._device)

    def _param_args(self) -> tuple:
        if not self.param_names:
            return ()
        return _lib.ptr(self.param_ranges), _lib.ptr(self.params), self.params.stride(0)

    def player_param_args(self, rows: int):
        if not self.param_names:
            return (), None
        par = torch.zeros(int(rows), len(self.param_names), dtype=torch.float32, device=self._device)
        return (_lib.ptr(self.param_ranges), _lib.ptr(par), par.stride(0)), par

    def set_param(self, name: str, value) -> None:
        """Fix parameter ``name`` (a number) or give it a range (a pair): written into ``param_ranges`` in place, on
        the current stream, so every env takes it at its next reset -- also the envs of a rollout graph that keeps
        replaying, whose launches read the ranges through the tensor's pointer."""
        if name not in self.param_names:
            raise TypeError(f'{self._env_id} has no parameter {name!r} (its parameters: {list(self.param_names)})')
        k = self.param_names.index(name)
        pair = param_ranges(type(self), {name: value})[:, k]
        self.param_ranges[:, k].copy_(torch.from_numpy(pair.copy()))

    def _render_kind(self, lane: int):
        kind = self.render_kind(self._env_id)
        return kind._replace(par=self.params[lane]) if self.param_names else kind

    @classmethod
    def library(cls):
        _lib.load(require_gpu=True)  # (no GPU: the same loud failure as the built-in envs; error texts come from there)
        return cls._cdll

    @classmethod
    def render_kind(cls, env_id: str):
        from . import render as render_mod

        return render_mod.CustomScene(cls, cls.levels.get(env_id, 0))

    def render(self, *args, **kwargs):
        if self.draws:
            return super().render(*args, **kwargs)
        # (the ValueError of Evaluator.render for an env without a drawable state row)
        raise ValueError(f'{self._env_id} has no state row to draw: render() takes the geometric device envs '
                         '(SynthReach-v0, SynthNav*-v0)')


def param_ranges(cls, env_cfgs: dict) -> np.ndarray:
    """The (2, P) float32 ranges ``[lo; hi]`` of a custom class's runtime parameters from the keys of ``env_cfgs``: a
    number fixes the parameter (``lo == hi``), a pair is the range each env draws it from at every reset, an absent
    key takes the description's default.  TypeError: a key that is neither a parameter nor ``horizon`` / ``seed``;
    ValueError: ``lo > hi`` or a value that is not finite.  A class without parameters ignores every key, as it always
    did, and gives a (2, 0) array.  Needs no GPU."""
    names = tuple(getattr(cls, 'param_names', ()))
    out = np.zeros((2, len(names)), np.float32)
    if not names:
        return out
    unknown = sorted(k for k in env_cfgs if k not in names and k not in ('horizon', 'seed'))
    if unknown:
        raise TypeError(f'{cls.__name__} takes no env_cfgs {unknown}: its parameters are {list(names)} (besides '
                        'horizon and seed)')
    out[:] = np.asarray(cls.param_defaults, np.float32)
    for k, name in enumerate(names):
        if name not in env_cfgs:
            continue
        value = env_cfgs[name]
        pair = tuple(value) if isinstance(value, (tuple, list, np.ndarray)) else (value, value)
        if len(pair) != 2:
            raise ValueError(f'{name}={value!r}: a number, or a pair (lo, hi)')
        lo, hi = (np.float32(v) for v in pair)
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f'{name}={value!r} is not finite')
        if lo > hi:
            raise ValueError(f'{name}={value!r}: lo > hi')
        out[:, k] = lo, hi
    return out


def _bind_custom(path: str):
    """dlopen a custom library and declare its prototypes (include/omnisafe_amd_env.h); returns
    (CDLL, info[8], (draws, OSA_DRAW_MAX, DRAW_VIEW, DRAW_TRACK))."""
    import ctypes as C

    lib = C.CDLL(path)
    lib.osa_custom_render_info.restype = C.c_int
    lib.osa_custom_render_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.osa_custom_render_episode.restype, lib.osa_custom_render_episode.argtypes = \
        _lib.SIGNATURES['osa_render_episode']
    lib.osa_custom_env_info.restype, lib.osa_custom_env_info.argtypes = C.c_int, [C.POINTER(C.c_int)]
    lib.osa_custom_env_step.restype, lib.osa_custom_env_step.argtypes = _lib.SIGNATURES['osa_nav_env_step']
    lib.osa_custom_eval_episodes.restype, lib.osa_custom_eval_episodes.argtypes = _lib.SIGNATURES['osa_eval_episodes']
    lib.osa_custom_collect_episodes.restype, lib.osa_custom_collect_episodes.argtypes = \
        _lib.SIGNATURES['osa_collect_episodes']
    # the parameter-taking forms: range, par, ld_par (render: the episode's row) in front of the stream
    for plain, extra in (('osa_custom_env_step', 3), ('osa_custom_eval_episodes', 3),
                         ('osa_custom_collect_episodes', 3), ('osa_custom_render_episode', 1)):
        fn, old = getattr(lib, plain + '_params'), getattr(lib, plain)
        fn.restype = old.restype
        fn.argtypes = list(old.argtypes[:-1]) + [C.c_void_p, C.c_void_p, C.c_int][:extra] + [old.argtypes[-1]]
    lib.osa_custom_param_info.restype = C.c_int
    lib.osa_custom_param_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_char_p, C.c_int]
    info = (C.c_int * 8)()
    _lib_code = lib.osa_custom_env_info(info)
    if _lib_code != 0:
        raise _lib.OsaError(f'osa_custom_env_info of {path} failed ({_lib_code})')
    draw_i, draw_f = (C.c_int * 4)(), (C.c_float * 2)()
    _lib_code = lib.osa_custom_render_info(draw_i, draw_f)
    if _lib_code != 0:
        raise _lib.OsaError(f'osa_custom_render_info of {path} failed ({_lib_code})')
    lib.osa_custom_row_info.restype, lib.osa_custom_row_info.argtypes = C.c_int, [C.POINTER(C.c_int)]
    return lib, list(info), (bool(draw_i[0]), draw_i[1], draw_f[0], draw_f[1])


def _custom_row(lib, path: str) -> bool:
    """The row kind of a bound custom library (osa_custom_row_info): True for an object row in LDS."""
    import ctypes as C

    row_i = (C.c_int * 4)()
    _lib_code = lib.osa_custom_row_info(row_i)
    if _lib_code != 0:
        raise _lib.OsaError(f'osa_custom_row_info of {path} failed ({_lib_code})')
    return bool(row_i[0])


def _custom_params(lib, path: str) -> tuple[tuple, tuple]:
    """(names, defaults) of the runtime parameters of a bound custom library: empty tuples without PARAMS."""
    import ctypes as C

    count, defaults, names = C.c_int(), (C.c_float * 16)(), C.create_string_buffer(1024)
    _lib_code = lib.osa_custom_param_info(C.byref(count), defaults, names, len(names))
    if _lib_code != 0:
        raise _lib.OsaError(f'osa_custom_param_info of {path} failed ({_lib_code})')
    return tuple(names.value.decode().split()), tuple(float(v) for v in defaults[:count.value])


def register_device_env(header: str, struct: str, ids, default_horizon: int = 1000) -> type:
    """Make the env description ``struct`` of the C++ header ``header`` available as device envs.  ``ids``: an
    ``{env_id: level}`` dict, or a list of ids that are all level 0.  Builds (or finds cached) the description's
    library, reads every dimension from it and returns the env class; ``make``, ``Agent``, ``AgentGroup`` and
    ``Evaluator`` then take the ids like built-in ones.  KeyError: an id is taken already; ValueError: a level the
    description does not have."""
    from . import build as _build

    levels = dict(ids) if isinstance(ids, dict) else {env_id: 0 for env_id in ids}
    if not levels:
        raise ValueError('register_device_env needs at least one env id')
    for env_id in levels:
        if env_id in ENV_REGISTRY or env_id in CUSTOM_ENV_REGISTRY:
            raise KeyError(f'{env_id} is registered already')
    path = _build.build_custom_env(header, struct)
    cdll, (state, obs, _dyn, act, trace, max_level, lanes, terminates), (draws, draw_max, view, track) = \
        _bind_custom(path)
    lds_row = _custom_row(cdll, path)
    param_names, param_defaults = _custom_params(cdll, path)
    for env_id, level in levels.items():
        if not isinstance(level, int) or not 0 <= level <= max_level:
            raise ValueError(f'{env_id}: level {level!r}, but {struct} has levels 0 .. {max_level}')
    # one class per struct name (the plugin's key is 'OmnisafeAmdCustom' + struct): further ids of the same library and
    # default horizon join the class that is there, anything else under that name is refused
    cls = next((c for c in custom_env_classes() if c.struct == struct), None)
    if cls is not None:
        if cls.lib_path != path or cls.default_horizon != int(default_horizon):
            raise ValueError(f'a struct {struct} is registered already ({cls.header}, default_horizon '
                             f'{cls.default_horizon}, ids {cls._support_envs}): unregister its ids first, or name '  # noqa: SLF001
                             'the other description differently')
        cls.levels.update(levels)
        cls._support_envs.extend(levels)  # noqa: SLF001
    else:
        cls = type(struct + 'VectorEnv', (CustomDeviceEnv,), {
            '__doc__': f'Device env {struct} of {header} (register_device_env).', '__module__': __name__,
            '_support_envs': list(levels), 'levels': levels, 'obs_act_dims': (obs, act), 'state_width': state,
            'trace_state_floats': trace, 'default_horizon': int(default_horizon), 'max_level': max_level,
            'lanes': lanes, 'terminates': bool(terminates), 'draws': draws, 'render_state': draws, 'draw_max': draw_max,
            'draw_view': (view, track), 'header': header, 'struct': struct, 'lib_path': path, '_cdll': cdll,
            'param_names': param_names, 'param_defaults': param_defaults, 'lds_row': lds_row})
        if param_names:  # (the plain forms of such a library refuse: they would run with unbound parameters)
            for attr in ('entry_point', 'eval_entry_point', 'collect_entry_point'):
                setattr(cls, attr, getattr(CustomDeviceEnv, attr) + '_params')
    for env_id in levels:
        CUSTOM_ENV_REGISTRY[env_id] = cls
    return cls


def unregister_device_env(*ids: str) -> None:
    """Drop ids that ``register_device_env`` entered (KeyError for any other); envs that exist keep working."""
    for env_id in ids:
        if env_id not in CUSTOM_ENV_REGISTRY:
            raise KeyError(f'{env_id} is no registered custom env (known: {custom_envs()})')
    for env_id in ids:
        cls = CUSTOM_ENV_REGISTRY.pop(env_id)
        cls._support_envs.remove(env_id)  # noqa: SLF001
        del cls.levels[env_id]


def custom_envs() -> list[str]:
    return sorted(CUSTOM_ENV_REGISTRY)


def custom_env_classes() -> list[type]:
    """The classes with at least one registered id, in the order of their first registration."""
    return list(dict.fromkeys(CUSTOM_ENV_REGISTRY.values()))
