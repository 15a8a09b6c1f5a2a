"""``Evaluator`` -- deterministic evaluation and rendering of a saved checkpoint (mirror of
omnisafe/evaluator.py:355-629).

``load_saved(save_dir, model_name)`` reads what this package's logger writes (``config.json``,
``torch_save/<model_name>`` with keys ``pi`` and, with ``obs_normalize``, ``obs_normalizer``); ``evaluate()`` plays
``num_episodes`` episodes and returns ``(episode_rewards, episode_costs)`` as the reference does; ``render()`` plays them
the same way and writes one animated PNG per episode, rasterised on the device from the state rows of the trace
(osa_render_episode, csrc/render_kernels.hip; the picture is specified in include/omnisafe_amd.h -- or, for a class of
register_device_env whose description has a draw(), osa_custom_render_episode of its library with the picture that
draw() states, include/omnisafe_amd_env.h).

Two paths, one semantics:
  persistent  a fused-family actor on a device env (SynthReach-v0, SynthNavGoal*-v0, SynthNavCircle*-v0,
              SynthNavCarGoal*-v0, SynthNavCarCircle*-v0, Synth*-v0, and the ids of register_device_env):
              every episode in ONE launch of osa_eval_episodes (csrc/eval_kernels.hip; a custom env: its own library's
              osa_custom_eval_episodes, the same kernel template), episode k = env index k of a fresh env.
  per-step    everything else (general networks, host envs, an env object given as ``env=``): the existing launches
              per vector step -- Normalizer.apply, ConstraintActorCritic.step(deterministic=True, nets_mask=1) with
              ActionScale fused, env.step -- and the same float64 sums in the same order.
``OSA_EVAL_PATH=per-step|persistent`` forces a path (the persistent one raises when it cannot take the case).

Deviations from the reference, decided for parallel episodes:
  * Episodes run side by side in the lanes of a vector env, not one after another.
  * The observation statistics stay FROZEN at the checkpoint's values.  The reference's Evaluator wraps the env in
    ObsNormalize, whose ``normalize`` always pushes (omnisafe/common/normalizer.py:103), so its episode k sees
    statistics moved by episodes 0 .. k-1; no parallel schedule can reproduce that drift.
  * Device envs end episodes through their own ``horizon`` (env_cfgs); other envs get the reference's TimeLimit of
    1000 steps (evaluator.py:179-180).
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from . import _lib, apng
from . import envs as envs_mod
from . import render as render_mod
from .config import Config
from .models import ConstraintActorCritic
from .normalizer import Normalizer
from .saved_policy import (DEVICE_ENVS, build_policy, choose_path, device_env_class, load_checkpoint, policy_args,
                           scale_bounds)

TIME_LIMIT = 1000  # evaluator.py:179-180


def _is_device_env(env) -> bool:
    return isinstance(env, DEVICE_ENVS + (envs_mod.CustomDeviceEnv,))


def _env_kind(env) -> int:
    """env_kind of osa_eval_episodes (OSA_EVAL_ENV_* of the family + level; the level alone for a custom env, whose
    library has one description); an env of the caller's own counts as OSA_EVAL_ENV_SYNTH, whose trace record has no
    state floats."""
    return env.eval_kind(env._env_id) if _is_device_env(env) else 0


class Evaluator:  # pylint: disable=too-many-instance-attributes
    def __init__(self, seed: int = 0, device='cuda:0', verbose: bool = True, env=None) -> None:
        self._seed = int(seed)
        self._device = torch.device(device)
        self._verbose = verbose
        self._user_env = env
        self._cfgs: Config | None = None
        self._actor: ConstraintActorCritic | None = None
        self._normalizer: Normalizer | None = None
        self.episode_lengths: list[float] = []
        self.episode_params = np.zeros((0, 0), np.float32)  # (K, P) of the last evaluate(): each episode's parameters
        self.path: str | None = None  # path of the last evaluate(): 'persistent' or 'per-step'
        self.render_clock: dict[str, float] = {}  # seconds of the last render(): play, raster, copy, encode

    # ------------------------------------------------------------------ loading
    def load_saved(self, save_dir: str, model_name: str, render_mode: str = 'rgb_array',
                   camera_name: str | None = None, width: int = 256, height: int = 256) -> None:
        """evaluator.py:355-398.  The render options are the defaults of later ``render()`` calls; the device envs
        render to arrays only."""
        if render_mode != 'rgb_array':
            raise NotImplementedError(f'render_mode={render_mode!r}: the device envs render to rgb_array only')
        if camera_name is not None:
            render_mod.camera_index(camera_name)
        self._render_defaults = {'camera_name': camera_name or 'fixed', 'width': int(width), 'height': int(height)}
        self._save_dir, self._model_name = save_dir, model_name
        self.load_policy(*load_checkpoint(save_dir, model_name)[::2])

    def load_policy(self, dict_cfgs: dict, ck: dict) -> None:
        """A policy that is not on disk (yet): a run's settings as config.json holds them and its checkpoint dict (the
        offline algorithms' evaluation at each epoch)."""
        if not hasattr(self, '_render_defaults'):
            self._render_defaults = {'camera_name': 'fixed', 'width': 256, 'height': 256}
        self._dict_cfgs, self._cfgs = dict_cfgs, Config.dict2config(dict_cfgs)
        self._env_id = self._cfgs.env_id
        self._env_cfgs = dict(self._dict_cfgs.get('env_cfgs') or {})
        algo = str(self._cfgs.algo)
        a = self._cfgs.algo_cfgs
        self._saute = 'Saute' in algo or 'Simmer' in algo
        if self._saute:  # evaluator.py:165-172 (the float64 expression, then float32 through torch.ones(1))
            self._budget = float(np.float32(a.safety_budget * (1 - a.saute_gamma ** a.max_ep_len)
                                             / (1 - a.saute_gamma) / a.max_ep_len))
            self._saute_gamma = float(a.saute_gamma)
        self._early_terminated = 'EarlyTerminated' in algo
        self._cost_limit = float(a.cost_limit) if self._early_terminated else 0.0
        obs_dim, act_dim = self._env_dims()
        self._actor, self._normalizer = build_policy(self._cfgs, ck, obs_dim, act_dim, self._device,
                                                     extra_inputs=int(self._saute))

    def _env_dims(self) -> tuple[int, int]:
        if self._user_env is not None:
            return (int(self._user_env.observation_space.shape[0]), int(self._user_env.action_space.shape[0]))
        cls = device_env_class(self._env_id)
        if cls is not None:
            return cls.dims(self._env_id)
        env = envs_mod.make(self._env_id, num_envs=1, device=self._device, **self._env_cfgs)
        dims = int(env.observation_space.shape[0]), int(env.action_space.shape[0])
        env.close()
        return dims

    # ------------------------------------------------------------------ evaluation
    def _persistent_ok(self) -> bool:
        return (self._user_env is None and not self._actor.general
                and device_env_class(self._env_id) is not None)

    def evaluate(self, num_episodes: int = 10, cost_criteria: float = 1.0, trace: bool = False,
                 env_params: dict | None = None):
        """evaluator.py:399-490: ``(episode_rewards, episode_costs)``; ``episode_lengths`` is kept as an attribute.
        ``trace=True`` also keeps the per-step record of osa_eval_episodes as ``self.trace`` (tests).
        ``env_params`` overlays the run's ``env_cfgs`` for this call: the runtime parameters of a custom device env
        (``{'wind': 0.4}``, or a pair for a range) at values the policy was not trained on.  ``episode_params`` is then
        the (K, P) array of the parameters every episode was played under (P = 0 for an env without any)."""
        if self._actor is None:
            raise ValueError('The policy must be loaded (load_saved) before evaluating the agent.')
        num_episodes = int(num_episodes)
        assert num_episodes >= 1
        self.path = choose_path('OSA_EVAL_PATH', self._persistent_ok(),
                                'the persistent kernel takes a fused-family actor on a '
                                f'device env (here {self._env_id}, general network: {self._actor.general})')
        run = self._run_persistent if self.path == 'persistent' else self._run_per_step
        self._env_overlay = dict(env_params or {})
        self._episode_par = None  # the device rows behind episode_params
        ret, cost, length = run(num_episodes, float(cost_criteria), trace)
        par = self._episode_par
        self.episode_params = (np.zeros((num_episodes, 0), np.float32) if par is None
                               else par[:num_episodes].cpu().numpy())
        rewards, costs = ret.cpu().tolist(), cost.cpu().tolist()
        self.episode_lengths = [float(x) for x in length.cpu().tolist()]
        if self._verbose:
            for i, (r, c, n) in enumerate(zip(rewards, costs, self.episode_lengths)):
                print(f'Episode {i} results:')
                print(f'Episode reward: {r}')
                print(f'Episode cost: {c}')
                print(f'Episode length: {n}')
            print('-' * 60)
            print('Evaluation results:')
            print(f'Average episode reward: {np.mean(a=rewards)}')
            print(f'Average episode cost: {np.mean(a=costs)}')
            print(f'Average episode length: {np.mean(a=self.episode_lengths)}')
        return rewards, costs

    def _make_env(self, K: int):
        cfgs = dict(self._env_cfgs, **getattr(self, '_env_overlay', {}))
        env = envs_mod.make(self._env_id, num_envs=K, device=self._device, **cfgs)
        env.set_seed(self._seed)
        return env

    def _trace_floats(self, env, obs_dim: int, act_dim: int) -> int:
        if isinstance(env, envs_mod.CustomDeviceEnv):  # (include/omnisafe_amd_env.h: osa_custom_eval_episodes)
            return obs_dim + int(self._saute) + act_dim + 3 + env.trace_state_floats
        return int(_lib.load().osa_eval_trace_floats(_env_kind(env), obs_dim, act_dim, int(self._saute)))

    def _run_persistent(self, K: int, cost_criteria: float, trace: bool):
        env = self._make_env(K)
        kind = _env_kind(env)
        entry = env.eval_entry_point
        play = getattr(env.library(), entry)
        obs_dim, act_dim = int(env.observation_space.shape[0]), int(env.action_space.shape[0])
        lo, hi = scale_bounds(env, self._device)
        horizon = int(env.max_episode_steps)
        dev = self._device
        ret = torch.zeros(K, dtype=torch.float64, device=dev)
        cost = torch.zeros(K, dtype=torch.float64, device=dev)
        length = torch.zeros(K, dtype=torch.int32, device=dev)
        tr = None
        if trace:
            tr = torch.zeros(horizon, K, self._trace_floats(env, obs_dim, act_dim), dtype=torch.float32, device=dev)
        par_args, self._episode_par = env.player_param_args(K)
        _lib.check(play(
            kind, K, *policy_args(self._actor, self._normalizer, obs_dim, act_dim, lo, hi),
            env._seed & 0xFFFFFFFFFFFFFFFF, horizon, env._cost_p, horizon,
            int(self._saute), self._budget if self._saute else 0.0, self._saute_gamma if self._saute else 0.0,
            int(self._early_terminated), self._cost_limit, cost_criteria, _lib.ptr(ret), _lib.ptr(cost),
            _lib.ptr(length), _lib.ptr(tr), *par_args, _lib.stream_ptr()), entry)
        self.trace = tr
        env.close()
        return ret, cost, length

    def _run_per_step(self, num_episodes: int, cost_criteria: float, trace: bool):
        rets, costs, lens = [], [], []
        done_eps = 0
        self.trace = None
        while done_eps < num_episodes:  # a user env plays batches of its num_envs lanes
            env = self._user_env if self._user_env is not None else self._make_env(num_episodes)
            r, c, n = self._per_step_batch(env, cost_criteria, trace)
            rets.append(r)
            costs.append(c)
            lens.append(n)
            done_eps += r.numel()
            if self._user_env is None:
                env.close()
        return (torch.cat(rets)[:num_episodes], torch.cat(costs)[:num_episodes], torch.cat(lens)[:num_episodes])

    def _per_step_batch(self, env, cost_criteria: float, trace: bool):  # pylint: disable=too-many-locals
        """evaluator.py:425-468 for the K lanes of `env`; a lane stops counting at its first terminated / truncated
        step (vector envs auto-reset; what a finished lane does afterwards is masked)."""
        dev = self._device
        K = int(env.num_envs)
        obs_dim, act_dim = int(env.observation_space.shape[0]), int(env.action_space.shape[0])
        lo, hi = scale_bounds(env, self._device)
        device_env = self._user_env is None and device_env_class(self._env_id) is not None
        max_steps = int(env.max_episode_steps) if device_env else TIME_LIMIT
        state_w = getattr(env, 'trace_state_floats', 0)  # state floats of a trace record
        f64 = dict(dtype=torch.float64, device=dev)
        ret, cost = torch.zeros(K, **f64), torch.zeros(K, **f64)
        length = torch.zeros(K, dtype=torch.int32, device=dev)
        alive = torch.ones(K, dtype=torch.bool, device=dev)
        act_env = torch.empty(K, act_dim, dtype=torch.float32, device=dev)
        z = torch.ones(K, 1, dtype=torch.float32, device=dev)
        if self._saute:
            budget = torch.tensor([self._budget], dtype=torch.float32, device=dev)
            gamma = torch.tensor([self._saute_gamma], dtype=torch.float32, device=dev)
        tr = None
        if trace:
            tr = torch.zeros(max_steps, K, self._trace_floats(env, obs_dim, act_dim), dtype=torch.float32,
                             device=dev)
        obs, _ = env.reset()
        if self._user_env is None and getattr(env, 'param_names', ()):  # an episode keeps the row of its reset
            self._episode_par = env.params.clone()
        for t in range(max_steps):
            x = obs.reshape(K, obs_dim).to(dev, torch.float32)
            if self._normalizer is not None:
                x = self._normalizer.apply(x)
            if self._saute:  # evaluator.py:432-433
                x = torch.cat([x, z], dim=1)
            state = env.state[:, :state_w].clone() if (tr is not None and state_w) else None
            self._actor.step(x, deterministic=True, nets_mask=1, out={'scale': (act_env, lo, hi, -1.0, 1.0)})
            obs, r, c, term, trunc, _ = env.step(act_env)
            r = r.reshape(K).to(dev, torch.float32)
            c = c.reshape(K).to(dev, torch.float32)
            if tr is not None:
                one = torch.ones(K, 1, dtype=torch.float32, device=dev)
                parts = [x, act_env, r[:, None], c[:, None], one] + ([state] if state is not None else [])
                tr[t] = torch.where(alive[:, None], torch.cat(parts, dim=1), torch.zeros((), device=dev))
            if self._saute:  # evaluator.py:456-458, float32 (tensor divisors: true division)
                z = (z - c[:, None] / budget) / gamma
            # evaluator.py:460-466 in float64; cost_criteria ** length with the common length t of the live lanes
            ret = torch.where(alive, ret + r.double(), ret)
            cost = torch.where(alive, cost + (cost_criteria ** t) * c.double(), cost)
            ended = term.reshape(K).to(dev).bool() | trunc.reshape(K).to(dev).bool()
            if self._early_terminated:
                ended = ended | (cost >= self._cost_limit)
            length = length + alive.to(torch.int32)
            alive = alive & ~ended
            if not bool(alive.any()):
                break
        self.trace = tr
        return ret, cost, length

    # ------------------------------------------------------------------ rendering
    def render(self, num_episodes: int = 1, save_replay_path: str | None = None,  # pylint: disable=too-many-locals
               max_render_steps: int = 2000, cost_criteria: float = 1.0, *, width: int | None = None,
               height: int | None = None, camera_name: str | None = None, trail: int = 50, supersample: int = 2,
               fps: float = 30, frame_skip: int = 1, env_params: dict | None = None):
        """evaluator.py:511-629: plays ``num_episodes`` episodes as ``evaluate`` does and writes, per episode k,
        ``<save_replay_path>/eval-episode-<k>.png`` (animated PNG of records 0 .. min(length, max_render_steps) - 1,
        every ``frame_skip``-th frame, 1 / fps seconds each) and ``eval-episode-<k>-path.png`` (the last of those
        records with the whole path behind it), and appends ``result.txt`` in the reference's wording.
        ``save_replay_path`` defaults to ``<save_dir>/video/<model name without .pt>``; ``width``, ``height`` and
        ``camera_name`` ('fixed' or 'track') default to what ``load_saved`` was given; ``env_params`` is
        ``evaluate``'s, and a description's draw() is told the parameters of the episode it draws.  Returns
        ``(episode_rewards, episode_costs)``."""
        if self._actor is None:
            raise ValueError('The policy must be loaded (load_saved) before rendering the agent.')
        opts = self._render_defaults
        width, height = int(width or opts['width']), int(height or opts['height'])
        camera = render_mod.camera_index(camera_name or opts['camera_name'])
        cls = device_env_class(self._env_id)
        if self._user_env is not None or cls is None or not (cls.trace_state_floats and cls.render_state):
            what = 'an env object given as env=' if self._user_env is not None else self._env_id
            raise ValueError(f'{what} has no state row to draw: render() takes the geometric device envs '
                             '(SynthReach-v0, SynthNav*-v0)')
        if frame_skip < 1 or max_render_steps < 1 or trail < 0 or fps <= 0:
            raise ValueError('render() needs frame_skip >= 1, max_render_steps >= 1, trail >= 0 and fps > 0')
        if save_replay_path is None:
            save_replay_path = os.path.join(self._save_dir, 'video', self._model_name.split('.')[0])
        os.makedirs(save_replay_path, exist_ok=True)
        result_path = os.path.join(save_replay_path, 'result.txt')
        if self._verbose:
            print(f'Saving the replay video to {save_replay_path},\n and the result to {result_path}.')
        clock = {'play': 0.0, 'raster': 0.0, 'copy': 0.0, 'encode': 0.0}
        t0 = time.perf_counter()
        rewards, costs = self.evaluate(num_episodes=num_episodes, cost_criteria=cost_criteria, trace=True,
                                       env_params=env_params)
        torch.cuda.synchronize(self._device)
        clock['play'] = time.perf_counter() - t0
        tr = self.trace.contiguous()  # [T][K][rec]; a record ends with the state row before its step
        T, K, rec = tr.shape
        state_w = cls.trace_state_floats
        kind = cls.render_kind(self._env_id)  # (env_kind of the built-in rasteriser, or the custom class and level)
        # hit[f]: record f - 1 had a positive cost (the cost column is two in front of the alive flag and the state)
        hit = torch.zeros(K, T, dtype=torch.uint8, device=tr.device)
        hit[:, 1:] = (tr[:-1, :, rec - state_w - 2] > 0).t()
        for k in range(int(num_episodes)):
            frames = int(min(self.episode_lengths[k], max_render_steps, T))
            if self._episode_par is not None:  # (a custom class with runtime parameters: this episode's row)
                kind = kind._replace(par=self._episode_par[k])
            at = (kind, tr, k * rec + rec - state_w, K * rec)
            chunks = render_mod.stream_frames(*at, frames, trail, hit[k], camera, width, height, supersample,
                                              frame_skip, clock)
            t0 = time.perf_counter()
            before = clock['raster'] + clock['copy']
            apng.write_apng(os.path.join(save_replay_path, f'eval-episode-{k}.png'), chunks, fps, level=1)
            still = render_mod.rasterise(*at, frames - 1, 1, frames, hit[k], camera, width, height, supersample)
            apng.write_png(os.path.join(save_replay_path, f'eval-episode-{k}-path.png'), still[0].cpu().numpy())
            clock['encode'] += time.perf_counter() - t0 - (clock['raster'] + clock['copy'] - before)
            with open(result_path, 'a+', encoding='utf-8') as f:
                print(f'Episode {k} results:', file=f)
                print(f'Episode reward: {rewards[k]}', file=f)
                print(f'Episode cost: {costs[k]}', file=f)
                print(f'Episode length: {self.episode_lengths[k]}', file=f)
        with open(result_path, 'a+', encoding='utf-8') as f:
            print('Evaluation results:', file=f)
            print(f'Average episode reward: {np.mean(rewards)}', file=f)
            print(f'Average episode cost: {np.mean(costs)}', file=f)
            print(f'Average episode length: {np.mean(self.episode_lengths)}', file=f)
        self.render_clock = clock
        return rewards, costs


__all__ = ['Evaluator']
