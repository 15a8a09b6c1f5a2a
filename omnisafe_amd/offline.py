"""``OfflineDataCollector`` -- datasets for the offline algorithms from saved policies (mirror of
omnisafe/common/offline/data_collector.py:42-212).

    col = OfflineDataCollector(size, env_name)
    for save_dir, model_name, n in agents:
        col.register_agent(save_dir, model_name, n)
    col.collect(data_dir)        # <data_dir>/<env_name>_data.npz, the file omnisafe's OfflineDataset reads

Every agent plays its policy STOCHASTICALLY and fills a block of ``n`` rows ``(obs, action, reward, cost, next_obs,
done)`` with the reference's row semantics: ``obs`` / ``next_obs`` are the raw env observations (the checkpoint's
normaliser, statistics frozen, is applied to the policy's input only), ``action`` is the actor's sample before
ActionScale (the env receives the scaled one), ``done = terminated or truncated``, the ``next_obs`` of a done row is the
observation of the state the episode ended in and the ``obs`` of the following row the fresh reset.  The rows stay on
the device (``col.data``) and are written once at the end.

Layout of an agent's block of S rows (``lane_layout``): K = ``num_envs`` lanes (default ``default_num_envs``: about one
full episode or more per lane), Q = ceil(S / K); lane k owns rows [k Q, min((k + 1) Q, S)) and fills them with
consecutive episodes, the last one cut off where its rows end -- the structure the reference gives the whole block.
Lane k is env index k of a fresh K-env vector env: reset at Philox stream position 0, step t at position t + 1, an
ending step resets at its own position.  The action noise of step t of lane k is what a fresh actor with
``set_seed(noise_seed)`` draws for row k on its (t + 1)-th ``step``.  Agent i of a collector seeded ``seed`` uses
``agent_seeds(seed, i)``: env seed ``seed + AGENT_STRIDE * i`` (mod 2^64), noise seed ``env seed ^ NOISE_KEY``, so
blocks do not repeat each other and the same ``seed`` reproduces the file.

Two paths, equal bit for bit where both apply (as ``Evaluator``):
  persistent  a fused-family actor on a device env (built-in or of register_device_env): the whole block in ONE launch
              of osa_collect_episodes (csrc/collect_kernels.hip; a custom env: its library's
              osa_custom_collect_episodes, the same kernel template).
  per-step    everything else (general networks, host envs behind the bridge): the existing launches per vector step
              -- Normalizer.apply, ConstraintActorCritic.step(deterministic=False) with ActionScale fused, env.step,
              info['final_observation'].  A device env class that ``terminates`` is refused here: its per-step kernel
              hands out no observation for a terminated step (final_obs is written for truncated envs only); the
              persistent path takes such classes.
``OSA_COLLECT_PATH=per-step|persistent`` forces a path (the persistent one raises OsaError when it cannot take the case).

Deviations from the reference: lanes in parallel instead of one env (above); Saute / Simmer checkpoints raise
NotImplementedError (their actor has the extra safety column; the reference's collector cannot build them either);
an agent that finishes no episode prints nan averages where the reference divides by zero.
"""
from __future__ import annotations

import math
import os
import zipfile
from dataclasses import dataclass, field
from typing import Any

import numpy as np
import torch

from . import _lib
from . import envs as envs_mod
from .evaluator import TIME_LIMIT
from .saved_policy import build_policy, choose_path, device_env_class, load_checkpoint, policy_args, scale_bounds

NOISE_KEY = 0x6A09E667F3BCC908
AGENT_STRIDE = 0x9E3779B1  # (odd and far above any seed a user counts up from: agents of neighbouring seeds differ too)
MAX_LANES = 4096
FIELDS = ('obs', 'action', 'reward', 'cost', 'next_obs', 'done')
PERSISTENT_MAX_OBS = 304  # include/omnisafe_amd.h: osa_collect_episodes


def agent_seeds(seed: int, i: int) -> tuple[int, int]:
    """(env seed, noise seed) of the i-th registered agent."""
    env_seed = (int(seed) + AGENT_STRIDE * int(i)) & 0xFFFFFFFFFFFFFFFF
    return env_seed, env_seed ^ NOISE_KEY


def default_num_envs(size: int, horizon: int) -> int:
    """Lanes of a block of ``size`` rows: every lane plays about one full episode or more."""
    return max(1, min(MAX_LANES, int(size) // int(horizon)))


def lane_layout(size: int, num_envs: int) -> tuple[int, list[tuple[int, int]]]:
    """``(Q, [(start, stop)] * K)``: rows per lane Q = ceil(S / K) and the rows [start, stop) of every lane inside
    the block (empty for a lane past the end of the block)."""
    S, K = int(size), int(num_envs)
    assert S >= 1 and K >= 1
    Q = -(-S // K)
    return Q, [(min(k * Q, S), min((k + 1) * Q, S)) for k in range(K)]


def write_dataset(save_dir: str, env_name: str, arrays: dict[str, np.ndarray]) -> str:
    """data_collector.py:197-212: ``<save_dir>/<env_name>_data.npz`` with the six float32 fields; returns its path."""
    if not os.path.exists(save_dir):
        os.makedirs(save_dir)
    save_path = os.path.join(save_dir, f'{env_name}_data.npz')
    if os.path.exists(save_path):
        print(f'Warning: {save_path} already exists.')
        print(f'Warning: {save_path} will be overwritten.')
    # np.savez's archive (stored .npy members, what np.load and the reference read) with a fixed member time instead of
    # the clock's, so that the same rows give the same file byte for byte
    with zipfile.ZipFile(save_path, 'w', zipfile.ZIP_STORED, allowZip64=True) as archive:
        for k in FIELDS:
            member = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            with archive.open(member, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arrays[k], dtype=np.float32), allow_pickle=False)
    return save_path


@dataclass
class OfflineAgent:
    """data_collector.py:34-39, with what this package's two paths need beside ``agent_step``."""

    agent_step: Any = field(repr=False)  # obs (K, obs_dim) -> unscaled action sample (the per-step path's policy)
    size: int = 0
    save_dir: str = ''
    model_name: str = ''
    actor: Any = field(default=None, repr=False)
    normalizer: Any = field(default=None, repr=False)


class OfflineDataCollector:  # pylint: disable=too-many-instance-attributes
    def __init__(self, size: int, env_name: str, *, seed: int = 0, device='cuda:0', num_envs: int | None = None,
                 env_cfgs: dict | None = None) -> None:
        self._size = int(size)
        self._env_name = env_name
        self._seed = int(seed)
        self._device = torch.device(device)
        self._num_envs = None if num_envs is None else int(num_envs)
        assert self._num_envs is None or self._num_envs >= 1
        self._env_cfgs = dict(env_cfgs or {})
        self._cls = device_env_class(env_name)
        if self._cls is not None:  # (a device env: its dimensions need neither the library nor a GPU)
            self._obs_dim, self._act_dim = self._cls.dims(env_name)
        else:
            env = envs_mod.make(env_name, num_envs=1, device=self._device, **self._env_cfgs)
            obs_space, act_space = env.observation_space, env.action_space
            env.close()
            for space in (obs_space, act_space):
                if not hasattr(space, 'low') or len(space.shape) != 1:
                    raise NotImplementedError('Only support Box observation space for now.'
                                              if space is obs_space else 'Only support Box action space for now.')
            self._obs_dim, self._act_dim = int(obs_space.shape[0]), int(act_space.shape[0])
        self.agents: list[OfflineAgent] = []
        self.path: str | None = None  # path of the last agent collected: 'persistent' or 'per-step'
        self.data: dict[str, torch.Tensor] = {}  # the six fields on the device, after collect()
        self.summaries: list[dict[str, float]] = []  # what collect() printed per agent

    # ------------------------------------------------------------------ agents
    def register_agent(self, save_dir: str, model_name: str, size: int) -> None:
        """data_collector.py:93-143."""
        try:
            kwargs, cfgs, model_params = load_checkpoint(save_dir, model_name)
        except FileNotFoundError as error:
            if os.path.basename(str(error.filename)) == 'config.json':
                raise FileNotFoundError('The config file is not found in the save directory.') from error
            raise FileNotFoundError(f'Model {model_name} not found in {save_dir}') from error
        algo = str(kwargs.get('algo', ''))
        if 'Saute' in algo or 'Simmer' in algo:
            raise NotImplementedError(f'{algo}: the actor of a Saute / Simmer checkpoint takes the safety column beside '
                                      'the observation; the collector plays plain policies (as the reference\'s)')
        actor, normalizer = build_policy(cfgs, model_params, self._obs_dim, self._act_dim, self._device)

        def agent_step(obs: torch.Tensor) -> torch.Tensor:
            x = normalizer.apply(obs) if normalizer is not None else obs
            return actor.step(x, deterministic=False, nets_mask=1)[0]

        self.agents.append(OfflineAgent(agent_step, int(size), save_dir, model_name, actor, normalizer))

    # ------------------------------------------------------------------ collection
    def _horizon(self) -> int:
        if self._cls is not None:
            return int(self._env_cfgs.get('horizon', self._cls.default_horizon))
        return TIME_LIMIT

    def _persistent_ok(self, agent: OfflineAgent) -> bool:
        return self._cls is not None and not agent.actor.general and self._obs_dim <= PERSISTENT_MAX_OBS

    def collect(self, save_dir: str) -> None:
        """data_collector.py:145-212."""
        total_size = 0
        for agent in self.agents:
            assert agent.size <= self._size, f'Agent {agent} size is larger than collector size.'
            total_size += agent.size
        assert total_size == self._size, 'Sum of agent size is not equal to collector size.'
        S, dev = self._size, self._device
        f32 = dict(dtype=torch.float32, device=dev)
        data = {'obs': torch.zeros(S, self._obs_dim, **f32), 'action': torch.zeros(S, self._act_dim, **f32),
                'reward': torch.zeros(S, 1, **f32), 'cost': torch.zeros(S, 1, **f32),
                'next_obs': torch.zeros(S, self._obs_dim, **f32), 'done': torch.zeros(S, 1, **f32)}
        self.summaries = []
        ptx = 0
        for i, agent in enumerate(self.agents):
            if agent.size == 0:
                continue
            self.path = choose_path('OSA_COLLECT_PATH', self._persistent_ok(agent),
                                    'the persistent kernel takes a fused-family actor on '
                                    f'a device env with at most {PERSISTENT_MAX_OBS} observation columns (here '
                                    f'{self._env_name}, general network: {agent.actor.general})')
            K = self._num_envs or default_num_envs(agent.size, self._horizon())
            block = {k: v[ptx:ptx + agent.size] for k, v in data.items()}
            run = self._run_persistent if self.path == 'persistent' else self._run_per_step
            ret, cost, count = run(agent, K, block, *agent_seeds(self._seed, i))
            # data_collector.py:178-194 with the lanes' float64 sums added up exactly
            ep_ret, ep_cost = math.fsum(ret.cpu().tolist()), math.fsum(cost.cpu().tolist())
            episode_num = int(count.sum().item())
            avg = (lambda x: x / episode_num) if episode_num else (lambda x: float('nan'))
            summary = {'return': avg(ep_ret), 'cost': avg(ep_cost), 'length': avg(float(agent.size)),
                       'episodes': episode_num}
            self.summaries.append(summary)
            print(f'Agent {agent} collected {agent.size} data points.')
            print(f'Average return: {summary["return"]}')
            print(f'Average cost: {summary["cost"]}')
            print(f'Average episode length: {summary["length"]}')
            print()
            ptx += agent.size
        self.data = data
        write_dataset(save_dir, self._env_name, {k: v.cpu().numpy() for k, v in data.items()})

    def _make_env(self, K: int, env_seed: int):
        env = envs_mod.make(self._env_name, num_envs=K, device=self._device, **self._env_cfgs)
        env.set_seed(env_seed)
        return env

    def _run_persistent(self, agent: OfflineAgent, K: int, block: dict, env_seed: int, noise_seed: int):
        env = self._make_env(K, env_seed)
        entry = env.collect_entry_point
        play = getattr(env.library(), entry)
        S = agent.size
        Q, _ = lane_layout(S, K)
        lo, hi = scale_bounds(env, self._device)
        dev = self._device
        ret = torch.zeros(K, dtype=torch.float64, device=dev)
        cost = torch.zeros(K, dtype=torch.float64, device=dev)
        count = torch.zeros(K, dtype=torch.int32, device=dev)
        for name in FIELDS:
            assert block[name].stride(-1) == 1
        par_args, _ = env.player_param_args(K)  # (a custom class with runtime parameters: its ranges)
        _lib.check(play(
            env.eval_kind(self._env_name), K, Q, S,
            *policy_args(agent.actor, agent.normalizer, self._obs_dim, self._act_dim, lo, hi), env_seed,
            noise_seed, int(env.max_episode_steps), env._cost_p,
            _lib.ptr(block['obs']), block['obs'].stride(0), _lib.ptr(block['action']), block['action'].stride(0),
            _lib.ptr(block['reward']), _lib.ptr(block['cost']), _lib.ptr(block['next_obs']),
            block['next_obs'].stride(0), _lib.ptr(block['done']), _lib.ptr(ret), _lib.ptr(cost), _lib.ptr(count),
            *par_args, _lib.stream_ptr()), entry)
        env.close()
        return ret, cost, count

    def _run_per_step(self, agent: OfflineAgent, K: int, block: dict,  # pylint: disable=too-many-locals
                      env_seed: int, noise_seed: int):
        """data_collector.py:165-189 for the K lanes side by side: step t of every lane in one set of launches, the
        rows of lane k gathered into [k Q, (k + 1) Q) afterwards."""
        if self._cls is not None and self._cls.terminates:
            raise NotImplementedError(
                f'{self._env_name} ends episodes per env, and its per-step kernel hands out no observation for a '
                'terminated step (final_obs is written for truncated envs only), so the per-step path cannot fill '
                'next_obs there; the persistent path (a fused-family actor) takes such classes')
        dev = self._device
        S = agent.size
        Q, ranges = lane_layout(S, K)
        env = self._make_env(K, env_seed)
        lo, hi = scale_bounds(env, self._device)
        ac, nm = agent.actor, agent.normalizer
        ac.set_seed(noise_seed)  # a fresh noise stream: the (t + 1)-th step draws at position t + 1
        ac._rng_offset = 0
        ac._rng_base.zero_()
        D, A = self._obs_dim, self._act_dim
        f32 = dict(dtype=torch.float32, device=dev)
        rows = {'obs': torch.zeros(Q, K, D, **f32), 'action': torch.zeros(Q, K, A, **f32),
                'reward': torch.zeros(Q, K, 1, **f32), 'cost': torch.zeros(Q, K, 1, **f32),
                'next_obs': torch.zeros(Q, K, D, **f32), 'done': torch.zeros(Q, K, 1, **f32)}
        act_env = torch.empty(K, A, **f32)
        ret = torch.zeros(K, dtype=torch.float64, device=dev)
        cost = torch.zeros(K, dtype=torch.float64, device=dev)
        count = torch.zeros(K, dtype=torch.int32, device=dev)
        lane_rows = torch.tensor([b - a for a, b in ranges], dtype=torch.int64, device=dev)
        obs, _ = env.reset()
        obs = obs.reshape(K, D).to(dev, torch.float32)
        for t in range(Q):
            x = nm.apply(obs) if nm is not None else obs
            ac.step(x, deterministic=False, nets_mask=1,
                    out={'act': rows['action'][t], 'scale': (act_env, lo, hi, -1.0, 1.0)})
            rows['obs'][t] = obs
            nobs, r, c, term, trunc, info = env.step(act_env)
            nobs = nobs.reshape(K, D).to(dev, torch.float32)
            r = r.reshape(K).to(dev, torch.float32)
            c = c.reshape(K).to(dev, torch.float32)
            done = term.reshape(K).to(dev).bool() | trunc.reshape(K).to(dev).bool()
            nxt = nobs
            if 'final_observation' in info:  # the observation of the state an ending episode ended in
                final = info['final_observation'].reshape(K, D).to(dev, torch.float32)
                mask = info['_final_observation'].reshape(K).to(dev).bool()
                nxt = torch.where(mask[:, None], final, nobs)
            rows['next_obs'][t] = nxt
            rows['reward'][t, :, 0] = r
            rows['cost'][t, :, 0] = c
            rows['done'][t, :, 0] = done.to(torch.float32)
            live = lane_rows > t
            ret = torch.where(live, ret + r.double(), ret)
            cost = torch.where(live, cost + c.double(), cost)
            count = count + (live & done).to(torch.int32)
            obs = nobs
        for name in FIELDS:
            block[name].copy_(rows[name].permute(1, 0, 2).reshape(K * Q, -1)[:S])
        env.close()
        return ret, cost, count


__all__ = ['OfflineDataCollector', 'OfflineAgent', 'agent_seeds', 'default_num_envs', 'lane_layout', 'write_dataset']
