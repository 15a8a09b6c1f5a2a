"""``omnisafe_amd.AgentGroup`` -- several independent trainings in one process on one GPU, their persistent-pass
launches issued together.

The reference runs the seeds and hyper-parameter variants of an experiment as one training per worker of a process
pool (ExperimentGrid.run, omnisafe/common/experiment_grid.py:387-471).  One agent's update occupies 3 compute units
(one workgroup per network) for 99 % of an epoch's GPU time; the only way to use the rest of the device is to run
OTHER agents there.  A group member is an ordinary :class:`omnisafe_amd.Agent`; its updater hands every plain
persistent pass to the group instead of launching it, and when every member that is still running waits with a pass,
the group issues ONE launch per kernel class (osa_ppo_pass_group) that carries all of them.

A member is the run its configuration describes: parameters, Adam state and logged curves are bit for bit those of a
solo ``Agent`` with the same configuration (the grouped launch runs the same kernel body on the same operands; every
member's shuffles come from its own device generator, in the state a solo run's global one would have).  Only the
``Time/*`` columns differ: inside a group they measure the group's wall time, not the member's own work.

Members run on one thread each, but never concurrently: a baton passes from the group to one member at a time (the
rollout captures and replays hipGraphs on the shared stream, and a capture must not overlap another member's launches
or allocations).  Everything stays on one stream.
"""
from __future__ import annotations

import copy
import ctypes as C
import os
import threading
import time

import torch

from . import _lib
from . import distributed as dist
from .agent import Agent
from .config import get_default_kwargs, recursive_check_config
from .models import PassMember
from .update import PPOUpdater

_EXCLUDE = ('exp_name', 'env_id', 'algo', 'exp_increment_cfgs')  # as Agent._init_config


def _merged(base: dict, over: dict) -> dict:
    out = copy.deepcopy(base)
    for k, v in over.items():
        out[k] = _merged(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else copy.deepcopy(v)
    return out


def member_cfgs(algo: str, seeds=None, variants=None, custom_cfgs: dict | None = None) -> list[dict]:
    """The members' ``custom_cfgs``: the shared ``custom_cfgs`` overlaid with one variant each (``seeds=`` is
    shorthand for ``variants=[{'seed': s}, ...]``), checked like ``Agent``'s, and with a log directory of its own per
    member -- ``<logger_cfgs.log_dir>/member-<k>`` -- so that two members with the same seed, started in the same
    second, do not share a ``seed-XXX-<timestamp>`` folder.  Needs no GPU."""
    if (seeds is None) == (variants is None):
        raise ValueError('AgentGroup: give either seeds= or variants=')
    variants = [{'seed': int(s)} for s in seeds] if variants is None else [dict(v) for v in variants]
    if not variants:
        raise ValueError('AgentGroup: no members')
    default = get_default_kwargs(algo)
    out = []
    for k, var in enumerate(variants):
        cfg = _merged(custom_cfgs or {}, var)
        recursive_check_config(cfg, default, exclude_keys=_EXCLUDE)
        base = cfg.get('logger_cfgs', {}).get('log_dir', default['logger_cfgs']['log_dir'])
        out.append(_merged(cfg, {'logger_cfgs': {'log_dir': os.path.join(base, f'member-{k:03d}')}}))
    return out


class _Abort(Exception):
    """Raised inside a waiting member when another member failed."""


class _Member:
    def __init__(self, agent: Agent) -> None:
        self.agent = agent
        self.go, self.back = threading.Event(), threading.Event()
        self.pending = None  # (updater, PassMember) while the member waits for the grouped launch
        self.carried = 0     # members of the launch that carried its last submission
        self.done = False
        self.result = None
        self.error: BaseException | None = None
        self.thread: threading.Thread | None = None


class AgentGroup:
    """``AgentGroup(algo, env_id, seeds=range(8), custom_cfgs={...})`` or ``variants=[{...}, ...]``: see the module
    docstring.  ``learn()`` returns the members' ``(ep_ret, ep_cost, ep_len)`` in member order; ``agents`` are the
    ``omnisafe_amd.Agent`` objects; after ``learn()``, ``wall_time`` and ``env_steps_per_second`` describe the whole
    group (all members' environment steps over the group's wall time)."""

    def __init__(self, algo: str, env_id: str, seeds=None, variants=None, train_terminal_cfgs: dict | None = None,
                 custom_cfgs: dict | None = None) -> None:
        self.algo, self.env_id = algo, env_id
        self.member_cfgs = member_cfgs(algo, seeds, variants, custom_cfgs)
        if dist.world_size() > 1 or int(os.environ.get('WORLD_SIZE', '1')) > 1:
            raise NotImplementedError('AgentGroup runs in one process on one GPU (world size 1): start the group '
                                      'without torchrun, or train the members as separate data-parallel Agents')
        # one after another: every constructor seeds the process-global generators and then draws its initial
        # parameters from them, exactly as the solo run does
        self.agents = [Agent(algo, env_id, train_terminal_cfgs=train_terminal_cfgs, custom_cfgs=cfg)
                       for cfg in self.member_cfgs]
        devices = {str(a.cfgs.train_cfgs.device) for a in self.agents}
        if len(devices) > 1:
            raise NotImplementedError(f'AgentGroup: all members must train on one device, got {sorted(devices)}')
        self._lib = _lib.load(require_gpu=True)
        self._device = torch.device(devices.pop())
        self._members = [_Member(a) for a in self.agents]
        self._ws: dict = {}  # kernel class -> staging workspace of osa_ppo_pass_group
        self._abort = False
        self.wall_time = self.env_steps_per_second = None
        for m in self._members:
            # the device generator of a solo run after seed_all(seed): the shuffles are its only draws
            gen = torch.Generator(device=self._device)
            gen.manual_seed(int(m.agent.cfgs.seed))
            for up in vars(m.agent.agent).values():
                if isinstance(up, PPOUpdater):
                    up.generator = gen
                    up.pass_submit = lambda updater, pm, m=m: self._submit(m, updater, pm)

    # ------------------------------------------------------------------ the baton
    def _submit(self, m: _Member, updater, pm) -> int:
        """Member side (its thread holds the baton): hand the pass over and wait until the group has enqueued it."""
        m.pending = (updater, pm)
        m.back.set()
        m.go.wait()
        m.go.clear()
        if self._abort:
            raise _Abort
        return m.carried

    def _run_member(self, m: _Member) -> None:
        m.go.wait()
        m.go.clear()
        try:
            if self._abort:
                raise _Abort
            torch.cuda.set_device(self._device)  # (the current device is per thread)
            m.result = m.agent.learn()
        except BaseException as exc:  # noqa: BLE001 - re-raised by learn() on the caller's thread
            m.error = exc
        finally:
            m.done = True
            m.back.set()

    def _resume(self, m: _Member) -> None:
        """Group side: the baton goes to m until it submits a pass or finishes."""
        m.back.clear()
        m.go.set()
        m.back.wait()

    @staticmethod
    def _class_of(updater, pm) -> tuple:
        """What one template instantiation of the grouped kernel covers (csrc/group_pass_kernel.hip)."""
        e = pm.ext
        extended = bool(pm.has_ext) and (e.kl_coef != 0.0 or e.kl_mask_eta >= 0.0 or e.cost_kappa > 0.0
                                         or e.ratio_scale != 1.0)
        ac = updater.ac
        return (ac.obs_dim, ac.act_dim, ac.hidden, pm.B > 64, extended)

    def _flush(self, waiting: list[_Member]) -> None:
        """One osa_ppo_pass_group launch per kernel class, classes in order of their first submission."""
        classes: dict = {}
        for m in waiting:
            classes.setdefault(self._class_of(*m.pending), []).append(m)
        for key, ms in classes.items():
            n = len(ms)
            need = self._lib.osa_ppo_pass_group_ws_bytes(n)
            ws = self._ws.get(key)
            if ws is None or ws.numel() < need:
                ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=self._device)
            arr = (PassMember * n)(*(m.pending[1] for m in ms))
            _lib.check(self._lib.osa_ppo_pass_group(key[0], key[1], key[2], C.cast(arr, C.c_void_p), n, _lib.ptr(ws),
                                                    ws.numel(), _lib.stream_ptr()), 'osa_ppo_pass_group')
            for m in ms:
                m.carried, m.pending = n, None

    def learn(self) -> list[tuple[float, float, float]]:
        torch.cuda.set_device(self._device)
        for m in self._members:
            m.thread = threading.Thread(target=self._run_member, args=(m,), daemon=True)
            m.thread.start()
        start = time.time()
        live = list(self._members)
        failed = None
        while live and failed is None:
            for m in live:
                self._resume(m)
                if m.error is not None:
                    failed = m
                    break
            else:
                live = [m for m in live if not m.done]
                if live:
                    self._flush(live)
        if failed is not None:
            self._abort = True
            for m in self._members:
                if not m.done:
                    self._resume(m)
        for m in self._members:
            m.thread.join()
        if failed is not None:
            raise failed.error
        torch.cuda.synchronize(self._device)
        self.wall_time = time.time() - start
        steps = sum(int(a.cfgs.train_cfgs.epochs) * int(a.cfgs.algo_cfgs.steps_per_epoch) for a in self.agents)
        self.env_steps_per_second = steps / self.wall_time
        return [m.result for m in self._members]

    def evaluate(self, num_episodes: int = 10, cost_criteria: float = 1.0,
                 env_params: dict | None = None) -> list[dict]:
        """``Agent.evaluate`` of every member, in member order."""
        return [a.evaluate(num_episodes=num_episodes, cost_criteria=cost_criteria, env_params=env_params)
                for a in self.agents]

    def render(self, num_episodes: int = 10, render_mode: str = 'rgb_array', camera_name: str = 'track',
               width: int = 256, height: int = 256, env_params: dict | None = None) -> list[dict]:
        """``Agent.render`` of every member, in member order."""
        return [a.render(num_episodes=num_episodes, render_mode=render_mode, camera_name=camera_name, width=width,
                         height=height, env_params=env_params) for a in self.agents]
