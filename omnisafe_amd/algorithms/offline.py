"""Offline CRR and CCRR trained on the device from a collected dataset -- mirror of
omnisafe/algorithms/offline/base.py:32-152, crr.py:30-200 and c_crr.py:30-206.

    col.collect(data_dir)
    agent = omnisafe_amd.Agent('CCRR', env_id, custom_cfgs={'train_cfgs': {'dataset': '<data_dir>/<env_id>_data.npz'}})
    agent.learn(); agent.evaluate(); agent.render()

The dataset rows stay on the device as float32 for the whole training; an epoch is ``steps_per_epoch`` train steps
enqueued on one stream (crr_step.CrrStep: csrc/crr_kernels.hip) whose per-step scalars reach the host once, at the
epoch's end; the epoch's evaluation plays ``evaluate_epoisodes`` deterministic episodes side by side through the
saved-policy players (evaluator.Evaluator) instead of one after another on a one-env adapter
(offline_adapter.py:115-149).  There is no observation normaliser in this family.

Deviations from the reference:
  * ``train_cfgs.dataset`` is the path of an ``.npz`` file (or an OfflineDataCollector); nothing is downloaded.
  * CCRR trains the cost critic pair on the cost targets with its own optimiser and values the sampled actions' cost
    with it.  c_crr.py:103-133 as written trains the reward pair a second time and :160-161 evaluates the sampled cost
    with the reward pair; ``OSA_CCRR_WIRING=reference`` selects that wiring.
  * Checkpoints hold the actor under ``actor`` (what the reference saves) and under ``pi`` (what every Evaluator,
    the reference's included, reads).
  * The ``total_steps % steps_per_epoch`` steps after the last epoch, which the reference trains but never logs,
    evaluates or saves, are not run.
"""
from __future__ import annotations

import os
import time

import torch

from ..crr_step import CRR_STATS, STAT_KEYS, CrrStep, load_dataset, make_desc
from ..evaluator import Evaluator
from ..logger import Logger
from ..saved_policy import device_env_class
from .. import envs as envs_mod
from .base_algo import BaseAlgo
from .registry import register

MAX_SLOTS = 8192  # steps whose draws and statistics are resident at a time (an epoch, unless it is longer)


class _ActorState:
    """What the logger's saver calls: the actor's state dict in the reference's names and order."""

    def __init__(self, step: CrrStep) -> None:
        self._step = step

    def state_dict(self):
        return self._step.actor_state_dict()


class BaseOffline(BaseAlgo):  # pylint: disable=too-many-instance-attributes
    """base.py:32-152."""

    pairs = 1

    def __init__(self, env_id: str, cfgs) -> None:
        self.epoch = 0
        super().__init__(env_id, cfgs)

    # ------------------------------------------------------------------ construction, in the reference's order
    def _init_env(self) -> None:
        """offline_adapter.py:46-75: only the dimensions are needed until an evaluation plays the env."""
        self._env_cfgs = dict(self._cfgs.env_cfgs.todict()) if hasattr(self._cfgs, 'env_cfgs') else {}
        cls = device_env_class(self._env_id)
        if cls is not None:
            self._obs_dim, self._act_dim = cls.dims(self._env_id)
        else:
            env = envs_mod.make(self._env_id, num_envs=1, device=self._device, **self._env_cfgs)
            self._obs_dim, self._act_dim = int(env.observation_space.shape[0]), int(env.action_space.shape[0])
            env.close()

    def _init_model(self) -> None:
        """crr.py:71-112, c_crr.py:64-89: actor, reward critic pair, (CCRR) cost critic pair; targets are copies."""
        m, a = self._cfgs.model_cfgs, self._cfgs.algo_cfgs
        assert isinstance(m.actor.lr, float), 'The learning rate must be a float number.'
        assert isinstance(m.critic.lr, float), 'The learning rate must be a float number.'
        desc = make_desc(self._obs_dim, self._act_dim, m.actor.hidden_sizes, m.critic.hidden_sizes, m.actor.activation,
                         m.critic.activation, a.batch_size, a.sampled_action_num, self.pairs)
        lag = self._cfgs.lagrange_cfgs if self.pairs == 2 else None
        if lag is not None and lag.lambda_optimizer != 'Adam':
            raise NotImplementedError(f'lambda_optimizer {lag.lambda_optimizer!r}: the device Lagrange step is Adam')
        self._nslots = min(int(a.steps_per_epoch), MAX_SLOTS)
        self._step = CrrStep(desc, None, gamma=float(a.gamma), beta=float(a.beta), polyak=float(a.polyak),
                             lr_actor=m.actor.lr, lr_critic=m.critic.lr, nslots=self._nslots,
                             cost_limit=float(lag.cost_limit) if lag else 0.0,
                             lambda_lr=float(lag.lambda_lr) if lag else 0.0,
                             lambda_init=float(lag.lagrangian_multiplier_init) if lag else 0.0, device=self._device)
        self._step.init_parameters(m.weight_initialization_mode)
        self._actor = _ActorState(self._step)

    def _init(self) -> None:
        """base.py:42-47: the dataset, on the device."""
        source = self._cfgs.train_cfgs.dataset
        self._step.set_data(load_dataset(source, self._obs_dim, self._act_dim, self._device))
        self._dataset_name = (os.path.splitext(os.path.basename(os.fspath(source)))[0]
                              if isinstance(source, (str, os.PathLike)) else f'{self._env_id}_data')
        if not isinstance(source, (str, os.PathLike)):  # (config.json holds the run's settings, not a collector)
            self._cfgs.train_cfgs.recurisve_update({'dataset': self._dataset_name})

    def _stat_columns(self) -> tuple[int, ...]:
        return CRR_STATS

    def _init_log(self) -> None:
        """base.py:52-96, crr.py:39-69."""
        lc = self._cfgs.logger_cfgs
        self._logger = Logger(output_dir=lc.log_dir, exp_name=self._cfgs.exp_name + f'-{self._dataset_name}',
                              seed=self._cfgs.seed, use_tensorboard=lc.use_tensorboard, use_wandb=lc.use_wandb,
                              config=self._cfgs, verbose=bool(getattr(lc, 'verbose', True)))
        for key in ('Metrics/EpRet', 'Metrics/EpCost', 'Metrics/EpLen', 'Time/Total', 'Time/Epoch', 'Time/Update',
                    'Time/Evaluate', 'Train/Epoch', 'TotalSteps'):
            self._logger.register_key(key)
        self._logger.setup_torch_saver({'actor': self._actor, 'pi': self._actor})
        for col in CRR_STATS:
            self._logger.register_key(STAT_KEYS[col])

    # ------------------------------------------------------------------ training
    def _lagrange_open(self) -> bool:
        return False

    def _train_epoch(self) -> torch.Tensor:
        """``steps_per_epoch`` train steps (base.py:105-107 that many times); the steps' statistics rows, on the
        device."""
        spe = int(self._cfgs.algo_cfgs.steps_per_epoch)
        first = self.epoch * spe
        rows = []
        for done in range(0, spe, self._nslots):
            n = min(self._nslots, spe - done)
            self._step.draw(self._seed, first + done, n)
            self._step.run(n, lagrange_open=self._lagrange_open())
            slots = (torch.arange(n, device=self._device) + (first + done)) % self._nslots
            rows.append(self._step.stats[slots])
        return rows[0] if len(rows) == 1 else torch.cat(rows)

    def learn(self) -> tuple[float, float, float]:
        """base.py:98-137."""
        self._logger.log('Start training ...')
        spe = int(self._cfgs.algo_cfgs.steps_per_epoch)
        start_time = epoch_time = time.time()
        try:
            for _ in range(int(self._cfgs.train_cfgs.total_steps) // spe):
                stats = self._train_epoch().cpu()  # the epoch's one read of the device
                for col in self._stat_columns():
                    self._logger.extend(STAT_KEYS[col], stats[:, col].tolist())
                self.epoch += 1
                self._logger.store({'Time/Update': time.time() - epoch_time})
                eval_time = time.time()
                self._evaluate()
                self._logger.store({'Time/Evaluate': time.time() - eval_time, 'Time/Epoch': time.time() - epoch_time,
                                    'Time/Total': time.time() - start_time, 'Train/Epoch': self.epoch,
                                    'TotalSteps': self.epoch * spe})
                epoch_time = time.time()
                ep_ret = self._logger.get_stats('Metrics/EpRet')[0]
                ep_cost = self._logger.get_stats('Metrics/EpCost')[0]
                ep_len = self._logger.get_stats('Metrics/EpLen')[0]
                self._logger.dump_tabular()
                if self.epoch % self._cfgs.logger_cfgs.save_model_freq == 0:
                    self._logger.torch_save()
        finally:
            self._logger.close()
        return ep_ret, ep_cost, ep_len

    def _evaluate(self) -> None:
        """offline_adapter.py:115-149: ``evaluate_epoisodes`` deterministic episodes of the current actor, all in one
        launch where the persistent player takes the actor, through the per-step player otherwise."""
        if not hasattr(self, '_evaluator'):
            self._evaluator = Evaluator(seed=self._seed, device=self._device, verbose=False)
        ev = self._evaluator
        ev.load_policy(self._cfgs.todict(), {'pi': self._step.actor_state_dict()})
        rets, costs = ev.evaluate(num_episodes=int(self._cfgs.train_cfgs.evaluate_epoisodes))
        self._logger.extend('Metrics/EpRet', [float(x) for x in rets])
        self._logger.extend('Metrics/EpCost', [float(x) for x in costs])
        self._logger.extend('Metrics/EpLen', [float(x) for x in ev.episode_lengths])


@register
class CRR(BaseOffline):
    """Critic Regularized Regression (crr.py:30-200)."""


@register
class CCRR(BaseOffline):
    """The constrained form (c_crr.py:30-206): a cost critic pair and a Lagrange multiplier stepped on the device."""

    pairs = 2

    def _stat_columns(self) -> tuple[int, ...]:
        return tuple(range(len(STAT_KEYS)))

    def _init_log(self) -> None:
        """c_crr.py:39-62."""
        super()._init_log()
        for col in (3, 4, 5, 8, 10):
            self._logger.register_key(STAT_KEYS[col])

    def _lagrange_open(self) -> bool:
        """c_crr.py:181-184; constant over an epoch's block of steps."""
        a = self._cfgs.algo_cfgs
        return self.epoch * a.steps_per_epoch > a.lagrange_start_step


__all__ = ['BaseOffline', 'CRR', 'CCRR']
