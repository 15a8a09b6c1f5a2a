"""Off-policy DDPG, TD3 and SAC trained on the device from a replay ring -- mirror of
omnisafe/algorithms/off_policy/ddpg.py:40-565, td3.py:28-116, sac.py:35-222 and adapter/offpolicy_adapter.py.

    agent = omnisafe_amd.Agent('TD3', 'SynthNavGoal1-v0')
    agent.learn(); agent.evaluate()

The env, the ring, the networks and the draws all live on the device.  An epoch is enqueued on one stream with no host
read inside it: ``steps_per_epoch / (update_cycle num_envs)`` rounds of act -> ``env.step`` -> store -> (``update_iters``
gradient steps of td3_step.Td3Step once ``step > start_learning_steps``).  Episode returns, costs and lengths are
accumulated on the device and read once at the epoch's end together with the steps' statistics rows.

Deviations from the reference:
  * The env must be a device env (a built-in family or one of ``register_device_env``); a host env raises
    NotImplementedError.
  * ``obs_normalize``, ``reward_normalize``, ``cost_normalize`` and ``linear_lr_decay`` set to True raise
    NotImplementedError (the YAML default is False for all four); DDPGLag, TD3Lag, DDPGPID and TD3PID, whose YAMLs set
    ``cost_normalize: True``, take it: the normaliser runs inside the store launch.
  * One ring of ``size`` rows shared by the envs, written ``vector_env_nums`` rows at a time (the reference keeps
    ``size`` rows per env).
  * All draws (warm-up actions, exploration noise, minibatch indices, target-policy noise) are Philox streams on the
    device keyed by the seed and the step.
  * The epoch's evaluation plays its ``eval_episodes`` side by side through ``Evaluator``.
"""
from __future__ import annotations

import time

import torch

from .. import envs as envs_mod
from .. import sac_step, td3_step
from ..evaluator import Evaluator
from ..logger import Logger
from ..saved_policy import device_env_class
from .base_algo import BaseAlgo
from .registry import register

K = td3_step.STAT_KEYS


class BaseOffPolicy(BaseAlgo):  # pylint: disable=too-many-instance-attributes
    """ddpg.py:40-565 around a Td3Step."""

    num_critics = 1
    stat_keys = K           # the columns of a statistics row
    actor_cols = (2,)       # ... that only an actor step writes
    step_mod = td3_step     # make_desc and the step class come from here
    round_cols = ()         # ... that a launch after the round's last step writes: one value per round
    refused = ('obs_normalize', 'reward_normalize', 'cost_normalize', 'linear_lr_decay')

    def _hparams(self) -> dict:
        """DDPG: TD3 with one critic, no target-policy noise and the online actor in the target (ddpg.py:424)."""
        return dict(policy_noise=0.0, policy_noise_clip=0.0, target_actor=False)

    # ------------------------------------------------------------------ construction, in the reference's order
    def _init_env(self) -> None:
        """ddpg.py:51-92."""
        t, a, m = self._cfgs.train_cfgs, self._cfgs.algo_cfgs, self._cfgs.model_cfgs
        if device_env_class(self._env_id) is None:
            raise NotImplementedError(f'{self._env_id} is a host env: the off-policy family trains on device envs only '
                                      '(the built-in families and those of register_device_env)')
        for name, on in (('obs_normalize', a.obs_normalize), ('reward_normalize', a.reward_normalize),
                         ('cost_normalize', a.cost_normalize), ('linear_lr_decay', m.linear_lr_decay)):
            if on and name in self.refused:
                raise NotImplementedError(f'{name}=True is not implemented for the off-policy family')
        self._num_envs = int(t.vector_env_nums)
        env_cfgs = dict(self._cfgs.env_cfgs.todict()) if hasattr(self._cfgs, 'env_cfgs') else {}
        self._env = envs_mod.make(self._env_id, num_envs=self._num_envs, device=self._device, **env_cfgs)
        self._env.set_seed(self._seed)
        self._obs_dim, self._act_dim = (int(self._env.observation_space.shape[0]),
                                        int(self._env.action_space.shape[0]))
        assert a.steps_per_epoch % self._num_envs == 0, \
            'The number of steps per epoch is not divisible by the number of environments.'
        assert int(t.total_steps) % a.steps_per_epoch == 0, \
            'The total number of steps is not divisible by the number of steps per epoch.'
        self._epochs = int(t.total_steps) // a.steps_per_epoch
        self._steps_per_epoch = a.steps_per_epoch // self._num_envs
        self._update_cycle = int(a.update_cycle)
        assert self._steps_per_epoch % self._update_cycle == 0, \
            'The number of steps per epoch is not divisible by the number of steps per sample.'
        self._samples_per_epoch = self._steps_per_epoch // self._update_cycle

    def _init_model(self) -> None:
        """ddpg.py:94-133: actor, critics, targets, the ring."""
        m, a = self._cfgs.model_cfgs, self._cfgs.algo_cfgs
        m.critic.recurisve_update({'num_critics': self.num_critics})
        desc = self.step_mod.make_desc(self._obs_dim, self._act_dim, m.actor.hidden_sizes, m.critic.hidden_sizes,
                                  m.actor.activation, m.critic.activation, a.batch_size, self.num_critics, a.use_cost)
        self._nslots = self._samples_per_epoch * int(a.update_iters)
        self._step = self._make_step(
            desc, size=int(a.size), gamma=float(a.gamma), polyak=float(a.polyak), lr_actor=float(m.actor.lr),
            lr_critic=float(m.critic.lr), nslots=self._nslots, policy_delay=int(a.policy_delay),
            max_grad_norm=float(a.max_grad_norm or 0.0),
            critic_norm_coeff=float(a.critic_norm_coeff) if a.use_critic_norm else 0.0, device=self._device,
            **self._hparams())
        self._step.init_parameters(m.weight_initialization_mode)

    def _make_step(self, desc, **kw):
        return td3_step.Td3Step(desc, **kw)

    def _act_into(self, warm: bool) -> None:
        """The acting launch of one vector step: ``MLPActor.predict`` with the exploration noise, or the warm-up's
        uniform draw."""
        a = self._cfgs.algo_cfgs
        noise = float(a.exploration_noise) if a.use_exploration_noise else 0.0
        self._step.act(self._obs, noise=noise, random=warm, seed=self._seed, offset=self._env_steps, out=self._act)

    def _idle_row(self) -> list:
        """What a round before ``start_learning_steps`` logs (``_log_when_not_update``): zeros."""
        return [0.0] * len(self.stat_keys)

    def _init(self) -> None:
        f32 = dict(dtype=torch.float32, device=self._device)
        cap = self._samples_per_epoch * self._update_cycle * self._num_envs
        self._episodes = (torch.zeros(self._num_envs, 3, **f32), torch.zeros(cap, 3, **f32),
                          torch.zeros(1, dtype=torch.int64, device=self._device))
        self._act = torch.zeros(self._num_envs, self._act_dim, **f32)
        self._obs = None
        self._env_steps = 0     # vector steps taken: the Philox offset of the acting draws
        self.total_env_steps = 0
        self.epoch_stats: list = []  # per epoch: the rounds' statistics rows (zeros before learning starts)

    def _init_log(self) -> None:
        """ddpg.py:135-252."""
        lc, a = self._cfgs.logger_cfgs, self._cfgs.algo_cfgs
        self._logger = Logger(output_dir=lc.log_dir, exp_name=self._cfgs.exp_name, seed=self._cfgs.seed,
                              use_tensorboard=lc.use_tensorboard, use_wandb=lc.use_wandb, config=self._cfgs,
                              verbose=bool(getattr(lc, 'verbose', True)))
        self._logger.setup_torch_saver({'pi': self._step})
        self._logger.torch_save()
        keys = [('Metrics/EpRet', lc.window_lens), ('Metrics/EpCost', lc.window_lens), ('Metrics/EpLen', lc.window_lens)]
        if self._cfgs.train_cfgs.eval_episodes > 0:
            keys += [(k, lc.window_lens) for k in ('Metrics/TestEpRet', 'Metrics/TestEpCost', 'Metrics/TestEpLen')]
        keys += [(k, None) for k in ('Train/Epoch', 'Train/LR', 'TotalEnvSteps')]
        keys += [(self.stat_keys[col], None) for col in self._logged_cols()]
        keys += [(k, None) for k in ('Time/Total', 'Time/Rollout', 'Time/Update', 'Time/Evaluate', 'Time/Epoch',
                                     'Time/FPS')]
        for key, window in keys:
            self._logger.register_key(key, window_length=window)

    def _after_round(self, epoch: int) -> None:
        """What follows the gradient steps of an update round on the stream (the multiplier's launch)."""

    def _after_epoch(self, n_ep: int) -> None:
        """What follows the epoch's one read of the device; ``n_ep`` episodes finished in it."""

    def _logged_cols(self) -> list:
        """The statistics columns this run logs: the cost critic's with ``use_cost`` only."""
        return [0, 1, 2] + ([3, 4] if self._cfgs.algo_cfgs.use_cost else [])

    # ------------------------------------------------------------------ training
    def _train_epoch(self, epoch: int) -> tuple[torch.Tensor, int]:
        """ddpg.py:277-305 for one epoch, enqueued without a host read: the statistics slots used and the number of
        rounds that logged zeros."""
        a, st, env = self._cfgs.algo_cfgs, self._step, self._env
        first_update, idle = st.update_count, 0
        if self._obs is None:
            self._obs, _ = env.reset()
        for sample_step in range(epoch * self._samples_per_epoch, (epoch + 1) * self._samples_per_epoch):
            step = sample_step * self._update_cycle * self._num_envs
            warm = step <= a.start_learning_steps  # known from the counter alone: no device read
            for _ in range(self._update_cycle):
                self._act_into(warm)
                obs = self._obs
                self._obs, r, c, term, trunc, info = env.step(self._act)
                st.store(obs, self._act, r, c, term, trunc, self._obs, info.get('final_observation'),
                         info.get('_final_observation'), self._episodes)
                self._env_steps += 1
            if warm:
                idle += 1
                continue
            for _ in range(int(a.update_iters)):
                st.draw(self._seed, st.update_count, 1)  # after the store: the fill count is read on the device
                st.run(1)
            self._after_round(epoch)
        env.commit()
        slots = (torch.arange(st.update_count - first_update, device=self._device) + first_update) % self._nslots
        return slots, idle

    def learn(self) -> tuple[float, float, float]:
        """ddpg.py:254-348."""
        self._logger.log('INFO: Start training')
        a, spe = self._cfgs.algo_cfgs, int(self._cfgs.algo_cfgs.steps_per_epoch)
        keys, idle_row = self.stat_keys, torch.tensor(self._idle_row())
        start_time = time.time()
        try:
            for epoch in range(self._epochs):
                epoch_time = time.time()
                slots, idle = self._train_epoch(epoch)
                # the epoch's one read of the device: the steps' rows, the finished episodes
                rows = self._step.stats[slots][:, :len(keys)].cpu() if slots.numel() else torch.zeros(0, len(keys))
                n_ep = int(self._episodes[2].cpu())
                eps = self._episodes[1][:min(n_ep, self._episodes[1].shape[0])].cpu()
                self._after_epoch(min(n_ep, self._episodes[1].shape[0]))
                self._episodes[2].zero_()
                update_time = time.time() - epoch_time
                iters, delay = int(a.update_iters), int(a.policy_delay)
                first = self._step.update_count - rows.shape[0]
                actor_rows = [(first + i + 1) % delay == 0 for i in range(rows.shape[0])]
                per_round = idle_row.repeat(idle + rows.shape[0] // iters, 1)
                if rows.shape[0]:
                    per_round[idle:] = rows[iters - 1::iters]
                self.epoch_stats.append(per_round.tolist())
                for col in self._logged_cols():
                    vals = [float(idle_row[col])] * idle + [float(v) for i, v in enumerate(rows[:, col].tolist())
                                                            if (col not in self.actor_cols or actor_rows[i])
                                                            and (col not in self.round_cols or (i + 1) % iters == 0)]
                    self._logger.extend(keys[col], vals or [0.0])
                for k, col in (('Metrics/EpRet', 0), ('Metrics/EpCost', 1), ('Metrics/EpLen', 2)):
                    self._logger.extend(k, eps[:, col].tolist())
                eval_start = time.time()
                self._evaluate()
                env_steps = (epoch + 1) * spe
                self.total_env_steps = env_steps
                self._logger.store({'Time/Update': update_time, 'Time/Rollout': 0.0,
                                    'Time/Evaluate': time.time() - eval_start, 'TotalEnvSteps': env_steps,
                                    'Time/FPS': spe / (time.time() - epoch_time), 'Time/Total': time.time() - start_time,
                                    'Time/Epoch': time.time() - epoch_time, 'Train/Epoch': epoch,
                                    'Train/LR': float(self._cfgs.model_cfgs.actor.lr)})
                ep_ret, ep_cost, ep_len = (self._logger.get_stats(k)[0] for k in
                                           ('Metrics/EpRet', 'Metrics/EpCost', 'Metrics/EpLen'))
                self._logger.dump_tabular()
                if (epoch + 1) % self._cfgs.logger_cfgs.save_model_freq == 0:
                    self._logger.torch_save()
        finally:
            self._logger.close()
            self._env.close()
        return ep_ret, ep_cost, ep_len

    def _evaluate(self) -> None:
        """offpolicy_adapter.py:71-117: ``eval_episodes`` deterministic episodes of the current actor."""
        n = int(self._cfgs.train_cfgs.eval_episodes)
        if n <= 0:
            return
        if not hasattr(self, '_evaluator'):
            self._evaluator = Evaluator(seed=self._seed, device=self._device, verbose=False)
        ev = self._evaluator
        ev.load_policy(self._cfgs.todict(), {'pi': self._step.state_dict()})
        rets, costs = ev.evaluate(num_episodes=n)
        self._logger.extend('Metrics/TestEpRet', [float(x) for x in rets])
        self._logger.extend('Metrics/TestEpCost', [float(x) for x in costs])
        self._logger.extend('Metrics/TestEpLen', [float(x) for x in ev.episode_lengths])


@register
class DDPG(BaseOffPolicy):
    """Deep Deterministic Policy Gradient (ddpg.py:40-565)."""


@register
class TD3(BaseOffPolicy):
    """Twin Delayed DDPG (td3.py:28-116): two reward critics, the target actor with clipped noise in the target."""

    num_critics = 2

    def _hparams(self) -> dict:
        a = self._cfgs.algo_cfgs
        return dict(policy_noise=float(a.policy_noise), policy_noise_clip=float(a.policy_noise_clip), target_actor=True)


@register
class SAC(BaseOffPolicy):
    """Soft Actor-Critic (sac.py:35-222): a tanh-squashed Gaussian actor that acts stochastically while training, the
    entropy term in the reward target, the min over both critics in the actor loss and, with ``auto_alpha``, the
    temperature step -- sac_step.SacStep.  ``use_exploration_noise`` has no effect, as in the reference's Gaussian
    actor, whose ``predict`` has no noise argument."""

    num_critics = 2
    stat_keys = sac_step.STAT_KEYS
    actor_cols = (2, 5, 6)  # (sac.py:163-183 stores Value/alpha and Loss/alpha_loss inside _update_actor)
    step_mod = sac_step

    def _hparams(self) -> dict:
        a = self._cfgs.algo_cfgs
        return dict(alpha=float(a.alpha), auto_alpha=bool(a.auto_alpha))

    def _make_step(self, desc, **kw):
        return sac_step.SacStep(desc, **kw)

    def _act_into(self, warm: bool) -> None:
        self._step.act(self._obs, mode=sac_step.ACT_UNIFORM if warm else sac_step.ACT_SAMPLE, seed=self._seed,
                       offset=self._env_steps, out=self._act)

    def _idle_row(self) -> list:
        """sac.py:209-222: zeros, and the temperature as it stands -- the initial one, known on the host, since no
        round idles once learning has started."""
        a = self._cfgs.algo_cfgs
        row = [0.0] * len(self.stat_keys)
        row[5] = 1.0 if a.auto_alpha else float(a.alpha)
        return row

    def _logged_cols(self) -> list:
        return super()._logged_cols() + [5] + ([6] if self._cfgs.algo_cfgs.auto_alpha else [])


class _OffPolicyLag(BaseOffPolicy):
    """What DDPGLag, TD3Lag, DDPGPID and TD3PID add to their base (ddpg_lag.py:38-112 and its three siblings): the cost
    critic in the actor loss, ``cost_normalize`` and the multiplier -- all on the device (td3_step.Td3LagStep).  After
    every update round of an epoch > ``warmup_epochs`` one launch takes the multiplier's step on the mean cost of the
    last ``window_lens`` finished episodes: a carry of the earlier epochs' tail, refreshed on the device after the
    epoch's one read, followed by the running epoch's episodes.

    Deviation: while no episode has finished, the step is skipped (the reference averages an empty window: nan)."""

    stat_keys = td3_step.LAG_STAT_KEYS
    round_cols = (5,)
    refused = ('obs_normalize', 'reward_normalize', 'linear_lr_decay')

    def _init_env(self) -> None:
        td3_step.check_lagrange_cfgs(self._cfgs.lagrange_cfgs.todict())  # (before any GPU is touched)
        self._cfgs.algo_cfgs.recurisve_update({'use_cost': True})
        super()._init_env()

    def _make_step(self, desc, **kw):
        return td3_step.Td3LagStep(desc, lagrange_cfgs=self._cfgs.lagrange_cfgs.todict(),
                                   window_lens=int(self._cfgs.logger_cfgs.window_lens),
                                   cost_normalize=bool(self._cfgs.algo_cfgs.cost_normalize), **kw)

    def _init(self) -> None:
        super()._init()
        self._carry = torch.zeros(int(self._cfgs.logger_cfgs.window_lens), dtype=torch.float32, device=self._device)
        self._ncarry = 0

    def _idle_row(self) -> list:
        """``_log_when_not_update``: the multiplier as it stands -- the initial one, since no round idles once learning
        has started."""
        row = super()._idle_row()
        row[5] = self._step.initial_multiplier
        return row

    def _logged_cols(self) -> list:
        return super()._logged_cols() + [5]

    def _after_round(self, epoch: int) -> None:
        self._step.update_multiplier(self._carry, self._ncarry, self._episodes,
                                     update=epoch > int(self._cfgs.algo_cfgs.warmup_epochs))

    def _after_epoch(self, n_ep: int) -> None:
        window = self._carry.shape[0]
        tail = torch.cat([self._carry[:self._ncarry], self._episodes[1][:n_ep, 1]])[-window:]
        self._ncarry = int(tail.shape[0])
        self._carry[:self._ncarry] = tail


@register
class DDPGLag(_OffPolicyLag):
    """DDPG with a Lagrange multiplier (ddpg_lag.py:28-112)."""


@register
class TD3Lag(_OffPolicyLag):
    """TD3 with a Lagrange multiplier (td3_lag.py:28-112)."""

    num_critics = 2
    _hparams = TD3._hparams  # noqa: SLF001


@register
class DDPGPID(_OffPolicyLag):
    """DDPG with a PID-controlled multiplier (ddpg_pid.py:28-111)."""


@register
class TD3PID(_OffPolicyLag):
    """TD3 with a PID-controlled multiplier (td3_pid.py:28-111)."""

    num_critics = 2
    _hparams = TD3._hparams  # noqa: SLF001


__all__ = ['BaseOffPolicy', 'DDPG', 'TD3', 'SAC', 'DDPGLag', 'TD3Lag', 'DDPGPID', 'TD3PID']
