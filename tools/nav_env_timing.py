"""Device time of one vector step of the SynthNavGoal envs next to SynthReach's, in the same process.

    python tools/nav_env_timing.py [--n 4096] [--steps 1000] [--reps 5] [--rollout-steps 100]

(1) env step alone: `--steps` calls of env.step() captured as one hipGraph (the form the rollout runs them in), replayed
    after a warm-up replay; HIP events around a replay, median of `--reps` replays, divided by `--steps`.  Also the same
    launches issued eagerly back to back (includes what the host adds when it cannot keep ahead).
(2) the whole vector step of OnPolicyAdapter.rollout (PPOLag: policy step, env step, normaliser push, normalise,
    accounting; captured graph) on SynthNavGoal1-v0 and on SynthPointGoal1-v0: events around epochs 3 .. 2 + reps.
(3) env-steps/s of whole PPOLag epochs at the BASELINE config-2 sizes (4096 envs x 16 steps) on the same two envs.
Prints one JSON line (profiles/nav_env_timing.json).  Under `rocprofv3 --kernel-trace --stats -- python ...` the
per-kernel split of the same run."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import omnisafe_amd  # noqa: E402
from omnisafe_amd import envs  # noqa: E402

DEV = 'cuda:0'
ENVS = ['SynthReach-v0', 'SynthNavGoal0-v0', 'SynthNavGoal1-v0', 'SynthNavGoal2-v0']


def timed(fn, reps: int) -> list[float]:
    """Milliseconds of `reps` calls of fn(), each between two HIP events."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def env_step_row(env_id: str, n: int, steps: int, reps: int) -> dict:
    env = envs.make(env_id, num_envs=n, device=DEV, horizon=1000, seed=0)
    env.reset()
    act = (torch.randn(n, 2, generator=torch.Generator(device='cpu').manual_seed(0)) * 1.5).to(DEV)

    def run():
        for _ in range(steps):
            env.step(act)

    run()  # warm-up: code objects
    torch.cuda.synchronize()
    eager = timed(run, reps)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            run()
        graph.replay()
        stream.synchronize()
        graphed = timed(graph.replay, reps)
    return {'env': env_id, 'n': n, 'steps': steps,
            'graph_us_per_step': round(1e3 * statistics.median(graphed) / steps, 3),
            'graph_us_per_step_min_max': [round(1e3 * min(graphed) / steps, 3), round(1e3 * max(graphed) / steps, 3)],
            'eager_us_per_step': round(1e3 * statistics.median(eager) / steps, 3)}


def rollout_row(env_id: str, n: int, t_steps: int, reps: int) -> dict:
    cfg = {'seed': 0, 'train_cfgs': {'device': DEV, 'total_steps': (2 + reps) * n * t_steps, 'vector_env_nums': n},
           'algo_cfgs': {'steps_per_epoch': n * t_steps},
           'logger_cfgs': {'log_dir': tempfile.mkdtemp(prefix='osa_nav_timing_'), 'verbose': False},
           'env_cfgs': {'horizon': t_steps}}  # every epoch ends its episodes (EpCost feeds the multiplier)
    algo = omnisafe_amd.Agent('PPOLag', env_id, custom_cfgs=cfg).agent

    def epoch():
        algo._env.rollout(steps_per_epoch=algo._steps_per_epoch, agent=algo._actor_critic, buffer=algo._buf,
                          logger=algo._logger)

    ms = []
    for e in range(2 + reps):  # the second epoch captures the graph; the update between rollouts is not timed
        torch.cuda.synchronize()
        t = timed(epoch, 1)
        if e >= 2:
            ms += t
        algo._update()
        algo._logger.dump_tabular()
    assert algo._env.last_rollout_graphed
    return {'env': env_id, 'n': n, 'vector_steps_per_epoch': t_steps,
            'rollout_us_per_vector_step': round(1e3 * statistics.median(ms) / t_steps, 2),
            'rollout_us_per_vector_step_min_max': [round(1e3 * min(ms) / t_steps, 2),
                                                   round(1e3 * max(ms) / t_steps, 2)]}


def end_to_end_row(env_id: str, n: int, t_steps: int, warm: int = 3, epochs: int = 5) -> dict:
    """env-steps/s of whole epochs (rollout + update, the reference's Time/FPS) at the BASELINE config-2 sizes, as
    tools/baseline_configs.py measures them (YAML defaults, kl_early_stop off = maximum work)."""
    import time

    cfg = {'seed': 0, 'train_cfgs': {'device': DEV, 'vector_env_nums': n, 'total_steps': n * t_steps * (warm + epochs + 1)},
           'algo_cfgs': {'steps_per_epoch': n * t_steps, 'kl_early_stop': False},
           'logger_cfgs': {'log_dir': tempfile.mkdtemp(prefix='osa_nav_timing_'), 'save_model_freq': 10 ** 9,
                           'verbose': False},
           'env_cfgs': {'horizon': t_steps}}
    a = omnisafe_amd.Agent('PPOLag', env_id, custom_cfgs=cfg).agent

    def run(k):
        for _ in range(k):
            a._env.rollout(steps_per_epoch=a._steps_per_epoch, agent=a._actor_critic, buffer=a._buf, logger=a._logger)
            a._update()
            a._logger.dump_tabular()
        torch.cuda.synchronize()

    run(warm)
    t0 = time.perf_counter()
    run(epochs)
    dt = (time.perf_counter() - t0) / epochs
    return {'env': env_id, 'n': n, 'steps_per_env': t_steps, 'ms_per_epoch': round(dt * 1e3, 2),
            'env_steps_per_s': round(n * t_steps / dt, 1), 'update_path': getattr(a._updater, 'last_path', None)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rollout-steps', type=int, default=100)
    args = ap.parse_args()
    rows = [env_step_row(e, args.n, args.steps, args.reps) for e in ENVS]
    for r in rows:
        print(json.dumps(r), file=sys.stderr, flush=True)
    rollouts = [rollout_row(e, args.n, args.rollout_steps, args.reps)
                for e in ('SynthPointGoal1-v0', 'SynthNavGoal1-v0')]
    e2e = [end_to_end_row(e, args.n, 16) for e in ('SynthPointGoal1-v0', 'SynthNavGoal1-v0')]
    print(json.dumps({'tool': 'nav_env_timing', 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
                      'env_step': rows, 'rollout': rollouts, 'end_to_end': e2e}))


if __name__ == '__main__':
    main()
