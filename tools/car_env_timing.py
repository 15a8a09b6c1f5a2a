"""Device time of one vector step of the Car envs next to the point envs of the same task and level, in the same
process.

    python tools/car_env_timing.py [--n 4096] [--steps 1000] [--reps 5] [--variant-lib PATH] [--learning]

(1) env step alone: `--steps` calls of env.step() captured as one hipGraph (the form the rollout runs them in), replayed
    after a warm-up replay; HIP events around a replay, median and min / max of `--reps` replays, divided by `--steps`.
    Also the same launches issued eagerly back to back (includes what the host adds when it cannot keep ahead).
    Every Car row carries `ratio_to_point` (its median over the point env's of the same level in this run) next to
    `row_bytes_ratio` (72 / 60 or 40 / 28), the gap the wider observation row alone would explain.
(2) env-steps/s of whole CPO epochs at the BASELINE config-3 sizes (4096 envs x 16 steps) on SynthNavCarGoal1-v0 and on
    the noise env of the same shape, SynthCarGoal1-v0.
--variant-lib: a build of the library with one wave per env in osa_circle_env_kernel<OsaCar, LANES>
    (tools/build_variant_lib.sh carwave64 rollout_kernels.hip -DOSA_CAR_CIRCLE_LANES=64); part (1) for the CarCircle ids
    is repeated on it in a child process (OSA_LIB_PATH) and reported as `env_step_variant`.
--learning: seed-mean EpRet / EpCost per epoch of 4 seeds in one AgentGroup (256 envs, horizon 200, 10 epochs of
    51 200 steps): PPO on SynthNavCarGoal0-v0 and PPOLag on SynthNavCarCircle1-v0 (YAML cost_limit 25), reported as
    `learning` (profiles/car_learning.md).
Prints one JSON line (profiles/car_env_timing.json)."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import omnisafe_amd  # noqa: E402
from omnisafe_amd import envs  # noqa: E402

DEV = 'cuda:0'
CAR_CIRCLE = [f'SynthNavCarCircle{k}-v0' for k in range(3)]
POINT_OF = {**{f'SynthNavCarGoal{k}-v0': f'SynthNavGoal{k}-v0' for k in range(3)},
            **{f'SynthNavCarCircle{k}-v0': f'SynthNavCircle{k}-v0' for k in range(3)}}
ENVS = [e for pair in ((p, c) for c, p in POINT_OF.items()) for e in pair]


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
    return {'env': env_id, 'n': n, 'steps': steps, 'obs_dim': int(env.observation_space.shape[0]),
            'graph_us_per_step': round(1e3 * statistics.median(graphed) / steps, 3),
            'graph_us_per_step_min_max': [round(1e3 * min(graphed) / steps, 3), round(1e3 * max(graphed) / steps, 3)],
            'eager_us_per_step': round(1e3 * statistics.median(eager) / steps, 3)}


def end_to_end_row(env_id: str, n: int, t_steps: int, warm: int = 3, epochs: int = 5) -> dict:
    """env-steps/s of whole CPO epochs (rollout + update, the reference's Time/FPS) at the BASELINE config-3 sizes, as
    tools/baseline_configs.py measures them (YAML defaults)."""
    cfg = {'seed': 0,
           'train_cfgs': {'device': DEV, 'vector_env_nums': n, 'total_steps': n * t_steps * (warm + epochs + 1)},
           'algo_cfgs': {'steps_per_epoch': n * t_steps},
           'logger_cfgs': {'log_dir': tempfile.mkdtemp(prefix='osa_car_timing_'), 'save_model_freq': 10 ** 9,
                           'verbose': False},
           'env_cfgs': {'horizon': t_steps}}
    a = omnisafe_amd.Agent('CPO', env_id, custom_cfgs=cfg).agent

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
    return {'algo': 'CPO', 'env': env_id, 'n': n, 'steps_per_env': t_steps, 'ms_per_epoch': round(dt * 1e3, 2),
            'env_steps_per_s': round(n * t_steps / dt, 1)}


def learning_row(algo: str, env_id: str, seeds: int = 4, n: int = 256, horizon: int = 200, epochs: int = 10) -> dict:
    custom = {'train_cfgs': {'device': DEV, 'total_steps': n * horizon * epochs, 'vector_env_nums': n},
              'algo_cfgs': {'steps_per_epoch': n * horizon},
              'logger_cfgs': {'log_dir': tempfile.mkdtemp(prefix='osa_car_learning_'), 'verbose': False,
                              'save_model_freq': 10 ** 9},
              'env_cfgs': {'horizon': horizon}}
    group = omnisafe_amd.AgentGroup(algo, env_id, seeds=list(range(seeds)), custom_cfgs=custom)
    t0 = time.perf_counter()
    group.learn()
    dt = time.perf_counter() - t0
    ret, cost = [], []
    for member in group.agents:
        rows = list(csv.DictReader(open(os.path.join(member.agent.logger.log_dir, 'progress.csv'))))
        ret.append([float(r['Metrics/EpRet']) for r in rows])
        cost.append([float(r['Metrics/EpCost']) for r in rows])
    ret_t, cost_t = torch.tensor(ret, dtype=torch.float64), torch.tensor(cost, dtype=torch.float64)

    def tail_minus_first(x):
        d = x[:, -3:].mean(1) - x[:, 0]
        return [round(float(d.mean()), 3), round(float(d.std(unbiased=True) / seeds ** 0.5), 3)]

    return {'algo': algo, 'env': env_id, 'seeds': seeds, 'n': n, 'horizon': horizon, 'epochs': epochs,
            'seconds': round(dt, 2), 'EpRet': [round(v, 3) for v in ret_t.mean(0).tolist()],
            'EpCost': [round(v, 3) for v in cost_t.mean(0).tolist()],
            'EpRet_tail_minus_first_and_se': tail_minus_first(ret_t),
            'EpCost_tail_minus_first_and_se': tail_minus_first(cost_t)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--variant-lib', default='')
    ap.add_argument('--learning', action='store_true')
    ap.add_argument('--env-step-only', default='', help='comma-separated ids: part (1) for these alone')
    args = ap.parse_args()
    ids = args.env_step_only.split(',') if args.env_step_only else ENVS
    rows = [env_step_row(e, args.n, args.steps, args.reps) for e in ids]
    by_id = {r['env']: r for r in rows}
    for r in rows:
        point = by_id.get(POINT_OF.get(r['env'], ''))
        if point:
            r['ratio_to_point'] = round(r['graph_us_per_step'] / point['graph_us_per_step'], 3)
            r['row_bytes_ratio'] = round(r['obs_dim'] / point['obs_dim'], 3)
        print(json.dumps(r), file=sys.stderr, flush=True)
    out = {'tool': 'car_env_timing', 'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'env_step': rows}
    if not args.env_step_only:
        out['end_to_end'] = [end_to_end_row(e, args.n, 16) for e in ('SynthCarGoal1-v0', 'SynthNavCarGoal1-v0')]
    if args.learning:
        out['learning'] = [learning_row('PPO', 'SynthNavCarGoal0-v0'), learning_row('PPOLag', 'SynthNavCarCircle1-v0')]
    if args.variant_lib:  # a fresh process: the library is bound once per process
        child = subprocess.run(
            [sys.executable, os.path.abspath(__file__), '--n', str(args.n), '--steps', str(args.steps), '--reps',
             str(args.reps), '--env-step-only', ','.join(CAR_CIRCLE)],
            env=dict(os.environ, OSA_LIB_PATH=os.path.abspath(args.variant_lib)), check=True, capture_output=True,
            text=True)
        out['env_step_variant'] = {'lib': os.path.basename(args.variant_lib),
                                   'rows': json.loads(child.stdout.strip().split('\n')[-1])['env_step']}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
