"""Device time of one vector step of the SynthNavCircle envs next to SynthReach's and SynthNavGoal0's, in the same
process.

    python tools/circle_env_timing.py [--n 4096] [--steps 1000] [--reps 5] [--variant-lib PATH]

(1) env step alone: `--steps` calls of env.step() captured as one hipGraph (the form the rollout runs them in), replayed
    after a warm-up replay; HIP events around a replay, median and min / max of `--reps` replays, divided by `--steps`.
    Also the same launches issued eagerly back to back (includes what the host adds when it cannot keep ahead).
(2) env-steps/s of whole PPOLag epochs at the BASELINE config-2 sizes (4096 envs x 16 steps) on SynthNavCircle1-v0 and
    on SynthPointGoal1-v0.
--variant-lib: a build of the library with another lane mapping of osa_circle_env_kernel<OsaPoint, LANES>
    (tools/build_variant_lib.sh wave64 rollout_kernels.hip -DOSA_CIRCLE_LANES=64: one wave per env); part (1) for the
    Circle ids is repeated on it in a child process (OSA_LIB_PATH) and reported as `env_step_variant`.
Prints one JSON line (profiles/circle_env_timing.json)."""
from __future__ import annotations

import argparse
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
CIRCLE = ['SynthNavCircle0-v0', 'SynthNavCircle1-v0', 'SynthNavCircle2-v0']
ENVS = ['SynthReach-v0', 'SynthNavGoal0-v0'] + CIRCLE


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


def end_to_end_row(env_id: str, n: int, t_steps: int, warm: int = 3, epochs: int = 5) -> dict:
    """env-steps/s of whole epochs (rollout + update, the reference's Time/FPS) at the BASELINE config-2 sizes, as
    tools/baseline_configs.py measures them (YAML defaults, kl_early_stop off = maximum work)."""
    cfg = {'seed': 0,
           'train_cfgs': {'device': DEV, 'vector_env_nums': n, 'total_steps': n * t_steps * (warm + epochs + 1)},
           'algo_cfgs': {'steps_per_epoch': n * t_steps, 'kl_early_stop': False},
           'logger_cfgs': {'log_dir': tempfile.mkdtemp(prefix='osa_circle_timing_'), 'save_model_freq': 10 ** 9,
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
    ap.add_argument('--variant-lib', default='')
    ap.add_argument('--env-step-only', default='', help='comma-separated ids: part (1) for these alone')
    args = ap.parse_args()
    ids = args.env_step_only.split(',') if args.env_step_only else ENVS
    rows = [env_step_row(e, args.n, args.steps, args.reps) for e in ids]
    for r in rows:
        print(json.dumps(r), file=sys.stderr, flush=True)
    out = {'tool': 'circle_env_timing', 'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'env_step': rows}
    if not args.env_step_only:
        out['end_to_end'] = [end_to_end_row(e, args.n, 16) for e in ('SynthPointGoal1-v0', 'SynthNavCircle1-v0')]
    if args.variant_lib:  # a fresh process: the library is bound once per process
        child = subprocess.run(
            [sys.executable, os.path.abspath(__file__), '--n', str(args.n), '--steps', str(args.steps), '--reps',
             str(args.reps), '--env-step-only', ','.join(CIRCLE)],
            env=dict(os.environ, OSA_LIB_PATH=os.path.abspath(args.variant_lib)), check=True, capture_output=True,
            text=True)
        out['env_step_variant'] = {'lib': os.path.basename(args.variant_lib),
                                   'rows': json.loads(child.stdout.strip().split('\n')[-1])['env_step']}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
