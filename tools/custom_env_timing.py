"""Device time of one vector step of device envs registered from a header (register_device_env), next to the built-in
SynthReach-v0, in the same process.

    python tools/custom_env_timing.py [--n 4096] [--steps 1000] [--reps 5] [--build-only]

Rows: SynthReach-v0 (osa_reach_env_kernel: one wave per env, 60-column rows); the same description through the generic
kernel osa_custom_env_kernel at 16 / 32 / 64 lanes per env with the same 60-column row (tools/custom_envs/reach_lanes.h)
and with its 6 native columns; the example env of the tests (tests/custom_envs/glider.h: 70 columns, 3 actions).
Each: `--steps` calls of env.step() captured as one hipGraph (the form the rollout runs them in), replayed after a
warm-up replay; HIP events around a replay, median and min / max of `--reps` replays, divided by `--steps`; also the
same launches issued eagerly back to back.  --build-only compiles the libraries and stops (no GPU needed).
Prints one JSON line (profiles/custom_env_timing.json)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import omnisafe_amd  # noqa: E402
from omnisafe_amd import envs  # noqa: E402

DEV = 'cuda:0'
REACH = os.path.join(ROOT, 'tools', 'custom_envs', 'reach_lanes.h')
GLIDER = os.path.join(ROOT, 'tests', 'custom_envs', 'glider.h')
CUSTOM = [(REACH, 'ReachWide16'), (REACH, 'ReachWide32'), (REACH, 'ReachWide64'), (REACH, 'Reach6'),
          (GLIDER, 'Glider')]


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
    obs_dim, act_dim = env.observation_space.shape[0], env.action_space.shape[0]
    act = (torch.randn(n, act_dim, generator=torch.Generator(device='cpu').manual_seed(0)) * 1.5).to(DEV)

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
    return {'env': env_id, 'kernel': 'osa_custom_env_kernel' if isinstance(env, envs.CustomDeviceEnv) else 'built-in',
            'lanes_per_env': getattr(env, 'lanes', 64), 'obs_columns': obs_dim, 'act_columns': act_dim, 'n': n,
            'steps': steps, 'graph_us_per_step': round(1e3 * statistics.median(graphed) / steps, 3),
            'graph_us_per_step_min_max': [round(1e3 * min(graphed) / steps, 3), round(1e3 * max(graphed) / steps, 3)],
            'eager_us_per_step': round(1e3 * statistics.median(eager) / steps, 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--build-only', action='store_true')
    args = ap.parse_args()
    ids = ['SynthReach-v0']
    for header, struct in CUSTOM:
        omnisafe_amd.register_device_env(header, struct, [struct + '-v0'])
        ids.append(struct + '-v0')
    if args.build_only:
        print(json.dumps({'built': [envs.CUSTOM_ENV_REGISTRY[e].lib_path for e in ids[1:]]}))
        return
    rows = [env_step_row(e, args.n, args.steps, args.reps) for e in ids]
    for r in rows:
        print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({'tool': 'custom_env_timing', 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
                      'env_step': rows}))


if __name__ == '__main__':
    main()
