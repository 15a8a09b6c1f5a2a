"""What runtime parameters cost a custom device env per vector step (include/omnisafe_amd_env.h, PARAMETERS).

    python tools/custom_param_timing.py [--n 4096] [--steps 1000] [--reps 5] [--runs 3] [--parent DIR] [--build-only]

Rows, each measured in `--runs` fresh processes that take turns (so the spread between runs is seen next to every
difference): `Gust` of tests/custom_envs/gust.h (four runtime parameters: the row load, bind() and at a reset the
redraw), `GustFixed` (the same description with the four values as compile-time constants), `Glider`
(tests/custom_envs/glider.h, no parameters) on this tree and -- with `--parent DIR`, a built checkout of the parent
commit -- on the parent's package, whose generic kernel has no parameter code at all.
A run: `--steps` calls of env.step() at horizon 1000 captured as one hipGraph, replayed after a warm-up replay; HIP
events around a replay, median of `--reps` replays, divided by `--steps` (tools/custom_env_timing.py's form).
--build-only compiles this tree's libraries and stops (no GPU needed).
Prints one JSON line (profiles/custom_param_timing.json)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [('Gust', 'gust.h'), ('GustFixed', 'gust.h'), ('Glider', 'glider.h')]


def child(root: str, struct: str, header: str, n: int, steps: int, reps: int) -> None:
    """One run of one row with the package of `root`; prints its JSON."""
    sys.path.insert(0, root)
    import torch

    import omnisafe_amd
    from omnisafe_amd import envs

    omnisafe_amd.register_device_env(header, struct, [struct + '-v0'])
    env = envs.make(struct + '-v0', num_envs=n, device='cuda:0', horizon=1000, seed=0)
    env.reset()
    act_dim = env.action_space.shape[0]
    act = (torch.randn(n, act_dim, generator=torch.Generator(device='cpu').manual_seed(0)) * 1.5).to('cuda:0')

    def run():
        for _ in range(steps):
            env.step(act)

    run()  # warm-up: code objects
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    ms = []
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            run()
        graph.replay()
        stream.synchronize()
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
    print(json.dumps({'us_per_step': round(1e3 * statistics.median(ms) / steps, 3),
                      'params': len(getattr(env, 'param_names', ())), 'device': torch.cuda.get_device_name(0)}))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--build-only', action='store_true')
    ap.add_argument('--child', nargs=3, metavar=('ROOT', 'STRUCT', 'HEADER'))
    args = ap.parse_args()
    if args.child:
        child(*args.child, args.n, args.steps, args.reps)
        return
    examples = os.path.join(ROOT, 'tests', 'custom_envs')
    if args.build_only:
        sys.path.insert(0, ROOT)
        from omnisafe_amd import build

        print(json.dumps({'built': [build.build_custom_env(os.path.join(examples, h), s) for s, h in ROWS]}))
        return
    jobs = [(s, ROOT, 'this commit', os.path.join(examples, h)) for s, h in ROWS]
    if args.parent:
        parent = os.path.abspath(args.parent)
        jobs.append(('Glider', parent, 'parent commit', os.path.join(parent, 'tests', 'custom_envs', 'glider.h')))
    runs: dict = {(s, where): [] for s, _, where, _ in jobs}
    device = None
    for _ in range(args.runs):  # the rows take turns, one fresh process each
        for struct, root, where, header in jobs:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', root, struct, header, '--n', str(args.n),
                   '--steps', str(args.steps), '--reps', str(args.reps)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=300)
            row = json.loads(done.stdout.strip().splitlines()[-1])
            device = row['device']
            runs[(struct, where)].append(row['us_per_step'])
    rows = [{'env': s, 'package': where, 'us_per_step_runs': v, 'us_per_step': round(statistics.median(v), 3),
             'run_to_run_spread': round(max(v) - min(v), 3)} for (s, where), v in runs.items()]
    for r in rows:
        print(json.dumps(r), file=sys.stderr, flush=True)
    by = {(r['env'], r['package']): r for r in rows}
    out = {'tool': 'custom_param_timing', 'device': device, 'n': args.n, 'steps': args.steps, 'reps': args.reps,
           'runs': args.runs, 'rows': rows,
           'params_cost_us_per_step': round(by[('Gust', 'this commit')]['us_per_step']
                                            - by[('GustFixed', 'this commit')]['us_per_step'], 3)}
    if args.parent:
        here, there = by[('Glider', 'this commit')], by[('Glider', 'parent commit')]
        spread = max(here['run_to_run_spread'], there['run_to_run_spread'])
        diff = round(here['us_per_step'] - there['us_per_step'], 3)
        out['glider_against_parent'] = {'difference_us_per_step': diff, 'run_to_run_spread': spread,
                                        'within_spread': abs(diff) <= spread}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
