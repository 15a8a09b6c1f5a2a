"""Device time of one vector step of custom device envs with an object row in LDS (LDS_ROW = true: the generic row
kernel osa_custom_row_env_kernel, csrc/env_frame.h), next to the built-in Goal kernels, in the same process.

    python tools/custom_row_env_timing.py [--n 4096] [--steps 1000] [--reps 5] [--runs 3] [--parent DIR] [--build-only]

`env_step` rows: SynthNavGoal{0,1,2}-v0 and SynthNavCarGoal{0,1,2}-v0 (osa_goal_env_kernel: one wave per env, a
lane-per-object pass ahead of the columns); the same descriptions re-declared out of tree
(tests/custom_envs/goal_again.h) through the generic row kernel at 16 / 32 / 64 lanes per env; the Button example
(tests/custom_envs/button.h) on both robots and all levels at the default lane count; Field (tests/custom_envs/field.h:
150 state floats, 73 discs) at 16 / 32 / 64 lanes.  Each: `--steps` calls of env.step() at horizon 1000 captured as
one hipGraph, replayed after a warm-up replay; HIP events around a replay, median and min / max of `--reps` replays,
divided by `--steps` (tools/custom_env_timing.py's form).  `fastest_lanes`: per Goal description and level, the lane count with
the least median.
`against_parent` (with `--parent DIR`, a built checkout of the parent commit): Glider (tests/custom_envs/glider.h, the
register-state kernel) and SynthNavGoal1-v0 on this tree and on the parent's package, `--runs` fresh processes each
taking turns; the difference next to the run-to-run spread.
--build-only compiles this tree's libraries and stops (no GPU needed).
Prints one JSON line (profiles/custom_row_env_timing.json)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = os.path.join(ROOT, 'tests', 'custom_envs')
GOALS = [('GoalAgain', 'SynthNavGoal'), ('CarGoalAgain', 'SynthNavCarGoal')]
PARENT_ROWS = [('Glider', 'glider.h'), ('SynthNavGoal1-v0', None)]


def custom_structs() -> list[tuple[str, str, int]]:
    """(header, struct, highest level) of every custom row."""
    out = [('goal_again.h', f'{name}{lanes}', 2) for name, _ in GOALS for lanes in (16, 32, 64)]
    out += [('button.h', 'Button', 2), ('button.h', 'CarButton', 2)]
    return out + [('field.h', 'Field16', 0), ('field.h', 'Field32', 0), ('field.h', 'Field64', 0)]


def graph_us_per_step(env, n: int, steps: int, reps: int) -> list[float]:
    """Microseconds per env.step() of `reps` replays of a graph of `steps` steps."""
    import torch

    env.reset()
    act_dim = env.action_space.shape[0]
    act = (torch.randn(n, act_dim, generator=torch.Generator(device='cpu').manual_seed(0)) * 1.5).to('cuda:0')

    def run():
        for _ in range(steps):
            env.step(act)

    run()  # warm-up: code objects
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    us = []
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
            us.append(1e3 * a.elapsed_time(b) / steps)
    return us


def env_step_row(env_id: str, n: int, steps: int, reps: int) -> dict:
    from omnisafe_amd import envs

    env = envs.make(env_id, num_envs=n, device='cuda:0', horizon=1000, seed=0)
    us = graph_us_per_step(env, n, steps, reps)
    custom = isinstance(env, envs.CustomDeviceEnv)
    return {'env': env_id, 'kernel': 'osa_custom_row_env_kernel' if custom else 'osa_goal_env_kernel',
            'level': env.level, 'lanes_per_env': getattr(env, 'lanes', 64), 'state_floats': type(env).state_width,
            'obs_columns': env.observation_space.shape[0], 'n': n, 'steps': steps,
            'graph_us_per_step': round(statistics.median(us), 3),
            'graph_us_per_step_min_max': [round(min(us), 3), round(max(us), 3)]}


def child(root: str, name: str, header: str, n: int, steps: int, reps: int) -> None:
    """One run of one `against_parent` row with the package of `root`; prints its JSON."""
    sys.path.insert(0, root)
    import torch

    import omnisafe_amd
    from omnisafe_amd import envs

    env_id = name
    if header != '-':
        env_id = name + '-v0'
        omnisafe_amd.register_device_env(header, name, [env_id])
    env = envs.make(env_id, num_envs=n, device='cuda:0', horizon=1000, seed=0)
    us = graph_us_per_step(env, n, steps, reps)
    print(json.dumps({'us_per_step': round(statistics.median(us), 3), 'device': torch.cuda.get_device_name(0)}))


def against_parent(parent: str, n: int, steps: int, reps: int, runs: int) -> dict:
    jobs = []
    for where, root in (('this commit', ROOT), ('parent commit', os.path.abspath(parent))):
        for name, header in PARENT_ROWS:
            jobs.append((name, where, root, os.path.join(root, 'tests', 'custom_envs', header) if header else '-'))
    got: dict = {(name, where): [] for name, where, _, _ in jobs}
    for _ in range(runs):  # the rows take turns, one fresh process each
        for name, where, root, header in jobs:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', root, name, header, '--n', str(n), '--steps',
                   str(steps), '--reps', str(reps)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=300)
            got[(name, where)].append(json.loads(done.stdout.strip().splitlines()[-1])['us_per_step'])
    rows = [{'env': name, 'package': where, 'us_per_step_runs': v, 'us_per_step': round(statistics.median(v), 3),
             'run_to_run_spread': round(max(v) - min(v), 3)} for (name, where), v in got.items()]
    by = {(r['env'], r['package']): r for r in rows}
    verdict = {}
    for name, _ in PARENT_ROWS:
        here, there = by[(name, 'this commit')], by[(name, 'parent commit')]
        spread = max(here['run_to_run_spread'], there['run_to_run_spread'])
        diff = round(here['us_per_step'] - there['us_per_step'], 3)
        verdict[name] = {'difference_us_per_step': diff, 'run_to_run_spread': spread,
                         'within_spread': abs(diff) <= spread}
    return {'runs': runs, 'rows': rows, 'verdict': verdict}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--build-only', action='store_true')
    ap.add_argument('--child', nargs=3, metavar=('ROOT', 'NAME', 'HEADER'))
    args = ap.parse_args()
    if args.child:
        child(*args.child, args.n, args.steps, args.reps)
        return
    sys.path.insert(0, ROOT)
    if args.build_only:
        from omnisafe_amd import build

        built = [build.build_custom_env(os.path.join(EXAMPLES, h), s) for h, s, _ in custom_structs()]
        print(json.dumps({'built': built + [build.build_custom_env(os.path.join(EXAMPLES, 'glider.h'), 'Glider')]}))
        return
    import torch

    import omnisafe_amd

    ids = [f'{builtin}{level}-v0' for _, builtin in GOALS for level in range(3)]
    for header, struct, top in custom_structs():
        levels = {f'{struct}-{level}-v0': level for level in range(top + 1)}
        omnisafe_amd.register_device_env(os.path.join(EXAMPLES, header), struct, levels)
        ids += list(levels)
    rows = [env_step_row(e, args.n, args.steps, args.reps) for e in ids]
    for r in rows:
        print(json.dumps(r), file=sys.stderr, flush=True)
    by = {r['env']: r for r in rows}
    fastest = []
    for name, builtin in GOALS:
        for level in range(3):
            at = {lanes: by[f'{name}{lanes}-{level}-v0']['graph_us_per_step'] for lanes in (16, 32, 64)}
            best = min(at, key=at.get)
            there = by[f'{builtin}{level}-v0']['graph_us_per_step']
            fastest.append({'description': name, 'level': level, 'us_per_step_by_lanes': at, 'fastest_lanes': best,
                            'built_in_us_per_step': there, 'generic_over_built_in': round(at[best] / there, 3)})
    out = {'tool': 'custom_row_env_timing', 'device': torch.cuda.get_device_name(0), 'n': args.n, 'steps': args.steps,
           'reps': args.reps, 'env_step': rows, 'fastest_lanes': fastest}
    if args.parent:
        out['against_parent'] = against_parent(args.parent, args.n, args.steps, args.reps, args.runs)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
