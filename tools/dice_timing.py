#!/usr/bin/env python
"""Time and launches of one offline COptiDICE train step at the YAML shape (nu, chi and the actor hidden 256 x 256 x 256,
relu, batch 256, softchi, observation / action columns 28 / 2, a 4096-row dataset) on both routes of OSA_DICE_ROUTE
-> profiles/dice_timing.json.

    python tools/dice_timing.py                      # on the GPU: graph-replayed times of both routes
    python tools/dice_timing.py --kernel-split       # + launches per step and the per-kernel split from ONE rocprofv3
                                                     #   run of its own per route

Protocol (tools/bcq_timing.py's): one step of each route captured into a single-stream graph in the SAME process; the
windows of the two routes alternate (list, single, list, ...), `--steps` replays between two synchronisations each,
median of 5 windows per route after a warm-up window each; the spread is (max - min) / median of a route's windows.
The baseline is the `single` route at the same commit: the same kernel with every problem in a launch of its own.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HID, B, N, D, A = [256, 256, 256], 256, 4096, 28, 2
ROUTES = ('list', 'single')
NETS = ('nu', 'chi', 'actor')


def make_step(route):
    import numpy as np
    import torch

    from omnisafe_amd import dice_step

    rng = np.random.default_rng(0)
    data = {'obs': rng.standard_normal((N, D)), 'action': rng.uniform(-1, 1, (N, A)), 'reward': rng.standard_normal((N, 1)),
            'cost': rng.random((N, 1)), 'next_obs': rng.standard_normal((N, D)), 'done': rng.random((N, 1)) < 0.01,
            'init_obs': rng.standard_normal((N, D))}
    data = {k: torch.from_numpy(v.astype(np.float32)).cuda() for k, v in data.items()}
    desc = dice_step.make_desc(D, A, {n: HID for n in NETS}, {n: 'relu' for n in NETS}, B, 'softchi')
    st = dice_step.DiceStep(desc, data, gamma=0.99, alpha=0.0008, cost_limit=0.06, cost_ub_eps=0.05, lr_nu=0.003,
                            lr_chi=0.003, lr_actor=0.003, lr_lamb=0.035, lr_tau=0.003, lamb_init=0.0, tau_init=1.0,
                            nslots=256, route=route)
    torch.manual_seed(0)
    st.init_parameters()
    st.draw(0, 0, 256)
    return st


def time_routes(steps):
    import torch

    assert torch.cuda.is_available(), 'the timing legs need the GPU'
    graphs, steps_of = {}, {}
    for route in ROUTES:
        st = steps_of[route] = make_step(route)
        st.run(8)  # every shape's first launches
        torch.cuda.synchronize()
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(side):
            graph.capture_begin()
            st.run(1)
            graph.capture_end()
        graphs[route] = graph
    torch.cuda.synchronize()
    windows = {r: [] for r in ROUTES}
    for _ in range(6):
        for route in ROUTES:
            t0 = time.perf_counter()
            for _ in range(steps):
                graphs[route].replay()
            torch.cuda.synchronize()
            windows[route].append((time.perf_counter() - t0) / steps * 1e6)
    out = {}
    for route in ROUTES:
        timed = sorted(windows[route][1:])
        us = timed[len(timed) // 2]
        st = steps_of[route]
        out[route] = {'us_graph_median_of_5': us, 'us_windows': windows[route][1:],
                      'window_spread': (timed[-1] - timed[0]) / us, 'replays_per_window': steps,
                      'finite': bool(all(torch.isfinite(getattr(st, n)).all() for n in NETS + ('mult', 'stats')))}
    l, s = (out[r]['us_graph_median_of_5'] for r in ROUTES)
    out['list_over_single'] = l / s
    out['faster_by_more_than_the_spread'] = ('list' if l < s else 'single') if abs(l - s) / min(l, s) > max(
        out[r]['window_spread'] for r in ROUTES) else 'neither'
    return out


def kernel_split(out_dir):
    """One rocprofv3 --kernel-trace --stats run of its own per route over 50 eager steps (the program goes after `--`);
    returns launches per step and {kernel name: [calls, total ns]} per route."""
    import csv
    import glob

    res = {}
    for route in ROUTES:
        d = os.path.join(out_dir, f'rocprof_dice_{route}')
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'dice', '--output-format', 'csv', '--',
               sys.executable, os.path.abspath(__file__), '--profiled-child', route]
        subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
        rows = {}
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            with open(path, encoding='utf-8') as f:
                for r in csv.DictReader(f):
                    rows[r['Name'][:80]] = [int(r['Calls']), int(r['TotalDurationNs'])]
        step_rows = {k: v for k, v in rows.items() if 'dice_' in k and v[0] % 50 == 0}  # (the draws run once)
        res[route] = {'launches_per_step': sum(v[0] for v in step_rows.values()) // 50,
                      'kernels': dict(sorted(step_rows.items(), key=lambda kv: -kv[1][1]))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--kernel-split', action='store_true')
    ap.add_argument('--profiled-child', default='', help=argparse.SUPPRESS)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dice_timing.json'))
    args = ap.parse_args()
    import torch

    if args.profiled_child:
        st = make_step(args.profiled_child)
        st.run(50)
        torch.cuda.synchronize()
        return
    result = {'shape': {'hidden': HID, 'batch': B, 'rows': N, 'obs_dim/act_dim': [D, A], 'fn_type': 'softchi'},
              'device': torch.cuda.get_device_name(0), 'step': time_routes(args.steps)}
    if args.kernel_split:
        result['kernel_split_rocprofv3'] = kernel_split(os.path.dirname(os.path.abspath(args.out)))
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == '__main__':
    main()
