#!/usr/bin/env python
"""Time of one offline BCQ / BCQ-Lag train step at the YAML shape (hidden 256 x 256 x 256, batch 256, 10 sampled
actions, observation / action columns 28 / 2 and 60 / 2, a 4096-row dataset) on both routes of OSA_BCQ_CHAIN, and of the
target chain alone -> profiles/bcq_timing.json.

    python tools/bcq_timing.py                      # on the GPU: graph-replayed times of both routes, share of peak
    python tools/bcq_timing.py --kernel-split       # + launches per step and the per-kernel split from ONE rocprofv3
                                                    #   run of its own per route (BCQ-Lag, 28 / 2)

Protocol (tools/vae_timing.py's): one step of each route captured into a single-stream graph in the SAME process; the
windows of the two routes alternate (layer, fused, layer, ...), `--steps` replays between two synchronisations each,
median of 5 windows per route after a warm-up window each; the spread is (max - min) / median of a route's windows.
The baseline is the `layer` route at the same commit.  The chain alone is `target_q` (the chain's launches and one
device copy of its B S values) timed the same way; its FLOP are counted from the shapes (2 M N K per layer, four
networks) and its share of peak is that count over its time over the 157.3 TFLOP/s float32-MFMA peak.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 157.3e12
HID, B, S, N = [256, 256, 256], 256, 10, 4096
SHAPES = {'28/2': (28, 2), '60/2': (60, 2)}
ALGOS = {'BCQ': 1, 'BCQLag': 2}
ROUTES = ('layer', 'fused')


def chain_flop(D, A):
    nets = ([D + 2 * A] + HID + [A], [D + A] + HID + [A], [D + A] + HID + [1], [D + A] + HID + [1])
    return 2 * B * S * sum(a * b for sizes in nets for a, b in zip(sizes[:-1], sizes[1:]))


def make_step(D, A, pairs, route):
    import numpy as np
    import torch

    from omnisafe_amd import bcq_step

    rng = np.random.default_rng(0)
    data = {'obs': rng.standard_normal((N, D)), 'action': rng.uniform(-1, 1, (N, A)), 'reward': rng.standard_normal((N, 1)),
            'cost': rng.random((N, 1)), 'next_obs': rng.standard_normal((N, D)), 'done': rng.random((N, 1)) < 0.01}
    data = {k: torch.from_numpy(v.astype(np.float32)).cuda() for k, v in data.items()}
    st = bcq_step.BcqStep(bcq_step.make_desc(D, A, HID, HID, 'relu', 'relu', B, S, pairs), data, gamma=0.99, polyak=0.005,
                          phi=0.05, minimum_weighting=0.75, lr_actor=1e-3, lr_critic=1e-3, nslots=256, cost_limit=25.0,
                          lambda_lr=1e-3, lambda_init=1.0, route=route)
    torch.manual_seed(0)
    st.init_parameters()
    st.draw(0, 0, 256)
    return st


def windows_of(graphs, steps):
    import torch

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
        out[route] = {'us_graph_median_of_5': us, 'us_windows': windows[route][1:],
                      'window_spread': (timed[-1] - timed[0]) / us, 'replays_per_window': steps}
    l, f = (out[r]['us_graph_median_of_5'] for r in ROUTES)
    out['fused_over_layer'] = f / l
    out['faster_by_more_than_the_spread'] = ('fused' if f < l else 'layer') if abs(l - f) / min(l, f) > max(
        out[r]['window_spread'] for r in ROUTES) else 'neither'
    return out


def time_shape(D, A, pairs, steps):
    import torch

    assert torch.cuda.is_available(), 'the timing legs need the GPU'
    step_graphs, chain_graphs, steps_of = {}, {}, {}
    for route in ROUTES:
        st = steps_of[route] = make_step(D, A, pairs, route)
        st.run(8)  # every shape's first launches
        z = st.z_r[0].clone()
        st.target_q(0, z)
        torch.cuda.synchronize()
        for graphs, fn in ((step_graphs, lambda: st.run(1)), (chain_graphs, lambda: st.target_q(0, z))):
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            with torch.cuda.stream(side):
                graph.capture_begin()
                fn()
                graph.capture_end()
            graphs[route] = graph
    torch.cuda.synchronize()
    out = {'step': windows_of(step_graphs, steps), 'chain': windows_of(chain_graphs, steps)}
    flop = chain_flop(D, A)
    for route in ROUTES:
        c, s = (out[k][route]['us_graph_median_of_5'] for k in ('chain', 'step'))
        out['chain'][route].update({'flop': flop, 'fraction_of_f32_mfma_peak': flop / (c * 1e-6) / PEAK,
                                    'share_of_step': pairs * c / s})
        out['step'][route]['finite'] = bool(torch.isfinite(steps_of[route].pert).all()
                                            and torch.isfinite(steps_of[route].critic).all())
    return out


def kernel_split(out_dir, D, A):
    """One rocprofv3 --kernel-trace --stats run of its own per route over 50 eager BCQ-Lag steps (the program goes after
    `--`); returns launches per step and {kernel name: [calls, total ns]} per route."""
    import csv
    import glob

    res = {}
    for route in ROUTES:
        d = os.path.join(out_dir, f'rocprof_bcq_{route}')
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'bcq', '--output-format', 'csv', '--',
               sys.executable, os.path.abspath(__file__), '--profiled-child', route, '--dims', str(D), str(A)]
        subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
        rows = {}
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            with open(path, encoding='utf-8') as f:
                for r in csv.DictReader(f):
                    rows[r['Name'][:80]] = [int(r['Calls']), int(r['TotalDurationNs'])]
        step_rows = {k: v for k, v in rows.items() if v[0] % 50 == 0}  # (set-up kernels run once)
        res[route] = {'launches_per_step': sum(v[0] for v in step_rows.values()) // 50,
                      'top': dict(sorted(step_rows.items(), key=lambda kv: -kv[1][1])[:12])}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--kernel-split', action='store_true')
    ap.add_argument('--profiled-child', default='', help=argparse.SUPPRESS)
    ap.add_argument('--dims', type=int, nargs=2, default=[28, 2], help=argparse.SUPPRESS)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bcq_timing.json'))
    args = ap.parse_args()
    import torch

    if args.profiled_child:
        st = make_step(*args.dims, 2, args.profiled_child)
        st.run(50)
        torch.cuda.synchronize()
        return
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result['shape'] = {'hidden': HID, 'batch': B, 'sampled_action_num': S, 'rows': N, 'obs_dim/act_dim': list(SHAPES)}
    result['device'] = torch.cuda.get_device_name(0)
    for key, (D, A) in SHAPES.items():
        for algo, pairs in ALGOS.items():
            result[f'{algo} {key}'] = time_shape(D, A, pairs, args.steps)
    if args.kernel_split:
        result['kernel_split_rocprofv3_BCQLag_28/2'] = kernel_split(os.path.dirname(os.path.abspath(args.out)), 28, 2)
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == '__main__':
    main()
