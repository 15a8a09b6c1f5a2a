#!/usr/bin/env python
"""Time of one offline VAE-BC train step at the YAML shape (hidden 750 x 750, batch 256, observation / action columns
28 / 2 and 60 / 2, a 4096-row dataset) on both routes of OSA_VAE_GEMM -> profiles/vae_timing.json.

    python tools/vae_timing.py                      # on the GPU: graph-replayed step time of both routes, share of peak
    python tools/vae_timing.py --kernel-split       # + the per-kernel split from ONE rocprofv3 run of its own per route
    python tools/vae_timing.py --reference-cpu 8    # context only: the same step in plain torch on the CPU, 8 threads

Step time: one step of each route captured into a single-stream graph in the SAME process; the windows of the two routes
alternate (tile, skinny, tile, ...), `--steps` replays between two synchronisations each, median of 5 windows per route
after a warm-up window each; the spread is (max - min) / median of a route's windows.  The baseline is the `tile`
route: the tile GEMM of the general networks on the same launches.  FLOP per step are counted from the shapes
(2 M N K per layer product: forward, backward-data, weight-gradient); the share of peak is that count over step time
over the 157.3 TFLOP/s float32-MFMA peak: a whole-step rate, not a kernel's.
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
HID, B, N = [750, 750], 256, 4096
SHAPES = {'28/2': (28, 2), '60/2': (60, 2)}
ROUTES = ('tile', 'skinny')


def flop_per_step(D, A):
    total = 0
    for sizes, latent in (([D + A] + HID + [4 * A], 0), ([D + 2 * A] + HID + [A], 2 * A)):
        mk = sum(a * b for a, b in zip(sizes[:-1], sizes[1:]))
        dgrad = sum(a * b for a, b in zip(sizes[1:-1], sizes[2:])) + latent * sizes[1]
        total += 2 * B * (2 * mk + dgrad)
    return total


def make_step(D, A, route):
    import numpy as np
    import torch

    from omnisafe_amd import vae_step

    rng = np.random.default_rng(0)
    data = {'obs': rng.standard_normal((N, D)), 'action': rng.uniform(-1, 1, (N, A))}
    data = {k: torch.from_numpy(v.astype(np.float32)).cuda() for k, v in data.items()}
    st = vae_step.VaeStep(vae_step.make_desc(D, A, HID, 'relu', B), data, lr=1e-3, nslots=1024, route=route)
    torch.manual_seed(0)
    st.init_parameters()
    st.draw(0, 0, 1024)
    return st


def time_shape(D, A, steps):
    import torch

    assert torch.cuda.is_available(), 'the timing legs need the GPU'
    graphs, steps_of = {}, {}
    for route in ROUTES:
        st = steps_of[route] = make_step(D, A, route)
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
    out, flop = {}, flop_per_step(D, A)
    for route in ROUTES:
        timed = sorted(windows[route][1:])
        us = timed[len(timed) // 2]
        out[route] = {'us_per_step_graph_median_of_5': us, 'us_per_step_windows': windows[route][1:],
                      'window_spread': (timed[-1] - timed[0]) / us, 'steps_per_window': steps, 'flop_per_step': flop,
                      'fraction_of_f32_mfma_peak_whole_step': flop / (us * 1e-6) / PEAK,
                      'finite': bool(torch.isfinite(steps_of[route].params).all())}
    t, s = (out[r]['us_per_step_graph_median_of_5'] for r in ROUTES)
    out['skinny_over_tile'] = s / t
    out['faster_by_more_than_the_spread'] = ('skinny' if s < t else 'tile') if abs(t - s) / min(t, s) > max(
        out[r]['window_spread'] for r in ROUTES) else 'neither'
    return out


def kernel_split(out_dir, D, A):
    """One rocprofv3 --kernel-trace --stats run of its own per route over 50 eager steps (the program goes after
    `--`); returns {kernel name: [calls, total ns]} per route."""
    import csv
    import glob

    res = {}
    for route in ROUTES:
        d = os.path.join(out_dir, f'rocprof_vae_{route}')
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'vae', '--output-format', 'csv', '--',
               sys.executable, os.path.abspath(__file__), '--profiled-child', route, '--dims', str(D), str(A)]
        subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
        rows = {}
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            with open(path, encoding='utf-8') as f:
                for r in csv.DictReader(f):
                    rows[r['Name'][:80]] = [int(r['Calls']), int(r['TotalDurationNs'])]
        res[route] = dict(sorted(rows.items(), key=lambda kv: -kv[1][1])[:12])
    return res


def reference_cpu(threads, D, A, steps=20):
    """Context only: VAE.loss and torch.optim.Adam in plain torch modules on the CPU (what the reference's step does)."""
    import torch

    torch.set_num_threads(threads)

    def mlp(sizes):
        layers = []
        for a, b in zip(sizes[:-1], sizes[1:]):
            layers += [torch.nn.Linear(a, b), torch.nn.ReLU()]
        return torch.nn.Sequential(*layers[:-1])

    enc, dec = mlp([D + A] + HID + [4 * A]), mlp([D + 2 * A] + HID + [A])
    opt = torch.optim.Adam(list(enc.parameters()) + list(dec.parameters()), lr=1e-3)
    obs, act = torch.randn(B, D), torch.rand(B, A)

    def train():
        mean, log_std = torch.chunk(enc(torch.cat([obs, act], -1)), 2, dim=-1)
        dist = torch.distributions.Normal(mean, torch.clamp(log_std, -20, 2).exp())
        recon = torch.nn.functional.mse_loss(dec(torch.cat([obs, dist.rsample()], -1)), act)
        kl = torch.distributions.kl.kl_divergence(dist, torch.distributions.Normal(0, 1)).mean()
        opt.zero_grad()
        (recon + kl).backward()
        opt.step()

    for _ in range(3):
        train()
    t0 = time.perf_counter()
    for _ in range(steps):
        train()
    return {'ms_per_step': (time.perf_counter() - t0) / steps * 1e3, 'threads': threads, 'steps': steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--kernel-split', action='store_true')
    ap.add_argument('--reference-cpu', type=int, default=0, metavar='THREADS')
    ap.add_argument('--profiled-child', default='', help=argparse.SUPPRESS)
    ap.add_argument('--dims', type=int, nargs=2, default=[28, 2], help=argparse.SUPPRESS)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vae_timing.json'))
    args = ap.parse_args()
    if args.profiled_child:
        import torch

        st = make_step(*args.dims, args.profiled_child)
        st.run(50)
        torch.cuda.synchronize()
        return
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result['shape'] = {'hidden': HID, 'batch': B, 'rows': N, 'obs_dim/act_dim': list(SHAPES)}
    if args.reference_cpu:
        result['reference_cpu_context'] = {k: reference_cpu(args.reference_cpu, *da) for k, da in SHAPES.items()}
    else:
        import torch

        result['device'] = torch.cuda.get_device_name(0)
        for key, (D, A) in SHAPES.items():
            result[key] = time_shape(D, A, args.steps)
        if args.kernel_split:
            result['kernel_split_rocprofv3_28/2'] = kernel_split(os.path.dirname(os.path.abspath(args.out)), 28, 2)
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == '__main__':
    main()
