#!/usr/bin/env python
"""Time of one offline CRR / CCRR train step at the YAML shape (hidden 256 x 256 x 256, batch 256, 10 sampled actions,
28 / 2 observation / action columns of SynthNavCircle1-v0, a 4096-row dataset) -> profiles/crr_timing.json.

    python tools/crr_timing.py                      # on the GPU: graph-replayed step time, launches, FLOP, share of peak
    python tools/crr_timing.py --kernel-split       # + the per-kernel split from ONE rocprofv3 run of its own (a child)
    python tools/crr_timing.py --reference-cpu 8    # context only: the reference's step on the CPU with 8 threads

Step time: one step captured into a single-stream graph, replayed `--steps` times between two synchronisations, median
of 5 windows after a warm-up window.  FLOP per step are counted from the shapes (2 M N K per layer product, forward,
backward-data and weight-gradient), launches per step from the launch plan.  The share of peak is that FLOP count over
step time over the 157.3 TFLOP/s float32-MFMA peak: a whole-step rate, not a kernel's.  The GPU legs read nothing of the
reference; a leg that finds no GPU fails.
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
D, A, HID, B, S, N = 28, 2, [256, 256, 256], 256, 10, 4096


def flop_per_step(pairs):
    def net(sizes, fwd_rows, bwd_rows):
        mk = sum(a * b for a, b in zip(sizes[:-1], sizes[1:]))
        mk_dgrad = sum(a * b for a, b in zip(sizes[1:-1], sizes[2:]))
        return 2 * mk * sum(fwd_rows) + sum(2 * (mk + mk_dgrad) * r for r in bwd_rows)
    actor = net([D] + HID + [A], [2 * B], [B])
    critic_update = 2 * net([D + A] + HID + [1], [B], [B]) + 2 * net([D + A] + HID + [1], [B], [])  # online + target
    critic_eval = 2 * net([D + A] + HID + [1], [B * (1 + S)], [])
    return actor + pairs * (critic_update + critic_eval)


def launches_per_step(pairs, L=len(HID) + 1):
    per_pair = 2 * L + 1 + (2 * L - 1) + 1
    return 1 + L + 1 + pairs * per_pair + pairs * L + 1 + 1 + (2 * L - 1) + 1 + 1


def make_step(pairs):
    import numpy as np
    import torch

    from omnisafe_amd import crr_step

    rng = np.random.default_rng(0)
    data = {'obs': rng.standard_normal((N, D)), 'action': rng.uniform(-1, 1, (N, A)), 'reward': rng.standard_normal((N, 1)),
            'cost': (rng.random((N, 1)) < 0.3) * 1.0, 'next_obs': rng.standard_normal((N, D)),
            'done': (rng.random((N, 1)) < 0.01) * 1.0}
    data = {k: torch.from_numpy(v.astype(np.float32)).cuda() for k, v in data.items()}
    desc = crr_step.make_desc(D, A, HID, HID, 'relu', 'relu', B, S, pairs)
    st = crr_step.CrrStep(desc, data, gamma=0.99, beta=1.0, polyak=0.005, lr_actor=1e-3, lr_critic=1e-3, nslots=1024,
                          cost_limit=25.0, lambda_lr=1e-3, lambda_init=1.0, wiring='intended')
    torch.manual_seed(0)
    st.init_parameters()
    st.draw(0, 0, 1024)
    return st


def time_step(pairs, steps):
    import torch

    assert torch.cuda.is_available(), 'the timing legs need the GPU'
    st = make_step(pairs)
    st.run(8, lagrange_open=True)  # every shape's first launches
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        graph.capture_begin()
        st.run(1, lagrange_open=True)
        graph.capture_end()
    torch.cuda.synchronize()
    windows = []
    for _ in range(6):
        t0 = time.perf_counter()
        for _ in range(steps):
            graph.replay()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / steps * 1e6)
    t0 = time.perf_counter()
    st.run(steps, lagrange_open=True)
    torch.cuda.synchronize()
    eager = (time.perf_counter() - t0) / steps * 1e6
    timed = sorted(windows[1:])
    us = timed[len(timed) // 2]
    flop = flop_per_step(pairs)
    return {'us_per_step_graph_median_of_5': us, 'us_per_step_windows': windows[1:], 'us_per_step_eager_one_call': eager,
            'steps_per_window': steps, 'launches_per_step': launches_per_step(pairs), 'flop_per_step': flop,
            'fraction_of_f32_mfma_peak_whole_step': flop / (us * 1e-6) / PEAK,
            'finite': bool(torch.isfinite(st.actor).all() and torch.isfinite(st.critic).all())}


def kernel_split(out_dir):
    """One rocprofv3 --kernel-trace --stats run of its own over 50 eager steps of each algorithm (the program goes
    after `--`); returns {kernel name: [calls, total ns]} per algorithm."""
    import csv
    import glob

    res = {}
    for algo, pairs in (('CRR', 1), ('CCRR', 2)):
        d = os.path.join(out_dir, f'rocprof_{algo}')
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'crr', '--output-format', 'csv', '--',
               sys.executable, os.path.abspath(__file__), '--profiled-child', str(pairs)]
        subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
        rows = {}
        for path in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            with open(path, encoding='utf-8') as f:
                for r in csv.DictReader(f):
                    rows[r['Name'][:80]] = [int(r['Calls']), int(r['TotalDurationNs'])]
        res[algo] = dict(sorted(rows.items(), key=lambda kv: -kv[1][1])[:16])
    return res


def reference_cpu(threads, steps=20):
    """Context only: the unmodified reference's CRR / CCRR `_train` on the CPU (needs the reference checkout)."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import torch

    torch.set_num_threads(threads)
    import crr_twin as T
    import test_crr_twin as TT

    out = {}
    for algo in ('CRR', 'CCRR'):
        spec = T._spec('yaml', algo, 1)
        run = T.make_run(**spec['run'])
        stub, _ = TT._reference_stub(algo, run, spec)
        batch = tuple(torch.from_numpy(x) for x in T.gather(run['data'], run['idx'][0]))
        for _ in range(3):
            stub._train(batch)
        t0 = time.perf_counter()
        for _ in range(steps):
            stub._train(batch)
        out[algo] = {'ms_per_step': (time.perf_counter() - t0) / steps * 1e3, 'threads': threads, 'steps': steps}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--kernel-split', action='store_true')
    ap.add_argument('--reference-cpu', type=int, default=0, metavar='THREADS')
    ap.add_argument('--profiled-child', type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'crr_timing.json'))
    args = ap.parse_args()
    if args.profiled_child:
        import torch

        st = make_step(args.profiled_child)
        st.run(50, lagrange_open=True)
        torch.cuda.synchronize()
        return
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result['shape'] = {'obs_dim': D, 'act_dim': A, 'hidden': HID, 'batch': B, 'sampled_action_num': S, 'rows': N}
    if args.reference_cpu:
        result['reference_cpu_context'] = reference_cpu(args.reference_cpu)
    else:
        import torch

        result['device'] = torch.cuda.get_device_name(0)
        for algo, pairs in (('CRR', 1), ('CCRR', 2)):
            result[algo] = time_step(pairs, args.steps)
        if args.kernel_split:
            result['kernel_split_rocprofv3'] = kernel_split(os.path.dirname(os.path.abspath(args.out)))
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == '__main__':
    main()
