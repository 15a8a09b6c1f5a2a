#!/usr/bin/env python
"""Time of one off-policy SAC gradient step at the YAML shape (batch 256, hidden [256, 256], obs 60 / act 2 of
SynthNavGoal1-v0) on both routes of OSA_SAC_HEAD, the TD3 layer-route step in the same run for scale, and the
env-steps/s of a default Agent('SAC') run while warming up and while learning -> profiles/sac_timing.json.

    python tools/sac_timing.py

Protocol: HIP events on the launch stream around `--steps` eager steps (policy_delay 2: every second one is an actor
step); after one warm-up window each, five windows per subject, alternating layer, fused, TD3, layer, ...; the median
and the spread (max - min) / median of a subject's windows.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, A, HID, B, N, NSLOTS = 60, 2, [256, 256], 256, 4096, 512


def make_step(kind, auto):
    import torch

    from omnisafe_amd import sac_step, td3_step

    kw = dict(size=N, gamma=0.99, polyak=0.005, lr_actor=3e-4, lr_critic=3e-4, nslots=NSLOTS, policy_delay=2,
              max_grad_norm=40.0)
    if kind == 'td3':
        st = td3_step.Td3Step(td3_step.make_desc(D, A, HID, HID, 'relu', 'relu', B, 2), policy_noise=0.2,
                              policy_noise_clip=0.5, route='layer', **kw)
    else:
        st = sac_step.SacStep(sac_step.make_desc(D, A, HID, HID, 'relu', 'relu', B), alpha=0.2, auto_alpha=auto,
                              head=kind, **kw)
    torch.manual_seed(0)
    st.init_parameters()
    g = torch.Generator().manual_seed(0)
    for k, v in st.ring.items():
        v.copy_(torch.randn(v.shape, generator=g) if k != 'done' else (torch.rand(v.shape, generator=g) < 0.01).float())
    st.pos.copy_(torch.tensor([0, N]))
    st.draw(0, 0, NSLOTS)
    return st


def time_steps(steps, auto):
    import torch

    subjects = {k: make_step(k, auto) for k in ('layer', 'fused', 'td3')}
    windows = {k: [] for k in subjects}
    for _ in range(6):
        for k, st in subjects.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            st.run(steps)
            t1.record()
            t1.synchronize()
            windows[k].append(t0.elapsed_time(t1) * 1e3 / steps)
    out = {}
    for k, st in subjects.items():
        timed = sorted(windows[k][1:])
        us = timed[len(timed) // 2]
        out[k] = {'us_per_step_median_of_5': us, 'us_windows': windows[k][1:], 'window_spread': (timed[-1] - timed[0]) / us,
                  'steps_per_window': steps, 'finite': bool(torch.isfinite(st.actor).all() and torch.isfinite(st.critic).all())}
    l, f = (out[k]['us_per_step_median_of_5'] for k in ('layer', 'fused'))
    out['fused_over_layer'] = f / l
    out['faster_by_more_than_the_spread'] = ('fused' if f < l else 'layer') if abs(l - f) / min(l, f) > max(
        out[k]['window_spread'] for k in ('layer', 'fused')) else 'neither'
    return out


def agent_rate(start_learning_steps, log_dir):
    import torch

    import omnisafe_amd

    cfgs = {'train_cfgs': {'total_steps': 4000, 'eval_episodes': 0},
            'algo_cfgs': {'start_learning_steps': start_learning_steps, 'size': 100000},
            'logger_cfgs': {'log_dir': log_dir, 'verbose': False}}
    agent = omnisafe_amd.Agent('SAC', 'SynthNavGoal1-v0', custom_cfgs=cfgs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    agent.learn()
    torch.cuda.synchronize()
    return 4000 / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sac_timing.json'))
    ap.add_argument('--log-dir', default=os.path.join(ROOT, 'runs', 'sac_timing'))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), 'the timing legs need the GPU'
    result = {'shape': {'obs_dim': D, 'act_dim': A, 'hidden': HID, 'batch': B, 'policy_delay': 2},
              'device': torch.cuda.get_device_name(0), 'step': time_steps(args.steps, False),
              'step_auto_alpha': time_steps(args.steps, True),
              'agent_env_steps_per_s': {'warming_up': agent_rate(10000, args.log_dir),
                                        'learning': agent_rate(0, args.log_dir)}}
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == '__main__':
    main()
