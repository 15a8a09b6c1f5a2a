"""Epoch wall time and aggregate env-steps/s of an AgentGroup of S members against a solo Agent of the same
configuration: BASELINE config 2 (PPOLag, SynthPointGoal1 60/2, 4096 envs, 65 536 steps per epoch, batch 64 x 40
passes, no KL early stop).

    python tools/group_timing.py [--sizes 1,2,4,8,16,32,64,80,96] [--warmup 2] [--epochs 4] [--no-solo] [--out FILE]

For every S, in one process and alternating: a solo ``Agent.learn()`` and an ``AgentGroup(seeds=range(S)).learn()``
of warmup + epochs epochs.  The epoch time is the median ``Time/Epoch`` of the timed epochs in the first member's
progress.csv (in a group that column is the group's wall time for one epoch of EVERY member: the members advance in
lockstep); aggregate env-steps/s = S x 65 536 / that.  ``solo_spread`` is (max - min) / median over the repeated solo
runs of the call -- the yardstick for the S = 1 and S = 8 comparisons.  Prints one JSON line.

Kernel time per launch: run it under ``rocprofv3 --kernel-trace --stats`` with one size at a time, e.g.
``rocprofv3 --kernel-trace --stats -d out -- python tools/group_timing.py --sizes 8`` and compare
osa_ppo_pass_group_kernel with osa_ppo_pass_kernel in the kernel statistics."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import omnisafe_amd  # noqa: E402

N, T = 4096, 16


def cfgs(epochs: int) -> dict:
    return {'train_cfgs': {'device': 'cuda:0', 'vector_env_nums': N, 'total_steps': N * T * epochs},
            'algo_cfgs': {'steps_per_epoch': N * T, 'kl_early_stop': False},
            'logger_cfgs': {'log_dir': tempfile.mkdtemp(), 'save_model_freq': 10 ** 9, 'verbose': False},
            'env_cfgs': {'horizon': T, 'cost_p': 0.05}}


def epoch_ms(agent, warmup: int) -> float:
    rows = list(csv.DictReader(open(os.path.join(agent.agent.logger.log_dir, 'progress.csv'))))
    return 1e3 * statistics.median(float(r['Time/Epoch']) for r in rows[warmup:])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1,2,4,8,16,32,64,80,96')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--epochs', type=int, default=4)
    ap.add_argument('--no-solo', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    total = args.warmup + args.epochs
    rows, solo = [], []
    for S in (int(s) for s in args.sizes.split(',')):
        if not args.no_solo:
            a = omnisafe_amd.Agent('PPOLag', 'SynthPointGoal1-v0', custom_cfgs=dict(cfgs(total), seed=0))
            a.learn()
            solo.append(epoch_ms(a, args.warmup))
            assert a.agent._updater.last_path == 'persistent' and a.agent._updater.last_group == 0  # noqa: SLF001
            del a
        g = omnisafe_amd.AgentGroup('PPOLag', 'SynthPointGoal1-v0', seeds=range(S), custom_cfgs=cfgs(total))
        g.learn()
        assert all(m.agent._updater.last_group == S for m in g.agents)  # noqa: SLF001
        ms = epoch_ms(g.agents[0], args.warmup)
        rows.append({'S': S, 'group_epoch_ms': round(ms, 2), 'env_steps_per_s': round(S * N * T / ms * 1e3, 1),
                     'solo_epoch_ms': round(solo[-1], 2) if solo else None,
                     'whole_run_env_steps_per_s': round(g.env_steps_per_second, 1)})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        del g
    out = {'config': 'BASELINE 2: PPOLag 60/2, 4096 envs x 16 steps, batch 64 x 40 passes, kl_early_stop off',
           'warmup_epochs': args.warmup, 'timed_epochs': args.epochs, 'rows': rows}
    if solo:
        med = statistics.median(solo)
        out.update(solo_epoch_ms_runs=[round(v, 2) for v in solo], solo_epoch_ms=round(med, 2),
                   solo_env_steps_per_s=round(N * T / med * 1e3, 1),
                   solo_spread=round((max(solo) - min(solo)) / med, 4))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, 'w'), indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
