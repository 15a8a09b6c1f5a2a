#!/usr/bin/env python
"""One worked run of the whole pipeline on the device -> profiles/crr_learning.md: PPOLag on SynthNavCircle1-v0, a
dataset collected from three of its checkpoints, CCRR and CRR trained on that file, EpRet / EpCost per epoch next to the
behaviour policies' averages.

    python tools/crr_learning.py [--out profiles/crr_learning.md]
"""
import argparse
import csv
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENV = 'SynthNavCircle1-v0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'crr_learning.md'))
    ap.add_argument('--offline-steps', type=int, default=10000)
    args = ap.parse_args()
    import omnisafe_amd

    work = tempfile.mkdtemp(prefix='crr_learning_')
    lines = ['# CRR / CCRR on a collected dataset: one worked run', '',
             f'`python tools/crr_learning.py` on one MI355X; env `{ENV}`, seed 0 everywhere.', '']
    # ---- behaviour policies
    t0 = time.time()
    n_env, spe, epochs = 256, 256 * 500, 12  # (one full 500-step episode per env and epoch)
    on = omnisafe_amd.Agent('PPOLag', ENV, custom_cfgs={
        'seed': 0, 'train_cfgs': {'device': 'cuda:0', 'total_steps': spe * epochs, 'vector_env_nums': n_env},
        'algo_cfgs': {'steps_per_epoch': spe},
        'logger_cfgs': {'log_dir': os.path.join(work, 'on'), 'save_model_freq': 4, 'verbose': False}})
    on.learn()
    on_dir = on.agent.logger.log_dir
    lines += [f'PPOLag: {epochs} epochs of {spe} steps ({time.time() - t0:.1f} s), checkpoints of epochs 4, 8, 12.', '']
    # ---- dataset
    per = 20000
    col = omnisafe_amd.OfflineDataCollector(3 * per, ENV, seed=0)
    for e in (4, 8, 12):
        col.register_agent(on_dir, f'epoch-{e}.pt', per)
    t0 = time.time()
    col.collect(os.path.join(work, 'data'))
    lines += [f'Dataset: {3 * per} rows, {per} per checkpoint, path `{col.path}` ({time.time() - t0:.2f} s).', '',
              '| behaviour policy | episodes | average return | average cost |', '|---|---|---|---|']
    for e, s in zip((4, 8, 12), col.summaries):
        lines.append(f'| PPOLag epoch {e} | {s["episodes"]} | {s["return"]:.2f} | {s["cost"]:.2f} |')
    lines.append('')
    # ---- offline
    path = os.path.join(work, 'data', f'{ENV}_data.npz')
    spe_off = 1000
    for algo in ('CCRR', 'CRR'):
        cfgs = {'seed': 0, 'train_cfgs': {'device': 'cuda:0', 'dataset': path, 'total_steps': args.offline_steps},
                'algo_cfgs': {'steps_per_epoch': spe_off},
                'logger_cfgs': {'log_dir': os.path.join(work, algo), 'save_model_freq': 100, 'verbose': False}}
        if algo == 'CCRR':
            cfgs['algo_cfgs']['lagrange_start_step'] = 2000
        agent = omnisafe_amd.Agent(algo, ENV, custom_cfgs=cfgs)
        t0 = time.time()
        agent.learn()
        wall = time.time() - t0
        with open(os.path.join(agent.agent.logger.log_dir, 'progress.csv'), encoding='utf-8') as f:
            rows = list(csv.DictReader(f))
        upd = sum(float(r['Time/Update']) for r in rows)
        lines += [f'## {algo}', '',
                  f'YAML defaults (hidden 256 x 256 x 256, batch 256, 10 sampled actions), {args.offline_steps} steps in '
                  f'epochs of {spe_off}; wall {wall:.1f} s, of which {upd:.1f} s in the train steps '
                  f'({upd / args.offline_steps * 1e6:.0f} us per step, the epoch\'s one device read included) and the '
                  'rest in the 10-episode evaluations.', '',
                  '| epoch | EpRet | EpCost | EpLen | Loss_actor | Loss_reward_critic | PolicyStd'
                  + (' | LagrangeMultiplier |' if algo == 'CCRR' else ' |'),
                  '|---|---|---|---|---|---|---' + ('|---|' if algo == 'CCRR' else '|')]
        for r in rows:
            lines.append(f'| {int(float(r["Train/Epoch"]))} | {float(r["Metrics/EpRet"]):.2f} | '
                         f'{float(r["Metrics/EpCost"]):.2f} | {float(r["Metrics/EpLen"]):.0f} | '
                         f'{float(r["Loss/Loss_actor"]):.4f} | {float(r["Loss/Loss_reward_critic"]):.4f} | '
                         f'{float(r["Train/PolicyStd"]):.3f}'
                         + (f' | {float(r["Metrics/LagrangeMultiplier"]):.4f} |' if algo == 'CCRR' else ' |'))
        lines.append('')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w', encoding='utf-8') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
