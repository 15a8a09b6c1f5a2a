"""Device time of OfflineDataCollector's persistent kernel next to the two things it can be measured against, for a
randomly initialised PPOLag checkpoint with an active observation normaliser:

    python tools/collect_timing.py [--k 4096] [--q 200] [--horizon 100] [--reps 5] [--variant-lib PATH] [--out PATH]

Per env (SynthReach-v0 and SynthNavGoal1-v0) and in ONE process, K lanes of Q rows each:
  collect    osa_collect_episodes: the whole block in one launch (rows/s, us per step of the K lanes, ns per lane-step)
  per_step   the same agent on the collector's per-step path (the launches of Q vector steps)
  eval       osa_eval_episodes on the same env and K, horizon = max_steps = Q: the deterministic kernel that the
             collection kernel extends, which stores nothing per step
and collect / eval per step, beside the bytes a row adds: (2 obs_dim + act_dim + 3) * 4.
HIP events round each call; one warm-up call, then the median of --reps.
--variant-lib: another build of the library (a parent commit's, or one of tools/build_variant_lib.sh); `collect` is
    repeated on it in a child process (OSA_LIB_PATH) and reported as `collect_variant` and `variant_over_collect`.
    (profiles/collect_row_stores.json: the row-wise store form of commit 9b8c2dd measured this way.)
Writes --out (default profiles/collect_timing.json) and prints the same JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from omnisafe_amd import _lib  # noqa: E402
from omnisafe_amd.config import Config, get_default_kwargs  # noqa: E402
from omnisafe_amd.models import ConstraintActorCritic  # noqa: E402
from omnisafe_amd.normalizer import Normalizer  # noqa: E402
from omnisafe_amd.offline import OfflineDataCollector, agent_seeds  # noqa: E402
from omnisafe_amd.saved_policy import policy_args, scale_bounds  # noqa: E402
from omnisafe_amd.spaces import Box  # noqa: E402

DEV = 'cuda:0'
CASES = [('SynthReach-v0', 60, 2), ('SynthNavGoal1-v0', 60, 2)]


def checkpoint(root: str, env_id: str, obs_dim: int, act_dim: int, horizon: int) -> str:
    d = get_default_kwargs('PPOLag')
    d.update({'algo': 'PPOLag', 'env_id': env_id, 'exp_name': 'collect_timing', 'seed': 0,
              'env_cfgs': {'horizon': horizon}})
    os.makedirs(os.path.join(root, 'torch_save'), exist_ok=True)
    with open(os.path.join(root, 'config.json'), 'w', encoding='utf-8') as f:
        json.dump(d, f)
    torch.manual_seed(0)
    ac = ConstraintActorCritic(Box(-np.inf, np.inf, (obs_dim,)), Box(-1.0, 1.0, (act_dim,)),
                               Config.dict2config(d).model_cfgs, epochs=1, device=DEV)
    norm = Normalizer((obs_dim,), clip=5, device=DEV)
    norm.push(torch.randn(1024, obs_dim, device=DEV))
    torch.save({'pi': {k: v.cpu() for k, v in ac.actor.state_dict().items()},
                'obs_normalizer': {k: v.cpu() for k, v in norm.state_dict().items()}},
               os.path.join(root, 'torch_save', 'epoch-0.pt'))
    return root


def median_ms(call, reps: int) -> float:
    call()  # warm-up (code objects, allocations)
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times)


def figures(ms: float, K: int, Q: int) -> dict:
    return {'ms': round(ms, 4), 'rows_per_s': round(K * Q / (ms * 1e-3)), 'us_per_step': round(1e3 * ms / Q, 3),
            'ns_per_lane_step': round(1e6 * ms / (K * Q), 3)}


def measure(env_id: str, obs_dim: int, act_dim: int, K: int, Q: int, horizon: int, reps: int, only_collect: bool):
    root = checkpoint(tempfile.mkdtemp(prefix='osa_collect_timing_'), env_id, obs_dim, act_dim, horizon)
    S = K * Q
    col = OfflineDataCollector(S, env_id, seed=0, device=DEV, num_envs=K, env_cfgs={'horizon': horizon})
    col.register_agent(root, 'epoch-0.pt', S)
    agent = col.agents[0]
    f32 = dict(dtype=torch.float32, device=DEV)
    block = {'obs': torch.zeros(S, obs_dim, **f32), 'action': torch.zeros(S, act_dim, **f32),
             'reward': torch.zeros(S, 1, **f32), 'cost': torch.zeros(S, 1, **f32),
             'next_obs': torch.zeros(S, obs_dim, **f32), 'done': torch.zeros(S, 1, **f32)}
    seeds = agent_seeds(0, 0)
    row = {'env': env_id, 'K': K, 'Q': Q, 'horizon': horizon, 'rows': S,
           'row_bytes': (2 * obs_dim + act_dim + 3) * 4}
    row['collect'] = figures(median_ms(lambda: col._run_persistent(agent, K, block, *seeds), reps), K, Q)
    if only_collect:
        return row
    kept = {k: v.clone() for k, v in block.items()}
    row['per_step'] = figures(median_ms(lambda: col._run_per_step(agent, K, block, *seeds), reps), K, Q)
    row['paths_equal'] = all(bool(torch.equal(kept[k], block[k])) for k in kept)
    # the deterministic kernel on the same env and K: one episode of Q steps per lane, nothing stored per step
    env = col._make_env(K, seeds[0])
    lo, hi = scale_bounds(env, DEV)
    ret = torch.zeros(K, dtype=torch.float64, device=DEV)
    cost = torch.zeros(K, dtype=torch.float64, device=DEV)
    length = torch.zeros(K, dtype=torch.int32, device=DEV)
    play = getattr(env.library(), env.eval_entry_point)

    def evaluate():
        _lib.check(play(env.eval_kind(env_id), K, *policy_args(agent.actor, agent.normalizer, obs_dim, act_dim, lo, hi),
                        seeds[0], Q, 0.0, Q, 0, 0.0, 0.0, 0, 0.0, 1.0, _lib.ptr(ret), _lib.ptr(cost), _lib.ptr(length),
                        None, _lib.stream_ptr()))

    row['eval'] = figures(median_ms(evaluate, reps), K, Q)
    assert int(length.min()) == Q
    row['collect_over_eval'] = round(row['collect']['ms'] / row['eval']['ms'], 3)
    row['per_step_over_collect'] = round(row['per_step']['ms'] / row['collect']['ms'], 2)
    row['collect_store_GBps'] = round(S * row['row_bytes'] / (row['collect']['ms'] * 1e-3) / 1e9, 1)
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=4096)
    ap.add_argument('--q', type=int, default=200)
    ap.add_argument('--horizon', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--variant-lib', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'collect_timing.json'))
    ap.add_argument('--only-collect', action='store_true')
    args = ap.parse_args()
    rows = [measure(env_id, D, A, args.k, args.q, args.horizon, args.reps, args.only_collect) for env_id, D, A in CASES]
    out = {'tool': 'collect_timing', 'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'rows': rows}
    if args.only_collect:
        print(json.dumps(out))
        return
    if args.variant_lib:  # a fresh process: the library is bound once per process
        child = subprocess.run(
            [sys.executable, os.path.abspath(__file__), '--only-collect', '--k', str(args.k), '--q', str(args.q),
             '--horizon', str(args.horizon), '--reps', str(args.reps)],
            env=dict(os.environ, OSA_LIB_PATH=os.path.abspath(args.variant_lib)), check=True, capture_output=True,
            text=True, timeout=300)
        variant = json.loads(child.stdout.strip().splitlines()[-1])
        for row, other in zip(rows, variant['rows']):
            row['collect_variant'] = other['collect']
            row['variant_over_collect'] = round(other['collect']['ms'] / row['collect']['ms'], 3)
        out['variant_lib'] = os.path.basename(args.variant_lib)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
