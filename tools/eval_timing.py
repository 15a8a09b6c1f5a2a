"""Wall time of Evaluator.evaluate on both paths (persistent osa_eval_episodes vs per-step launches) for a randomly
initialised PPOLag checkpoint with an active observation normaliser.

    python tools/eval_timing.py [--ks 16,1024,16384] [--reps 3]

Cases: SynthReach-v0, SynthPointGoal1-v0, SynthHumanoid-v0, SynthNavGoal1-v0 and SynthNavCircle1-v0, all at horizon
1000 (--cases picks some by id).  One warm-up call per
(case, K, path), then the median of --reps timed calls (host clock around evaluate() + device synchronisation).
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omnisafe_amd.config import Config, get_default_kwargs  # noqa: E402
from omnisafe_amd.envs import SYNTH_DIMS  # noqa: E402
from omnisafe_amd.evaluator import Evaluator  # noqa: E402
from omnisafe_amd.models import ConstraintActorCritic  # noqa: E402
from omnisafe_amd.normalizer import Normalizer  # noqa: E402
from omnisafe_amd.spaces import Box  # noqa: E402

DEV = 'cuda:0'
CASES = [('SynthReach-v0', {'horizon': 1000}), ('SynthPointGoal1-v0', {'horizon': 1000}),
         ('SynthHumanoid-v0', {'horizon': 1000}), ('SynthNavGoal1-v0', {'horizon': 1000}),
         ('SynthNavCircle1-v0', {'horizon': 1000})]


def checkpoint(root: str, env_id: str, env_cfgs: dict) -> str:
    d = get_default_kwargs('PPOLag')
    d.update({'algo': 'PPOLag', 'env_id': env_id, 'exp_name': 'eval_timing', 'seed': 0, 'env_cfgs': env_cfgs})
    os.makedirs(os.path.join(root, 'torch_save'), exist_ok=True)
    with open(os.path.join(root, 'config.json'), 'w', encoding='utf-8') as f:
        json.dump(d, f)
    obs_dim, act_dim = dict(SYNTH_DIMS, **{'SynthReach-v0': (60, 2), 'SynthNavGoal1-v0': (60, 2),
                                           'SynthNavCircle1-v0': (28, 2)})[env_id]
    torch.manual_seed(0)
    ac = ConstraintActorCritic(Box(-np.inf, np.inf, (obs_dim,)), Box(-1.0, 1.0, (act_dim,)),
                               Config.dict2config(d).model_cfgs, epochs=1, device=DEV)
    norm = Normalizer((obs_dim,), clip=5, device=DEV)
    norm.push(torch.randn(1024, obs_dim, device=DEV))
    torch.save({'pi': {k: v.cpu() for k, v in ac.actor.state_dict().items()},
                'obs_normalizer': {k: v.cpu() for k, v in norm.state_dict().items()}},
               os.path.join(root, 'torch_save', 'epoch-0.pt'))
    return root


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--ks', default='16,1024,16384')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cases', default='')
    args = ap.parse_args()
    ks = [int(k) for k in args.ks.split(',')]
    rows = []
    for env_id, env_cfgs in CASES:
        if args.cases and env_id not in args.cases.split(','):
            continue
        root = checkpoint(tempfile.mkdtemp(prefix='osa_eval_timing_'), env_id, env_cfgs)
        for K in ks:
            row = {'env': env_id, 'horizon': env_cfgs['horizon'], 'K': K}
            for path in ('persistent', 'per-step'):
                os.environ['OSA_EVAL_PATH'] = path
                ev = Evaluator(seed=0, device=DEV, verbose=False)
                ev.load_saved(root, 'epoch-0.pt')
                ev.evaluate(num_episodes=K)  # warm-up (code objects, allocations)
                ts = []
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r, _ = ev.evaluate(num_episodes=K)
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                assert np.isfinite(r).all() and ev.path == path
                key = path.replace('-', '_')
                row[f'{key}_s'] = round(statistics.median(ts), 6)
                row[f'{key}_us_per_step'] = round(1e6 * statistics.median(ts) / env_cfgs['horizon'], 2)
            row['speedup'] = round(row['per_step_s'] / row['persistent_s'], 2)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps({'tool': 'eval_timing', 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
                      'rows': rows}))


if __name__ == '__main__':
    main()
