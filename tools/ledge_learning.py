"""PPO on Ledge0-v0 (tests/custom_envs/ledge.h, a device env that ends its own episodes) for ten short epochs:
Metrics/EpLen, EpRet and EpCost per epoch, directional only (profiles/ledge_learning.md).

    python tools/ledge_learning.py

Prints one JSON line."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import omnisafe_amd  # noqa: E402

LEDGE = os.path.join(ROOT, 'tests', 'custom_envs', 'ledge.h')
omnisafe_amd.register_device_env(LEDGE, 'Ledge', {'Ledge0-v0': 0, 'Ledge1-v0': 1}, default_horizon=60)
n, t, epochs = 256, 120, 10
cfg = {'seed': 0, 'train_cfgs': {'device': 'cuda:0', 'total_steps': epochs * n * t, 'vector_env_nums': n},
       'algo_cfgs': {'steps_per_epoch': n * t},
       'logger_cfgs': {'log_dir': tempfile.mkdtemp(prefix='ledge_learning_'), 'verbose': False}}
agent = omnisafe_amd.Agent('PPO', 'Ledge0-v0', custom_cfgs=cfg)
agent.learn()
lines = [ln for ln in open(os.path.join(agent.agent.logger.log_dir, 'progress.csv')).read().split('\n') if ln]
hdr = lines[0].split(',')
cols = [hdr.index(k) for k in ('Metrics/EpLen', 'Metrics/EpRet', 'Metrics/EpCost')]
rows = [[float(ln.split(',')[c]) for c in cols] for ln in lines[1:]]
print(json.dumps({'env': 'Ledge0-v0', 'algo': 'PPO', 'envs': n, 'steps_per_env': t, 'horizon': 60,
                  'epoch_rows_EpLen_EpRet_EpCost': rows}))
