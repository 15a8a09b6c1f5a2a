"""Time of rendered replays (osa_render_episode, Evaluator.render) and of the numpy twin of the picture.

    python tools/render_timing.py [--out profiles/render_timing.json] [--examples tests/golden/render_examples]

Cases: SynthNavGoal2-v0 and SynthNavCircle1-v0, one episode of 1000 records, 256 x 256, 2 x 2 sub-samples, a 50-step
trail, fixed camera; a randomly initialised PPOLag checkpoint with an active observation normaliser.  Per case:
  kernel_us_per_frame   device events round one launch for the 1000 frames; median of 5 after a warm-up launch
  render_s              host clock round Evaluator.render (ends in a device synchronisation), the median call of 3
                        after a warm-up, split into play (evaluate with the trace), raster (launches until done), copy
                        (device to pinned host) and encode (zlib level 1 and file writes; the rest of the call)
  twin_s_1000_frames    tests/render_twin.py on the same rows on the host: 20 frames timed, scaled by 50
--examples trains PPOLag (seed 0, 256 envs, horizon 200, 10 epochs of 51 200 steps: the set-up of
profiles/circle_learning.md and nav_learning.md) on SynthNavCircle1-v0 and SynthNavGoal1-v0 and writes the path still of
one episode of each final checkpoint there.  Prints one JSON line and writes it to --out."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import render_twin  # noqa: E402

import omnisafe_amd  # noqa: E402
from omnisafe_amd import render as render_mod  # noqa: E402
from omnisafe_amd.config import Config, get_default_kwargs  # noqa: E402
from omnisafe_amd.envs import ENV_REGISTRY  # noqa: E402
from omnisafe_amd.evaluator import Evaluator  # noqa: E402
from omnisafe_amd.models import ConstraintActorCritic  # noqa: E402
from omnisafe_amd.normalizer import Normalizer  # noqa: E402
from omnisafe_amd.spaces import Box  # noqa: E402

DEV = 'cuda:0'
CASES = ['SynthNavGoal2-v0', 'SynthNavCircle1-v0']
RECORDS, SIZE, S, TRAIL, TWIN_FRAMES = 1000, 256, 2, 50, 20


def checkpoint(root: str, env_id: str) -> str:
    d = get_default_kwargs('PPOLag')
    d.update({'algo': 'PPOLag', 'env_id': env_id, 'exp_name': 'render_timing', 'seed': 0,
              'env_cfgs': {'horizon': RECORDS}})
    os.makedirs(os.path.join(root, 'torch_save'), exist_ok=True)
    with open(os.path.join(root, 'config.json'), 'w', encoding='utf-8') as f:
        json.dump(d, f)
    obs_dim, act_dim = ENV_REGISTRY[env_id].dims(env_id)
    torch.manual_seed(0)
    ac = ConstraintActorCritic(Box(-np.inf, np.inf, (obs_dim,)), Box(-1.0, 1.0, (act_dim,)),
                               Config.dict2config(d).model_cfgs, epochs=1, device=DEV)
    norm = Normalizer((obs_dim,), clip=5, device=DEV)
    norm.push(torch.randn(1024, obs_dim, device=DEV))
    torch.save({'pi': {k: v.cpu() for k, v in ac.actor.state_dict().items()},
                'obs_normalizer': {k: v.cpu() for k, v in norm.state_dict().items()}},
               os.path.join(root, 'torch_save', 'epoch-0.pt'))
    return root


def time_case(env_id: str) -> dict:
    root = checkpoint(tempfile.mkdtemp(prefix='osa_render_timing_'), env_id)
    out = os.path.join(root, 'replay')
    ev = Evaluator(seed=0, device=DEV, verbose=False)
    ev.load_saved(root, 'epoch-0.pt')
    kw = dict(num_episodes=1, save_replay_path=out, width=SIZE, height=SIZE, trail=TRAIL, supersample=S)
    ev.render(**kw)  # warm-up (code objects, allocations)
    calls = []
    for _ in range(3):
        shutil.rmtree(out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.render(**kw)
        torch.cuda.synchronize()
        calls.append((time.perf_counter() - t0, dict(ev.render_clock)))
    wall, clock = sorted(calls, key=lambda c: c[0])[1]
    size = os.path.getsize(os.path.join(out, 'eval-episode-0.png'))
    # the kernel alone, on the rows of that episode
    cls = ENV_REGISTRY[env_id]
    kind, state_w = cls.eval_kind(env_id), cls.trace_state_floats
    tr = ev.trace.contiguous()
    T, K, rec = tr.shape
    assert (T, K) == (RECORDS, 1) and ev.episode_lengths == [float(RECORDS)]
    frames = torch.empty(RECORDS * SIZE * SIZE * 3, dtype=torch.uint8, device=DEV)
    at = (kind, tr, rec - state_w, rec, 0, RECORDS, TRAIL, None, 0, SIZE, SIZE, S, frames)
    render_mod.rasterise(*at)
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        render_mod.rasterise(*at)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    # the twin on the host: the last TWIN_FRAMES frames (full trails), scaled to the episode
    rows = tr[:, 0, rec - state_w:].cpu().numpy()
    t0 = time.perf_counter()
    want = render_twin.render(kind, rows, RECORDS - TWIN_FRAMES, TWIN_FRAMES, TRAIL, None, 0, SIZE, SIZE, S)
    twin = time.perf_counter() - t0
    got = frames.view(RECORDS, SIZE, SIZE, 3)[RECORDS - TWIN_FRAMES:].cpu().numpy()
    assert np.array_equal(got, want), 'kernel and twin disagree'
    return {'env': env_id, 'records': RECORDS, 'width': SIZE, 'height': SIZE, 'supersample': S, 'trail': TRAIL,
            'kernel_ms_1000_frames': round(statistics.median(ms), 3),
            'kernel_us_per_frame': round(statistics.median(ms), 3),  # ms per 1000 frames = us per frame
            'kernel_ms_all_5': [round(m, 3) for m in ms],
            'render_s': round(wall, 4), 'render_split_s': {k: round(v, 4) for k, v in clock.items()},
            'render_s_all_3': [round(c[0], 4) for c in calls], 'apng_bytes': size,
            'twin_s_timed_frames': round(twin, 3), 'twin_frames_timed': TWIN_FRAMES,
            'twin_s_1000_frames': round(twin * RECORDS / TWIN_FRAMES, 1),
            'twin_note': f'{TWIN_FRAMES} frames rendered on the host and scaled by {RECORDS // TWIN_FRAMES}; their '
                         'bytes equal the kernel\'s'}


def examples(folder: str) -> list:
    """Path stills of trained policies (PPOLag, seed 0, the budget of the learning reports)."""
    os.makedirs(folder, exist_ok=True)
    made = []
    for env_id, lagrange in (('SynthNavCircle1-v0', {}), ('SynthNavGoal1-v0', {'cost_limit': 5.0})):
        log_dir = tempfile.mkdtemp(prefix='osa_render_examples_')
        custom = {'seed': 0, 'train_cfgs': {'device': DEV, 'total_steps': 512_000, 'vector_env_nums': 256},
                  'algo_cfgs': {'steps_per_epoch': 51_200},
                  'logger_cfgs': {'log_dir': log_dir, 'verbose': False, 'save_model_freq': 10},
                  'env_cfgs': {'horizon': 200}}
        if lagrange:
            custom['lagrange_cfgs'] = lagrange
        agent = omnisafe_amd.Agent('PPOLag', env_id, custom_cfgs=custom)
        ret, cost, _ = agent.learn()
        run = agent.agent.logger.log_dir
        last = agent._saved_models()[-1]  # noqa: SLF001
        ev = Evaluator(seed=0, device=DEV, verbose=False)
        ev.load_saved(run, last)
        out = os.path.join(log_dir, 'replay')
        rewards, costs = ev.render(num_episodes=1, save_replay_path=out, width=256, height=256)
        name = f'{env_id[:-3]}_PPOLag_seed0_{last[:-3]}_path.png'
        shutil.copy(os.path.join(out, 'eval-episode-0-path.png'), os.path.join(folder, name))
        made.append({'file': name, 'env': env_id, 'checkpoint': last, 'episode_reward': rewards[0],
                     'episode_cost': costs[0], 'episode_length': ev.episode_lengths[0],
                     'last_epoch_EpRet': ret, 'last_epoch_EpCost': cost})
    return made


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render_timing.json'))
    ap.add_argument('--examples', default='')
    args = ap.parse_args()
    result = {'tool': 'render_timing', 'device': torch.cuda.get_device_name(0), 'rows': []}
    for env_id in CASES:
        result['rows'].append(time_case(env_id))
        print(json.dumps(result['rows'][-1]), file=sys.stderr, flush=True)
    if args.examples:
        result['examples'] = examples(args.examples)
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
