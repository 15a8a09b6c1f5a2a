"""Time of the generic scene rasteriser (osa_custom_render_episode) against the built-in one (osa_render_episode) on
the same rows, and of the hipcc run that makes a custom library.

    python tools/custom_render_timing.py                      # the kernels (needs the GPU)
    python tools/custom_render_timing.py --compile [--parent-tree DIR]    # the compiler (needs none)

Both write their section ('kernel' / 'compile') into --out (profiles/custom_render_timing.json) and keep the other.

Kernel: 1000 records of a synthetic walk, 256 x 256, 2 x 2 sub-samples, a 50-step trail, fixed camera.  Per pair
  (ReachDrawn, SynthReach-v0) and (CircleDrawn level 1, SynthNavCircle1-v0)
device events round one launch of the 1000 frames, median of 5 after a warm-up launch, both kernels in this process;
the two outputs must be equal byte for byte.  ms per 1000 frames = us per frame.
Compile: wall seconds of the one hipcc command of omnisafe_amd.build.build_custom_env, straight to a scratch file (no
cache), best of --repeats runs, for ReachAgain (no draw(): what every existing description pays for the two new entry
points) and ReachDrawn / CircleDrawn / LedgeDrawn (four more kernels).  --parent-tree names a checkout of the commit
before the rasteriser; its csrc/custom/custom_env.hip compiles ReachAgain the same way for the 'before' figure."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENVS = os.path.join(ROOT, 'tests', 'custom_envs')
RECORDS, SIZE, S, TRAIL = 1000, 256, 2, 50
PAIRS = [('reach_drawn.h', 'ReachDrawn', 0, 'SynthReach-v0'), ('circle_drawn.h', 'CircleDrawn', 1, 'SynthNavCircle1-v0')]


def rows_of(width: int):
    """A walk that stays in the arena: p on a slow spiral with a heading u along it; a goal and a hazard behind."""
    import numpy as np

    t = np.linspace(0, 16 * np.pi, RECORDS, dtype=np.float32)
    rows = np.zeros((RECORDS, width), np.float32)
    rows[:, 0], rows[:, 1] = 1.2 * np.cos(t) * (0.3 + 0.7 * t / t[-1]), 1.2 * np.sin(t) * (0.3 + 0.7 * t / t[-1])
    rows[:, 2], rows[:, 3] = -np.sin(t), np.cos(t)
    if width == 6:  # SynthReach: goal and hazard in place of the heading
        rows[:, 2:4], rows[:, 4:6] = (0.8, -0.6), (-0.5, 0.7)
    return rows


def time_kernels() -> dict:
    import numpy as np
    import torch

    import omnisafe_amd
    from omnisafe_amd import envs, render as render_mod

    out = {'device': torch.cuda.get_device_name(0), 'records': RECORDS, 'width': SIZE, 'height': SIZE,
           'supersample': S, 'trail': TRAIL, 'rows': []}
    for header, struct, level, env_id in PAIRS:
        custom_id = f'{struct}Timing-v0'
        cls = omnisafe_amd.register_device_env(os.path.join(ENVS, header), struct, {custom_id: level})
        built_in = envs.ENV_REGISTRY[env_id]
        rows = torch.from_numpy(rows_of(cls.trace_state_floats)).to('cuda:0')
        frames = [torch.empty(RECORDS * SIZE * SIZE * 3, dtype=torch.uint8, device='cuda:0') for _ in range(2)]
        kinds = {'scene': cls.render_kind(custom_id), 'built_in': built_in.render_kind(env_id)}
        ms = {}
        for (name, kind), buf in zip(kinds.items(), frames):
            at = (kind, rows, 0, rows.shape[1], 0, RECORDS, TRAIL, None, 0, SIZE, SIZE, S, buf)
            render_mod.rasterise(*at)  # warm-up (code object)
            ms[name] = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                render_mod.rasterise(*at)
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        assert torch.equal(frames[0], frames[1]), f'{struct} and {env_id} disagree'
        med = {k: statistics.median(v) for k, v in ms.items()}
        out['rows'].append({'custom': struct, 'level': level, 'built_in': env_id,
                            'scene_us_per_frame': round(med['scene'], 3),
                            'built_in_us_per_frame': round(med['built_in'], 3),
                            'ratio': round(med['scene'] / med['built_in'], 3),
                            'scene_ms_all_5': [round(m, 3) for m in ms['scene']],
                            'built_in_ms_all_5': [round(m, 3) for m in ms['built_in']], 'bytes_equal': True})
        omnisafe_amd.unregister_device_env(custom_id)
        print(json.dumps(out['rows'][-1]), file=sys.stderr, flush=True)
    assert np.isfinite([r['ratio'] for r in out['rows']]).all()
    return out


def hipcc_seconds(tree: str, header: str, struct: str, repeats: int) -> list:
    from omnisafe_amd import build

    src = os.path.join(tree, 'omnisafe_amd', 'csrc', 'custom', 'custom_env.hip')
    took = []
    with tempfile.TemporaryDirectory(prefix='osa_custom_render_timing_') as tmp:
        for _ in range(repeats):
            cmd = [build._hipcc(), *build.CUSTOM_FLAGS, f'-DOSA_CUSTOM_ENV_HEADER="{os.path.join(ENVS, header)}"',  # noqa: SLF001
                   f'-DOSA_CUSTOM_ENV={struct}', src, '-o', os.path.join(tmp, 'lib.so')]
            t0 = time.perf_counter()
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            took.append(round(time.perf_counter() - t0, 2))
    return took


def time_compiles(parent_tree: str, repeats: int) -> dict:
    out = {'cpus': os.cpu_count(), 'repeats': repeats, 'rows': []}
    cases = [(ROOT, 'after', 'reach_again.h', 'ReachAgain'), (ROOT, 'after', 'reach_drawn.h', 'ReachDrawn'),
             (ROOT, 'after', 'circle_drawn.h', 'CircleDrawn'), (ROOT, 'after', 'ledge.h', 'Ledge'),
             (ROOT, 'after', 'ledge_drawn.h', 'LedgeDrawn')]
    if parent_tree:
        cases = [(parent_tree, 'before', 'reach_again.h', 'ReachAgain'), (parent_tree, 'before', 'ledge.h', 'Ledge')] + cases
    for tree, when, header, struct in cases:
        took = hipcc_seconds(tree, header, struct, repeats)
        out['rows'].append({'when': when, 'struct': struct, 'hipcc_s': min(took), 'hipcc_s_all': took})
        print(json.dumps(out['rows'][-1]), file=sys.stderr, flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'custom_render_timing.json'))
    ap.add_argument('--compile', action='store_true')
    ap.add_argument('--parent-tree', default='')
    ap.add_argument('--repeats', type=int, default=2)
    args = ap.parse_args()
    result = {'tool': 'custom_render_timing'}
    if os.path.exists(args.out):
        with open(args.out, encoding='utf-8') as f:
            result.update(json.load(f))
    if args.compile:
        result['compile'] = time_compiles(args.parent_tree, args.repeats)
    else:
        result['kernel'] = time_kernels()
    with open(args.out, 'w', encoding='utf-8') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
