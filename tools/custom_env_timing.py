"""Device time of one vector step of device envs registered from a header (register_device_env), next to the built-in
SynthReach-v0, in the same process.

    python tools/custom_env_timing.py [--n 4096] [--steps 1000] [--reps 5] [--rollout-steps 100] [--build-only]

Rows: SynthReach-v0 (osa_reach_env_kernel: one wave per env, 60-column rows); the same description through the generic
kernel osa_custom_env_kernel at 16 / 32 / 64 lanes per env with the same 60-column row (tools/custom_envs/reach_lanes.h)
and with its 6 native columns; the example env of the tests (tests/custom_envs/glider.h: 70 columns, 3 actions); the
terminating example env (tests/custom_envs/ledge.h: 20 columns, a terminal() member) and the same env without the
member, each at 16 / 32 / 64 lanes.
Each: `--steps` calls of env.step() captured as one hipGraph (the form the rollout runs them in), replayed after a
warm-up replay; HIP events around a replay, median and min / max of `--reps` replays, divided by `--steps`; also the
same launches issued eagerly back to back.  `terminal_hook`: Ledge minus LedgeEndless per lane count (what asking
terminal() and ending episodes per env costs; the envs of a Ledge run reset at different steps).
`rollout`: the whole vector step of OnPolicyAdapter.rollout (PPOLag, captured graph, as tools/nav_env_timing.py times
it) with `--rollout-steps` steps per env at a horizon of a quarter of that, on Ledge1-v0 and LedgeEndless1-v0: a
terminating class hands out the final observations on every step from the horizon on (3/4 of the steps), the other on
every horizon-th step; the difference is what the always-on path costs.  --rollout-steps 0 leaves it out.
--build-only compiles the libraries and stops (no GPU needed).
Prints one JSON line (profiles/custom_env_timing.json)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import omnisafe_amd  # noqa: E402
from omnisafe_amd import envs  # noqa: E402

DEV = 'cuda:0'
REACH = os.path.join(ROOT, 'tools', 'custom_envs', 'reach_lanes.h')
GLIDER = os.path.join(ROOT, 'tests', 'custom_envs', 'glider.h')
LEDGE = os.path.join(ROOT, 'tests', 'custom_envs', 'ledge.h')
LEDGE_LANES = os.path.join(ROOT, 'tools', 'custom_envs', 'ledge_lanes.h')
CUSTOM = [(REACH, 'ReachWide16'), (REACH, 'ReachWide32'), (REACH, 'ReachWide64'), (REACH, 'Reach6'),
          (GLIDER, 'Glider'),
          (LEDGE_LANES, 'LedgeEndless16'), (LEDGE, 'LedgeEndless'), (LEDGE_LANES, 'LedgeEndless64'),
          (LEDGE, 'Ledge16'), (LEDGE, 'Ledge'), (LEDGE, 'Ledge64')]
HOOK_PAIRS = [('Ledge16', 'LedgeEndless16'), ('Ledge', 'LedgeEndless'), ('Ledge64', 'LedgeEndless64')]


def timed(fn, reps: int) -> list[float]:
    """Milliseconds of `reps` calls of fn(), each between two HIP events."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def env_step_row(env_id: str, n: int, steps: int, reps: int) -> dict:
    env = envs.make(env_id, num_envs=n, device=DEV, horizon=1000, seed=0)
    env.reset()
    obs_dim, act_dim = env.observation_space.shape[0], env.action_space.shape[0]
    act = (torch.randn(n, act_dim, generator=torch.Generator(device='cpu').manual_seed(0)) * 1.5).to(DEV)

    def run():
        for _ in range(steps):
            env.step(act)

    run()  # warm-up: code objects
    torch.cuda.synchronize()
    eager = timed(run, reps)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            run()
        graph.replay()
        stream.synchronize()
        graphed = timed(graph.replay, reps)
    return {'env': env_id, 'kernel': 'osa_custom_env_kernel' if isinstance(env, envs.CustomDeviceEnv) else 'built-in',
            'lanes_per_env': getattr(env, 'lanes', 64), 'terminates': bool(getattr(env, 'terminates', False)),
            'obs_columns': obs_dim, 'act_columns': act_dim, 'n': n,
            'steps': steps, 'graph_us_per_step': round(1e3 * statistics.median(graphed) / steps, 3),
            'graph_us_per_step_min_max': [round(1e3 * min(graphed) / steps, 3), round(1e3 * max(graphed) / steps, 3)],
            'eager_us_per_step': round(1e3 * statistics.median(eager) / steps, 3)}


def rollout_row(env_id: str, n: int, t_steps: int, horizon: int, reps: int) -> dict:
    """tools/nav_env_timing.py's rollout_row at a horizon below the epoch's steps per env."""
    import tempfile

    cfg = {'seed': 0, 'train_cfgs': {'device': DEV, 'total_steps': (2 + reps) * n * t_steps, 'vector_env_nums': n},
           'algo_cfgs': {'steps_per_epoch': n * t_steps},
           'logger_cfgs': {'log_dir': tempfile.mkdtemp(prefix='osa_custom_timing_'), 'verbose': False},
           'env_cfgs': {'horizon': horizon}}
    algo = omnisafe_amd.Agent('PPOLag', env_id, custom_cfgs=cfg).agent

    def epoch():
        algo._env.rollout(steps_per_epoch=algo._steps_per_epoch, agent=algo._actor_critic, buffer=algo._buf,
                          logger=algo._logger)

    ms = []
    for e in range(2 + reps):  # the second epoch captures the graph; the update between rollouts is not timed
        torch.cuda.synchronize()
        t = timed(epoch, 1)
        if e >= 2:
            ms += t
        algo._update()
        algo._logger.dump_tabular()
    assert algo._env.last_rollout_graphed
    terminates = bool(algo._env._env.terminates)
    with_final = t_steps - horizon + 1 if terminates else t_steps // horizon
    return {'env': env_id, 'terminates': terminates, 'n': n, 'vector_steps_per_epoch': t_steps, 'horizon': horizon,
            'steps_with_final_observation': with_final,
            'rollout_us_per_vector_step': round(1e3 * statistics.median(ms) / t_steps, 2),
            'rollout_us_per_vector_step_min_max': [round(1e3 * min(ms) / t_steps, 2),
                                                   round(1e3 * max(ms) / t_steps, 2)]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rollout-steps', type=int, default=100)
    ap.add_argument('--build-only', action='store_true')
    args = ap.parse_args()
    ids = ['SynthReach-v0']
    for header, struct in CUSTOM:
        omnisafe_amd.register_device_env(header, struct, [struct + '-v0'])
        ids.append(struct + '-v0')
    omnisafe_amd.register_device_env(LEDGE, 'Ledge', {'Ledge1-v0': 1})
    omnisafe_amd.register_device_env(LEDGE, 'LedgeEndless', {'LedgeEndless1-v0': 1})
    if args.build_only:
        print(json.dumps({'built': [envs.CUSTOM_ENV_REGISTRY[e].lib_path for e in ids[1:]]}))
        return
    rows = [env_step_row(e, args.n, args.steps, args.reps) for e in ids]
    for r in rows:
        print(json.dumps(r), file=sys.stderr, flush=True)
    by_env = {r['env']: r for r in rows}
    hook = [{'lanes_per_env': by_env[a + '-v0']['lanes_per_env'], 'with': a + '-v0', 'without': b + '-v0',
             'graph_us_per_step_difference': round(by_env[a + '-v0']['graph_us_per_step']
                                                   - by_env[b + '-v0']['graph_us_per_step'], 3)}
            for a, b in HOOK_PAIRS]
    out = {'tool': 'custom_env_timing', 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'env_step': rows, 'terminal_hook': hook}
    if args.rollout_steps > 0:
        T = args.rollout_steps
        ro = [rollout_row(e, args.n, T, max(1, T // 4), args.reps) for e in ('LedgeEndless1-v0', 'Ledge1-v0')]
        for r in ro:
            print(json.dumps(r), file=sys.stderr, flush=True)
        extra = ro[1]['steps_with_final_observation'] - ro[0]['steps_with_final_observation']
        diff = ro[1]['rollout_us_per_vector_step'] - ro[0]['rollout_us_per_vector_step']
        out['rollout'] = ro
        out['final_observation_path'] = {
            'rollout_us_per_vector_step_difference': round(diff, 2),
            'us_per_additional_step_with_final_observation': round(diff * T / extra, 2) if extra else None}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
