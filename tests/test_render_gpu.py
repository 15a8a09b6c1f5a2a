"""GPU: osa_render_episode against its numpy twin (render_twin.py) byte for byte, and the public rendering surface
(Evaluator.render, Agent.render, DeviceVectorEnv.render) end to end.  Every comparison is np.array_equal on uint8."""
import json
import os

import numpy as np
import pytest
import torch

import car_twin
import circle_twin
import nav_twin
import render_twin as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RECORDS = 8
STILL, CORNER, ON_OBJECT = 4, 5, 6  # records made by hand: p of record 3 again, the arena's corner, on an object
SENTINEL = 0xA5


def walk(env_kind):
    """RECORDS state rows of one episode: a short random walk of the family's twin, then by hand two consecutive
    identical positions, the robot at the arena's corner (2, 2) (SynthReach: (1.5, 1.5)) and the robot exactly on an
    object (a hazard where the level has one, else the goal; the circle's centre on the circle tasks)."""
    rng = np.random.default_rng(env_kind)
    if env_kind == R.REACH:
        rows = rng.uniform(-1.5, 1.5, (RECORDS, 6)).astype(np.float32)
        rows[:, 2:] = rows[0, 2:]
        corner, obj = 1.5, rows[0, 4:6]
    else:
        family, level = env_kind // 16 * 16, env_kind % 16
        reset, step = {
            R.NAV0: (lambda: nav_twin.nav_reset(7, 0, 1, level),
                     lambda s, a, t: nav_twin.nav_step(s, a, level, 7, t)[0]),
            R.CIRCLE0: (lambda: circle_twin.circle_reset(7, 0, 1),
                        lambda s, a, t: circle_twin.circle_step(s, a, level)[0]),
            R.CARGOAL0: (lambda: car_twin.car_goal_reset(7, 0, 1, level),
                         lambda s, a, t: car_twin.car_goal_step(s, a, level, 7, t)[0]),
            R.CARCIRCLE0: (lambda: car_twin.car_circle_reset(7, 0, 1),
                           lambda s, a, t: car_twin.car_circle_step(s, a, level)[0]),
        }[family]
        s = reset()
        rows = np.zeros((RECORDS, s.shape[1]), np.float32)
        for t in range(RECORDS):
            rows[t] = s[0]
            # a strong, steady drive: the walk must cover more than a pixel per step
            s = step(s, np.array([[1.0, 0.6 * rng.uniform(-1, 1)]], np.float32), t + 1)
            s[0, 0:2] = np.clip(s[0, 0:2] + np.float32(0.15) * s[0, 2:4], -2, 2).astype(np.float32)
        corner = 2.0
        circle = family in (R.CIRCLE0, R.CARCIRCLE0)
        obj = (0.0, 0.0) if circle else (rows[0, 12:14] if level >= 1 else rows[0, 8:10])
    rows[STILL, 0:2] = rows[STILL - 1, 0:2]
    rows[CORNER, 0:2] = corner
    rows[ON_OBJECT, 0:2] = obj
    return rows


KINDS = {'reach': R.REACH, 'goal0': R.NAV0, 'goal2': R.NAV0 + 2, 'circle0': R.CIRCLE0, 'circle1': R.CIRCLE0 + 1,
         'circle2': R.CIRCLE0 + 2, 'cargoal1': R.CARGOAL0 + 1, 'carcircle2': R.CARCIRCLE0 + 2}
# (W, H): three workgroups per frame exactly; rows that are no multiple of 16 bytes, not square, one partial
# workgroup; the smallest frame; two workgroups per frame, the second partial (count * W * H / 4 = 8 * 300 lanes)
SHAPES = [(64, 48), (36, 20), (4, 1), (40, 30)]
HIT = np.array([0, 1, 0, 0, 1, 1, 0, 1], np.uint8)


def device_rows(rows, gap=5):
    """The rows on the device at a stride larger than a row, NaN in the gaps (and in front)."""
    F, w = rows.shape
    buf = torch.full((F + 1, w + gap), float('nan'), dtype=torch.float32, device=DEV)
    buf[1:, :w] = torch.from_numpy(rows).to(DEV)
    return buf, w + gap, w + gap  # tensor, offset of record 0, stride


def launch(env_kind, buf, offset, stride, first, count, trail, hit, camera, W, H, S):
    """One launch into the middle of a larger buffer; the 16 bytes on either side must stay as they were."""
    from omnisafe_amd import render as render_mod

    n = count * H * W * 3
    out = torch.full((n + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
    frames = render_mod.rasterise(env_kind, buf, offset, stride, first, count, trail, hit, camera, W, H, S,
                                  out=out[16:16 + n])
    got = frames.cpu().numpy()
    edge = out.cpu().numpy()
    assert (edge[:16] == SENTINEL).all() and (edge[16 + n:] == SENTINEL).all()
    return got


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name', list(KINDS))
def test_kernel_equals_twin(name, shape):
    env_kind, (W, H) = KINDS[name], shape
    rows = walk(env_kind)
    buf, offset, stride = device_rows(rows)
    hit_dev = torch.from_numpy(HIT).to(DEV)
    for S in (1, 2, 3):
        for trail in (0, 3, RECORDS + 3):
            for camera in (0, 1):
                for hit in (None, HIT):
                    want = R.render(env_kind, rows, 0, RECORDS, trail, hit, camera, W, H, S)
                    for first in (0, 2):
                        got = launch(env_kind, buf, offset, stride, first, RECORDS - first, trail,
                                     None if hit is None else hit_dev, camera, W, H, S)
                        assert np.array_equal(got, want[first:]), (name, shape, S, trail, camera, hit is None, first)


def test_walks_hold_the_cases_the_picture_must_survive():
    """The rows of test_kernel_equals_twin: a zero-length trail segment, the arena's corner, an object under the
    robot, and a walk long enough to leave a trail."""
    for name, env_kind in KINDS.items():
        rows = walk(env_kind)
        assert (rows[STILL, 0:2] == rows[STILL - 1, 0:2]).all(), name
        assert (rows[CORNER, 0:2] == (1.5 if env_kind == R.REACH else 2.0)).all(), name
        assert np.abs(rows[1:STILL, 0:2] - rows[0:STILL - 1, 0:2]).max() > 0.1, name
    assert (walk(R.NAV0 + 2)[ON_OBJECT, 0:2] == walk(R.NAV0 + 2)[0, 12:14]).all()
    assert (walk(R.NAV0)[ON_OBJECT, 0:2] == walk(R.NAV0)[0, 8:10]).all()


def test_chunked_launches_give_the_same_bytes():
    rng = np.random.default_rng(3)
    rows = np.zeros((10, 64), np.float32)
    rows[:, :] = nav_twin.nav_reset(11, 0, 1, 2)[0]
    rows[:, 0:2] = np.cumsum(rng.uniform(-0.2, 0.2, (10, 2)), 0).astype(np.float32)
    buf, offset, stride = device_rows(rows)
    args = (6, None, 1, 64, 48, 2)
    whole = launch(R.NAV0 + 2, buf, offset, stride, 0, 10, *args)
    parts = [launch(R.NAV0 + 2, buf, offset, stride, 0, 4, *args), launch(R.NAV0 + 2, buf, offset, stride, 4, 6, *args)]
    assert np.array_equal(whole, np.concatenate(parts))
    assert np.array_equal(whole, R.render(R.NAV0 + 2, rows, 0, 10, 6, None, 1, 64, 48, 2))


def test_trail_longer_than_a_staging_chunk():
    """600 records: the trail of the last frames is staged in three rounds."""
    t = np.linspace(0, 12 * np.pi, 600, dtype=np.float32)
    rows = np.zeros((600, 8), np.float32)
    rows[:, 0], rows[:, 1] = (1.5 * np.cos(t) * t / t[-1]).astype(np.float32), (1.5 * np.sin(t) * t / t[-1])
    rows[:, 2] = 1
    buf, offset, stride = device_rows(rows)
    got = launch(R.CIRCLE0 + 1, buf, offset, stride, 598, 2, 600, None, 0, 64, 48, 2)
    assert np.array_equal(got, R.render(R.CIRCLE0 + 1, rows, 598, 2, 600, None, 0, 64, 48, 2))


# ---------------------------------------------------------------------------------------------- end to end
def make_checkpoint(root, env_id, algo='PPOLag', env_cfgs=None, seed=0):
    """config.json + torch_save/epoch-0.pt as the logger writes them: a randomly initialised actor and observation
    statistics pushed from random data."""
    from omnisafe_amd.config import Config, get_default_kwargs
    from omnisafe_amd.envs import ENV_REGISTRY
    from omnisafe_amd.models import ConstraintActorCritic
    from omnisafe_amd.normalizer import Normalizer
    from omnisafe_amd.spaces import Box

    d = get_default_kwargs(algo)
    d.update({'algo': algo, 'env_id': env_id, 'exp_name': f'{algo}-{{{env_id}}}', 'seed': seed,
              'env_cfgs': dict(env_cfgs or {})})
    cfg = Config.dict2config(d)
    os.makedirs(os.path.join(root, 'torch_save'), exist_ok=True)
    with open(os.path.join(root, 'config.json'), 'w', encoding='utf-8') as f:
        json.dump(d, f)
    obs_dim, act_dim = ENV_REGISTRY[env_id].dims(env_id)
    torch.manual_seed(seed)
    ac = ConstraintActorCritic(Box(-np.inf, np.inf, (obs_dim,)), Box(-1.0, 1.0, (act_dim,)), cfg.model_cfgs,
                               epochs=1, device=DEV)
    norm = Normalizer((obs_dim,), clip=5, device=DEV)
    g = torch.Generator(device='cpu').manual_seed(seed + 1)
    for _ in range(3):
        norm.push((torch.randn(256, obs_dim, generator=g) * 0.7 + 0.1).to(DEV))
    torch.save({'pi': {k: v.detach().cpu() for k, v in ac.actor.state_dict().items()},
                'obs_normalizer': {k: v.detach().cpu() for k, v in norm.state_dict().items()}},
               os.path.join(root, 'torch_save', 'epoch-0.pt'))
    return str(root)


def files_of(folder):
    return {n: open(os.path.join(folder, n), 'rb').read() for n in sorted(os.listdir(folder))}


@pytest.mark.parametrize('env_id', ['SynthNavCircle1-v0', 'SynthNavCarGoal1-v0'])
def test_evaluator_render_end_to_end(tmp_path, monkeypatch, env_id):
    from omnisafe_amd import apng
    from omnisafe_amd.envs import ENV_REGISTRY
    from omnisafe_amd.evaluator import Evaluator

    root = make_checkpoint(tmp_path / 'run', env_id, env_cfgs={'horizon': 12})
    cls = ENV_REGISTRY[env_id]
    kind, state_w = cls.eval_kind(env_id), cls.trace_state_floats
    written = {}
    for path in ('persistent', 'per-step'):
        monkeypatch.setenv('OSA_EVAL_PATH', path)
        ev = Evaluator(seed=5, device=DEV, verbose=False)
        ev.load_saved(root, 'epoch-0.pt')
        out = str(tmp_path / path)
        rewards, costs = ev.render(num_episodes=3, width=64, height=48, trail=4, save_replay_path=out)
        assert ev.path == path and ev.episode_lengths == [12.0] * 3
        tr = ev.trace.cpu().numpy()
        written[path] = files_of(out)
        assert sorted(written[path]) == sorted([f'eval-episode-{k}.png' for k in range(3)]
                                               + [f'eval-episode-{k}-path.png' for k in range(3)] + ['result.txt'])
        rec = tr.shape[2]
        for k in range(3):
            rows = tr[:, k, rec - state_w:]
            hit = np.zeros(12, np.uint8)
            hit[1:] = tr[:-1, k, rec - state_w - 2] > 0
            frames = apng.read_apng(os.path.join(out, f'eval-episode-{k}.png'))
            assert len(frames) == 12
            assert np.array_equal(np.stack(frames), R.render(kind, rows, 0, 12, 4, hit, 0, 64, 48, 2))
            still = apng.read_apng(os.path.join(out, f'eval-episode-{k}-path.png'))
            assert len(still) == 1
            assert np.array_equal(still[0], R.render(kind, rows, 11, 1, 12, hit, 0, 64, 48, 2)[0])
        text = written[path]['result.txt'].decode()
        assert text.count('Episode reward:') == 3 and 'Average episode cost:' in text
        assert f'Episode reward: {rewards[0]}' in text and 'Episode length: 12.0' in text
        ev2 = Evaluator(seed=5, device=DEV, verbose=False)
        ev2.load_saved(root, 'epoch-0.pt')
        assert ev2.evaluate(num_episodes=3) == (rewards, costs)
    assert written['persistent'] == written['per-step']


def test_evaluator_render_options(tmp_path):
    """load_saved's render options are the defaults of render(); frame_skip and max_render_steps pick the frames."""
    from omnisafe_amd import apng
    from omnisafe_amd.evaluator import Evaluator

    root = make_checkpoint(tmp_path / 'run', 'SynthNavCircle2-v0', env_cfgs={'horizon': 12})
    ev = Evaluator(seed=2, device=DEV, verbose=False)
    ev.load_saved(root, 'epoch-0.pt', camera_name='track', width=36, height=20)
    ev.render(num_episodes=1, max_render_steps=9, frame_skip=4, trail=2, supersample=1)
    folder = os.path.join(root, 'video', 'epoch-0')  # the reference's default place
    frames = apng.read_apng(os.path.join(folder, 'eval-episode-0.png'))
    tr = ev.trace.cpu().numpy()
    rows = tr[:, 0, -8:]
    hit = np.zeros(12, np.uint8)
    hit[1:] = tr[:-1, 0, -10] > 0
    want = R.render(R.CIRCLE0 + 2, rows, 0, 9, 2, hit, 1, 36, 20, 1)
    assert len(frames) == 3 and np.array_equal(np.stack(frames), want[::4])
    with pytest.raises(ValueError):
        ev.render(camera_name='side')


def test_agent_render_round_trip(tmp_path):
    """Agent.learn() then Agent.render(): one folder of replays per epoch-N.pt of the run (reference quick-start)."""
    import omnisafe_amd
    from omnisafe_amd import apng

    horizon = 50
    cfg = {'seed': 1, 'train_cfgs': {'device': DEV, 'total_steps': 2 * 32 * horizon, 'vector_env_nums': 32},
           'algo_cfgs': {'steps_per_epoch': 32 * horizon, 'update_iters': 2, 'batch_size': 64},
           'logger_cfgs': {'log_dir': str(tmp_path), 'verbose': False, 'save_model_freq': 1},
           'env_cfgs': {'horizon': horizon}}
    agent = omnisafe_amd.Agent('PPOLag', 'SynthReach-v0', custom_cfgs=cfg)
    agent.learn()
    out = agent.render(num_episodes=2, width=32, height=32)
    names = list(out)
    assert len(names) >= 2 and names == sorted(names, key=lambda n: int(n[len('epoch-'):-len('.pt')]))
    for name, folder in out.items():
        assert folder == os.path.join(agent.agent.logger.log_dir, 'video', name[:-len('.pt')])
        animations = [n for n in sorted(os.listdir(folder)) if n.endswith('.png') and not n.endswith('-path.png')]
        assert animations == ['eval-episode-0.png', 'eval-episode-1.png']
        for n in animations:
            frames = apng.read_apng(os.path.join(folder, n))
            assert len(frames) == horizon and frames[0].shape == (32, 32, 3)


def test_env_render_is_the_twin_of_its_state():
    from omnisafe_amd import envs

    env = envs.make('SynthNavGoal1-v0', num_envs=3, device=DEV)
    env.set_seed(4)
    env.reset()
    state = env.state.cpu().numpy()
    for lane, camera in ((0, 'fixed'), (2, 'track')):
        img = env.render(lane=lane, width=64, height=48, camera_name=camera)
        assert img.dtype == np.uint8 and img.shape == (48, 64, 3)
        want = R.render(R.NAV0 + 1, state[lane:lane + 1], 0, 1, 0, None, int(camera == 'track'), 64, 48, 2)[0]
        assert np.array_equal(img, want)
    noise = envs.make('SynthTiny-v0', num_envs=2, device=DEV)
    with pytest.raises(NotImplementedError):
        noise.render()


def test_render_refuses_an_env_without_a_state_row(tmp_path):
    from omnisafe_amd.evaluator import Evaluator

    root = make_checkpoint(tmp_path / 'run', 'SynthPointGoal1-v0', env_cfgs={'horizon': 8})
    ev = Evaluator(seed=0, device=DEV, verbose=False)
    ev.load_saved(root, 'epoch-0.pt')
    with pytest.raises(ValueError, match='no state row'):
        ev.render(num_episodes=1, save_replay_path=str(tmp_path / 'out'))
