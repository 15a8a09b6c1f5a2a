"""GPU: the generic scene rasteriser (osa_custom_render_episode, csrc/scene_render.h) byte for byte against the
built-in osa_render_episode where a draw() restates a built-in picture, and against its numpy twin (scene_twin.py)
where the picture is the description's own; then the public surface (CustomDeviceEnv.render, Evaluator.render,
AgentGroup.render) end to end.  Every comparison is np.array_equal on uint8."""
import os

import numpy as np
import pytest
import torch

import ledge_twin as L
import render_twin as R
import scene_twin as T
from test_scene_twin import HIT, RECORDS, SCENES, walk

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ENVS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'custom_envs')
SENTINEL = 0xA5
EINVAL, EUNSUPPORTED = -1, -3  # OSA_EINVAL, OSA_EUNSUPPORTED (include/omnisafe_amd.h)
# (W, H): three workgroups per frame exactly; rows that are no multiple of 16 bytes and one partial workgroup; the
# smallest frame; two workgroups per frame, the second partial
SHAPES = [(64, 48), (36, 20), (4, 1), (40, 30)]
_LIBS = {}


def library(header, struct):
    """The struct's library (cached by build()), its prototypes declared."""
    from omnisafe_amd import _lib, build, envs

    if struct not in _LIBS:
        _lib.load(require_gpu=True)
        _LIBS[struct] = envs._bind_custom(build.build_custom_env(os.path.join(ENVS, header), struct))[0]
    return _LIBS[struct]


def device_rows(rows, gap=5):
    """The rows on the device at a stride larger than a row, NaN in the gaps (and in front)."""
    n, w = rows.shape
    buf = torch.full((n + 1, w + gap), float('nan'), dtype=torch.float32, device=DEV)
    buf[1:, :w] = torch.from_numpy(rows).to(DEV)
    return buf, w + gap, w + gap  # tensor, offset of record 0, stride


def launch(lib, level, buf, offset, stride, first, count, trail, hit, camera, W, H, S, expect=0):
    """One launch into the middle of a sentinel-filled buffer; the 16 bytes on either side must stay as they were
    (and with ``expect`` an error code, every byte)."""
    from omnisafe_amd import _lib

    n = count * H * W * 3
    out = torch.full((n + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
    code = lib.osa_custom_render_episode(level, buf.data_ptr() + 4 * offset, stride, first, count, trail, _lib.ptr(hit),
                                         camera, W, H, S, out.data_ptr() + 16, _lib.stream_ptr())
    assert code == expect, code
    whole = out.cpu().numpy()
    assert (whole[:16] == SENTINEL).all() and (whole[16 + n:] == SENTINEL).all()
    if expect:
        assert (whole == SENTINEL).all()
    return whole[16:16 + n].reshape(count, H, W, 3)


def built_in(env_kind, buf, offset, stride, first, count, trail, hit, camera, W, H, S):
    from omnisafe_amd import render as render_mod

    return render_mod.rasterise(env_kind, buf, offset, stride, first, count, trail, hit, camera, W, H, S).cpu().numpy()


# ------------------------------------------------------------------ 1. a restated picture equals the built-in kernel
@pytest.mark.parametrize('name', list(SCENES))
def test_a_restated_picture_equals_the_built_in_kernel(name):
    env_kind, _, _, level = SCENES[name]
    lib = library('reach_drawn.h', 'ReachDrawn') if name == 'reach' else library('circle_drawn.h', 'CircleDrawn')
    buf, offset, stride = device_rows(walk(env_kind))
    hit_dev = torch.from_numpy(HIT).to(DEV)
    for W, H in ((64, 48), (36, 20)):
        for S in (1, 2, 3, 4):
            for trail in (0, 3, RECORDS + 3):
                for camera in (0, 1):
                    for hit in (None, hit_dev):
                        for first in (0, 2):
                            args = (buf, offset, stride, first, RECORDS - first, trail, hit, camera, W, H, S)
                            assert np.array_equal(launch(lib, level, *args), built_in(env_kind, *args)), \
                                (name, W, H, S, trail, camera, hit is None, first)


# ------------------------------------------------------------------ 2. a picture of its own equals the twin
def ledge_rows(n=RECORDS):
    """Records of a walk along the ledge: p, v, steps.  By hand: two consecutive identical positions (a trail segment
    of length zero), a walker at rest (a velocity segment of length zero) and one off the ledge."""
    rng = np.random.default_rng(9)
    rows = np.zeros((n, L.TRACE), np.float32)
    rows[:, 0] = np.cumsum(rng.uniform(0.2, 0.5, n)).astype(np.float32) - 0.3
    rows[:, 1] = rng.uniform(-0.9, 0.9, n).astype(np.float32)
    rows[:, 2:4] = rng.uniform(-0.12, 0.12, (n, 2)).astype(np.float32)
    rows[:, 4] = np.arange(n)
    rows[4, 0:2] = rows[3, 0:2]
    rows[5, 2:4] = 0
    rows[6, 1] = 1.25
    return rows


def ledge_twin(rows, first, count, trail, hit, camera, W, H, S, level):
    return T.render(T.ledge_draw, T.position, T.LEDGE_VIEW, rows, first, count, trail, hit, camera, W, H, S,
                    level=level, track=T.LEDGE_TRACK)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_ledge_drawn_equals_the_twin(shape):
    W, H = shape
    lib = library('ledge_drawn.h', 'LedgeDrawn')
    rows = ledge_rows()
    buf, offset, stride = device_rows(rows)
    hit_dev = torch.from_numpy(HIT).to(DEV)
    cases = [(S, trail, camera, hit) for S in (1, 2, 3) for trail in (0, 3, RECORDS + 3) for camera in (0, 1)
             for hit in (None, HIT)]
    if shape == (36, 20):
        cases.append((4, 3, 1, HIT))
    for n, (S, trail, camera, hit) in enumerate(cases):
        level = n % 2
        want = ledge_twin(rows, 0, RECORDS, trail, hit, camera, W, H, S, level)
        for first in (0, 2):
            got = launch(lib, level, buf, offset, stride, first, RECORDS - first, trail,
                         None if hit is None else hit_dev, camera, W, H, S)
            assert np.array_equal(got, want[first:]), (shape, S, trail, camera, hit is None, first, level)
    # the picture has something of everything: floor, cost strip, goal, line, trail, halo (both colours), walker, velocity
    seen = {tuple(p) for p in ledge_twin(rows, 0, RECORDS, 3, HIT, 0, 64, 48, 1, 1).reshape(-1, 3)}
    for colour in (T.COLOUR['FLOOR'], T.COLOUR['COST'], T.COLOUR['GOAL'], 0x9098A0, T.COLOUR['TRAIL'], 0x3070C0,
                   T.COLOUR['HIT'], T.COLOUR['POINT'], T.COLOUR['HEADING'], T.COLOUR['OUTSIDE']):
        assert (colour >> 16, (colour >> 8) & 255, colour & 255) in seen, hex(colour)


# ------------------------------------------------------------------ 3. a trail longer than a staging chunk
def test_trail_staged_in_two_rounds():
    """300 records, frames 298 and 299, trail 300: 298 and 299 segments, staged as 256 + the rest."""
    t = np.linspace(0, 10 * np.pi, 300, dtype=np.float32)
    rows = np.zeros((300, L.TRACE), np.float32)
    rows[:, 0] = (1.25 + 1.6 * np.cos(t) * t / t[-1]).astype(np.float32)
    rows[:, 1] = (0.9 * np.sin(t) * t / t[-1]).astype(np.float32)
    rows[:, 2] = 0.05
    buf, offset, stride = device_rows(rows)
    got = launch(library('ledge_drawn.h', 'LedgeDrawn'), 1, buf, offset, stride, 298, 2, 300, None, 0, 64, 48, 2)
    assert np.array_equal(got, ledge_twin(rows, 298, 2, 300, None, 0, 64, 48, 2, 1))


# ------------------------------------------------------------------ 4. the size of a scene
def test_scene_size():
    rows = walk(R.REACH)
    buf, offset, stride = device_rows(rows)
    args = (buf, offset, stride, 0, RECORDS, 5, None, 0, 64, 64, 1)
    nothing = launch(library('scene_caps.h', 'DrawNothing'), 0, *args)
    assert (nothing == R.PALETTE[R.OUTSIDE]).all()
    full = launch(library('scene_caps.h', 'DrawFull'), 0, *args)
    want = T.render(T.caps_draw(T.DRAW_MAX), T.position, 2.0, rows, 0, RECORDS, 5, None, 0, 64, 64, 1)
    assert np.array_equal(full, want)
    seen = {tuple(p) for p in full[0].reshape(-1, 3)}
    for k in range(T.DRAW_MAX):  # every one of the OSA_DRAW_MAX primitives shows
        colour = 0x010203 * (k + 1)
        assert (colour >> 16, (colour >> 8) & 255, colour & 255) in seen, k
    over = launch(library('scene_caps.h', 'DrawOver'), 0, *args)
    assert np.array_equal(over, full)  # the three past the cap (a box, the trail, a disc over everything) are dropped
    assert not np.array_equal(
        want, T.render(lambda *a: T.caps_draw(T.DRAW_MAX + 3)(*a)[3:], T.position, 2.0, rows, 0, RECORDS, 5, None, 0,
                       64, 64, 1))  # (they would have shown)


# ------------------------------------------------------------------ 5. argument checks, without a launch
def test_bad_arguments_start_no_kernel():
    drawn, plain = library('ledge_drawn.h', 'LedgeDrawn'), library('ledge.h', 'Ledge')
    buf, offset, stride = device_rows(ledge_rows())
    good = dict(level=0, first=0, count=2, trail=3, camera=0, W=8, H=4, S=2)

    def code_of(lib, expect, **change):
        a = dict(good, **change)
        launch(lib, a['level'], buf, offset, stride, a['first'], a['count'], a['trail'], None, a['camera'], a['W'],
               a['H'], a['S'], expect=expect)

    code_of(drawn, 0)
    for change in (dict(level=2), dict(level=-1), dict(first=-1), dict(trail=-1), dict(camera=2), dict(W=6), dict(W=0),
                   dict(W=4100), dict(H=0), dict(H=4097), dict(S=0), dict(S=5), dict(first=2147483647)):
        code_of(drawn, EINVAL, **change)  # level 2: Ledge has LEVELS = 1
    from omnisafe_amd import _lib

    out = torch.full((8 * 4 * 3 * 2 + 8,), SENTINEL, dtype=torch.uint8, device=DEV)
    call = drawn.osa_custom_render_episode
    tail = (0, 8, 4, 2)
    assert call(0, buf.data_ptr() + 4 * offset, stride, 0, 0, 3, None, *tail, out.data_ptr(), _lib.stream_ptr()) == EINVAL
    assert call(0, None, stride, 0, 2, 3, None, *tail, out.data_ptr(), _lib.stream_ptr()) == EINVAL
    assert call(0, buf.data_ptr() + 4 * offset, stride, 0, 2, 3, None, *tail, None, _lib.stream_ptr()) == EINVAL
    assert call(0, buf.data_ptr() + 4 * offset, stride, 0, 2, 3, None, *tail, out.data_ptr() + 2,
                _lib.stream_ptr()) == EINVAL  # rgb not 4-byte aligned
    assert (out.cpu().numpy() == SENTINEL).all()
    code_of(plain, EUNSUPPORTED)  # a description without draw()
    code_of(plain, EINVAL, level=2)


# ------------------------------------------------------------------ 6. end to end
@pytest.fixture
def ledge_drawn():
    import omnisafe_amd

    ids = {'LedgeDrawn0-v0': 0, 'LedgeDrawn1-v0': 1}
    cls = omnisafe_amd.register_device_env(os.path.join(ENVS, 'ledge_drawn.h'), 'LedgeDrawn', ids, default_horizon=40)
    yield cls
    omnisafe_amd.unregister_device_env(*[e for e in ids if e in omnisafe_amd.custom_envs()])


def cfgs(log_dir, horizon, n=16):
    return {'train_cfgs': {'device': DEV, 'total_steps': 2 * n * 2 * horizon, 'vector_env_nums': n},
            'algo_cfgs': {'steps_per_epoch': n * 2 * horizon, 'update_iters': 2},
            'logger_cfgs': {'log_dir': log_dir, 'verbose': False, 'save_model_freq': 2},
            'env_cfgs': {'horizon': horizon}}


def files_of(folder):
    return {n: open(os.path.join(folder, n), 'rb').read() for n in sorted(os.listdir(folder))}


def test_evaluator_render_of_a_drawing_custom_env(ledge_drawn, tmp_path, monkeypatch):
    """Two epochs of PPOLag on LedgeDrawn1-v0 at horizon 16, then Evaluator.render of the last checkpoint on both
    evaluator paths: the same files, whose frames are the twin's picture of the trace's rows, one frame per step that
    the episode lasted -- and an episode that ended before the horizon ended where terminal() says so."""
    import omnisafe_amd
    from omnisafe_amd import apng
    from omnisafe_amd.evaluator import Evaluator

    H, K, seed = 16, 6, 3
    agent = omnisafe_amd.Agent('PPOLag', 'LedgeDrawn1-v0', custom_cfgs=dict(cfgs(str(tmp_path / 'run'), H), seed=2))
    agent.learn()
    log_dir = agent.agent.logger.log_dir
    name = sorted(os.listdir(os.path.join(log_dir, 'torch_save')), key=lambda s: int(s[len('epoch-'):-len('.pt')]))[-1]
    written = {}
    for path in ('persistent', 'per-step'):
        monkeypatch.setenv('OSA_EVAL_PATH', path)
        ev = Evaluator(seed=seed, device=DEV, verbose=False)
        ev.load_saved(log_dir, name)
        out = str(tmp_path / path)
        ev.render(num_episodes=K, width=64, height=48, trail=4, save_replay_path=out)
        assert ev.path == path
        written[path] = files_of(out)
        tr = ev.trace.cpu().numpy()
        rec = tr.shape[2]
        act = tr[:, :, L.OBS:L.OBS + 2]
        lengths = [int(n) for n in ev.episode_lengths]
        print(f'{path}: lengths {lengths}')
        for k in range(K):
            n = lengths[k]
            rows = tr[:, k, rec - L.TRACE:]
            hit = np.zeros(H, np.uint8)
            hit[1:] = tr[:-1, k, rec - L.TRACE - 2] > 0
            frames = apng.read_apng(os.path.join(out, f'eval-episode-{k}.png'))
            assert len(frames) == n and 1 <= n <= H
            assert np.array_equal(np.stack(frames), ledge_twin(rows, 0, n, 4, hit, 0, 64, 48, 2, 1))
            still = apng.read_apng(os.path.join(out, f'eval-episode-{k}-path.png'))
            assert len(still) == 1 and np.array_equal(still[0], ledge_twin(rows, n - 1, 1, n, hit, 0, 64, 48, 2, 1)[0])
            # the step out of the last record ends the episode: terminal() of the twin, or the horizon
            before = np.zeros((K, L.STATE), np.float32)
            before[:, :L.TRACE] = tr[n - 1, :, rec - L.TRACE:]
            after = L.ledge_step(before, act[n - 1], 1, seed, n)[0]
            assert n == H or L.ledge_terminal(after)[k], (k, n)
            for t in range(n - 1):  # ... and no earlier step did
                before[:, :L.TRACE] = tr[t, :, rec - L.TRACE:]
                assert not L.ledge_terminal(L.ledge_step(before, act[t], 1, seed, t + 1)[0])[k], (k, t)
    assert written['persistent'] == written['per-step']
    assert sorted(written['persistent']) == sorted(
        [f'eval-episode-{k}.png' for k in range(K)] + [f'eval-episode-{k}-path.png' for k in range(K)] + ['result.txt'])


def test_env_render_and_group_render(ledge_drawn, tmp_path):
    """env.render() of a live drawing env is the twin's frame of its state row; AgentGroup.render writes every
    member's replays; a class without draw() keeps refusing in the words it had."""
    import omnisafe_amd
    from omnisafe_amd import apng, envs

    env = envs.make('LedgeDrawn1-v0', num_envs=3, device=DEV)
    assert type(env) is ledge_drawn and env.level == 1
    env.set_seed(4)
    env.reset()
    env.step(torch.full((3, 2), 0.7, device=DEV))
    state = env.state.cpu().numpy()
    for lane, camera in ((0, 'fixed'), (2, 'track')):
        img = env.render(lane=lane, width=64, height=48, camera_name=camera)
        assert img.dtype == np.uint8 and img.shape == (48, 64, 3)
        assert np.array_equal(img, ledge_twin(state[lane:lane + 1], 0, 1, 0, None, int(camera == 'track'), 64, 48, 2, 1)[0])
    with pytest.raises(IndexError):
        env.render(lane=3)
    # without arguments, as the reference's Evaluator calls it over the plugin: lane 0, 256 x 256, the fixed camera
    assert np.array_equal(env.render(), ledge_twin(state[0:1], 0, 1, 0, None, 0, 256, 256, 2, 1)[0])

    plain = omnisafe_amd.register_device_env(os.path.join(ENVS, 'ledge.h'), 'Ledge', ['LedgeUndrawn-v0'])
    try:
        with pytest.raises(ValueError) as err:
            envs.make('LedgeUndrawn-v0', num_envs=2, device=DEV).render()
        assert str(err.value) == ('LedgeUndrawn-v0 has no state row to draw: render() takes the geometric device envs '
                                  '(SynthReach-v0, SynthNav*-v0)')
        assert plain.draws is False
    finally:
        omnisafe_amd.unregister_device_env('LedgeUndrawn-v0')

    H = 16
    group = omnisafe_amd.AgentGroup('PPOLag', 'LedgeDrawn0-v0', seeds=[0, 1], custom_cfgs=cfgs(str(tmp_path), H))
    group.learn()
    outs = group.render(num_episodes=2, width=32, height=32)
    assert len(outs) == 2
    for member, out in zip(group.agents, outs):
        assert len(out) >= 1
        for name, folder in out.items():
            assert folder == os.path.join(member.agent.logger.log_dir, 'video', name[:-len('.pt')])
            for k in range(2):
                frames = apng.read_apng(os.path.join(folder, f'eval-episode-{k}.png'))
                assert 1 <= len(frames) <= H and frames[0].shape == (32, 32, 3)
                assert (np.stack(frames) != R.PALETTE[R.OUTSIDE]).any()
