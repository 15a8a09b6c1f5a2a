"""CPU: osa_render_episode rejects bad arguments before any launch; the numpy twin of the picture (render_twin.py)
on hand-made rows; the PNG / APNG writer round trip; the Python surface of rendering exists."""
import struct

import numpy as np
import pytest

import render_twin as R

EINVAL, EUNSUPPORTED = -1, -3
FAKE = 256  # a non-NULL, 4-byte aligned pointer value: never dereferenced, every call below returns before it launches


def call(lib, env_kind=R.NAV0 + 1, state=FAKE, stride=64, first=0, count=1, trail=0, hit=None, camera=0, width=32,
         height=32, supersample=2, rgb=FAKE):
    return lib.osa_render_episode(env_kind, state, stride, first, count, trail, hit, camera, width, height,
                                  supersample, rgb, None)


def test_render_episode_rejects_bad_arguments():
    from omnisafe_amd import _lib

    lib = _lib.load()
    assert call(lib, width=30) == EINVAL
    assert call(lib, width=0) == EINVAL and call(lib, width=4100) == EINVAL
    assert call(lib, height=0) == EINVAL and call(lib, height=4097) == EINVAL
    assert call(lib, supersample=0) == EINVAL and call(lib, supersample=5) == EINVAL
    assert call(lib, camera=2) == EINVAL and call(lib, camera=-1) == EINVAL
    assert call(lib, count=0) == EINVAL
    assert call(lib, first=-1) == EINVAL
    assert call(lib, trail=-1) == EINVAL
    assert call(lib, state=None) == EINVAL
    assert call(lib, rgb=None) == EINVAL
    assert call(lib, rgb=FAKE + 2) == EINVAL
    assert call(lib, env_kind=0) == EUNSUPPORTED  # OSA_EVAL_ENV_SYNTH: no state to draw
    assert call(lib, env_kind=2) == EUNSUPPORTED
    assert call(lib, env_kind=R.NAV0 + 3) == EUNSUPPORTED


def nav_rows(F=6):
    """A Goal level-1 walk: hazards and a vase in place, the robot moving right from (-1, -1), standing still once."""
    rows = np.zeros((F, 64), np.float32)
    rows[:, 0] = -1 + 0.25 * np.array([0, 1, 2, 2, 3, 4][:F], np.float32)
    rows[:, 1] = -1
    rows[:, 2] = 1  # u = (1, 0)
    rows[:, 8:10] = (1.0, 1.0)  # goal
    rows[:, 12:28] = np.array([(-1.5 + 0.4 * h, 1.5) for h in range(8)], np.float32).reshape(-1)  # hazards
    rows[:, 12:14] = (1.0, -1.0)
    rows[:, 32:34] = (-1.0, 0.5)  # the vase of level 1
    return rows


def pixel_of(x, y, W, H, half):
    """Pixel (i, j) of the fixed camera that holds the point (x, y), for S = 1."""
    h = half / min(W, H)
    return int((H - y / h) // 2), int((x / h + W) // 2)


def test_twin_colours_on_hand_made_rows():
    rows, W, H = nav_rows(), 128, 128
    kind = R.NAV0 + 1
    img = R.render(kind, rows, 0, 1, 0, None, 0, W, H, 1)[0]
    assert set(map(tuple, img.reshape(-1, 3))) <= set(map(tuple, R.PALETTE))  # S = 1: palette colours only
    assert tuple(img[pixel_of(1.0, -1.0, W, H, 2.25)]) == tuple(R.PALETTE[R.HAZARD])
    assert tuple(img[pixel_of(1.0, 1.0, W, H, 2.25)]) == tuple(R.PALETTE[R.GOAL])
    assert tuple(img[pixel_of(-1.0, 0.5, W, H, 2.25)]) == tuple(R.PALETTE[R.VASE])
    for corner in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert tuple(img[corner]) == tuple(R.PALETTE[R.OUTSIDE])
    assert tuple(img[pixel_of(0.0, 0.0, W, H, 2.25)]) == tuple(R.PALETTE[R.FLOOR])
    # the heading segment covers the robot's centre: look just behind the robot
    behind = pixel_of(-1.0 - 0.06, -1.0, W, H, 2.25)
    assert tuple(img[behind]) == tuple(R.PALETTE[R.POINT])
    hit = np.array([1], np.uint8)
    assert tuple(R.render(kind, rows, 0, 1, 0, hit, 0, W, H, 1)[0][behind]) == tuple(R.PALETTE[R.HIT])
    car = R.render(R.CARGOAL0 + 1, rows, 0, 1, 0, None, 0, W, H, 1)[0]
    assert tuple(car[behind]) == tuple(R.PALETTE[R.CAR])
    # Reach has no heading: the robot's centre itself has the robot colour (and the hit colour when hit)
    reach = np.array([[0.3, -0.4, 1.0, 1.0, -1.0, 0.5]], np.float32)
    img = R.render(R.REACH, reach, 0, 1, 0, None, 0, W, H, 1)[0]
    assert tuple(img[pixel_of(0.3, -0.4, W, H, 1.75)]) == tuple(R.PALETTE[R.POINT])
    assert tuple(img[pixel_of(-1.0, 0.5, W, H, 1.75)]) == tuple(R.PALETTE[R.HAZARD])
    assert tuple(img[pixel_of(1.0, 1.0, W, H, 1.75)]) == tuple(R.PALETTE[R.GOAL])
    img = R.render(R.REACH, reach, 0, 1, 0, hit, 0, W, H, 1)[0]
    assert tuple(img[pixel_of(0.3, -0.4, W, H, 1.75)]) == tuple(R.PALETTE[R.HIT])
    # the trail of frame 5 crosses the pixel column of x = -0.75 (the strip is wider than a pixel); none with trail = 0
    column = pixel_of(-0.75, -1.0, W, H, 2.25)[1]
    trail_colour = R.PALETTE[R.TRAIL]
    assert (R.render(kind, rows, 5, 1, 5, None, 0, W, H, 1)[0][:, column] == trail_colour).all(-1).any()
    assert not (R.render(kind, rows, 5, 1, 0, None, 0, W, H, 1)[0] == trail_colour).all(-1).any()


def test_twin_circle_layers():
    rows = np.zeros((1, 8), np.float32)
    rows[0, :4] = (0.1, 0.2, 0.0, 1.0)
    W = H = 288
    for level in range(3):
        img = R.render(R.CIRCLE0 + level, rows, 0, 1, 0, None, 0, W, H, 1)[0]
        assert tuple(img[pixel_of(1.5, 0.0, W, H, 2.25)]) == tuple(R.PALETTE[R.COST if level >= 1 else R.FLOOR])
        assert tuple(img[pixel_of(0.0, 1.5, W, H, 2.25)]) == tuple(R.PALETTE[R.COST if level == 2 else R.FLOOR])
        assert tuple(img[pixel_of(0.70711, 0.70711, W, H, 2.25)]) == tuple(R.PALETTE[R.RING])  # |q| = 1
        assert tuple(img[pixel_of(0.4, 0.4, W, H, 2.25)]) == tuple(R.PALETTE[R.FLOOR])


@pytest.mark.parametrize('S', [1, 2, 3])
@pytest.mark.parametrize('camera', [0, 1])
def test_twin_mirror_in_x(S, camera):
    rows = nav_rows()
    rows[:, 2:4] = (0.6, 0.8)
    mirrored = rows.copy()
    for col in [0, 2, 8] + list(range(12, 52, 2)):
        mirrored[:, col] = -mirrored[:, col]
    a = R.render(R.NAV0 + 2, rows, 0, 6, 3, None, camera, 36, 20, S)
    b = R.render(R.NAV0 + 2, mirrored, 0, 6, 3, None, camera, 36, 20, S)
    assert np.array_equal(a, b[:, :, ::-1])


def test_twin_chunked_calls_agree():
    rows = nav_rows()
    hit = np.array([0, 0, 1, 0, 1, 0], np.uint8)
    whole = R.render(R.NAV0 + 1, rows, 0, 6, 2, hit, 0, 36, 20, 2)
    parts = [R.render(R.NAV0 + 1, rows, first, 3, 2, hit, 0, 36, 20, 2) for first in (0, 3)]
    assert np.array_equal(whole, np.concatenate(parts))


def test_twin_zero_length_segment_is_a_disc():
    """Records 2 and 3 of nav_rows share a position: the trail's zero-length segment is a disc, not NaN."""
    rows = nav_rows()
    x = np.array([[-0.5, -0.5 + 0.019, -0.5 + 0.021]], np.float32)
    y = np.full_like(x, -1)
    inside = R.segment(x, y, rows[2, 0], rows[2, 1], np.float32(0), np.float32(0), np.float32(0.0004))
    assert inside.tolist() == [[True, True, False]]


def frames_for_files(n, H=8, W=12):
    return np.random.default_rng(5).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize('n', [3, 1])
def test_apng_round_trip(tmp_path, n):
    from omnisafe_amd import apng

    frames = frames_for_files(n)
    path = str(tmp_path / 'a.png')
    # an iterator of chunks and single frames, as a long replay hands them over
    assert apng.write_apng(path, iter([frames[:2], frames[2]] if n == 3 else [frames[0]]), fps=25) == n
    raw = open(path, 'rb').read()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    kinds = [k for k, _ in apng.chunks(path)]
    assert kinds[:4] == [b'IHDR', b'acTL', b'fcTL', b'IDAT'] and kinds[-1] == b'IEND'
    assert kinds.count(b'fcTL') == n and kinds.count(b'fdAT') == n - 1
    actl = dict(apng.chunks(path))[b'acTL']
    assert struct.unpack('>II', actl) == (n, 0)
    fctl = [d for k, d in apng.chunks(path) if k == b'fcTL'][0]
    assert struct.unpack('>HH', fctl[20:24]) == (1, 25)
    back = apng.read_apng(path)
    assert len(back) == n and all(np.array_equal(a, b) for a, b in zip(back, frames))


def test_png_round_trip_and_bad_frames(tmp_path):
    from omnisafe_amd import apng

    frames = frames_for_files(1)
    path = str(tmp_path / 's.png')
    apng.write_png(path, frames[0])
    back = apng.read_apng(path)
    assert len(back) == 1 and np.array_equal(back[0], frames[0])
    with pytest.raises(ValueError):
        apng.write_apng(str(tmp_path / 'e.png'), [], fps=30)
    with pytest.raises(ValueError):
        apng.write_apng(str(tmp_path / 'f.png'), [frames[0].astype(np.float32)], fps=30)


def test_apng_is_read_by_pillow(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from omnisafe_amd import apng

    frames = frames_for_files(3)
    path = str(tmp_path / 'a.png')
    apng.write_apng(path, frames, fps=30)
    with Image.open(path) as im:
        assert im.n_frames == 3 and im.size == (12, 8)
        for k in range(3):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert('RGB')), frames[k])
    apng.write_png(str(tmp_path / 's.png'), frames[1])
    with Image.open(str(tmp_path / 's.png')) as im:
        assert np.array_equal(np.asarray(im.convert('RGB')), frames[1])


@pytest.mark.parametrize('name', ['SynthNavCircle1_PPOLag_seed0_epoch-10_path.png',
                                  'SynthNavGoal1_PPOLag_seed0_epoch-10_path.png'])
def test_committed_stills_read_back(golden_dir, name):
    """The path stills that Evaluator.render wrote on the device (tests/golden/render_examples, shown in
    profiles/circle_learning.md and nav_learning.md) decode with read_apng: one 256 x 256 frame of the fixed camera,
    whose border is outside the arena, with the robot, its heading and its trail in it."""
    import os

    from omnisafe_amd import apng

    frames = apng.read_apng(os.path.join(golden_dir, 'render_examples', name))
    assert len(frames) == 1 and frames[0].shape == (256, 256, 3) and frames[0].dtype == np.uint8
    img = frames[0]
    outside = R.PALETTE[R.OUTSIDE]
    for edge in (img[0], img[-1], img[:, 0], img[:, -1]):
        assert (edge == outside).all()
    for layer in (R.FLOOR, R.TRAIL, R.POINT, R.HEADING):
        assert (img == R.PALETTE[layer]).all(-1).any(), layer


def test_render_surface():
    import omnisafe_amd
    from omnisafe_amd import envs
    from omnisafe_amd.evaluator import Evaluator

    assert callable(Evaluator.render) and callable(omnisafe_amd.Agent.render)
    assert callable(omnisafe_amd.AgentGroup.render) and callable(envs.DeviceVectorEnv.render)
    with pytest.raises(ValueError):
        Evaluator(seed=0, verbose=False).render()
    ev = Evaluator(seed=0, verbose=False)
    with pytest.raises(NotImplementedError):
        ev.load_saved('nowhere', 'epoch-0.pt', render_mode='human')
    with pytest.raises(ValueError):
        ev.load_saved('nowhere', 'epoch-0.pt', camera_name='side')
