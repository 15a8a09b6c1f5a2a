"""CPU: the numpy twin of the generic scene rasteriser (scene_twin.py) against the twin of the built-in picture
(render_twin.py).  With SynthReach's and the circle tasks' pictures restated as scenes the two must agree byte for
byte: a box is the complement of the `abs > bound` tests of the arena and the cost region, and a ring around the
origin has dx = x.  If this fails the scene twin is wrong, not the bound."""
import numpy as np
import pytest

import circle_twin
import render_twin as R
import scene_twin as T

RECORDS = 8
STILL, CORNER, ON_OBJECT = 4, 5, 6  # (the hand-made records of test_render_gpu.py's walk())
HIT = np.array([0, 1, 0, 0, 1, 1, 0, 1], np.uint8)
SCENES = {'reach': (R.REACH, T.reach_draw, 1.75, 0), 'circle0': (R.CIRCLE0, T.circle_draw, 2.25, 0),
          'circle1': (R.CIRCLE0 + 1, T.circle_draw, 2.25, 1), 'circle2': (R.CIRCLE0 + 2, T.circle_draw, 2.25, 2)}


def walk(env_kind):
    """test_render_gpu.py's rows for SynthReach and the point circle tasks: a short random walk, then by hand two
    identical consecutive positions, the arena's corner and the robot on an object (the circle's centre)."""
    rng = np.random.default_rng(env_kind)
    if env_kind == R.REACH:
        rows = rng.uniform(-1.5, 1.5, (RECORDS, 6)).astype(np.float32)
        rows[:, 2:] = rows[0, 2:]
        corner, obj = 1.5, rows[0, 4:6]
    else:
        level = env_kind % 16
        s = circle_twin.circle_reset(7, 0, 1)
        rows = np.zeros((RECORDS, s.shape[1]), np.float32)
        for t in range(RECORDS):
            rows[t] = s[0]
            s = circle_twin.circle_step(s, np.array([[1.0, 0.6 * rng.uniform(-1, 1)]], np.float32), level)[0]
            s[0, 0:2] = np.clip(s[0, 0:2] + np.float32(0.15) * s[0, 2:4], -2, 2).astype(np.float32)
        corner, obj = 2.0, (0.0, 0.0)
    rows[STILL, 0:2] = rows[STILL - 1, 0:2]
    rows[CORNER, 0:2] = corner
    rows[ON_OBJECT, 0:2] = obj
    return rows


@pytest.mark.parametrize('name', list(SCENES))
def test_scene_twin_equals_the_built_in_twin(name):
    env_kind, draw, view, level = SCENES[name]
    rows = walk(env_kind)
    assert np.abs(rows[1:STILL, 0:2] - rows[0:STILL - 1, 0:2]).max() > 0.1  # a walk long enough to leave a trail
    for W, H in ((36, 20), (16, 12)):
        for S in (1, 2, 3):
            for trail in (0, RECORDS + 3):
                for camera in (0, 1):
                    for hit in (None, HIT):
                        want = R.render(env_kind, rows, 0, RECORDS, trail, hit, camera, W, H, S)
                        got = T.render(draw, T.position, view, rows, 0, RECORDS, trail, hit, camera, W, H, S,
                                       level=level)
                        assert np.array_equal(got, want), (name, W, H, S, trail, camera, hit is None)


def test_the_scene_keeps_the_first_primitives_and_one_trail():
    prims = [('trail', 1, 0)] + [('disc', 0, 0, 1, k) for k in range(70)] + [('trail', 2, 0)]
    kept = T.staged(prims)
    assert len(kept) == T.DRAW_MAX and kept[0] == ('trail', 1, 0) and kept[-1] == ('disc', 0, 0, 1, 62)
    assert T.staged([('trail', 1, 0), ('trail', 2, 0), ('disc', 0, 0, 1, 5)]) == [('trail', 1, 0), ('disc', 0, 0, 1, 5)]


def test_a_frame_starts_as_the_background():
    rows = np.zeros((1, 6), np.float32)
    got = T.render(lambda rec, level, hit: [], T.position, 2.0, rows, 0, 1, 0, None, 0, 8, 4, 2)
    assert (got == R.PALETTE[R.OUTSIDE]).all()
