"""CPU: the numpy twins of the object-row examples (tests/button_twin.py: Button, CarButton, Field) against their own
specification and against the twins of the built-in robots, and the event coverage of the scripted runs that the GPU
tests replay (tests/test_custom_row_env_gpu.py imports the same constants)."""
import numpy as np

import button_twin as B
import car_twin
import nav_twin


def test_level_0_places_neither_hazards_nor_gremlins():
    for level, (H, G) in B.LEVEL.items():
        s = B.button_reset(3, 0, 9, level)
        assert np.all(s[:, B.BUTTONS:B.HAZ] != 0)  # four buttons on every level
        assert np.all(s[:, B.HAZ:B.HAZ + 2 * H] != 0) and np.all(s[:, B.HAZ + 2 * H:B.GREM] == 0)
        centres = s[:, B.GREM:B.GREM + 3 * G].reshape(9, G, 3)[:, :, :2]
        assert np.all(centres != 0) and np.all(s[:, B.GREM + 3 * G:] == 0) and np.all(s[:, 14:16] == 0)
        phase = s[:, B.GREM + 2:B.GREM + 3 * G:3]
        assert np.all((phase >= 0) & (phase < B.PERIOD) & (phase == np.floor(phase)))
        goal = s[:, B.GOAL_COL].astype(int)
        assert np.all((goal >= 0) & (goal < 4)) and np.array_equal(s[:, 8:10], B.button_at(s, goal))
    assert B.LEVEL[0] == (0, 0) and B.LEVEL[1] == (4, 4) and B.LEVEL[2] == (8, 6)


def test_a_gremlin_returns_to_its_start_after_16_S_steps_bit_for_bit():
    s = B.button_reset(7, 0, 33, 2)
    for i in range(6):
        for k in (0, 1, 77):
            here = B.gremlin_at(s, np.full(33, k, np.float32), i)
            assert np.array_equal(here, B.gremlin_at(s, np.full(33, k + 16 * B.S, np.float32), i))
            assert not np.array_equal(here, B.gremlin_at(s, np.full(33, k + 1, np.float32), i))
            # on the 16-gon round its centre: never further than the orbit's radius (plus rounding)
            away = nav_twin.dist(here, s[:, B.GREM + 3 * i:B.GREM + 3 * i + 2])
            assert np.all(away <= B.ORBIT * np.float32(1.000001)) and np.all(away >= np.float32(0.39))


def test_point_and_car_share_the_arena_under_the_same_commands():
    rng = np.random.default_rng(0)
    point, car = B.RowTwin('point', 2, 6, 5, 21), B.RowTwin('car', 2, 6, 5, 21)
    assert np.array_equal(point.reset()[:, 12:], car.reset()[:, 24:])  # the lidars of the common start
    for _ in range(12):  # two truncations
        a = rng.uniform(-1.5, 1.5, (6, 2)).astype(np.float32)
        point.step(a)
        car.step(a)
        assert np.array_equal(point.state[:, 14:], car.state[:, 14:])
    assert not np.array_equal(point.state[:, 0:2], car.state[:, 0:2])


def test_the_robots_move_as_the_built_in_twins_do():
    rng = np.random.default_rng(1)
    for car in (False, True):
        s = B.button_reset(5, 0, 17, 1)
        for pos in range(1, 9):
            a = rng.uniform(-1.5, 1.5, (17, 2)).astype(np.float32)
            theirs = np.zeros((17, 64), np.float32)
            theirs[:, :12] = s[:, :12]
            if car:
                moved = car_twin.car_goal_step(theirs, a, 0, 5, pos)[0]
            else:
                moved = nav_twin.nav_step(theirs, a, 0, 5, pos)[0]
            s = B.button_step(s, a, 1, 5, pos, car)[0]
            assert np.array_equal(s[:, 0:8], moved[:, 0:8]) and np.array_equal(s[:, 10:12], moved[:, 10:12])
            assert np.array_equal(s[:, B.K_COL], np.full(17, pos, np.float32))


def scripted(kind, level, N, horizon, seed, steps):
    """The scripted run on the twin: events counted over all envs and steps."""
    twin = B.RowTwin(kind, level, N, horizon, seed)
    twin.reset()
    seen = {}
    ends = []
    for t in range(steps):
        _, _, cost, term, trunc, _ = twin.step(twin.controller(t))
        for name, on in twin.events.items():
            seen[name] = seen.get(name, 0) + int(on.sum())
        seen['truncation'] = seen.get('truncation', 0) + int(trunc.sum())
        seen['cost'] = seen.get('cost', 0) + int(cost.sum())
        ends.append(term.copy())
    return seen, np.array(ends)


def test_the_scripted_button_runs_show_every_event():
    for kind in ('point', 'car'):
        for level in (0, 1, 2):
            seen, _ = scripted(kind, level, B.SCRIPT_N, B.SCRIPT_HORIZON, B.SCRIPT_SEED, B.SCRIPT_STEPS)
            assert seen['press'] > 0 and seen['wrong'] > 0 and seen['truncation'] > 0
            assert (seen['hazard'] > 0) == (level > 0) and (seen['gremlin'] > 0) == (level > 0)


def test_the_scripted_field_run_terminates_truncates_and_costs():
    seen, ends = scripted('field', 0, B.FIELD_N, B.FIELD_HORIZON, B.FIELD_SEED, B.FIELD_STEPS)
    assert seen['terminal'] > 0 and seen['truncation'] > 0 and seen['cost'] > 0
    # envs that share a workgroup of the per-step kernel (N = 5 at 16 or 32 lanes) end on different steps
    first = [int(np.argmax(ends[:, n])) if ends[:, n].any() else -1 for n in range(B.FIELD_N)]
    assert first[0] != first[1] and first[2] == -1
    assert np.any(ends.sum(axis=1) == 1)  # a step on which one env terminates and its neighbours do not
