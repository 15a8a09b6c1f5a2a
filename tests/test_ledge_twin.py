"""CPU: known answers for tests/ledge_twin.py, the numpy twin of the terminating example env tests/custom_envs/ledge.h,
and the conditions that the GPU trace test relies on (enough terminations, truncations and workgroups whose envs end
differently on one step), established from the twin alone."""
import numpy as np

import ledge_twin as L

F = np.float32


def rows(*r):
    return np.array(r, np.float32)


def test_known_answers_one_step_from_each_edge_and_from_the_end():
    """Hand-placed rows at rest in y with a sideways speed that carries them over an edge (the gust is at most 0.04,
    the push 0.05): over the right edge, over the left one, behind x = 3, and one that stays."""
    s = rows([0.5, 0.95, 0.1, 0.2, 3, 0],    # v_y' >= 0.18 - 0.05 - 0.04 = 0.09: p_y' > 1.04
             [0.5, -0.95, 0.1, -0.2, 7, 0],  # the mirror image
             [2.9, 0.0, 0.3, 0.0, 9, 0],     # v_x' >= 0.27 - 0.05: p_x' > 3.12
             [1.0, 0.2, 0.1, 0.0, 2, 0])     # nowhere near an end
    act = rows([0, -5], [0, 5], [-5, 0], [0.5, 0.25])
    for level in (0, 1):
        s1, r, c = L.ledge_step(s, act, level, seed=3, pos=4)
        np.testing.assert_array_equal(L.ledge_terminal(s1), [True, True, True, False])
        assert s1[0, 1] > 1.04 and s1[1, 1] < -1.04 and s1[2, 0] > 3.12
        np.testing.assert_array_equal(s1[:, 4], [4, 8, 10, 3])  # the episode's step count
        np.testing.assert_array_equal(s1[:, 5], 0)
        # the velocity in two roundings, clipped actions; x has no gust
        vx = (F(0.9) * s[:, 2]).astype(np.float32) + (F(0.05) * np.clip(act[:, 0], -1, 1)).astype(np.float32)
        np.testing.assert_array_equal(s1[:, 2], vx.astype(np.float32))
        np.testing.assert_array_equal(s1[:, 0], (s[:, 0] + s1[:, 2]).astype(np.float32))
        np.testing.assert_array_equal(r, (s1[:, 2] + rows(0, 0, 1, 0)).astype(np.float32))  # + 1 on arriving
        np.testing.assert_array_equal(c, [level, level, 0, 0])  # |p_y| > 0.5 on level 1 only
        gust = s1[:, 3] - ((F(0.9) * s[:, 3]).astype(np.float32) + (F(0.05) * np.clip(act[:, 1], -1, 1)).astype(np.float32))
        assert (np.abs(gust) <= 0.04 + 1e-6).all() and len(set(gust.tolist())) == 4  # per env
    # the gust is the transition's own Philox block: another position, another gust; the same position, the same
    again = L.ledge_step(s, act, 1, seed=3, pos=4)[0]
    other = L.ledge_step(s, act, 1, seed=3, pos=5)[0]
    np.testing.assert_array_equal(again, s1)
    assert (other[:, 3] != s1[:, 3]).all() and (other[:, 2] == s1[:, 2]).all()


def test_reset_and_observation():
    s = L.ledge_reset(seed=9, pos=2, N=200)
    assert s.dtype == np.float32 and s.shape == (200, 6)
    assert not s[:, [0, 2, 3, 4, 5]].any() and (np.abs(s[:, 1]) <= 0.4).all() and s[:, 1].std() > 0.15
    np.testing.assert_array_equal(L.ledge_reset(9, 2, 200, n=[7, 150]), s[[7, 150]])  # keyed by the env index
    assert (L.ledge_reset(9, 3, 200)[:, 1] != s[:, 1]).all()
    s = rows([0.5, -0.75, 0.25, 0.125, 3, 0])
    o = L.ledge_obs(s, 23)
    assert o.shape == (1, 23) and not o[:, 20:].any()
    np.testing.assert_array_equal(o[0, :5], [0.5, -0.75, 0.25, 0.125, 0.25])
    # column 5 + j: x[j % 5] * (x[j // 5] + (j + 1) / 8)
    assert o[0, 5] == F(0.5) * F(0.5 + 0.125) and o[0, 9] == F(3) * F(0.5 + 0.625)
    assert o[0, 11] == F(-0.75) * F(-0.75 + 0.875) and o[0, 19] == F(3) * F(0.25 + 1.875)
    assert L.ledge_obs(s).shape == (1, 20)


def test_per_env_counters_flags_and_the_reset_position():
    """Three envs at horizon 4: env 1 is pushed over the edge on its second step, the others truncate at step 4; env 1
    then truncates at step 6 by its own count.  A reset takes the position of the step that ended the episode."""
    seed, H = 11, 4
    tw = L.LedgeTwin(1, 3, H, seed)
    tw.reset()
    np.testing.assert_array_equal(tw.state, L.ledge_reset(seed, 0, 3))
    # env 1 from p_y = 0.75 at v_y = 0.15, pushed for two steps: v_y in [0.145, 0.225] then >= 0.1405, so p_y <= 0.975
    # after the first step and >= 1.0355 after the second.  From the reset on the gusts alone (0.4 + 0.36 at most)
    # cannot carry it over an edge within four steps.
    tw.state[1, 1], tw.state[1, 3] = F(0.75), F(0.15)
    seen = []
    for t in range(1, 9):
        act = rows([1, 0], [1, 1 if t <= 2 else 0], [1, 0])
        before = tw.state.copy()
        o, r, c, term, trunc, final = tw.step(act)
        stepped = L.ledge_step(before, act, 1, seed, t)[0]
        assert not (term & trunc).any()
        ended = term | trunc
        fresh = L.ledge_reset(seed, t, 3)
        np.testing.assert_array_equal(tw.state[ended], fresh[ended])  # fresh at the transition's position
        np.testing.assert_array_equal(tw.state[~ended], stepped[~ended])
        np.testing.assert_array_equal(final[trunc], L.ledge_obs(stepped)[trunc])  # the pre-reset observation
        assert np.isnan(final[~trunc]).all()
        np.testing.assert_array_equal(o, L.ledge_obs(tw.state))
        seen.append((term.tolist(), trunc.tolist(), tw.steps.tolist()))
    T_, F_ = True, False
    assert seen[0] == ([F_, F_, F_], [F_, F_, F_], [1, 1, 1])
    assert seen[1] == ([F_, T_, F_], [F_, F_, F_], [2, 0, 2])
    assert seen[2] == ([F_, F_, F_], [F_, F_, F_], [3, 1, 3])
    assert seen[3] == ([F_, F_, F_], [T_, F_, T_], [0, 2, 0])
    assert seen[4] == ([F_, F_, F_], [F_, F_, F_], [1, 3, 1])
    assert seen[5] == ([F_, F_, F_], [F_, T_, F_], [2, 0, 2])
    assert seen[7] == ([F_, F_, F_], [T_, F_, T_], [0, 2, 0])


def test_termination_wins_over_the_time_limit_and_the_endless_twin_never_terminates():
    seed, H = 2, 3
    for terminates in (True, False):
        tw = L.LedgeTwin(0, 2, H, seed, terminates=terminates)
        tw.reset()
        tw.steps[:] = H - 1  # the next step reaches the time limit
        tw.state[0] = rows([0.5, 0.95, 0.1, 0.2, 2, 0])[0]  # ... and carries env 0 over the edge
        _, _, _, term, trunc, final = tw.step(rows([0, 0], [0, 0]))
        if terminates:
            assert term.tolist() == [True, False] and trunc.tolist() == [False, True]
            assert np.isnan(final[0]).all() and not np.isnan(final[1]).any()
        else:
            assert term.tolist() == [False, False] and trunc.tolist() == [True, True]
        assert tw.steps.tolist() == [0, 0]


def test_the_trace_of_the_gpu_test_has_every_kind_of_end():
    """N = 130, horizon 12, 48 steps, uniform actions in [-1.5, 1.5] at TRACE_SEED: at least 40 terminations and 150
    truncations, and per lane count at least 3 (step, workgroup) pairs whose envs end differently on that step -- at 16
    lanes (4 consecutive envs) a terminating, a truncating and a continuing env, at 32 lanes (2 envs) a terminating and
    a truncating one.  The level only changes the cost."""
    N = 130
    acts = L.trace_actions(N)
    assert acts.shape == (L.TRACE_STEPS, N, 2) and acts.dtype == np.float32
    assert np.abs(acts).max() <= 1.5 and (np.abs(acts) > 1).mean() > 0.25
    tw = L.LedgeTwin(1, N, L.TRACE_HORIZON, L.TRACE_SEED)
    tw.reset()
    n_term = n_trunc = mixed4 = mixed2 = n_cost = 0
    for t in range(L.TRACE_STEPS):
        _, _, c, term, trunc, _ = tw.step(acts[t])
        assert not (term & trunc).any()
        n_term, n_trunc, n_cost = n_term + int(term.sum()), n_trunc + int(trunc.sum()), n_cost + int(c.sum())
        mixed4 += L.mixed_groups(term, trunc, 4)
        mixed2 += L.mixed_groups(term, trunc, 2)
    print(f'terminations {n_term}, truncations {n_trunc}, mixed workgroups: {mixed4} of 4 envs, {mixed2} of 2 envs')
    assert n_term >= 40 and n_trunc >= 150 and mixed4 >= 3 and mixed2 >= 3 and n_cost > 100
