"""CPU: the evaluation entry point rejects bad arguments before any launch (OSA_EINVAL / OSA_EUNSUPPORTED), and the
Python surface (omnisafe_amd.Evaluator, Agent.evaluate) exists."""
import pytest

EINVAL, EUNSUPPORTED = -1, -3
SYNTH, REACH = 0, 1
FAKE = 256  # a non-NULL pointer value: never dereferenced, every call below returns before it launches


def call(lib, env_kind=SYNTH, K=16, obs_dim=60, act_dim=2, hidden=64, params=FAKE, norm=(FAKE, FAKE, FAKE),
         bounds=(FAKE, FAKE), min_a=-1.0, max_a=1.0, horizon=10, max_steps=10, saute=0, budget=1.0, gamma=0.999,
         outs=(FAKE, FAKE, FAKE)):
    return lib.osa_eval_episodes(env_kind, K, obs_dim, act_dim, hidden, params, *norm, 5.0, *bounds, min_a, max_a,
                                 0, horizon, 0.05, max_steps, saute, budget, gamma, 0, 25.0, 1.0, *outs, None, None)


def test_eval_episodes_rejects_bad_arguments():
    from omnisafe_amd import _lib

    lib = _lib.load()
    assert call(lib, K=0) == EINVAL
    assert call(lib, max_steps=0) == EINVAL
    assert call(lib, horizon=0) == EINVAL
    assert call(lib, params=None) == EINVAL
    for i in range(3):
        outs = [FAKE, FAKE, FAKE]
        outs[i] = None
        assert call(lib, outs=tuple(outs)) == EINVAL
    assert call(lib, bounds=(None, FAKE)) == EINVAL
    assert call(lib, min_a=1.0, max_a=1.0) == EINVAL
    assert call(lib, norm=(FAKE, None, FAKE)) == EINVAL
    assert call(lib, saute=1, budget=0.0) == EINVAL
    assert call(lib, env_kind=REACH, obs_dim=4) == EINVAL
    assert call(lib, env_kind=2) == EUNSUPPORTED
    assert call(lib, env_kind=-1) == EUNSUPPORTED
    assert call(lib, hidden=48) == EUNSUPPORTED
    assert call(lib, hidden=64 | (7 << 16)) == EUNSUPPORTED
    assert call(lib, act_dim=33) == EUNSUPPORTED
    assert call(lib, obs_dim=1000) == EUNSUPPORTED  # policy input wider than the kernel's LDS rows
    assert lib.osa_eval_trace_floats(REACH, 60, 2, 0) == 60 + 2 + 3 + 6
    assert lib.osa_eval_trace_floats(SYNTH, 376, 17, 1) == 377 + 17 + 3
    assert lib.osa_eval_trace_floats(SYNTH, 0, 17, 0) == 0


def test_evaluator_surface():
    import omnisafe_amd
    from omnisafe_amd.evaluator import Evaluator

    assert omnisafe_amd.Evaluator is Evaluator
    assert callable(omnisafe_amd.Agent.evaluate)
    ev = Evaluator(seed=0, verbose=False)
    with pytest.raises(ValueError):
        ev.evaluate(num_episodes=1)
