"""CPU: runtime parameters of custom device envs up to the GPU's edge (include/omnisafe_amd_env.h, PARAMETERS).  What
the library of the example tests/custom_envs/gust.h reports, what a library without PARAMS answers, what the contract's
static_asserts reject, the parsing of env_cfgs, and the numpy twin's own properties; the kernels run in
test_custom_env_params_gpu.py."""
import ctypes
import os

import numpy as np
import pytest

import gust_twin as G

HERE = os.path.dirname(os.path.abspath(__file__))
GUST = os.path.join(HERE, 'custom_envs', 'gust.h')
GLIDER = os.path.join(HERE, 'custom_envs', 'glider.h')
OSA_EUNSUPPORTED = -3

ARRAYS = '''
  static constexpr int PARAMS = 4;
  static constexpr float PARAM_DEFAULT[4] = {0.f, 0.f, 0.f, 0.f};
  static constexpr const char* PARAM_NAMES[4] = {"a", "b", "c", "d"};
'''
BAD = {
    'params_17': ('struct Bad : Gust {\n  static constexpr int PARAMS = 17;\n};\n', 'PARAMS must be 1 .. 16'),
    'no_bind': ('struct Bad : GustFlight {' + ARRAYS + '};\n', 'needs bind(Regs&, const float* par)'),
    'names_length': ('struct Bad : Gust {\n  static constexpr const char* PARAM_NAMES[3] = {"a", "b", "c"};\n};\n',
                     'PARAM_NAMES must have PARAMS elements'),
    'bind_uncallable': ('struct Bad : GustFlight {' + ARRAYS + '  static __device__ void bind(Regs&, int) {}\n};\n',
                        'a member bind that cannot be called'),
}
MESSAGES = [expect for _, expect in BAD.values()] + ['PARAM_DEFAULT must have', 'needs PARAM_DEFAULT',
                                                      'needs PARAM_NAMES', 'must be an identifier']


def _param_info(lib):
    count, defaults, names = ctypes.c_int(-1), (ctypes.c_float * 16)(), ctypes.create_string_buffer(256)
    lib.osa_custom_param_info.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float),
                                          ctypes.c_char_p, ctypes.c_int]
    assert lib.osa_custom_param_info(ctypes.byref(count), defaults, names, len(names)) == 0
    return count.value, list(defaults)[:max(count.value, 0)], names.value.decode()


def test_gust_builds_and_reports_its_parameters():
    from omnisafe_amd import build

    lib = ctypes.CDLL(build.build_custom_env(GUST, 'Gust'))
    count, defaults, names = _param_info(lib)
    assert count == 4 and names == 'wind drag band reach'
    np.testing.assert_array_equal(np.array(defaults, np.float32), G.DEFAULT)
    info = (ctypes.c_int * 8)()
    assert lib.osa_custom_env_info(info) == 0
    assert list(info) == [6, 8, 4, 2, 6, 0, 32, 1]  # STATE OBS DYN ACT TRACE LEVELS LANES terminates: the layout as it was
    # a buffer too small for the names is refused, not overrun
    small = ctypes.create_string_buffer(8)
    assert lib.osa_custom_param_info(ctypes.byref(ctypes.c_int()), None, small, len(small)) == -1


def test_a_library_without_params_reports_none_and_refuses_the_parameter_forms():
    from omnisafe_amd import build, envs

    lib = envs._bind_custom(build.build_custom_env(GLIDER, 'Glider'))[0]
    assert _param_info(lib) == (0, [], '')
    assert envs._custom_params(lib, 'glider') == ((), ())
    for name in ('osa_custom_env_step_params', 'osa_custom_eval_episodes_params',
                 'osa_custom_collect_episodes_params'):
        fn = getattr(lib, name)
        args = [0.0 if t is ctypes.c_float or t is ctypes.c_double else (None if t is ctypes.c_void_p else 0)
                for t in fn.argtypes]
        assert fn(*args) == OSA_EUNSUPPORTED, name  # (before any other check, and before any launch)


@pytest.mark.parametrize('case', list(BAD))
def test_each_rejected_contract_gives_its_own_message(tmp_path, case):
    from omnisafe_amd import _lib, build

    source, expect = BAD[case]
    header = str(tmp_path / 'bad.h')
    with open(header, 'w', encoding='utf-8') as f:
        f.write(f'#include "{GUST}"\n' + source)
    with pytest.raises(_lib.OsaError) as err:
        build.build_custom_env(header, 'Bad')
    text = str(err.value)
    assert expect in text and 'error' in text
    assert not [m for m in MESSAGES if m != expect and m in text], text  # one message per fault, no cascade
    assert not os.path.exists(build.custom_env_path(header, 'Bad'))


@pytest.fixture
def gust():
    import omnisafe_amd

    cls = omnisafe_amd.register_device_env(GUST, 'Gust', ['Gust-v0'], default_horizon=40)
    try:
        yield cls
    finally:
        omnisafe_amd.unregister_device_env('Gust-v0')


def test_the_class_carries_the_parameters_and_its_entry_points(gust):
    assert gust.param_names == G.NAMES
    np.testing.assert_array_equal(np.array(gust.param_defaults, np.float32), G.DEFAULT)
    assert gust.entry_point == 'osa_custom_env_step_params' and gust.graph_safe is True and gust.terminates
    assert gust.eval_entry_point == 'osa_custom_eval_episodes_params'
    assert gust.collect_entry_point == 'osa_custom_collect_episodes_params'


def test_param_ranges_parses_env_cfgs(gust):
    from omnisafe_amd import envs

    got = envs.param_ranges(gust, {'wind': 0.3, 'band': (0.4, 0.8), 'horizon': 9, 'seed': 1})
    assert got.dtype == np.float32 and got.shape == (2, 4)
    np.testing.assert_array_equal(got, G.ranges(wind=0.3, band=(0.4, 0.8)))
    np.testing.assert_array_equal(got[:, 0], np.float32([0.3, 0.3]))  # a scalar: (v, v)
    np.testing.assert_array_equal(got[:, 2], np.float32([0.4, 0.8]))  # a pair: (lo, hi)
    np.testing.assert_array_equal(got[:, [1, 3]], np.stack([G.DEFAULT, G.DEFAULT])[:, [1, 3]])  # absent: the default
    np.testing.assert_array_equal(envs.param_ranges(gust, {'reach': [0.1, 0.1]})[:, 3], np.float32([0.1, 0.1]))
    with pytest.raises(TypeError) as err:
        envs.param_ranges(gust, {'wnid': 0.3})
    assert 'wnid' in str(err.value) and all(name in str(err.value) for name in G.NAMES)
    for bad in ({'wind': (0.5, 0.1)}, {'wind': float('nan')}, {'band': (0.1, float('inf'))}, {'drag': (1, 2, 3)}):
        with pytest.raises(ValueError):
            envs.param_ranges(gust, bad)


def test_a_class_without_params_ignores_unknown_keys_as_before():
    import omnisafe_amd
    from omnisafe_amd import envs

    cls = omnisafe_amd.register_device_env(GLIDER, 'Glider', ['GliderP-v0'])
    try:
        assert cls.param_names == () and cls.param_defaults == ()
        assert cls.entry_point == 'osa_custom_env_step' and cls.eval_entry_point == 'osa_custom_eval_episodes'
        assert envs.param_ranges(cls, {'wind': 0.3, 'anything': None}).shape == (2, 0)
    finally:
        omnisafe_amd.unregister_device_env('GliderP-v0')
    assert envs.param_ranges(envs.ReachVectorEnv, {'wind': 0.3}).shape == (2, 0)


# ------------------------------------------------------------------ the twin's own properties
def test_twin_a_fixed_range_returns_exactly_lo():
    rng = G.ranges(wind=0.3, drag=0.1, band=0.7, reach=0.15)
    for pos in (0, 1, 77):
        rows = G.param_draw(rng, 5, pos, np.arange(130))
        np.testing.assert_array_equal(rows, np.broadcast_to(rng[0], (130, 4)))


def test_twin_ranged_draws_stay_inside_their_range():
    """10 000 draws per parameter, with ranges whose lo + (hi - lo) * u can round past hi (u reaches 1): the clamp
    keeps every value inside -- not a statistical statement."""
    rng = np.float32([[0.1, 0.25, 1.0000001, -0.3], [0.1000001, 0.75, 1.0000004, 16777217.0]])
    rows = np.concatenate([G.param_draw(rng, 9, pos, np.arange(1000)) for pos in range(10)])
    assert rows.shape == (10000, 4) and rows.dtype == np.float32
    assert (rows >= rng[0]).all() and (rows <= rng[1]).all()
    assert len(np.unique(rows[:, 1])) > 9000  # (and they are draws, not one value)


def test_twin_rows_differ_between_envs_and_episodes_and_repeat_with_the_seed():
    rng = G.ranges(wind=(0.0, 0.5), band=(0.4, 0.8))
    N, H = 6, 5

    def play(seed):
        twin = G.GustTwin(rng, N, H, seed, terminates=False)
        twin.reset()
        rows = [twin.par.copy()]
        for _ in range(2 * H):
            twin.step(np.zeros((N, 2), np.float32))
            rows.append(twin.par.copy())
        return np.stack(rows)

    rows = play(3)
    assert len(np.unique(rows[0, :, 0])) == N and len(np.unique(rows[0, :, 2])) == N  # between envs
    np.testing.assert_array_equal(rows[1:H], np.broadcast_to(rows[0], (H - 1, N, 4)))  # constant inside an episode
    assert (rows[H, :, 0] != rows[0, :, 0]).all() and (rows[2 * H, :, 0] != rows[H, :, 0]).all()  # between episodes
    np.testing.assert_array_equal(rows[:, :, [1, 3]], np.broadcast_to(G.DEFAULT[[1, 3]], (2 * H + 1, N, 2)))
    np.testing.assert_array_equal(play(3), rows)  # the same seed repeats them
    assert (play(4)[0, :, 0] != rows[0, :, 0]).all()


def test_twin_steered_episodes_end_by_arriving_and_by_the_time_limit():
    """The trace test_custom_env_params_gpu.py plays against the device: under `steer` with noise, at horizon 12 over 40
    steps, envs arrive (terminate) at differing steps and some run into the time limit."""
    N, H = 130, 12
    twin = G.GustTwin(G.ranges(wind=(0.0, 0.5), reach=(0.05, 0.3)), N, H, 11)
    twin.reset()
    noise = np.random.default_rng(N).uniform(-1.5, 1.5, (40, N, 2)).astype(np.float32)
    n_term = n_trunc = n_cost = 0
    for t in range(40):
        _, _, c, term, trunc, _ = twin.step(G.steer(twin.state, noise[t]))
        assert not (term & trunc).any()
        n_term, n_trunc, n_cost = n_term + int(term.sum()), n_trunc + int(trunc.sum()), n_cost + int(c.sum())
    assert n_term >= 50 and n_trunc >= 50 and n_cost >= 10, (n_term, n_trunc, n_cost)
