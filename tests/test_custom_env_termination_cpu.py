"""CPU: the optional terminal() member of a device env description (include/omnisafe_amd_env.h) up to the GPU's edge.
hipcc cross-compiles gfx950 without a GPU: what the library reports about termination, what the contract rejects at
build time, and what register_device_env makes of it.  The kernels run in test_custom_env_termination_gpu.py."""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LEDGE = os.path.join(HERE, 'custom_envs', 'ledge.h')
GLIDER = os.path.join(HERE, 'custom_envs', 'glider.h')

# members named terminal that the kernels could not call: ignoring them would give an env that never ends
TERMINAL_WITHOUT_AT = '''
struct Bad : OsaReachEnv {
  static __device__ bool terminal(const Regs& s, const float*) { return s.s[0] > 1.f; }
};
'''
TERMINAL_TAKES_AN_ACTION = '''
struct Bad : OsaReachEnv {
  static __device__ bool terminal(const Regs& s, const float*, const OsaEnvAt&, float a0) { return s.s[0] > a0; }
};
'''
TERMINAL_IS_A_CONSTANT = '''
struct Bad : OsaReachEnv {
  static constexpr bool terminal = true;
};
'''
TERMINAL_RETURNS_NOTHING = '''
struct Bad : OsaReachEnv {
  static __device__ void terminal(const Regs&, const float*, const OsaEnvAt&) {}
};
'''
# ... and one the kernels can call although it is not spelled like the contract (an int for the bool)
TERMINAL_RETURNS_AN_INT = '''
struct Fine : OsaReachEnv {
  static __device__ int terminal(const Regs& s, const float*, const OsaEnvAt&) { return s.s[0] > 1.f; }
};
'''


def info_of(header, struct):
    from omnisafe_amd import build

    lib = ctypes.CDLL(build.build_custom_env(header, struct))
    info = (ctypes.c_int * 8)()
    assert lib.osa_custom_env_info(info) == 0
    return list(info)


def test_info_reports_whether_the_description_terminates():
    assert info_of(LEDGE, 'Ledge') == [6, 20, 5, 2, 5, 1, 32, 1]  # STATE OBS DYN ACT TRACE LEVELS LANES terminates
    assert info_of(LEDGE, 'LedgeEndless') == [6, 20, 5, 2, 5, 1, 32, 0]
    assert info_of(LEDGE, 'Ledge16') == [6, 20, 5, 2, 5, 1, 16, 1]
    assert info_of(LEDGE, 'Ledge64') == [6, 20, 5, 2, 5, 1, 64, 1]
    assert info_of(GLIDER, 'Glider')[7] == 0


@pytest.mark.parametrize('source', [TERMINAL_WITHOUT_AT, TERMINAL_TAKES_AN_ACTION, TERMINAL_IS_A_CONSTANT,
                                    TERMINAL_RETURNS_NOTHING],
                         ids=['without_at', 'takes_an_action', 'a_constant', 'returns_nothing'])
def test_a_terminal_that_cannot_be_called_is_rejected_at_build_time(tmp_path, source):
    from omnisafe_amd import _lib, build

    header = str(tmp_path / 'bad.h')
    with open(header, 'w', encoding='utf-8') as f:
        f.write(source)
    with pytest.raises(_lib.OsaError) as err:
        build.build_custom_env(header, 'Bad')
    text = str(err.value)
    assert 'has a member terminal that cannot be called as bool terminal(const Regs&' in text and 'error' in text
    assert not os.path.exists(build.custom_env_path(header, 'Bad'))
    assert not [f for f in os.listdir(build.CUSTOM_DIR) if f.startswith('Bad')]


def test_a_terminal_that_converts_to_bool_is_taken(tmp_path):
    from omnisafe_amd import build

    header = str(tmp_path / 'fine.h')
    with open(header, 'w', encoding='utf-8') as f:
        f.write(TERMINAL_RETURNS_AN_INT)
    try:
        assert info_of(header, 'Fine') == [8, 6, 6, 2, 6, 2, 32, 1]
    finally:
        path = build.custom_env_path(header, 'Fine')
        if os.path.exists(path):
            os.remove(path)


def test_register_device_env_sets_terminates():
    import omnisafe_amd
    from omnisafe_amd import envs

    assert envs.DeviceEnvProtocol.terminates is False
    assert not any(cls.terminates for cls in envs.DeviceVectorEnv.__subclasses__())  # no built-in family terminates
    ledge = omnisafe_amd.register_device_env(LEDGE, 'Ledge', {'Ledge0-v0': 0, 'Ledge1-v0': 1}, default_horizon=60)
    endless = omnisafe_amd.register_device_env(LEDGE, 'LedgeEndless', ['LedgeEndless-v0'])
    glider = omnisafe_amd.register_device_env(GLIDER, 'Glider', ['GliderT-v0'])
    try:
        assert ledge.terminates is True and endless.terminates is False and glider.terminates is False
        assert ledge.graph_safe is True and ledge.dims('Ledge1-v0') == (20, 2) and ledge.state_width == 6
        assert ledge.trace_state_floats == 5 and ledge.max_level == 1 and ledge.default_horizon == 60
    finally:
        omnisafe_amd.unregister_device_env('Ledge0-v0', 'Ledge1-v0', 'LedgeEndless-v0', 'GliderT-v0')
