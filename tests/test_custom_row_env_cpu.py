"""CPU: custom device envs with an object row in LDS (LDS_ROW = true), up to the GPU's edge.  hipcc cross-compiles
gfx950 without a GPU, so what the contract admits and rejects, what the libraries report and what register_device_env
makes of it are checked here; the kernels run in test_custom_row_env_gpu.py."""
import ctypes
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ENVS = os.path.join(HERE, 'custom_envs')
# struct -> header, (STATE, OBS, DYN, ACT, TRACE, LEVELS, LANES, terminates)
ROW_ENVS = {
    'GoalAgain': ('goal_again.h', [64, 60, 10, 2, 64, 2, None, 0]),
    'GoalAgain16': ('goal_again.h', [64, 60, 10, 2, 64, 2, 16, 0]),
    'GoalAgain32': ('goal_again.h', [64, 60, 10, 2, 64, 2, 32, 0]),
    'GoalAgain64': ('goal_again.h', [64, 60, 10, 2, 64, 2, 64, 0]),
    'CarGoalAgain': ('goal_again.h', [64, 72, 12, 2, 64, 2, None, 0]),
    'CarGoalAgain16': ('goal_again.h', [64, 72, 12, 2, 64, 2, 16, 0]),
    'CarGoalAgain32': ('goal_again.h', [64, 72, 12, 2, 64, 2, 32, 0]),
    'CarGoalAgain64': ('goal_again.h', [64, 72, 12, 2, 64, 2, 64, 0]),
    'Button': ('button.h', [64, 76, 14, 2, 64, 2, None, 0]),
    'CarButton': ('button.h', [64, 88, 14, 2, 64, 2, None, 0]),
    'Field': ('field.h', [150, 20, 4, 2, 150, 0, None, 1]),
    'Field16': ('field.h', [150, 20, 4, 2, 150, 0, 16, 1]),
    'Field32': ('field.h', [150, 20, 4, 2, 150, 0, 32, 1]),
    'Field64': ('field.h', [150, 20, 4, 2, 150, 0, 64, 1]),
    'FieldParam': ('field.h', [150, 20, 4, 2, 150, 0, None, 1]),
}

STATE_257 = '''
struct Bad : OsaPointGoal {
  static constexpr int STATE = 257;
};
'''
BAD_FRESH_OBJ = '''
struct Bad : OsaReachEnv {
  static constexpr bool LDS_ROW = true;
  static __device__ float fresh_obj(int col) { return 0.f; }
};
'''
WIDEST = '''
struct Widest : OsaReachEnv {
  static constexpr int STATE = 256, TRACE = 256;
  static constexpr bool LDS_ROW = true;
  static __device__ float fresh_obj(const OsaEnvAt&, int col) { return (float)col; }
};
'''


def test_the_manifest_names_every_row_example():
    with open(os.path.join(ENVS, 'MANIFEST.row.json'), encoding='utf-8') as f:
        manifest = json.load(f)
    assert {s: h for h, structs in manifest.items() for s in structs} == {s: h for s, (h, _) in ROW_ENVS.items()}


@pytest.mark.parametrize('struct', list(ROW_ENVS))
def test_an_object_row_description_builds_and_reports_its_widths(struct):
    from omnisafe_amd import build

    header, expect = ROW_ENVS[struct]
    lib = ctypes.CDLL(build.build_custom_env(os.path.join(ENVS, header), struct))
    info, row = (ctypes.c_int * 8)(), (ctypes.c_int * 4)()
    assert lib.osa_custom_env_info(info) == 0 and lib.osa_custom_row_info(row) == 0
    assert [v for v, e in zip(info, expect) if e is not None] == [e for e in expect if e is not None]
    assert info[6] in (16, 32, 64)  # (None above: the row kernel's default, whatever was measured fastest)
    assert list(row) == [1, 256, 0, 0]


def test_a_register_state_library_reports_its_row_kind_too():
    from omnisafe_amd import build

    lib = ctypes.CDLL(build.build_custom_env(os.path.join(ENVS, 'glider.h'), 'Glider'))
    row = (ctypes.c_int * 4)()
    assert lib.osa_custom_row_info(row) == 0 and list(row) == [0, 64, 0, 0]


def test_the_widest_row_is_within_the_contract(tmp_path):
    from omnisafe_amd import build

    header = str(tmp_path / 'widest.h')
    with open(header, 'w', encoding='utf-8') as f:
        f.write(WIDEST)
    path = build.build_custom_env(header, 'Widest')
    try:
        info = (ctypes.c_int * 8)()
        assert ctypes.CDLL(path).osa_custom_env_info(info) == 0 and list(info)[:5] == [256, 6, 6, 2, 256]
    finally:
        os.remove(path)


@pytest.mark.parametrize('source, expect', [
    (STATE_257, 'with LDS_ROW = true STATE must be 1 .. 256'),
    (BAD_FRESH_OBJ, 'a member fresh_obj that cannot be called as float fresh_obj(const OsaEnvAt&, int col)'),
], ids=['state_257', 'fresh_obj_signature'])
def test_the_row_contract_is_enforced_at_build_time(tmp_path, source, expect):
    from omnisafe_amd import _lib, build

    header = str(tmp_path / 'bad.h')
    with open(header, 'w', encoding='utf-8') as f:
        f.write(source)
    with pytest.raises(_lib.OsaError) as err:
        build.build_custom_env(header, 'Bad')
    text = str(err.value)
    assert expect in text and 'error' in text
    # each rejection has a message of its own: neither is told what a register-state description is told
    assert 'LDS_ROW must be false' not in text and 'STATE must be 1 .. 64' not in text
    assert not os.path.exists(build.custom_env_path(header, 'Bad'))


def test_registration_reports_the_row_kind_on_the_class():
    import omnisafe_amd
    from omnisafe_amd import envs

    ids = {'SynthNavButton0-v0': 0, 'SynthNavButton1-v0': 1, 'SynthNavButton2-v0': 2}
    before = sorted(envs.ENV_REGISTRY)
    cls = omnisafe_amd.register_device_env(os.path.join(ENVS, 'button.h'), 'Button', ids, default_horizon=1000)
    flat = omnisafe_amd.register_device_env(os.path.join(ENVS, 'glider.h'), 'Glider', ['GliderRowKind-v0'])
    try:
        assert cls.lds_row is True and flat.lds_row is False and envs.CustomDeviceEnv.lds_row is False
        assert cls.dims('SynthNavButton1-v0') == (76, 2) and cls.state_width == 64 and cls.trace_state_floats == 64
        assert cls.graph_safe is True and cls.draws is True and cls.terminates is False and cls.max_level == 2
        assert cls.entry_point == 'osa_custom_env_step' and cls.eval_kind('SynthNavButton2-v0') == 2
        assert sorted(envs.ENV_REGISTRY) == before and not any('Button' in e for e in before)
        field = omnisafe_amd.register_device_env(os.path.join(ENVS, 'field.h'), 'Field', ['FieldRowKind-v0'], 12)
        try:
            assert field.lds_row is True and field.state_width == 150 and field.trace_state_floats == 150
            assert field.terminates is True and field.draws is False
        finally:
            omnisafe_amd.unregister_device_env('FieldRowKind-v0')
    finally:
        omnisafe_amd.unregister_device_env(*ids, 'GliderRowKind-v0')
