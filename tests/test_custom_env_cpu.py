"""CPU: register_device_env up to the GPU's edge.  hipcc cross-compiles gfx950 without a GPU, so the out-of-tree build,
its cache, what the contract's static_asserts reject, the registry and the plugin are all checked here; the kernels
themselves run in test_custom_env_gpu.py."""
import ctypes
import os
import shutil
import sys
import types

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GLIDER = os.path.join(HERE, 'custom_envs', 'glider.h')

BAD_LDS_ROW = '''
struct Bad : OsaReachEnv {
  static constexpr bool LDS_ROW = true;
};
'''
BAD_STATE = '''
struct Bad : OsaReachEnv {
  static constexpr int STATE = 65;
};
'''
NO_OBS_COL = '''
struct Bad {
  static constexpr int STATE = 4, OBS = 4, DYN = 4, ACT = 2, TRACE = 4;
  static constexpr bool LDS_ROW = false;
  struct Regs { float x[4]; };
  static __device__ void load(Regs&, const float*) {}
  static __device__ void store(const Regs&, float*) {}
  static __device__ void fresh(Regs&, const OsaEnvAt&, const float*) {}
  static __device__ void transition(Regs&, const float*, const OsaEnvAt&, float, float, float& r, float& c) { r = c = 0.f; }
  static __device__ float state_col(const Regs&, const float*, int) { return 0.f; }
};
'''


def test_build_reports_the_headers_constants_and_caches():
    from omnisafe_amd import build

    path = build.build_custom_env(GLIDER, 'Glider')
    assert os.path.dirname(path) == os.path.join(build.LIB_DIR, 'custom')
    assert os.path.basename(path).startswith('Glider-') and path.endswith('.so')
    lib = ctypes.CDLL(path)
    info = (ctypes.c_int * 8)()
    assert lib.osa_custom_env_info(info) == 0
    assert list(info) == [12, 70, 10, 3, 10, 1, 32, 0]  # STATE OBS DYN ACT TRACE LEVELS LANES 0
    for name in ('osa_custom_env_step', 'osa_custom_eval_episodes'):
        assert hasattr(lib, name)
    assert not [f for f in os.listdir(os.path.dirname(path)) if f.endswith(('.o', '.tmp'))]
    # the other lane counts are other structs of the same header
    for struct, lanes in (('Glider16', 16), ('Glider64', 64)):
        other = ctypes.CDLL(build.build_custom_env(GLIDER, struct))
        assert other.osa_custom_env_info(info) == 0 and info[6] == lanes and list(info)[:6] == [12, 70, 10, 3, 10, 1]


def test_second_build_starts_no_compiler(monkeypatch):
    from omnisafe_amd import build

    path = build.build_custom_env(GLIDER, 'Glider')
    mtime = os.stat(path).st_mtime_ns

    def no_compiler(*args, **kwargs):
        raise AssertionError('a cached library must not start the compiler')

    monkeypatch.setattr(build.subprocess, 'run', no_compiler)
    monkeypatch.setattr(build, '_hipcc', no_compiler)
    assert build.build_custom_env(GLIDER, 'Glider') == path
    assert os.stat(path).st_mtime_ns == mtime


def test_a_changed_header_is_another_library(tmp_path):
    from omnisafe_amd import build

    copy = str(tmp_path / 'glider.h')
    shutil.copy(GLIDER, copy)
    same = build.custom_env_path(copy, 'Glider')
    assert os.path.basename(same) == os.path.basename(build.custom_env_path(GLIDER, 'Glider'))  # content, not location
    with open(copy, 'a', encoding='utf-8') as f:
        f.write('// a comment\n')
    assert build.custom_env_path(copy, 'Glider') != same
    assert build.custom_env_path(GLIDER, 'Glider16') != build.custom_env_path(GLIDER, 'Glider')


def test_the_digest_covers_the_custom_translation_unit(tmp_path, monkeypatch):
    """source_digest() globs csrc/*.hip; csrc/custom/custom_env.hip, which defines the entry points, is hashed too."""
    from omnisafe_amd import build

    before = build.custom_env_path(GLIDER, 'Glider')
    copy = str(tmp_path / 'custom_env.hip')
    shutil.copy(build.CUSTOM_SRC, copy)
    monkeypatch.setattr(build, 'CUSTOM_SRC', copy)
    assert build.custom_env_path(GLIDER, 'Glider') == before
    with open(copy, 'a', encoding='utf-8') as f:
        f.write('// a comment\n')
    assert build.custom_env_path(GLIDER, 'Glider') != before


def test_one_action_column_is_within_the_contract():
    from omnisafe_amd import build

    lib = ctypes.CDLL(build.build_custom_env(os.path.join(HERE, 'custom_envs', 'slider.h'), 'Slider'))
    info = (ctypes.c_int * 8)()
    assert lib.osa_custom_env_info(info) == 0
    assert list(info) == [2, 3, 2, 1, 2, 0, 32, 0]  # ACT = 1; the GPU tests step it with a row stride of 1


def test_concurrent_builds_share_one_library_and_prune_older_ones(tmp_path):
    """Two threads that build the same (header, struct) at once each write a file of their own and leave one library;
    libraries of the struct from earlier versions of the header go, those of other structs stay."""
    from concurrent.futures import ThreadPoolExecutor

    from omnisafe_amd import build

    header = str(tmp_path / 'prune.h')
    with open(header, 'w', encoding='utf-8') as f:
        f.write('struct PruneMe : OsaReachEnv {};\n')
    os.makedirs(build.CUSTOM_DIR, exist_ok=True)
    older = os.path.join(build.CUSTOM_DIR, 'PruneMe-0123456789abcdef.so')
    other = os.path.join(build.CUSTOM_DIR, 'PruneMeNot-0123456789abcdef.so')
    for stale in (older, other):
        open(stale, 'wb').close()
    try:
        with ThreadPoolExecutor(max_workers=2) as ex:
            paths = list(ex.map(lambda _: build.build_custom_env(header, 'PruneMe'), range(2)))
        assert paths[0] == paths[1] == build.custom_env_path(header, 'PruneMe')
        info = (ctypes.c_int * 8)()
        assert ctypes.CDLL(paths[0]).osa_custom_env_info(info) == 0 and info[0] == 8
        left = sorted(f for f in os.listdir(build.CUSTOM_DIR) if f.startswith('PruneMe'))
        assert left == sorted([os.path.basename(paths[0]), os.path.basename(other)])
    finally:
        for f in os.listdir(build.CUSTOM_DIR):
            if f.startswith('PruneMe'):
                os.remove(os.path.join(build.CUSTOM_DIR, f))


@pytest.mark.parametrize('source, struct, expect', [
    (BAD_LDS_ROW, 'Bad', 'LDS_ROW must be false'),
    (BAD_STATE, 'Bad', 'STATE must be 1 .. 64'),
    (NO_OBS_COL, 'Bad', 'has no obs_col'),
    (BAD_STATE, 'Absent', 'Absent'),  # no such struct: the compiler's own error names it
], ids=['lds_row', 'state_65', 'no_obs_col', 'missing_struct'])
def test_the_contract_is_enforced_at_build_time(tmp_path, source, struct, expect):
    from omnisafe_amd import _lib, build

    header = str(tmp_path / 'bad.h')
    with open(header, 'w', encoding='utf-8') as f:
        f.write(source)
    with pytest.raises(_lib.OsaError) as err:
        build.build_custom_env(header, struct)
    assert expect in str(err.value) and 'error' in str(err.value)
    assert not os.path.exists(build.custom_env_path(header, struct))


@pytest.fixture
def glider_ids():
    import omnisafe_amd

    ids = {'Glider0-v0': 0, 'Glider1-v0': 1}
    cls = omnisafe_amd.register_device_env(GLIDER, 'Glider', ids, default_horizon=40)
    try:
        yield cls
    finally:
        left = [e for e in ids if e in omnisafe_amd.custom_envs()]
        omnisafe_amd.unregister_device_env(*left)


def _closed_lists():
    from omnisafe_amd import envs, evaluator

    return (sorted(envs.ENV_REGISTRY), envs.support_envs(), evaluator.DEVICE_ENVS,
            envs.DeviceVectorEnv.__subclasses__())


def test_registration_leaves_the_built_in_lists_alone():
    import omnisafe_amd
    from omnisafe_amd import envs

    before = _closed_lists()
    assert len(before[0]) == 18 and len(before[3]) == 6 and omnisafe_amd.custom_envs() == []
    cls = omnisafe_amd.register_device_env(GLIDER, 'Glider', {'Glider0-v0': 0, 'Glider1-v0': 1}, default_horizon=40)
    try:
        assert _closed_lists() == before
        assert omnisafe_amd.custom_envs() == ['Glider0-v0', 'Glider1-v0']
        assert envs.CUSTOM_ENV_REGISTRY == {'Glider0-v0': cls, 'Glider1-v0': cls}
        # the class: its facts are the library's, and it is no built-in family
        assert issubclass(cls, envs.CustomDeviceEnv) and issubclass(cls, envs.DeviceEnvProtocol)
        assert not issubclass(cls, envs.DeviceVectorEnv) and issubclass(envs.DeviceVectorEnv, envs.DeviceEnvProtocol)
        assert cls.dims('Glider1-v0') == (70, 3) and cls.state_width == 12 and cls.trace_state_floats == 10
        assert cls.levels == {'Glider0-v0': 0, 'Glider1-v0': 1} and cls.eval_kind('Glider1-v0') == 1
        assert cls.default_horizon == 40 and cls.graph_safe is True and cls.lanes == 32
        assert cls.entry_point == 'osa_custom_env_step' and cls.struct == 'Glider'
        with pytest.raises(KeyError):
            omnisafe_amd.register_device_env(GLIDER, 'Glider', ['Glider1-v0'])  # a custom id, taken
        with pytest.raises(KeyError):
            omnisafe_amd.register_device_env(GLIDER, 'Glider', ['SynthReach-v0'])  # a built-in id
        with pytest.raises(ValueError):
            omnisafe_amd.register_device_env(GLIDER, 'Glider', {'Glider2-v0': 2})  # LEVELS = 1
        assert omnisafe_amd.custom_envs() == ['Glider0-v0', 'Glider1-v0']
    finally:
        omnisafe_amd.unregister_device_env('Glider0-v0', 'Glider1-v0')
    assert _closed_lists() == before
    assert omnisafe_amd.custom_envs() == [] and envs.CUSTOM_ENV_REGISTRY == {}
    with pytest.raises(KeyError):
        omnisafe_amd.unregister_device_env('Glider0-v0')


def test_a_list_of_ids_is_level_zero():
    import omnisafe_amd

    cls = omnisafe_amd.register_device_env(GLIDER, 'Glider', ['GliderFlat-v0'])
    try:
        assert cls.levels == {'GliderFlat-v0': 0} and cls.default_horizon == 1000
    finally:
        omnisafe_amd.unregister_device_env('GliderFlat-v0')


def test_further_ids_of_a_struct_join_its_class(glider_ids):
    """One class per struct name, which is the plugin's key: a second registration with the same library and default
    horizon extends the class, any other is refused, and unregistering takes ids out one by one."""
    import omnisafe_amd
    from omnisafe_amd import envs

    again = omnisafe_amd.register_device_env(GLIDER, 'Glider', {'GliderMore-v0': 1}, default_horizon=40)
    try:
        assert again is glider_ids
        assert again._support_envs == ['Glider0-v0', 'Glider1-v0', 'GliderMore-v0']
        assert again.levels == {'Glider0-v0': 0, 'Glider1-v0': 1, 'GliderMore-v0': 1}
        assert envs.custom_env_classes() == [glider_ids]
        with pytest.raises(ValueError, match='registered already'):
            omnisafe_amd.register_device_env(GLIDER, 'Glider', ['GliderLong-v0'], default_horizon=1000)
        assert 'GliderLong-v0' not in omnisafe_amd.custom_envs()
    finally:
        omnisafe_amd.unregister_device_env('GliderMore-v0')
    assert glider_ids._support_envs == ['Glider0-v0', 'Glider1-v0'] and 'GliderMore-v0' not in glider_ids.levels
    # with every id gone the name is free again, for another default horizon as well
    omnisafe_amd.unregister_device_env('Glider0-v0', 'Glider1-v0')
    fresh = omnisafe_amd.register_device_env(GLIDER, 'Glider', ['GliderLong-v0'], default_horizon=1000)
    try:
        assert fresh is not glider_ids and fresh.default_horizon == 1000 and glider_ids.levels == {}
    finally:
        omnisafe_amd.unregister_device_env('GliderLong-v0')


def test_the_evaluator_learns_the_dimensions_from_the_class(glider_ids):
    from omnisafe_amd import saved_policy

    assert saved_policy.device_env_class('Glider1-v0') is glider_ids
    assert saved_policy.device_env_class('SynthReach-v0').__name__ == 'ReachVectorEnv'
    assert saved_policy.device_env_class('NoSuchEnv-v0') is None


def test_plugin_registers_the_custom_class_under_its_own_key(monkeypatch, glider_ids):
    """install() against the stand-in registries of test_device_env_table.py: the six built-in keys as they are, and
    one more for the custom class."""
    from test_device_env_table import ENTRY_POINTS, TABLE

    from omnisafe_amd import envs, plugin

    class EnvRegistry:
        def __init__(self):
            self._class, self._support_envs = {}, {'Theirs': ['SynthNavGoal1-v0', 'Glider0-v0']}

        def support_envs(self):
            return [e for ids in self._support_envs.values() for e in ids]

    reg = EnvRegistry()
    mods = {'omnisafe': types.ModuleType('omnisafe'), 'omnisafe.algorithms': types.ModuleType('omnisafe.algorithms'),
            'omnisafe.algorithms.registry': types.ModuleType('omnisafe.algorithms.registry'),
            'omnisafe.envs': types.ModuleType('omnisafe.envs'), 'omnisafe.envs.core': types.ModuleType('omnisafe.envs.core')}
    mods['omnisafe.algorithms.registry'].REGISTRY = types.SimpleNamespace(_module_dict={})
    mods['omnisafe.envs.core'].ENV_REGISTRY = reg
    mods['omnisafe.algorithms'].registry = mods['omnisafe.algorithms.registry']
    mods['omnisafe.envs'].core = mods['omnisafe.envs.core']
    for name, mod in mods.items():
        monkeypatch.setitem(sys.modules, name, mod)
    assert plugin.install() == []
    assert set(reg._class) == {'OmnisafeAmd' + name for name in ENTRY_POINTS} | {'OmnisafeAmdCustomGlider'}
    assert reg._class['OmnisafeAmdCustomGlider'] is glider_ids
    assert reg._support_envs['OmnisafeAmdCustomGlider'] == ['Glider1-v0']  # (theirs knew Glider0-v0 already)
    for name in ENTRY_POINTS:
        assert reg._class['OmnisafeAmd' + name] is getattr(envs, name)
        ids = [e for e, row in TABLE.items() if row[0] == name and e != 'SynthNavGoal1-v0']
        assert reg._support_envs['OmnisafeAmd' + name] == ids
