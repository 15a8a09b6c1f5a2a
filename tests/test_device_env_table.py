"""CPU: the per-class facts of the device envs (envs.DeviceVectorEnv subclasses) against one table of literals, for
every registered id, and what the evaluator, the plugin and the ctypes table derive from them.  Needs neither the
library nor a GPU."""
import sys
import types

# id: class, (obs_dim, act_dim), level (None: the family has none), default horizon, floats per state row,
#     env_kind of osa_eval_episodes, state floats of an evaluator trace record
TABLE = {
    'SynthPointGoal1-v0': ('SynthVectorEnv', (60, 2), None, 1000, 0, 0, 0),
    'SynthCarGoal1-v0': ('SynthVectorEnv', (72, 2), None, 1000, 0, 0, 0),
    'SynthAnt-v0': ('SynthVectorEnv', (27, 8), None, 1000, 0, 0, 0),
    'SynthHumanoid-v0': ('SynthVectorEnv', (376, 17), None, 1000, 0, 0, 0),
    'SynthTiny-v0': ('SynthVectorEnv', (6, 2), None, 1000, 0, 0, 0),
    'SynthReach-v0': ('ReachVectorEnv', (60, 2), None, 50, 8, 1, 6),
    'SynthNavGoal0-v0': ('NavGoalVectorEnv', (60, 2), 0, 1000, 64, 16, 64),
    'SynthNavGoal1-v0': ('NavGoalVectorEnv', (60, 2), 1, 1000, 64, 17, 64),
    'SynthNavGoal2-v0': ('NavGoalVectorEnv', (60, 2), 2, 1000, 64, 18, 64),
    'SynthNavCircle0-v0': ('NavCircleVectorEnv', (28, 2), 0, 500, 8, 32, 8),
    'SynthNavCircle1-v0': ('NavCircleVectorEnv', (28, 2), 1, 500, 8, 33, 8),
    'SynthNavCircle2-v0': ('NavCircleVectorEnv', (28, 2), 2, 500, 8, 34, 8),
    'SynthNavCarGoal0-v0': ('NavCarGoalVectorEnv', (72, 2), 0, 1000, 64, 48, 64),
    'SynthNavCarGoal1-v0': ('NavCarGoalVectorEnv', (72, 2), 1, 1000, 64, 49, 64),
    'SynthNavCarGoal2-v0': ('NavCarGoalVectorEnv', (72, 2), 2, 1000, 64, 50, 64),
    'SynthNavCarCircle0-v0': ('NavCarCircleVectorEnv', (40, 2), 0, 500, 12, 64, 12),
    'SynthNavCarCircle1-v0': ('NavCarCircleVectorEnv', (40, 2), 1, 500, 12, 65, 12),
    'SynthNavCarCircle2-v0': ('NavCarCircleVectorEnv', (40, 2), 2, 500, 12, 66, 12),
}
ENTRY_POINTS = {'SynthVectorEnv': 'osa_synth_env_step', 'ReachVectorEnv': 'osa_reach_env_step',
                'NavGoalVectorEnv': 'osa_nav_env_step', 'NavCircleVectorEnv': 'osa_circle_env_step',
                'NavCarGoalVectorEnv': 'osa_car_goal_env_step', 'NavCarCircleVectorEnv': 'osa_car_circle_env_step'}


def test_every_registered_id_against_the_table():
    import inspect

    from omnisafe_amd import envs

    assert sorted(envs.ENV_REGISTRY) == sorted(TABLE) == envs.support_envs()
    for env_id, (name, dims, level, horizon, state_w, kind, trace_w) in TABLE.items():
        cls = envs.ENV_REGISTRY[env_id]
        assert cls is getattr(envs, name) and issubclass(cls, envs.DeviceVectorEnv), env_id
        assert env_id in cls._support_envs and cls.entry_point == ENTRY_POINTS[name], env_id
        assert cls.dims(env_id) == dims, env_id
        assert cls.levels.get(env_id) == level, env_id
        assert cls.default_horizon == horizon, env_id
        in_signature = inspect.signature(cls.__init__).parameters['horizon'].default
        assert in_signature in (None, horizon), env_id  # None: the class attribute decides
        assert cls.state_width == state_w, env_id
        assert cls.eval_kind(env_id) == kind, env_id
        assert cls.trace_state_floats == trace_w, env_id


def test_evaluator_and_ctypes_table_derive_from_the_classes():
    from omnisafe_amd import _lib, envs, evaluator

    assert set(evaluator.DEVICE_ENVS) == {getattr(envs, name) for name in ENTRY_POINTS}
    assert len(evaluator.DEVICE_ENVS) == 6
    with_level = [e for name, e in ENTRY_POINTS.items() if getattr(envs, name).levels]
    assert len(with_level) == 4
    for entry in with_level:
        assert _lib.SIGNATURES[entry] is _lib.SIGNATURES['osa_nav_env_step']
    restype, args = _lib.SIGNATURES['osa_nav_env_step']
    assert len(args) == 21 and len(_lib.SIGNATURES['osa_reach_env_step'][1]) == 20  # level is the one more
    assert len(_lib.SIGNATURES['osa_synth_env_step'][1]) == 18


def test_plugin_registers_each_class_under_its_own_key(monkeypatch):
    """install() against a stand-in for the reference's two registries: one key 'OmnisafeAmd' + class name per class,
    holding the ids the reference does not know yet."""
    from omnisafe_amd import envs, plugin

    class EnvRegistry:
        def __init__(self):
            self._class, self._support_envs = {}, {'Theirs': ['SynthNavGoal1-v0']}

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
    assert set(reg._class) == {'OmnisafeAmd' + name for name in ENTRY_POINTS}
    for name in ENTRY_POINTS:
        cls = getattr(envs, name)
        assert reg._class['OmnisafeAmd' + name] is cls
        ids = [e for e, row in TABLE.items() if row[0] == name and e != 'SynthNavGoal1-v0']
        assert reg._support_envs['OmnisafeAmd' + name] == ids
