"""CPU: the optional draw() member of a device env description (include/omnisafe_amd_env.h) up to the GPU's edge.
hipcc cross-compiles gfx950 without a GPU: the example headers build, what the two render entry points of a library
report, what the contract rejects at build time, and what register_device_env makes of it.  The kernel runs in
test_custom_render_gpu.py."""
import ctypes
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ENVS = os.path.join(HERE, 'custom_envs')
GLIDER = os.path.join(ENVS, 'glider.h')
EINVAL, EUNSUPPORTED = -1, -3  # OSA_EINVAL, OSA_EUNSUPPORTED (include/omnisafe_amd.h)
DRAW_MAX = 64

POSITION = 'static __device__ void position(const float* rec, float& x, float& y) { x = rec[0]; y = rec[1]; }'
DRAW = 'static __device__ void draw(const float*, const OsaDrawAt&, OsaScene& s) { s.disc(0.f, 0.f, 1.f, 0xFFFFFF); }'
DRAW_TAKES_NO_SCENE = f'''
struct Bad : OsaReachEnv {{
  static constexpr float DRAW_VIEW = 2.f;
  {POSITION}
  static __device__ void draw(const float*, const OsaDrawAt&) {{}}
}};
'''
DRAW_IS_A_CONSTANT = f'''
struct Bad : OsaReachEnv {{
  static constexpr float DRAW_VIEW = 2.f;
  {POSITION}
  static constexpr bool draw = true;
}};
'''
DRAW_WITHOUT_POSITION = f'''
struct Bad : OsaReachEnv {{
  static constexpr float DRAW_VIEW = 2.f;
  {DRAW}
}};
'''
DRAW_WITHOUT_VIEW = f'''
struct Bad : OsaReachEnv {{
  {POSITION}
  {DRAW}
}};
'''
DRAW_VIEW_ZERO = f'''
struct Bad : OsaReachEnv {{
  static constexpr float DRAW_VIEW = 0.f;
  {POSITION}
  {DRAW}
}};
'''
DRAW_WITHOUT_TRACE = f'''
struct Bad : OsaReachEnv {{
  static constexpr int TRACE = 0;
  static constexpr float DRAW_VIEW = 2.f;
  {POSITION}
  {DRAW}
}};
'''


def render_info(header, struct):
    from omnisafe_amd import build

    lib = ctypes.CDLL(build.build_custom_env(header, struct))
    out_i, out_f = (ctypes.c_int * 4)(), (ctypes.c_float * 2)()
    assert lib.osa_custom_render_info(out_i, out_f) == 0
    return lib, list(out_i), list(out_f)


def test_the_manifest_lists_the_example_headers():
    with open(os.path.join(ENVS, 'MANIFEST.render.json'), encoding='utf-8') as f:
        manifest = json.load(f)
    assert manifest['reach_drawn.h'] == ['ReachDrawn'] and manifest['circle_drawn.h'] == ['CircleDrawn']
    assert manifest['ledge_drawn.h'] == ['LedgeDrawn']
    for header in manifest:
        assert os.path.exists(os.path.join(ENVS, header))


@pytest.mark.parametrize('header, struct, trace, views', [
    ('reach_drawn.h', 'ReachDrawn', 6, [1.75, 1.0]), ('circle_drawn.h', 'CircleDrawn', 8, [2.25, 1.0]),
    ('ledge_drawn.h', 'LedgeDrawn', 5, [3.5, 1.5]), ('scene_caps.h', 'DrawOver', 6, [2.0, 1.0])])
def test_a_drawing_description_builds_and_says_so(header, struct, trace, views):
    lib, out_i, out_f = render_info(os.path.join(ENVS, header), struct)
    assert out_i == [1, DRAW_MAX, trace, 0] and out_f == views  # draws, OSA_DRAW_MAX, TRACE, reserved; the views
    assert hasattr(lib, 'osa_custom_render_episode')


def test_a_description_without_draw_has_both_symbols_and_does_not_draw():
    for header, struct, trace in ((GLIDER, 'Glider', 10), (os.path.join(ENVS, 'reach_again.h'), 'ReachAgain', 6)):
        lib, out_i, out_f = render_info(header, struct)
        assert out_i == [0, DRAW_MAX, trace, 0] and out_f == [0.0, 0.0]
        lib.osa_custom_render_episode.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_long] + [ctypes.c_int] * 3 + [
            ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
        # (never launches: the pointers are checked for NULL and alignment only, then the description does not draw)
        assert lib.osa_custom_render_episode(0, 64, 8, 0, 1, 0, None, 0, 8, 8, 1, 64, None) == EUNSUPPORTED
        assert lib.osa_custom_render_episode(0, None, 8, 0, 1, 0, None, 0, 8, 8, 1, 64, None) == EINVAL
        assert lib.osa_custom_render_episode(0, 64, 8, 0, 1, 0, None, 0, 6, 8, 1, 64, None) == EINVAL  # width % 4
        assert lib.osa_custom_render_episode(3, 64, 8, 0, 1, 0, None, 0, 8, 8, 1, 64, None) == EINVAL  # level > LEVELS
        # the env info of a description without draw() is what it was
        info = (ctypes.c_int * 8)()
        assert lib.osa_custom_env_info(info) == 0 and info[4] == trace


@pytest.mark.parametrize('source, expect', [
    (DRAW_TAKES_NO_SCENE, 'has a member draw that cannot be called as draw(const float* rec'),
    (DRAW_IS_A_CONSTANT, 'has a member draw that cannot be called as draw(const float* rec'),
    (DRAW_WITHOUT_POSITION, 'a description with draw() needs position(const float* rec, float& x, float& y)'),
    (DRAW_WITHOUT_VIEW, 'a description with draw() needs DRAW_VIEW'),
    (DRAW_VIEW_ZERO, 'DRAW_VIEW must be greater than 0'),
    (DRAW_WITHOUT_TRACE, 'a description with draw() needs TRACE >= 1'),
], ids=['takes_no_scene', 'a_constant', 'no_position', 'no_view', 'view_zero', 'trace_zero'])
def test_a_draw_that_cannot_work_is_rejected_at_build_time(tmp_path, source, expect):
    from omnisafe_amd import _lib, build

    header = str(tmp_path / 'bad.h')
    with open(header, 'w', encoding='utf-8') as f:
        f.write(source)
    with pytest.raises(_lib.OsaError) as err:
        build.build_custom_env(header, 'Bad')
    text = str(err.value)
    assert expect in text and 'error' in text
    assert text.count('static assertion failed') == 1  # one message, not a cascade
    assert not os.path.exists(build.custom_env_path(header, 'Bad'))


def test_register_device_env_sets_draws():
    import omnisafe_amd
    from omnisafe_amd import envs, render

    assert envs.CustomDeviceEnv.draws is False and envs.CustomDeviceEnv.render_state is False
    drawn = omnisafe_amd.register_device_env(os.path.join(ENVS, 'ledge_drawn.h'), 'LedgeDrawn',
                                             {'LedgeDrawn0-v0': 0, 'LedgeDrawn1-v0': 1}, default_horizon=60)
    plain = omnisafe_amd.register_device_env(os.path.join(ENVS, 'ledge.h'), 'Ledge', ['LedgePlain-v0'])
    again = omnisafe_amd.register_device_env(os.path.join(ENVS, 'reach_again.h'), 'ReachAgain', ['ReachPlain-v0'])
    try:
        assert drawn.draws is True and drawn.render_state is True and drawn.terminates is True
        assert drawn.draw_max == DRAW_MAX and drawn.draw_view == (3.5, 1.5) and drawn.trace_state_floats == 5
        assert drawn.render_kind('LedgeDrawn1-v0') == render.CustomScene(drawn, 1)
        assert render.row_floats(drawn.render_kind('LedgeDrawn0-v0')) == 5
        for cls in (plain, again):  # (ReachAgain = OsaReachEnv: the built-in descriptions have no draw())
            assert cls.draws is False and cls.render_state is False and cls.draw_view == (0.0, 0.0)
        assert envs.ENV_REGISTRY['SynthReach-v0'].render_kind('SynthReach-v0') == 1
    finally:
        omnisafe_amd.unregister_device_env('LedgeDrawn0-v0', 'LedgeDrawn1-v0', 'LedgePlain-v0', 'ReachPlain-v0')
