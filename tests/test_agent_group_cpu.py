"""AgentGroup without a GPU: variant expansion, configuration checks, log directories, the world-size refusal."""
import pytest


def test_seeds_are_shorthand_for_seed_variants():
    from omnisafe_amd.group import member_cfgs

    shared = {'algo_cfgs': {'batch_size': 64}, 'logger_cfgs': {'log_dir': '/tmp/x'}}
    a = member_cfgs('PPOLag', seeds=range(3), custom_cfgs=shared)
    b = member_cfgs('PPOLag', variants=[{'seed': 0}, {'seed': 1}, {'seed': 2}], custom_cfgs=shared)
    assert a == b and [c['seed'] for c in a] == [0, 1, 2]
    assert all(c['algo_cfgs'] == {'batch_size': 64} for c in a)
    assert shared == {'algo_cfgs': {'batch_size': 64}, 'logger_cfgs': {'log_dir': '/tmp/x'}}  # not modified


def test_variant_overlays_merge_into_the_shared_cfgs():
    from omnisafe_amd.group import member_cfgs

    shared = {'seed': 5, 'algo_cfgs': {'batch_size': 64, 'clip': 0.2}}
    out = member_cfgs('PPOLag', variants=[{'algo_cfgs': {'clip': 0.1}}, {'seed': 9}], custom_cfgs=shared)
    assert out[0]['seed'] == 5 and out[0]['algo_cfgs'] == {'batch_size': 64, 'clip': 0.1}
    assert out[1]['seed'] == 9 and out[1]['algo_cfgs'] == {'batch_size': 64, 'clip': 0.2}


def test_seeds_and_variants_together_or_neither_is_an_error():
    from omnisafe_amd.group import member_cfgs

    with pytest.raises(ValueError):
        member_cfgs('PPOLag', seeds=[0], variants=[{'seed': 1}])
    with pytest.raises(ValueError):
        member_cfgs('PPOLag')
    with pytest.raises(ValueError):
        member_cfgs('PPOLag', variants=[])


def test_unknown_key_raises_the_same_error_as_agent():
    import omnisafe_amd

    bad = {'algo_cfgs': {'no_such_key': 1}}
    with pytest.raises(Exception) as solo:
        omnisafe_amd.Agent('PPOLag', 'SynthReach-v0', custom_cfgs=bad)
    with pytest.raises(Exception) as grouped:
        omnisafe_amd.AgentGroup('PPOLag', 'SynthReach-v0', variants=[{'seed': 0}, bad])
    assert type(grouped.value) is type(solo.value) and str(grouped.value) == str(solo.value)
    with pytest.raises(type(solo.value)):
        omnisafe_amd.AgentGroup('PPOLag', 'SynthReach-v0', seeds=[0], custom_cfgs=bad)


def test_every_member_has_its_own_log_directory():
    from omnisafe_amd.config import get_default_kwargs
    from omnisafe_amd.group import member_cfgs

    out = member_cfgs('PPOLag', variants=[{'seed': 3}, {'seed': 3, 'algo_cfgs': {'clip': 0.1}}, {'seed': 3}],
                      custom_cfgs={'logger_cfgs': {'log_dir': '/tmp/base'}})
    dirs = [c['logger_cfgs']['log_dir'] for c in out]
    assert len(set(dirs)) == 3 and all(d.startswith('/tmp/base/') for d in dirs)
    default = get_default_kwargs('PPOLag')['logger_cfgs']['log_dir']
    dirs = [c['logger_cfgs']['log_dir'] for c in member_cfgs('PPOLag', seeds=[1, 1])]
    assert len(set(dirs)) == 2 and all(d.startswith(default) for d in dirs)


def test_world_size_above_one_is_refused(monkeypatch):
    import omnisafe_amd

    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(NotImplementedError, match='world size 1'):
        omnisafe_amd.AgentGroup('PPOLag', 'SynthReach-v0', seeds=[0, 1])
