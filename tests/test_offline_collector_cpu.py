"""CPU: omnisafe_amd.OfflineDataCollector up to the GPU's edge -- the reference's errors, the lane layout, the new
entry points' argument checks (no launch), the custom library's export, and the file the writer makes read back by the
unmodified reference's OfflineDataset.  The kernel itself runs in test_offline_collector_gpu.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = 'SynthNavCircle1-v0'


def write_config(root, algo='PPOLag'):
    from omnisafe_amd.config import get_default_kwargs

    d = get_default_kwargs(algo)
    d.update({'algo': algo, 'env_id': ENV, 'exp_name': f'{algo}-{{{ENV}}}', 'seed': 0, 'env_cfgs': {}})
    os.makedirs(os.path.join(root, 'torch_save'), exist_ok=True)
    with open(os.path.join(root, 'config.json'), 'w', encoding='utf-8') as f:
        json.dump(d, f)


def test_constructor_knows_the_device_envs_without_a_gpu():
    import omnisafe_amd

    col = omnisafe_amd.OfflineDataCollector(100, ENV)
    assert (col._obs_dim, col._act_dim) == (28, 2) and col.agents == [] and col.path is None
    assert omnisafe_amd.OfflineDataCollector(10, 'SynthNavCarGoal1-v0', seed=3, num_envs=4)._obs_dim == 72


def test_register_agent_raises_the_references_errors(tmp_path):
    import omnisafe_amd

    col = omnisafe_amd.OfflineDataCollector(100, ENV)
    with pytest.raises(FileNotFoundError, match='The config file is not found in the save directory.'):
        col.register_agent(str(tmp_path / 'nothing'), 'epoch-0.pt', 100)
    root = str(tmp_path / 'run')
    write_config(root)
    with pytest.raises(FileNotFoundError, match=f'Model epoch-7.pt not found in {root}'):
        col.register_agent(root, 'epoch-7.pt', 100)
    saute = str(tmp_path / 'saute')
    write_config(saute, 'PPOSaute')
    torch.save({'pi': {}}, os.path.join(saute, 'torch_save', 'epoch-0.pt'))
    with pytest.raises(NotImplementedError, match='Saute'):
        col.register_agent(saute, 'epoch-0.pt', 100)
    assert col.agents == []


def test_collect_asserts_the_sizes(tmp_path):
    import omnisafe_amd
    from omnisafe_amd.offline import OfflineAgent

    col = omnisafe_amd.OfflineDataCollector(100, ENV)
    col.agents.append(OfflineAgent(None, 101))
    with pytest.raises(AssertionError, match='size is larger than collector size'):
        col.collect(str(tmp_path))
    col.agents[:] = [OfflineAgent(None, 60), OfflineAgent(None, 30)]
    with pytest.raises(AssertionError, match='Sum of agent size is not equal to collector size'):
        col.collect(str(tmp_path))
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize('S,K', [(20, 1), (20, 3), (50, 17), (131, 130), (5, 9)])
def test_lane_layout(S, K):
    from omnisafe_amd.offline import lane_layout

    Q, ranges = lane_layout(S, K)
    assert Q == -(-S // K) and len(ranges) == K
    # the ranges tile [0, S) in lane order, every lane but the last non-empty one is full, the rest is empty
    at = 0
    for k, (a, b) in enumerate(ranges):
        assert a == min(k * Q, S) == at and b == min((k + 1) * Q, S) and 0 <= b - a <= Q
        at = b
    assert at == S
    sizes = [b - a for a, b in ranges]
    full = S // Q
    assert sizes[:full] == [Q] * full and sum(sizes[full + 1:]) == 0
    expect = {(20, 1): [(0, 20)], (20, 3): [(0, 7), (7, 14), (14, 20)]}
    if (S, K) in expect:
        assert ranges == expect[(S, K)]
    if (S, K) == (50, 17):
        assert Q == 3 and ranges[16] == (48, 50)
    if (S, K) == (131, 130):  # 65 full lanes, one short lane, 64 empty ones
        assert Q == 2 and ranges[64] == (128, 130) and ranges[65] == (130, 131) and ranges[66] == (131, 131)
    if (S, K) == (5, 9):  # K > S: one row per lane, then nothing
        assert Q == 1 and sizes == [1] * 5 + [0] * 4


def test_default_lanes_play_about_an_episode_each():
    from omnisafe_amd.offline import agent_seeds, default_num_envs

    assert default_num_envs(100, 500) == 1
    assert default_num_envs(5000, 500) == 10
    assert default_num_envs(10 ** 7, 500) == 4096
    assert default_num_envs(999, 500) == 1 and default_num_envs(1000, 500) == 2
    seeds = [agent_seeds(5, i) for i in range(3)]
    assert len({s for pair in seeds for s in pair}) == 6 and seeds[0][0] == 5 and seeds == [agent_seeds(5, i)
                                                                                            for i in range(3)]


def collect_args(**over):
    """The arguments of osa_collect_episodes behind env_kind, with host addresses that no launch ever reads."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    a = dict(K=4, Q=5, S=18, obs_dim=28, act_dim=2, hidden=64, params=p, mean=None, std=None, count=None, clip=5.0,
             lo=p, hi=p, min_a=-1.0, max_a=1.0, seed=1, noise=2, horizon=7, cost_p=0.0, obs=p, ld_obs=28, action=p,
             ld_act=2, reward=p, cost=p, next_obs=p, ld_next=28, done=p, ret=p, csum=p, count_out=p, stream=None)
    a.update(over)
    return tuple(a.values())


BAD_ARGUMENTS = [dict(K=0), dict(Q=0), dict(S=0), dict(S=21), dict(obs_dim=0), dict(act_dim=0), dict(horizon=0),
                 dict(params=None), dict(lo=None), dict(max_a=-1.0), dict(mean=1), dict(obs=None), dict(action=None),
                 dict(reward=None), dict(cost=None), dict(next_obs=None), dict(done=None), dict(ret=None),
                 dict(csum=None), dict(count_out=None), dict(ld_obs=27), dict(ld_next=27), dict(ld_act=1),
                 dict(obs_dim=27, ld_obs=27, ld_next=27)]  # (the last: narrower than the env's own row)


def test_library_exports_the_entry_point_and_checks_before_a_launch():
    from omnisafe_amd import _lib

    lib = _lib.load()
    assert 'osa_collect_episodes' in _lib.SIGNATURES and hasattr(lib, 'osa_collect_episodes')
    # obs_dim .. max_action: the slice saved_policy.policy_args packs for both players
    assert _lib.SIGNATURES['osa_eval_episodes'][1][2:14] == _lib.SIGNATURES['osa_collect_episodes'][1][4:16]
    circle1 = 32 + 1
    for bad in BAD_ARGUMENTS:
        assert lib.osa_collect_episodes(circle1, *collect_args(**bad)) == -1, bad
    # what osa_eval_episodes refuses: an unknown env kind, a width outside the fused family, too wide a row
    assert lib.osa_collect_episodes(7, *collect_args()) == _lib.OSA_EUNSUPPORTED
    assert lib.osa_collect_episodes(circle1, *collect_args(hidden=48)) == _lib.OSA_EUNSUPPORTED
    assert lib.osa_collect_episodes(0, *collect_args(obs_dim=376, ld_obs=376, ld_next=376)) == _lib.OSA_EUNSUPPORTED


def test_custom_library_exports_the_collect_entry_point():
    from omnisafe_amd import _lib, build, envs

    path = build.build_custom_env(os.path.join(HERE, 'custom_envs', 'glider.h'), 'Glider')
    lib, info, _ = envs._bind_custom(path)
    assert hasattr(lib, 'osa_custom_collect_episodes') and info[:5] == [12, 70, 10, 3, 10]
    args = collect_args(obs_dim=70, ld_obs=70, ld_next=70, act_dim=3, ld_act=3)
    for bad in (dict(K=0), dict(done=None), dict(ld_act=2), dict(S=21)):
        over = dict(obs_dim=70, ld_obs=70, ld_next=70, act_dim=3, ld_act=3)
        over.update(bad)
        assert lib.osa_custom_collect_episodes(0, *collect_args(**over)) == -1, bad
    assert lib.osa_custom_collect_episodes(2, *args) == -1  # (Glider has levels 0 and 1)
    assert lib.osa_custom_collect_episodes(0, *collect_args(obs_dim=69, ld_obs=70, ld_next=70, act_dim=3,
                                                            ld_act=3)) == -1
    assert envs.DeviceVectorEnv.collect_entry_point == 'osa_collect_episodes'
    assert envs.CustomDeviceEnv.collect_entry_point == 'osa_custom_collect_episodes'
    assert _lib.SIGNATURES['osa_collect_episodes'][1] == lib.osa_custom_collect_episodes.argtypes


def synthetic_arrays(S=37, D=28, A=2, seed=0):
    rng = np.random.default_rng(seed)
    return {'obs': rng.standard_normal((S, D)).astype(np.float32),
            'action': rng.standard_normal((S, A)).astype(np.float32),
            'reward': rng.standard_normal((S, 1)).astype(np.float32),
            'cost': (rng.random((S, 1)) < 0.2).astype(np.float32),
            'next_obs': rng.standard_normal((S, D)).astype(np.float32),
            'done': (rng.random((S, 1)) < 0.1).astype(np.float32)}


def test_writer_makes_the_references_file(tmp_path, capsys):
    from omnisafe_amd.offline import FIELDS, write_dataset

    arrays = synthetic_arrays()
    path = write_dataset(str(tmp_path / 'data'), ENV, arrays)
    assert path == os.path.join(str(tmp_path / 'data'), f'{ENV}_data.npz')
    assert 'Warning' not in capsys.readouterr().out
    with np.load(path) as back:
        assert sorted(back.files) == sorted(FIELDS)
        for k in FIELDS:
            assert back[k].dtype == np.float32 and np.array_equal(back[k], arrays[k])
        assert back['reward'].shape == back['cost'].shape == back['done'].shape == (37, 1)
    write_dataset(str(tmp_path / 'data'), ENV, arrays)
    out = capsys.readouterr().out
    assert f'Warning: {path} already exists.' in out and f'Warning: {path} will be overwritten.' in out


@pytest.mark.reference
def test_reference_dataset_reads_the_file(tmp_path):
    """The unmodified reference's OfflineDataset (common/offline/dataset.py) loads the writer's file."""
    import ref_harness

    ref_harness.import_reference()
    from omnisafe.common.offline.dataset import OfflineDataset

    from omnisafe_amd.offline import FIELDS, write_dataset

    arrays = synthetic_arrays(S=53, D=60, A=2, seed=1)
    path = write_dataset(str(tmp_path), 'SynthNavGoal1-v0', arrays)
    ds = OfflineDataset(path, batch_size=8, device=torch.device('cpu'))
    assert len(ds) == 53
    for k in FIELDS:
        got = getattr(ds, k)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), arrays[k])
    row = ds[5]
    for got, k in zip(row, FIELDS):
        assert np.array_equal(got.numpy(), arrays[k][5])
