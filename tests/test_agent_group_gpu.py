"""AgentGroup and the grouped persistent pass (osa_ppo_pass_group) on the GPU.

Every comparison is exact (``torch.equal`` / string equality): the grouped launch runs the same kernel body on the
same operands as the solo launch, so there is no tolerance to choose -- a difference is a bug, not rounding."""
import copy
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'learning_reach.json')
STATE = ('params', 'adam_m', 'adam_v', 'adam_step', 'stats')


def _make_ac(obs_dim, act_dim):
    from omnisafe_amd.models import ConstraintActorCritic
    from omnisafe_amd.spaces import Box

    ns = types.SimpleNamespace
    net = dict(hidden_sizes=[64, 64], activation='tanh', lr=3e-4)
    cfgs = ns(actor=ns(**net), critic=ns(**net), weight_initialization_mode='kaiming_uniform',
              actor_type='gaussian_learning', linear_lr_decay=True)
    return ConstraintActorCritic(Box(-np.inf, np.inf, (obs_dim,)), Box(-1, 1, (act_dim,)), cfgs, 4, device=DEV)


class _Case:
    """One member: a randomly initialised network with non-trivial Adam state, a random batch, and the arguments of
    its pass.  ``clone()`` gives an independent copy of everything the pass writes."""

    def __init__(self, k, obs_dim, act_dim, M, B, mask, ext=False):
        from omnisafe_amd.models import HParams, SurrogateExt

        torch.manual_seed(1000 + k)
        self.obs_dim, self.act_dim, self.M, self.B, self.mask = obs_dim, act_dim, M, B, mask
        ac = _make_ac(obs_dim, act_dim)
        self.params = ac.params.clone()
        self.adam_m = 1e-3 * torch.randn_like(ac.params) * (ac.params != 0)
        self.adam_v = 1e-5 * torch.rand_like(ac.params) * (ac.params != 0)
        self.adam_step = torch.tensor([3 + k, 5, 7 + 2 * k], dtype=torch.int32, device=DEV)
        ld = (obs_dim + 3) // 4 * 4  # 16-byte aligned rows
        self.obs = torch.randn(M, ld, device=DEV)[:, :obs_dim]
        mean, _, _, lp = ac.step(self.obs, deterministic=True)
        self.act = mean + 0.3 * torch.randn(M, act_dim, device=DEV)
        _, _, _, self.logp = ac.step(self.obs, eps=torch.zeros(M, act_dim, device=DEV))
        self.logp = self.logp - 0.1 * torch.rand(M, device=DEV)
        self.tgt_r, self.tgt_c, self.adv_r, self.adv_c = (torch.randn(M, device=DEV) for _ in range(4))
        self.lagrange = torch.tensor([0.1 * k], device=DEV)
        self.nmb = (M + B - 1) // B
        self.hp = HParams(clip=0.2, entropy_coef=0.01 * (k % 2), critic_norm_coef=0.001, max_grad_norm=40.0,
                          lr_actor=3e-4 * (1 + k % 5), lr_critic=1e-3 / (1 + k % 3), beta1=0.9, beta2=0.999,
                          adam_eps=1e-8, use_critic_norm=1, use_max_grad_norm=1, use_cost=1)
        self.loss_kind = 1 if ext else k % 2
        self.ext = None
        if ext:  # FOCOPS (first_order/focops.py:83-92): eta 0.02, lam 1.5
            self.old_mean = mean.clone()
            self.old_log_std = torch.zeros(ac.layout.OUTP, device=DEV)
            self.old_log_std[:act_dim] = ac.actor.log_std.reshape(-1)[:act_dim]
            self.ext = SurrogateExt(kl_coef=1.0, kl_mask_eta=0.02, ratio_scale=1.0 / 1.5)
            self.ext.old_mean, self.ext.ld_old_mean = self.old_mean.data_ptr(), self.old_mean.stride(0)
            self.ext.old_log_std = self.old_log_std.data_ptr()
        self.new_round(0)

    def new_round(self, r):
        g = torch.Generator().manual_seed(77 * r + self.M)
        self.perm = torch.randperm(self.M, generator=g).to(DEV)
        self.stats = torch.zeros(self.nmb, 16, device=DEV)

    def clone(self):
        c = copy.copy(self)
        for name in STATE:
            setattr(c, name, getattr(self, name).clone())
        return c

    def tail(self):
        return (self.params.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(), self.adam_step.data_ptr(),
                self.obs.data_ptr(), self.obs.stride(0), self.act.data_ptr(), self.act.stride(0), self.logp.data_ptr(),
                self.tgt_r.data_ptr(), self.tgt_c.data_ptr(), self.adv_r.data_ptr(), self.adv_c.data_ptr(),
                self.perm.data_ptr(), self.M, self.B)

    def solo(self, lib):
        from omnisafe_amd import _lib

        _lib.check(lib.osa_ppo_pass_ext(
            self.obs_dim, self.act_dim, 64, *self.tail(), self.lagrange.data_ptr(), C.byref(self.hp), self.loss_kind,
            self.mask, self.stats.data_ptr(), C.byref(self.ext) if self.ext is not None else None,
            _lib.stream_ptr()), 'osa_ppo_pass_ext')

    def member(self):
        from omnisafe_amd.models import PassMember

        m = PassMember()
        (m.params, m.adam_m, m.adam_v, m.adam_step, m.obs, m.ld_obs, m.act, m.ld_act, m.logp, m.target_value_r,
         m.target_value_c, m.adv_r, m.adv_c, m.perm, m.M, m.B) = self.tail()
        m.lagrange, m.loss_kind, m.nets_mask, m.step_stats = (self.lagrange.data_ptr(), self.loss_kind, self.mask,
                                                              self.stats.data_ptr())
        C.memmove(C.byref(m.hp), C.byref(self.hp), C.sizeof(self.hp))
        m.has_ext = int(self.ext is not None)
        if self.ext is not None:
            C.memmove(C.byref(m.ext), C.byref(self.ext), C.sizeof(self.ext))
        return m


def _group_call(lib, cases, ws, arr=None):
    from omnisafe_amd import _lib
    from omnisafe_amd.models import PassMember

    n = len(cases)
    if arr is None:
        arr = (PassMember * n)()
    for k, c in enumerate(cases):
        arr[k] = c.member()
    return lib.osa_ppo_pass_group(cases[0].obs_dim, cases[0].act_dim, 64, C.cast(arr, C.c_void_p), n, ws.data_ptr(),
                                  ws.numel(), _lib.stream_ptr())


def _cases(n, obs_dim, act_dim, B, ext):
    # different M (ragged last minibatches among them), learning rates, Lagrange values, masks (0b110: critics only,
    # as the trust-region algorithms run the pass; one member with mask 0) and permutations; n = 96: small M
    masks = [7, 6, 7, 3, 0, 7, 5, 2]
    out = []
    for k in range(n):
        steps = (1 + k % 3) if n > 16 else (3 + k % 4)
        M = steps * B - (0 if k % 2 == 0 else 1 + 5 * k % (B - 1))
        out.append(_Case(k, obs_dim, act_dim, M, B, 7 if n == 1 else masks[k % 8], ext))
    return out


def _assert_equal(grouped, solo):
    for k, (a, b) in enumerate(zip(grouped, solo)):
        for name in STATE:
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)


@pytest.mark.parametrize('kind', ['B64', 'B128', 'ext'])
@pytest.mark.parametrize('n', [1, 3, 8, 11, 96])
@pytest.mark.parametrize('obs_dim,act_dim', [(60, 2), (27, 8)])
def test_grouped_pass_equals_solo_launches(obs_dim, act_dim, n, kind):
    """One osa_ppo_pass_group launch on clones vs n calls of osa_ppo_pass_ext: parameters, Adam moments, step
    counters and statistics rows bit for bit, for the single-chunk, the one-workgroup multi-chunk and the
    extended-surrogate (FOCOPS) class."""
    from omnisafe_amd import _lib

    lib = _lib.load(require_gpu=True)
    solo = _cases(n, obs_dim, act_dim, 128 if kind == 'B128' else 64, kind == 'ext')
    grouped = [c.clone() for c in solo]
    before = [c.clone() for c in solo]
    ws = torch.empty(lib.osa_ppo_pass_group_ws_bytes(n), dtype=torch.uint8, device=DEV)
    _lib.check(_group_call(lib, grouped, ws), 'osa_ppo_pass_group')
    for c in solo:
        c.solo(lib)
    torch.cuda.synchronize()
    _assert_equal(grouped, solo)
    changed = [not torch.equal(a.params, b.params) for a, b in zip(solo, before)]
    assert changed == [c.mask != 0 for c in solo]  # the comparison is of passes that did something


def test_mixed_class_array_is_refused_and_launches_nothing():
    from omnisafe_amd import _lib

    lib = _lib.load(require_gpu=True)
    for pair in ([_Case(0, 60, 2, 200, 64, 7), _Case(1, 60, 2, 300, 128, 7)],
                 [_Case(0, 60, 2, 200, 64, 7), _Case(1, 60, 2, 200, 64, 7, ext=True)]):
        before = [c.clone() for c in pair]
        ws = torch.empty(lib.osa_ppo_pass_group_ws_bytes(2), dtype=torch.uint8, device=DEV)
        assert _group_call(lib, pair, ws) == -1  # OSA_EINVAL
        torch.cuda.synchronize()
        _assert_equal(pair, before)
    one = [_Case(0, 60, 2, 200, 64, 7)]
    small = torch.empty(8, dtype=torch.uint8, device=DEV)
    assert _group_call(lib, one, small) == -1  # workspace too small


def test_back_to_back_grouped_launches_without_host_sync():
    """Five grouped launches enqueued with no host synchronisation between them -- fresh permutations and statistics
    rows each, the SAME workspace and the SAME host array of members overwritten for every launch -- equal five
    rounds of solo launches: neither the staged device blocks nor their host source may be reused too early."""
    from omnisafe_amd import _lib
    from omnisafe_amd.models import PassMember

    lib = _lib.load(require_gpu=True)
    n, rounds = 11, 5
    solo = _cases(n, 60, 2, 64, False)
    grouped = [c.clone() for c in solo]
    perms = []
    for r in range(rounds):  # everything a round needs exists before the first launch
        for c in solo:
            c.new_round(r)
        perms.append([(c.perm, c.stats, c.stats.clone()) for c in solo])
    ws = torch.empty(lib.osa_ppo_pass_group_ws_bytes(n), dtype=torch.uint8, device=DEV)
    arr = (PassMember * n)()
    torch.cuda.synchronize()
    for r in range(rounds):
        for c, (p, _, st) in zip(grouped, perms[r]):
            c.perm, c.stats = p, st
        _lib.check(_group_call(lib, grouped, ws, arr), 'osa_ppo_pass_group')
    group_stats = [[st for _, _, st in perms[r]] for r in range(rounds)]
    for r in range(rounds):
        for c, (p, st, _) in zip(solo, perms[r]):
            c.perm, c.stats = p, st
            c.solo(lib)
    torch.cuda.synchronize()
    _assert_equal(grouped, solo)  # (incl. the last round's statistics)
    for r in range(rounds):
        for k in range(n):
            assert torch.equal(group_stats[r][k], perms[r][k][1]), (r, k)


# ---------------------------------------------------------------------------------------------- whole trainings
def _reach_cfgs(algo, cfg, log_dir, extra=None):
    """tests/test_learning_gpu.py:reach_custom_cfgs without the seed (the SynthReach configuration of
    test_same_seed_same_parameters_bit_for_bit)."""
    from omnisafe_amd.config import get_default_kwargs
    from omnisafe_amd.group import _merged

    defaults = get_default_kwargs(algo)
    custom = {
        'train_cfgs': {'device': DEV, 'total_steps': cfg['steps_per_epoch'] * cfg['epochs'],
                       'vector_env_nums': cfg['vector_env_nums']},
        'algo_cfgs': {'steps_per_epoch': cfg['steps_per_epoch']},
        'logger_cfgs': {'log_dir': log_dir, 'save_model_freq': 1000},
    }
    if 'cost_limit' in defaults.get('lagrange_cfgs', {}):
        custom['lagrange_cfgs'] = {'cost_limit': cfg['cost_limit']}
    if 'cost_limit' in defaults['algo_cfgs']:
        custom['algo_cfgs']['cost_limit'] = cfg['cost_limit']
    if 'safety_budget' in defaults['algo_cfgs']:
        custom['algo_cfgs'].update({'safety_budget': cfg['cost_limit'], 'max_ep_len': cfg['horizon']})
        if 'upper_budget' in defaults['algo_cfgs']:
            custom['algo_cfgs']['upper_budget'] = 2 * cfg['cost_limit']
    return _merged(custom, extra or {})


def _outcome(agent):
    """What a training leaves behind: network and Adam state, and progress.csv without the wall-clock columns."""
    ac = agent.agent._actor_critic  # noqa: SLF001
    torch.cuda.synchronize()
    lines = [ln for ln in open(os.path.join(agent.agent.logger.log_dir, 'progress.csv')).read().split('\n') if ln]
    hdr = lines[0].split(',')
    keep = [i for i, h in enumerate(hdr) if not h.startswith('Time/')]
    rows = [[ln.split(',')[i] for i in keep] for ln in lines]
    return {'params': ac.params.clone(), 'adam_m': ac.adam_m.clone(), 'adam_v': ac.adam_v.clone(), 'rows': rows,
            'last_path': agent.agent._updater.last_path, 'last_group': agent.agent._updater.last_group}  # noqa: SLF001


def _assert_same_run(member, solo, tag):
    for name in ('params', 'adam_m', 'adam_v'):
        assert torch.equal(member[name], solo[name]), (tag, name, float((member[name] - solo[name]).abs().max()))
    assert member['rows'] == solo['rows'], tag
    assert len(solo['rows']) > 1
    assert member['last_path'] == solo['last_path'], tag


def _column(out, name):
    return [r[out['rows'][0].index(name)] for r in out['rows'][1:]]


def _passes(out):
    """Persistent passes of the whole training: one per update iteration (Train/StopIter of every epoch)."""
    return sum(int(float(v)) for v in _column(out, 'Train/StopIter'))


def _assert_last_groups(members, grouped, tag):
    """``last_group`` of the members on the plain persistent pass, EXACTLY.  The group launches once per round, with
    the pass of every member that still has one, so member k's j-th pass travels with the passes of all members
    that have at least j -- its last one with #{i : passes_i >= passes_k} members.  That is >= 2 for every member
    but a single longest-running one: once the KL early stop has ended the others' last updates, its remaining
    passes have nobody to share a launch with and go through the grouped entry alone (1 -- never 0, the value of a
    solo launch).  Members off the plain pass launch on their own: 0."""
    total = {k: _passes(members[k]) for k in grouped}
    for k, m in enumerate(members):
        if k not in total:
            assert m['last_group'] == 0, (tag, k, m['last_path'], m['last_group'])
            continue
        want = sum(1 for t in total.values() if t >= total[k])
        assert m['last_group'] == want, (tag, k, m['last_group'], want, total)
        longest_alone = want == 1 and len(total) > 1
        assert m['last_group'] >= 2 or longest_alone, (tag, k, m['last_group'], total)
    if len(total) > 1:  # at most one member ends alone, all others shared their last launch
        assert sum(1 for k in total if members[k]['last_group'] >= 2) >= len(total) - 1, (tag, total)


# PPOLag: lowered from the YAML's 0.02 if needed so that the members' passes stop at DIFFERENT iterations (solo and
# group get the same value)
PPOLAG_TARGET_KL = 0.02


@pytest.mark.parametrize('algo,batch', [('PPOLag', None), ('CPO', None), ('TRPOLag', None), ('FOCOPS', None),
                                        ('PPOSaute', None), ('CPO', 64), ('TRPOLag', 64)])
def test_group_members_equal_solo_runs_bit_for_bit(algo, batch, tmp_path):
    """An AgentGroup of three seeds vs three solo Agents, 3 epochs of the SynthReach configuration: parameters, Adam
    moments and every non-Time/ column of progress.csv identical per member; where the solo run took the plain
    persistent pass the members' passes really travelled in shared launches (_assert_last_groups), where it took the
    cooperative chunked pass (trust-region critics at the YAML batch of 128) the member took it too, on its own.

    Measured on the MI355X (PPOLag, seeds 7 / 8 / 9, Train/StopIter per epoch 1,3,40 / 1,3,17 / 2,3,40): last_group
    2 / 3 / 1 -- seed 9 has 45 passes against 44 and 21, so its 45th is the only pass left in the group."""
    import omnisafe_amd

    cfg = dict(json.load(open(GOLDEN))['config'], epochs=3)
    extra = {'algo_cfgs': {'batch_size': batch}} if batch else {}
    if algo == 'PPOLag':
        extra = {'algo_cfgs': {'target_kl': PPOLAG_TARGET_KL}}
    seeds = [7, 8, 9]
    solos = []
    for s in seeds:
        a = omnisafe_amd.Agent(algo, cfg['env_id'], custom_cfgs=dict(_reach_cfgs(algo, cfg, str(tmp_path / f'solo{s}'),
                                                                                 extra), seed=s))
        a.learn()
        solos.append(_outcome(a))
        assert solos[-1]['last_group'] == 0
    group = omnisafe_amd.AgentGroup(algo, cfg['env_id'], seeds=seeds,
                                    custom_cfgs=_reach_cfgs(algo, cfg, str(tmp_path / 'group'), extra))
    results = group.learn()
    assert len(results) == 3 and group.env_steps_per_second > 0
    members = [_outcome(a) for a in group.agents]
    for s, m, o in zip(seeds, members, solos):
        _assert_same_run(m, o, (algo, s))
        print(algo, batch, s, 'last_path', o['last_path'], 'last_group', m['last_group'], 'passes', _passes(m))
    grouped = [k for k, o in enumerate(solos) if o['last_path'] == 'persistent']
    _assert_last_groups(members, grouped, algo)
    if batch is None and algo in ('PPOLag', 'FOCOPS', 'PPOSaute'):
        assert all(o['last_path'] == 'persistent' for o in solos)
    if batch == 64:  # the trust-region family grouped (critic passes, no early stop: nobody ends alone)
        assert grouped == [0, 1, 2] and all(m['last_group'] >= 2 for m in members)
    if algo == 'PPOLag':  # members really leave an update early while others continue
        stop = [_column(m, 'Train/StopIter') for m in members]
        assert any(len({st[e] for st in stop}) > 1 for e in range(len(stop[0]))), stop


def test_mixed_group_of_six(tmp_path):
    """Variants that differ in hyper-parameters, one on the chunked pass (batch 128), one on the general-network path,
    two with the SAME seed: each equals its solo run, six distinct log directories, last_group 0 exactly on the two
    ungrouped members."""
    import omnisafe_amd
    from omnisafe_amd.group import _merged

    cfg = dict(json.load(open(GOLDEN))['config'], epochs=2)
    wide = {'hidden_sizes': [256, 128]}
    variants = [
        {'seed': 0, 'lagrange_cfgs': {'lagrangian_multiplier_init': 0.5}, 'model_cfgs': {'actor': {'lr': 1e-4}}},
        {'seed': 1, 'lagrange_cfgs': {'lagrangian_multiplier_init': 0.01}, 'model_cfgs': {'actor': {'lr': 5e-4}}},
        {'seed': 2, 'algo_cfgs': {'batch_size': 128}},
        {'seed': 3, 'model_cfgs': {'actor': dict(wide), 'critic': dict(wide)}},
        {'seed': 4, 'algo_cfgs': {'clip': 0.1}},
        {'seed': 4, 'algo_cfgs': {'entropy_coef': 0.01}},
    ]
    group = omnisafe_amd.AgentGroup('PPOLag', cfg['env_id'], variants=variants,
                                    custom_cfgs=_reach_cfgs('PPOLag', cfg, str(tmp_path / 'group')))
    group.learn()
    members = [_outcome(a) for a in group.agents]
    dirs = [a.agent.logger.log_dir for a in group.agents]
    assert len(set(dirs)) == 6 and all(os.path.isfile(os.path.join(d, 'progress.csv')) for d in dirs)
    for k, var in enumerate(variants):
        a = omnisafe_amd.Agent('PPOLag', cfg['env_id'],
                               custom_cfgs=_merged(_reach_cfgs('PPOLag', cfg, str(tmp_path / f'solo{k}')), var))
        a.learn()
        _assert_same_run(members[k], _outcome(a), k)
    print('mixed group', [(m['last_path'], m['last_group']) for m in members])
    assert members[2]['last_path'] == 'persistent-chunked' and members[3]['last_path'].startswith('general-')
    assert [m['last_group'] == 0 for m in members] == [False, False, True, True, False, False]
    _assert_last_groups(members, [0, 1, 4, 5], 'mixed')


def test_group_of_one_goes_through_the_grouped_entry(tmp_path):
    import omnisafe_amd

    cfg = dict(json.load(open(GOLDEN))['config'], epochs=1)
    group = omnisafe_amd.AgentGroup('PPOLag', cfg['env_id'], seeds=[5],
                                    custom_cfgs=_reach_cfgs('PPOLag', cfg, str(tmp_path / 'group')))
    group.learn()
    a = omnisafe_amd.Agent('PPOLag', cfg['env_id'],
                           custom_cfgs=dict(_reach_cfgs('PPOLag', cfg, str(tmp_path / 'solo')), seed=5))
    a.learn()
    member, solo = _outcome(group.agents[0]), _outcome(a)
    _assert_same_run(member, solo, 'one')
    assert member['last_group'] == 1 and solo['last_group'] == 0


def test_group_evaluate_equals_members_evaluate(tmp_path):
    import omnisafe_amd

    cfg = dict(json.load(open(GOLDEN))['config'], epochs=1)
    group = omnisafe_amd.AgentGroup('PPOLag', cfg['env_id'], seeds=[0, 1],
                                    custom_cfgs=_reach_cfgs('PPOLag', cfg, str(tmp_path)))
    group.learn()
    got = group.evaluate(num_episodes=3, cost_criteria=1.0)
    want = [a.evaluate(num_episodes=3, cost_criteria=1.0) for a in group.agents]
    assert len(got) == 2 and all(len(g) >= 1 for g in got)

    def text(x):
        return json.dumps(x, default=lambda t: np.asarray(t).tolist())

    assert text(got) == text(want)
    assert text(got[0]) != text(got[1])  # (two different agents)
