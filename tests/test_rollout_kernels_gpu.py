"""The rollout-side kernels of omnisafe_amd/csrc/rollout_kernels.hip, called directly and compared with their numpy twin
(tests/rollout_twin.py, pinned to the reference's recorded data by tests/test_rollout_twin.py): osa_rollout_post_step,
osa_saute_step, osa_action_scale, osa_normalizer_apply bit for bit; osa_normalizer_push against the float64 moments of
all rows pushed so far.

Every output is a view into a larger tensor filled with a sentinel -- guard elements before and behind it, padding
columns where the row stride is wider than the row -- and every test ends by checking that the sentinels are intact.

The normaliser's statistics.  The kernel keeps float32 state as the reference does, so its distance from the float64
truth is held against the REFERENCE's own: with e = max over columns of |mean - truth| / (|truth mean| + truth std), and
of |var - truth| / truth var, the kernel's e_k must satisfy e_k <= 4 max(e_ref, 2**-23), e_ref being np_oracle.Normalizer
(the float32 restatement pinned to the reference) fed the same selected rows.  A numpy statement of the kernel's
arithmetic (tests/test_rollout_twin.py: KernelStatement) has a worst e_k / max(e_ref, 2**-23) of 1.10 on mixed batch
sizes, 500 single rows, 16 x 4096 rows, offsets 1e3 and 1e4 and column scales 1e-3 ... 1e3, and of 1.67 on the very
sequences of this module; 4 is twice that and more, room for the order of the float64 partial sums and the last-bit luck
of two float32 roundings.  One row of 4097 dropped or counted twice moves the statistics by 3e-5 or more (D = 1; 1e-4 and
more at the wider shapes), two orders above the bound; a whole row block does more.
Worst e_k / max(e_ref, 2**-23) measured on the MI355X over the 198 state checks of this module: 1.10.
"""
import itertools

import numpy as np
import pytest
import torch

import np_oracle as O
import rollout_twin as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = np.float32
SENT = 777.25  # (exact in float32 / float64; 0xA5 for bytes, -77 for int64)


class Guarded:
    """A (rows, cols) tensor with row stride ld >= cols inside a sentinel-filled allocation with `guard` elements on
    either side."""

    def __init__(self, rows, cols, ld=None, dtype=torch.float32, guard=64):
        ld = cols if ld is None else ld
        self.sent = {torch.uint8: 0xA5, torch.int64: -77}.get(dtype, SENT)
        self.full = torch.full((guard + rows * ld + guard,), self.sent, dtype=dtype, device=DEV)
        self.t = self.full[guard:guard + rows * ld].view(rows, ld)[:, :cols]
        self.payload = torch.zeros_like(self.full, dtype=torch.bool)
        self.payload[guard:guard + rows * ld].view(rows, ld)[:, :cols] = True
        self.ld = ld

    def set(self, a):
        self.t.copy_(torch.as_tensor(np.asarray(a)).reshape(self.t.shape))
        return self

    @property
    def ptr(self):
        return self.t.data_ptr()

    def np(self):
        return self.t.cpu().numpy()

    def vec(self):
        return self.np().reshape(-1)

    def intact(self):
        return bool((self.full[~self.payload] == self.sent).all())


def vec(n, dtype=torch.float32, init=None):
    g = Guarded(1, n, dtype=dtype)
    return g if init is None else g.set(init)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope='module')
def lib():
    from omnisafe_amd import _lib

    return _lib.load(require_gpu=True)


def _check(code, what):
    from omnisafe_amd import _lib

    _lib.check(code, what)


def _stream():
    from omnisafe_amd import _lib

    return _lib.stream_ptr()


# ---- osa_rollout_post_step ---------------------------------------------------------------------------------------
POST_OUT = ('ep_ret', 'ep_cost', 'ep_len', 'path_end', 'boot_r', 'boot_c', 'ep_done', 'ep_ret_out', 'ep_cost_out',
            'ep_len_out')


def post_step_inputs(N, seed, p=None):
    """Rewards, costs, flags (env n: combination n mod 4 of (terminated, truncated), or random with probability p
    each), bootstrap values and accumulators of one step."""
    rng = np.random.default_rng(seed)
    d = {k: rng.standard_normal(N).astype(np.float32) for k in ('reward', 'vnext_r', 'vnext_c', 'vfinal_r', 'vfinal_c')}
    d['cost'] = (rng.random(N) < 0.3).astype(np.float32)
    if p is None:
        d['terminated'] = (np.arange(N) & 1).astype(np.uint8)
        d['truncated'] = ((np.arange(N) >> 1) & 1).astype(np.uint8)
    else:
        d['terminated'] = (rng.random(N) < p).astype(np.uint8)
        d['truncated'] = (rng.random(N) < p).astype(np.uint8)
    return d


def launch_post_step(lib, N, epoch_end, d, st, vnext, vfinal, rows):
    """One launch on the guarded state / output tensors `st`; returns the twin's expectation for it."""
    before = {k: st[k].vec().copy() for k in ('ep_ret', 'ep_cost', 'ep_len')}
    t = {k: dev(v) for k, v in d.items()}
    _check(lib.osa_rollout_post_step(
        N, int(epoch_end), ptr(t['reward']), ptr(t['cost']), ptr(t['terminated']), ptr(t['truncated']),
        ptr(t['vnext_r']) if vnext else None, ptr(t['vnext_c']) if vnext else None,
        ptr(t['vfinal_r']) if vfinal else None, ptr(t['vfinal_c']) if vfinal else None,
        st['ep_ret'].ptr, st['ep_cost'].ptr, st['ep_len'].ptr, st['path_end'].ptr, st['boot_r'].ptr, st['boot_c'].ptr,
        st['ep_done'].ptr, st['ep_ret_out'].ptr, st['ep_cost_out'].ptr, st['ep_len_out'].ptr,
        st['reward_row'].ptr if rows else None, st['cost_row'].ptr if rows else None, _stream()), 'osa_rollout_post_step')
    return R.post_step(epoch_end, d['reward'], d['cost'], d['terminated'], d['truncated'], before['ep_ret'],
                       before['ep_cost'], before['ep_len'], *((d['vnext_r'], d['vnext_c']) if vnext else (None, None)),
                       *((d['vfinal_r'], d['vfinal_c']) if vfinal else (None, None)), fill=SENT)


def post_step_state(N, rng):
    st = {k: vec(N) for k in ('ep_ret', 'ep_cost', 'ep_len', 'boot_r', 'boot_c', 'ep_ret_out', 'ep_cost_out',
                              'ep_len_out', 'reward_row', 'cost_row')}
    st.update({k: vec(N, torch.uint8) for k in ('path_end', 'ep_done')})
    st['ep_ret'].set(rng.standard_normal(N).astype(np.float32))
    st['ep_cost'].set(rng.integers(0, 9, N).astype(np.float32))
    st['ep_len'].set(rng.integers(0, 30, N).astype(np.float32))
    return st


def _fresh_outputs(st):
    for k in ('ep_ret_out', 'ep_cost_out', 'ep_len_out', 'reward_row', 'cost_row', 'boot_r', 'boot_c'):
        st[k].t.fill_(SENT)
    for k in ('path_end', 'ep_done'):
        st[k].t.fill_(0xA5)


@pytest.mark.parametrize('epoch_end,vnext,vfinal,rows', list(itertools.product((0, 1), (True, False), (True, False),
                                                                               (True, False))))
def test_post_step_branch_table(lib, epoch_end, vnext, vfinal, rows):
    """N = 300 (two workgroups, 44 live lanes in the second), env n with flag combination n mod 4."""
    N = 300
    d = post_step_inputs(N, seed=1)
    st = post_step_state(N, np.random.default_rng(2))
    _fresh_outputs(st)
    want = launch_post_step(lib, N, epoch_end, d, st, vnext, vfinal, rows)
    for k in POST_OUT:
        assert np.array_equal(st[k].vec(), want[k]), k
    done = want['ep_done'] != 0
    assert np.array_equal(done, (d['terminated'] | d['truncated']) != 0) and 0 < done.sum() < N
    assert (st['ep_ret_out'].vec()[~done] == F(SENT)).all() and (st['ep_len_out'].vec()[~done] == F(SENT)).all()
    # the table's corners, spelled out: envs 2 (truncated) and 1, 3 (terminated)
    got_r = st['boot_r'].vec()
    assert got_r[2] == (d['vfinal_r'][2] if vfinal else (d['vnext_r'][2] if epoch_end and vnext else 0))
    assert got_r[1] == 0 and got_r[3] == 0 and got_r[0] == (d['vnext_r'][0] if epoch_end and vnext else 0)
    for k, src in (('reward_row', 'reward'), ('cost_row', 'cost')):
        assert np.array_equal(st[k].vec(), d[src] if rows else np.full(N, SENT, np.float32)), k
    assert all(g.intact() for g in st.values())


def test_post_step_carried_state(lib):
    """48 consecutive steps on the same accumulators, random flags, the epoch's end on the last one."""
    N, T = 257, 48
    st = post_step_state(N, np.random.default_rng(4))
    for k in ('ep_ret', 'ep_cost', 'ep_len'):
        st[k].t.zero_()
    finished = 0
    for t in range(T):
        d = post_step_inputs(N, seed=100 + t, p=0.1)
        _fresh_outputs(st)
        last = t == T - 1
        want = launch_post_step(lib, N, last, d, st, vnext=last, vfinal=True, rows=True)
        for k in POST_OUT:
            assert np.array_equal(st[k].vec(), want[k]), (t, k)
        finished += int(want['ep_done'].sum())
    assert finished > 2 * N and st['ep_len'].vec().max() > 20  # episodes ended and long ones are still running
    assert all(g.intact() for g in st.values())


# ---- osa_saute_step ----------------------------------------------------------------------------------------------
SAUTE_COL = 5


def saute_inputs(N, t, seed=9):
    rng = np.random.default_rng(seed + t)
    return dict(cost=(rng.random(N) < 0.3).astype(np.float32), reward=rng.standard_normal(N).astype(np.float32),
                terminated=(rng.random(N) < 0.05).astype(np.uint8), truncated=(rng.random(N) < 0.05).astype(np.uint8))


def saute_params(N, seed=8):
    rng = np.random.default_rng(seed)
    return dict(budget=rng.uniform(0.8, 6.0, N).astype(np.float32), reset_value=rng.uniform(0.5, 1.0, N).astype(np.float32))


def _saute_run(lib, N, steps, saute_gamma, unsafe_reward, prm, inputs, final):
    col, ld = SAUTE_COL, SAUTE_COL + 4
    st = dict(safety_obs=vec(N, init=prm['reset_value']), ep_budget=vec(N, init=np.zeros(N, np.float32)),
              reward_out=vec(N), ep_budget_out=vec(N), next_rows=Guarded(N, col + 1, ld=ld),
              final_rows=Guarded(N, col + 1, ld=ld))
    budget, reset = dev(prm['budget']), dev(prm['reset_value'])
    seen = dict(unsafe=0, done=0)
    for t in range(steps):
        d = inputs(t)
        z0, eb0 = st['safety_obs'].vec().copy(), st['ep_budget'].vec().copy()
        for k in ('reward_out', 'ep_budget_out'):
            st[k].t.fill_(SENT)
        st['next_rows'].t.fill_(0.5)
        st['final_rows'].t.fill_(0.25)
        td = {k: dev(v) for k, v in d.items()}
        _check(lib.osa_saute_step(
            N, ptr(td['cost']), ptr(td['reward']), ptr(td['terminated']), ptr(td['truncated']), st['safety_obs'].ptr,
            ptr(budget), saute_gamma, unsafe_reward, ptr(reset), st['reward_out'].ptr, st['next_rows'].ptr, ld,
            st['final_rows'].ptr if final else None, ld if final else 0, col, st['ep_budget'].ptr,
            st['ep_budget_out'].ptr, _stream()), 'osa_saute_step')
        want = R.saute_step(z0, d['cost'], d['reward'], d['terminated'], d['truncated'], prm['budget'], saute_gamma,
                            unsafe_reward, prm['reset_value'], eb0, fill=SENT)
        for k in ('safety_obs', 'reward_out', 'ep_budget', 'ep_budget_out'):
            assert np.array_equal(st[k].vec(), want[k]), (t, k)
        rows = np.full((N, col + 1), 0.5, np.float32)
        rows[:, col] = want['safety_obs']
        assert np.array_equal(st['next_rows'].np(), rows), t
        rows[:, :col] = 0.25
        if not final:
            rows[:, col] = 0.25
        assert np.array_equal(st['final_rows'].np(), rows), t
        assert (st['ep_budget_out'].vec()[want['done'] == 0] == F(SENT)).all()
        seen['unsafe'] += int((want['reward_out'] == F(unsafe_reward)).sum())
        seen['done'] += int(want['done'].sum())
    assert all(g.intact() for g in st.values())
    return st, seen


@pytest.mark.parametrize('final', [True, False], ids=['final-rows', 'no-final-rows'])
def test_saute_step_carried_state(lib, final):
    """48 steps, N = 300, per-env budgets and reset values, unit costs, terminations and truncations; the safety state
    lands in the LAST column of rows four floats wider than that."""
    N = 300
    st, seen = _saute_run(lib, N, 48, 0.999, -0.5, saute_params(N), lambda t: saute_inputs(N, t), final)
    assert seen['unsafe'] > 100 and seen['done'] > N  # both branches of the reward, many restarts
    assert (st['safety_obs'].vec() > 0).any() and (st['safety_obs'].vec() <= 0).any()


def saute_zero_case(N, t):
    d = saute_inputs(N, t, seed=40)
    for k, v in (('cost', 0.25), ('reward', 3.0), ('terminated', 0), ('truncated', 0)):
        d[k][7] = v
    return d


def test_saute_step_z_exactly_zero_is_unsafe(lib):
    """Env 7: budget 0.5, saute_gamma 1, costs 0.25 and 0.25 take z from 1 to 0.5 to exactly 0, which is not `> 0`."""
    N = 300
    prm = saute_params(N)
    prm['budget'][7], prm['reset_value'][7] = 0.5, 1.0
    st, _ = _saute_run(lib, N, 1, 1.0, -7.0, prm, lambda t: saute_zero_case(N, t), True)
    assert st['safety_obs'].vec()[7] == F(0.5) and st['reward_out'].vec()[7] == F(3.0)
    # (a second run of two steps: _saute_run starts from the reset values)
    st, _ = _saute_run(lib, N, 2, 1.0, -7.0, prm, lambda t: saute_zero_case(N, t), True)
    assert st['safety_obs'].vec()[7] == 0.0 and st['reward_out'].vec()[7] == F(-7.0)
    assert st['ep_budget'].vec()[7] == F(0.5) and st['next_rows'].np()[7, SAUTE_COL] == 0.0


# ---- osa_action_scale ----------------------------------------------------------------------------------------------
def action_scale_inputs(N, D):
    rng = np.random.default_rng(N + D)
    lo, hi = np.linspace(-2.0, -0.5, D).astype(np.float32), np.linspace(0.7, 3.0, D).astype(np.float32)
    if D > 1:
        hi[D // 2] = lo[D // 2]  # a degenerate dimension: every action maps to that one value
    return (rng.standard_normal((N, D)) * 1.5).astype(np.float32), lo, hi


@pytest.mark.parametrize('N,D', [(1, 1), (300, 2), (130, 17)])
def test_action_scale(lib, N, D):
    act, lo, hi = action_scale_inputs(N, D)
    a = Guarded(N, D, ld=D + 3).set(act)
    out, tlo, thi = Guarded(N, D, ld=D + 5), dev(lo), dev(hi)
    _check(lib.osa_action_scale(a.ptr, a.ld, out.ptr, out.ld, N, D, ptr(tlo), ptr(thi), -1.0, 1.0, _stream()),
           'osa_action_scale')
    want = R.action_scale(act, lo, hi, -1.0, 1.0)
    assert np.array_equal(out.np(), want)
    if D > 1:
        assert (out.np()[:, D // 2] == lo[D // 2]).all()
    assert out.intact() and a.intact() and np.array_equal(a.np(), act)


# ---- osa_normalizer_apply --------------------------------------------------------------------------------------------
APPLY_CLIP = 1.5


def apply_inputs(N, D):
    rng = np.random.default_rng(N * D)
    mean = rng.uniform(-3, 3, D).astype(np.float32)
    std = rng.uniform(0.5, 2, D).astype(np.float32)
    std[D - 1] = 1e-2  # a column on the floor of the standard deviation
    x = (rng.standard_normal((N, D)) * 3).astype(np.float32)
    x.reshape(-1)[0] = 1e30  # far beyond the clip on either side, and a NaN
    if N * D > 4:
        x.reshape(-1)[[1, 2, 3]] = -1e30, np.nan, np.inf
    masks = {'none': None, 'mixed': (rng.random(N) < 0.5).astype(np.uint8), 'all-false': np.zeros(N, np.uint8)}
    if N > 1:
        masks['mixed'][:2] = 1, 0
    else:
        masks['mixed'][0] = 1
    return x, mean, std, masks


@pytest.mark.parametrize('N,D', [(1, 1), (300, 65), (129, 130)])
def test_normalize_apply(lib, N, D):
    x, mean, std, masks = apply_inputs(N, D)
    xin = Guarded(N, D, ld=D + 3).set(x)
    tm, ts = dev(mean), dev(std)
    for (mname, mask), count in itertools.product(masks.items(), (0, 1, 2)):
        y = Guarded(N, D, ld=D + 2)
        cnt, tmask = torch.tensor([count], dtype=torch.int64, device=DEV), dev(mask)
        _check(lib.osa_normalizer_apply(xin.ptr, xin.ld, y.ptr, y.ld, N, D, ptr(tmask), ptr(tm), ptr(ts), ptr(cnt),
                                        APPLY_CLIP, _stream()), 'osa_normalizer_apply')
        got, want = y.np(), R.normalize_apply(x, mean, std, count, APPLY_CLIP, mask)
        assert np.array_equal(got, want, equal_nan=True), (mname, count)
        if count <= 1 or mname == 'all-false':
            assert np.array_equal(got, x, equal_nan=True), (mname, count)  # pass-through
        else:
            flat = got.reshape(-1)  # (row 0 is selected by both masks)
            assert flat[0] == F(APPLY_CLIP)
            if N * D > 4:
                assert flat[1] == F(-APPLY_CLIP) and np.isnan(flat[2]) and flat[3] == F(APPLY_CLIP)
                on = np.ones(N, bool) if mask is None else mask != 0
                assert np.nanmax(np.abs(got[on])) == F(APPLY_CLIP) and (np.abs(got[on][:, D - 1]) == F(APPLY_CLIP)).any()
        assert y.intact(), (mname, count)
    assert xin.intact() and np.array_equal(xin.np(), x, equal_nan=True)


# ---- osa_normalizer_push ---------------------------------------------------------------------------------------------
RATIOS = []  # e_k / max(e_ref, 2**-23) of every state check of this module (printed by the last test)


class PushCase:
    """One device Normalizer whose state and workspace live in guarded tensors, next to the reference's float32 form
    (np_oracle.Normalizer) and the float64 truth (rollout_twin.RunningMoments), all fed the same selected rows."""

    def __init__(self, D, max_n, clip=5.0, skip_var=()):
        from omnisafe_amd.normalizer import Normalizer

        self.D, self.skip_var = D, skip_var
        self.norm = Normalizer((D,), clip=clip, device=DEV)
        self.g = {k: vec(D).set(np.zeros(D, np.float32)) for k in ('_mean', '_sumsq', '_var', '_std')}
        self.g['_count'] = vec(1, torch.int64).set(np.zeros(1, np.int64))
        need = self.norm._lib.osa_normalizer_ws_doubles(max_n, D)
        self.g['_ws'] = vec(need, torch.float64).set(np.zeros(need))
        for k, g in self.g.items():
            setattr(self.norm, k, g.t.view(-1))
        self.ref, self.truth = O.Normalizer((D,), clip=clip), R.RunningMoments(D)

    def state(self):
        return {k: self.g[k].vec().copy() for k in ('_mean', '_sumsq', '_var', '_std', '_count')}

    def push(self, x, mask=None, ld_extra=0, tag=''):
        """x (N, D) float32 numpy; ld_extra > 0: handed over as a column slice of a (N, D + ld_extra) tensor."""
        N = x.shape[0]
        if ld_extra:
            wide = torch.full((N, self.D + ld_extra), float('nan'), device=DEV)
            wide[:, 1:1 + self.D] = dev(x)
            xt = wide[:, 1:1 + self.D]
            assert xt.stride(0) == self.D + ld_extra
        else:
            xt = dev(x)
        self.norm.push(xt, mask=dev(mask))
        sel = x if mask is None else x[np.asarray(mask) != 0]
        if sel.shape[0]:
            self.ref.push(torch.from_numpy(sel.copy()))
        self.truth.push(sel)
        self.check(tag)

    def check(self, tag=''):
        s, n = self.state(), self.truth.count
        assert int(s['_count'][0]) == n == self.ref.count, tag
        assert int(self.g['_ws'].full.view(torch.int32)[2 * 64].item()) == 0, tag  # the ticket is re-armed
        if n == 0:
            assert all(not s[k].any() for k in s), tag
            return
        with np.errstate(invalid='ignore', divide='ignore'):
            var = s['_sumsq'] / F(n - 1)
            std = np.maximum(np.sqrt(var), F(1e-2))
        assert np.array_equal(s['_var'], var, equal_nan=True), tag
        assert np.array_equal(s['_std'], std, equal_nan=True), tag
        if n == 1:
            assert np.isnan(s['_var']).all() and np.isnan(s['_std']).all(), tag
            assert np.array_equal(s['_mean'], self.truth.rows[0].astype(np.float32)), tag
        ek = R.moment_errors(s['_mean'], s['_var'], self.truth, self.skip_var)
        er = R.moment_errors(self.ref.mean.numpy(), self.ref.var.numpy(), self.truth, self.skip_var)
        for a, b, what in zip(ek, er, ('mean', 'var')):
            floor = max(b, 2.0 ** -23)
            RATIOS.append(a / floor)
            print(f'{tag} count {n} {what}: e_k {a:.3e} e_ref {b:.3e} ratio {a / floor:.2f}')
            assert a <= R.MOMENT_FACTOR * floor, (tag, what, n, a, b)

    def intact(self):
        return all(g.intact() for g in self.g.values())


PUSH_SIZES = (1, 3, 4097, 127, 128, 8193, 129, 257)  # 4097: 33 row blocks; 8193: 65; small ones after large ones


def push_batch(rng, n, D):
    return (rng.standard_normal((n, D)) * np.linspace(0.5, 2, D) + np.linspace(-3, 3, D)).astype(np.float32)


@pytest.mark.parametrize('ld_extra', [0, 3], ids=['contiguous', 'column-slice'])
@pytest.mark.parametrize('D', [1, 63, 64, 65, 130])
def test_normalizer_push_shapes(D, ld_extra):
    rng = np.random.default_rng(D)
    case = PushCase(D, max(PUSH_SIZES))
    for n in PUSH_SIZES:
        case.push(push_batch(rng, n, D), ld_extra=ld_extra, tag=f'shapes D={D} ld+{ld_extra} N={n}')
    assert case.truth.count == sum(PUSH_SIZES) and case.intact()


def push_masks(N):
    """(name, mask) in the order they are pushed; None = every row."""
    only = lambda *rows: np.isin(np.arange(N), rows).astype(np.uint8)  # noqa: E731
    block = np.ones(N, np.uint8)
    block[128:256] = 0
    return [('all-false first', np.zeros(N, np.uint8)), ('one row, first push', only(N // 2)), ('only row 0', only(0)),
            ('only the last row', only(N - 1)), ('all-false in the middle', np.zeros(N, np.uint8)),
            ('a 128-row block unselected', block), ('every row', None), ('rows 0 and last', only(0, N - 1))]


@pytest.mark.parametrize('N', [300, 4097])
def test_normalizer_push_masks(N):
    D = 65
    rng = np.random.default_rng(N)
    case = PushCase(D, N)
    for name, mask in push_masks(N):
        x = push_batch(rng, N, D)
        before = case.state()
        if name == 'one row, first push':  # through normalize(): count 1 -> NaN statistics, the input comes back
            y = case.norm.normalize(dev(x), mask=dev(mask))
            case.ref.push(torch.from_numpy(x[mask != 0].copy()))
            case.truth.push(x, mask)
            case.check(name)
            assert case.truth.count == 1 and np.isnan(case.state()['_std']).all()
            assert np.array_equal(y.cpu().numpy(), x)
            continue
        case.push(x, mask, tag=f'masks N={N} {name}')
        if mask is not None and not mask.any():  # an empty push leaves every bit of the state alone ...
            after = case.state()
            assert all(np.array_equal(before[k], after[k], equal_nan=True) for k in before), name
        else:  # ... and the push behind it merges
            assert int(case.state()['_count'][0]) == int(before['_count'][0]) + (N if mask is None else int(mask.sum()))
            assert not np.array_equal(before['_mean'], case.state()['_mean'])
    assert case.intact()


HARD_SIZES, HARD_D, HARD_CONST, HARD_OFFSET = (257, 64, 1, 2000, 33), 130, 7, 11


def hard_batches():
    rng = np.random.default_rng(23)
    std, mean = np.logspace(-3, 3, HARD_D), np.linspace(-50, 50, HARD_D)
    std[HARD_CONST], mean[HARD_CONST] = 0.0, 3.5
    std[HARD_OFFSET], mean[HARD_OFFSET] = 0.1, 1e4
    return [(rng.standard_normal((n, HARD_D)) * std + mean).astype(np.float32) for n in HARD_SIZES]


def test_normalizer_push_hard_columns():
    """Standard deviations from 1e-3 to 1e3 with means from -50 to 50, a constant column, a column at 1e4 +- 0.1."""
    case = PushCase(HARD_D, max(HARD_SIZES), skip_var=(HARD_CONST,))
    for i, x in enumerate(hard_batches()):
        case.push(x, tag=f'hard columns batch {i}')
        s = case.state()
        assert s['_mean'][HARD_CONST] == F(3.5) and s['_sumsq'][HARD_CONST] == 0
        if i > 0:
            assert s['_var'][HARD_CONST] == 0 and s['_std'][HARD_CONST] == F(1e-2)
    y = case.norm.apply(dev(x)).cpu().numpy()
    assert np.isfinite(y).all() and np.abs(y).max() <= 5.0 and not y[:, HARD_CONST].any()
    assert case.intact()


def test_normalizer_statistics_ratio_report(capsys):
    """Not a check of its own: prints the worst e_k / max(e_ref, 2**-23) of the state checks above (each of them has
    asserted the bound already)."""
    with capsys.disabled():
        print(f'\n[normaliser statistics] {len(RATIOS)} state checks, worst e_k / max(e_ref, 2^-23): '
              f'{max(RATIOS, default=float("nan")):.2f}')
    assert all(r <= R.MOMENT_FACTOR for r in RATIOS)
