"""The data-parallel forms of the optimiser step -- every way PPOUpdater.run_pass_replicated computes the global step
of W ranks on one device, and the peer-exchange pass at a world of one -- against tests/step_twin.py's dp_step, the
float64 statement of that step: each rank clips by ITS gradient norm, the clipped gradients are averaged, one Adam
step is taken, every logged scalar is the mean over the ranks.  The checks, units and tolerances are those of
tests/test_step_oracle_gpu.py (imported, not copied); K_GRAD = K_SCALAR = 16 units of max(e32, 2^-22), e32 from
tests/golden/dp_twin_f32_error.json (the float32 run of the twin against its float64 run: step_twin.dp_f32_error),
nothing measured on the code under test.  tests/test_dp_twin.py shows on the CPU that these tolerances separate the
step from a step that clips after averaging, mixes the ranks' factors up, sums, or divides a tail by B.

  form              how reached                                        code
  dp-steps          run_pass_replicated(coop=False, use_graph=False)   osa_ppo_dp_step, osa_dp_apply_kernel, osa_ppo_dp_end_pass
  dp-steps-graph    the same, use_graph=True                           the same launches: eager, captured, replayed
  dp-coop           coop=True, B <= 64, OSA_DP_XCH=local               osa_ppo_dp_pass_placed, one XCC per network
  dp-coop-uncached  OSA_DP_XCH=uncached                                the same kernel, uncached exchange buffer
  dp-coop-walk      coop=True, B > 64, OSA_CHUNKED_PASS=0              one workgroup per rank walking the chunks
  dp-chunked        coop=True, B > 64                                  osa_ppo_dp_chunked_pass
  dp-split          wide observations, OSA_WIDE_DP=place               osa_ppo_split_dp_pass, owner groups on one XCC
  dp-split-spread   OSA_WIDE_DP=spread                                 the same kernel rank-major, uncached exchange

How a step is observed.  Minibatch k of a case is a pass of ONE minibatch through run_pass_replicated: the rows of
all W ranks for minibatch k as an all-gathered data set of their own (W n rows, the identity (W, n) permutation,
batch_size = B as in the case), from the state under test -- so a ragged tail meets the kernels as it does in a pass
(n < B rows, empty chunk workgroups).  From zero moments g_kernel = m' / (1 - b1) is the averaged clipped gradient:
rel_l2(g_kernel, g_64) <= K_GRAD unit per reference tensor.  The ranks' factors are not observable (the statistics
row carries the rank-mean of the unclipped norms only) and they are inside g_64, so there is no clip-factor row and
the chain tolerances are step_twin.dp_state_tolerances, state_tolerances without its clip-factor term.  v' against
(1 - b2) g_kernel^2 within 4 ulp, check_adam, check_seeded_step, check_structure as for a single rank; check_scalars
against the rank-mean scalars (the gradient-norm column: the mean of the ranks' unclipped norms); check_bias_columns
on the forms that tabulate Adam's bias corrections in columns 10..15 (all but the stepwise ones).

Chains (seeded moments): the cooperative forms are one launch per pass and are compared -- statistics rows of every
step, final state -- with dp_run_pass's float64 chain; dp-steps step by step from the kernel's own state, then the
whole pass against its launches bit for bit.  dp-steps-graph runs every step three times from the same state on the
same buffers -- eager, captured, replayed -- the bits must be identical and the twin is compared with the replay.

After every run: the form ran and did not fall back (_dp['coop_passes'] advanced, _dp['chunked'] / _dp['local'] /
_dp['wide_place'] as the form names them, the placement verified on placed forms), the sticky words are clear
(check_dp_sync / check_wide_dp_sync), adam_step advanced for the masked networks only.  Nothing skips; a form that
declines fails.

Peer exchange at a world of one: without a process group (_p2p_setup needs none there) three cases of
step_twin.case_table() run through run_pass_p2p against the single-rank twin with every check of
tests/test_step_oracle_gpu.py -- the kernel's own release / arrival / slab-sum / Adam-from-slab path.

Measured worst ratios per form, case and tensor: profiles/dp_twin_error.md -- gradient 4.11 (base-1x1-W1-B5-M12, the
cost critic's second hidden weight), scalar 3.25 on the data-parallel forms (same case, the reward critic's MSE) and
3.41 on the peer-exchange pass; no unit was re-derived.

What the table found.  The seeded cases at W = 3 missed check_seeded_step's 2 ulp on the first moment on dp-chunked
(2.11 / 2.06 / 2.32 ulp for actor / reward critic / cost critic) and dp-split (1.96 / 2.03 / 2.16), while the same
step on dp-steps, dp-coop and dp-coop-walk sat at 1.5 .. 1.7.  Those two kernels multiplied the rank sum by 1 / W
with the clip factor behind it a compile-time 1, and the product was contracted into the first moment's
fma(s, 1 / W, -m): m' saw the unrounded average, v' (and the step from zero moments) the rounded one -- half an ulp
apart wherever 1 / W is no power of two.  osa_scale_rounded (csrc/mlp_device.h) hands both the same float32 number;
since then 1.72 / 1.58 / 1.73 and 1.77 / 1.49 / 1.60.  Worlds of 1, 2, 4, 8, 16 keep their bits.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import step_twin as T
import test_step_forms_gpu as F
import test_step_oracle_gpu as S

pytestmark = pytest.mark.gpu
DEV = S.DEV
DP_TABLE = T.dp_table()
PAIRS = [(name, form) for name, e in DP_TABLE.items() for form in e['forms']]
E32, E32_SINGLE = T.load_f32_error(
    os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dp_twin_f32_error.json'))
P2P_CASES = ('base-60x2', 'mb-B64-M65-60x2', 'seeded-60x2')


@pytest.fixture(scope='module', autouse=True)
def _figures():
    """The figures of THIS module's cases (run one file at a time with OSA_STEP_TWIN_FIGURES)."""
    start = len(S.FIGURES)
    yield
    dst = os.environ.get('OSA_STEP_TWIN_FIGURES')
    if dst:
        with open(dst, 'w') as fh:
            json.dump(S.FIGURES[start:], fh)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case, its zero-moment twin and their float64 results -- computed once, shared by the case's forms."""
    torch.set_num_threads(1)
    kw = DP_TABLE[name]['kw']
    case = T.make_dp_case(**kw)
    zero = T.make_dp_case(**T.zero_moment_twin(kw)) if case['seeded_moments'] else case
    nmb = len(T.minibatches(case['M'], case['B']))
    ref = dict(case=case, zero=zero, first=[T.dp_case_step(zero, zero['state'], k) for k in range(nmb)])
    if case['seeded_moments']:
        ref['chain'] = T.dp_run_pass(case)[0]
    return ref


def dp_tolerances(r, e32, net):
    return T.dp_state_tolerances(r, {t: S.unit(e32, net, t) for t in r[net]['g']}, net, S.K_GRAD)


class DpHarness(S.Harness):
    """S.Harness on the all-gathered rows of W ranks, a step launched through PPOUpdater.run_pass_replicated."""

    def form(self):
        f = self.f = T.DP_FORMS[self.path]
        self._rows = {}
        one_launch = bool(f.get('coop') or f.get('wide'))
        return True, None, one_launch, one_launch

    def __init__(self, case, path):
        super().__init__(dict(case, M=case['W'] * case['M']), path)  # (the device arrays hold all W M rows)
        self.case = case
        if self.f.get('wide'):
            assert self.upd._wide_dp_fits(case['W'])
            self.upd._repl_wide = True

    def rows(self, k):
        """The W ranks' rows of minibatch k, rank-major, as a data set of their own (kept: a captured pass bakes the
        buffers' addresses in)."""
        if k not in self._rows:
            case = self.case
            s, n = T.minibatches(case['M'], case['B'])[k]
            idx = torch.cat([self.perm[r, s:s + n] + r * case['M'] for r in range(case['W'])])
            obs = torch.zeros(len(idx), self.data['obs'].stride(0), device=DEV)  # rows of whole float4s, as the case's
            obs[:, :case['obs_dim']] = self.data['obs'][idx]
            d = {key: v[idx].contiguous() for key, v in self.data.items() if key != 'obs'}
            d['obs'] = obs[:, :case['obs_dim']]
            self._rows[k] = (d, n, torch.arange(n, device=DEV).repeat(case['W'], 1).contiguous())
        return self._rows[k]

    def run_replicated(self, d, M, perms):
        upd, f, W = self.upd, self.f, self.case['W']
        st = upd._dp
        passes = st.get('coop_passes', 0) if (st.get('M'), st.get('W')) == (M, W) else 0  # (another M: fresh buffers)
        stats = torch.zeros((M + self.case['B'] - 1) // self.case['B'], S.NSTAT, device=DEV)
        upd.run_pass_replicated(d, M, W, self.lam, stats, perms_all=perms, use_graph=bool(f.get('graph')),
                                coop=bool(f.get('coop')))
        torch.cuda.synchronize()
        if f.get('wide'):
            upd.check_wide_dp_sync()
            assert st.get('wide_xch') and st['wide_place'] is f['place'], (st.get('wide_place'), f)
            assert st['wide_verified'] is f['place']
        elif f.get('coop'):
            assert st.get('coop_passes') == passes + 1, ('fell back to the stepwise form', st.get('coop_passes'))
            assert st['chunked'] is f['chunked'] and st['local'] is f['local'], (st['chunked'], st['local'], f)
            if f['local']:
                assert st.get('verified')
            else:
                assert st['xch'] is None and st['xch_ptr']  # (the uncached exchange buffer, not an ordinary tensor)
            upd.check_dp_sync()
        else:
            assert 'coop_passes' not in st and 'wide_xch' not in st and st.get('warm')
        return stats.cpu().numpy()

    def launch_step(self, k):
        d, n, ident = self.rows(k)
        stats = self.run_replicated(d, n, ident)
        assert stats.shape[0] == 1
        return stats[0]

    def one_step(self, state, k):
        if not self.f.get('graph'):
            return super().one_step(state, k)
        # eager (the warm pass), captured + replayed, replayed: the same bits; the twin is compared with the replay
        upd = self.upd
        upd._dp_free()
        upd._dp.clear()
        res = super().one_step(state, k)
        assert upd._dp.get('graph') is None
        for _ in range(2):
            again = super().one_step(state, k)
            assert upd._dp.get('graph') is not None and not upd._dp.get('graph_failed', False)
            for which, blk in res[1]['blocks'].items():
                assert np.array_equal(blk, again[1]['blocks'][which]), (which, 'graph replay against the eager pass')
            assert np.array_equal(res[2], again[2]) and res[1]['t'] == again[1]['t']
        return again

    def whole_pass(self, state):
        self.load(state)
        before = self.read()
        stats = self.run_replicated(self.data, self.case['M'], self.perm)
        return before, self.read(), stats


def check_first_step(name, form, h, ref, k, failures):
    """Minibatch k from the zero-moment state: the averaged clipped gradient, v', the rank-mean statistics, Adam, the
    bias-correction columns."""
    zero, r = ref['zero'], ref['first'][k]
    before, after, stats = h.one_step(zero['state'], k)
    S.check_structure(h, before, after, 1)
    e32, kind = E32[name], f'step{k}'
    S.check_scalars(name, form, kind, r, stats, e32, failures, case=zero, e32_single=E32_SINGLE[name])
    grads = {}
    for net in h.nets:
        g = grads[net] = S.kernel_gradient(h, after, stats, net)[0]
        for t, want in r[net]['g'].items():
            err = T.rel_l2(g[t], want.numpy())
            u = S.unit(e32, net, t)
            S.record(name, form, kind + '/grad', net, t, err / u, S.K_GRAD, err / S.unit(E32_SINGLE[name], net, t))
            if not err <= S.K_GRAD * u:
                failures.append((kind, net, t, 'averaged clipped gradient rel l2 / max(e32, 2^-22)', err / u))
        S.check_second_moment(name, form, kind, net, g, after['v'][net], failures)
    if h.bias_columns:
        S.check_bias_columns(h, kind, stats, after['t'], failures)
    S.check_adam(name, form, kind, h, before, after, failures)
    return grads, {net: after['v'][net] for net in h.nets}


def check_chain(name, form, h, ref, failures):
    """Seeded moments, the whole pass (S.check_chain on the data-parallel twin)."""
    case, e32 = ref['case'], E32[name]
    nmb = len(T.minibatches(case['M'], case['B']))
    scal = dict(case=case, e32_single=E32_SINGLE[name])
    if not h.one_launch:
        state = case['state']
        for k in range(nmb):
            before, after, stats = h.one_step(state, k)
            r = T.dp_case_step(case, {w: before[w] for w in ('params', 'm', 'v', 't')}, k)
            S.check_scalars(name, form, f'chain{k}', r, stats, e32, failures, **scal)
            for net in h.nets:
                S.check_step_moments(name, form, f'chain{k}', net, dp_tolerances(r, e32, net), after, r, failures)
            S.check_adam(name, form, f'chain{k}', h, before, after, failures)
            state = {w: after[w] for w in ('params', 'm', 'v', 't')}
        before, final, stats = h.whole_pass(case['state'])
        S.check_structure(h, before, final, nmb)
        for which in ('params', 'm', 'v'):
            assert np.array_equal(final['blocks'][which], after['blocks'][which]), (which, 'the pass against its launches')
        return
    before, final, stats = h.whole_pass(case['state'])
    S.check_structure(h, before, final, nmb)
    for k, r in enumerate(ref['chain']):
        S.check_scalars(name, form, f'chain{k}', r, stats[k], e32, failures, **scal)
        S.check_bias_columns(h, f'chain{k}', stats[k], {net: before['t'][net] + k + 1 for net in h.nets}, failures)
    S.check_final_state(name, form, h.nets, ref['chain'], e32, final, failures, tolerances=dp_tolerances)


@pytest.mark.parametrize('name,form', PAIRS)
def test_dp_form_against_the_float64_twin(name, form, monkeypatch):
    from omnisafe_amd import update as U

    for key in T.DP_ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for key, value in T.DP_FORMS[form]['env'].items():
        monkeypatch.setenv(key, value)
    monkeypatch.setitem(U._PLACEMENT, 'local_ok', None)
    ref = reference(name)
    case = ref['case']
    h = DpHarness(case, form)
    failures = []
    nmb = len(T.minibatches(case['M'], case['B']))
    for k in range(nmb):
        g = check_first_step(name, form, h, ref, k, failures)
        if k == 0:
            grads0, gsq0 = g
    if case['seeded_moments']:
        S.check_seeded_step(name, form, h, ref, grads0, gsq0, failures)
        check_chain(name, form, h, ref, failures)
    else:  # the pass as the updater runs it: the form, the step counters, the padding, the networks outside the mask
        before, final, stats = h.whole_pass(case['state'])
        S.check_structure(h, before, final, nmb)
        assert np.isfinite(stats).all()
        moved = [net for net in h.nets if not np.array_equal(
            final['blocks']['params'][T.NETS.index(net)], before['blocks']['params'][T.NETS.index(net)])]
        assert moved == list(h.nets)
    assert not failures, failures


class P2PHarness(F.FormHarness):
    """F.FormHarness with a step launched through PPOUpdater.run_pass_p2p at a world of one (no process group)."""

    def form(self):
        self._rows = {}
        return True, None, True, True

    def run_p2p(self, d, perm):
        upd = self.upd
        assert upd._p2p_setup() and upd._p2p['W'] == 1
        M = d['obs'].shape[0]
        nmb = (M + self.case['B'] - 1) // self.case['B']
        stats = torch.zeros(nmb, S.NSTAT, device=DEV)
        seq = upd._p2p['seq']
        upd.run_pass_p2p(d, perm, self.lam, stats)
        torch.cuda.synchronize()
        upd.check_p2p_sync()
        assert upd._p2p['seq'] == seq + nmb
        return stats.cpu().numpy()

    def launch_step(self, k):
        d, ident, _ = self.rows(k)
        stats = self.run_p2p(d, ident)
        assert stats.shape[0] == 1
        return stats[0]

    def whole_pass(self, state):
        self.load(state)
        before = self.read()
        stats = self.run_p2p(self.data, self.perm)
        return before, self.read(), stats


@pytest.mark.parametrize('name', P2P_CASES)
def test_peer_exchange_pass_at_world_one_against_the_float64_twin(name, monkeypatch):
    from omnisafe_amd import distributed as dist

    monkeypatch.setenv('OSA_P2P_TIMEOUT_S', '3')
    monkeypatch.delenv('OSA_P2P_FENCE', raising=False)
    assert not dist.is_initialized() and dist.world_size() == 1
    h = P2PHarness(S.reference(name)['case'], 'p2p')
    assert h.upd._p2p_setup() and h.upd._p2p['timeout'] == 3.0
    S.check_case(name, 'p2p', h)
    h.upd.check_p2p_sync()
