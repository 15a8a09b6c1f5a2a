"""CPU tests of the data-parallel part of tests/step_twin.py -- dp_step and dp_table(), the float64 statement and the
table that tests/test_dp_forms_gpu.py holds the data-parallel kernels to.

  * dp_step at W = 1 IS step (bit for bit, float64); at W = 2 with the same rows on both ranks it is the single-rank
    step to float64 rounding; the rank-mean scalars are the means of step()'s scalars;
  * the float32 run of dp_run_pass is finite on every case of the table;
  * every case reaches what it is named for (step_twin.dp_check_coverage): the clip cells on every rank's every
    minibatch, no clipped rank in a base case, ranks on both sides of max_grad_norm in a straddle case, every rank
    clipped in normclip-all; the named tails leave the named chunks empty;
  * THE TABLE CAN TELL RIGHT FROM WRONG: for every straddle-* and normclip-all case the float64 twin also computes
    what a kernel would get that clipped after averaging, applied the mean factor, applied its neighbour's factor or
    summed instead of averaging, and for a ragged tail what it would get dividing by B instead of n
    (step_twin.dp_wrong_statements).  Each must sit further than K x max(e32, 2^-22), K = 16 -- the whole tolerance of
    the GPU test -- from the right gradient on at least one tensor of the named network, in relative L2.  A case
    that does not meet this gets another scaling of its ranks, never another K.  (One pair is the same function:
    with every rank clipped, dividing a tail by B leaves max_grad_norm g_r / |g_r| where it was; normclip-all shows
    that statement through the critics' L2 term alone, the straddle cases show it on the ranks that do not clip);
  * tests/golden/dp_twin_f32_error.json (`python tests/test_dp_twin.py` writes it, through step_twin.pack_f32_error)
    reproduces within a factor 2 on max(e32, 2^-22), and the two earlier measuring sticks keep their bytes.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):  # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import step_twin as T  # noqa: E402

ERR_FILE = os.path.join(HERE, 'golden', 'dp_twin_f32_error.json')
DP_TABLE = T.dp_table()
K = 16  # K_GRAD of tests/test_dp_forms_gpu.py
# sha256 of the bytes of the two earlier measuring sticks: this table was added in a file of its own
EARLIER_FILES_SHA256 = {
    'step_twin_f32_error.json': '6e32d89d7c40c21f3c5d2573213094ecba0335226834657002de1fdd051a1eea',
    'general_twin_f32_error.json': '885d93db23c553d855ccb519bed138841e578dd743468857543af38f13aeeded'}
CLIPPED = [name for name, e in DP_TABLE.items() if e['kw'].get('norm_clip') is not None]


@pytest.fixture(scope='module', autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)  # (one summation order: the float32 figures below are compared with recorded ones)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope='module')
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = T.make_dp_case(**DP_TABLE[name]['kw'])
        return cache[name]

    return get


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_table_is_the_one_the_issue_names():
    assert not set(DP_TABLE) & (set(T.case_table()) | set(T.form_table()) | set(T.general_table()))
    shapes = {(e['kw']['obs_dim'], e['kw']['act_dim'], e['kw']['W'], e['kw']['B'], e['kw']['M'])
              for name, e in DP_TABLE.items() if name.startswith('base-')}
    assert shapes == set(T.DP_NARROW) | set(T.DP_CHUNK) | set(T.DP_WIDE)
    reached = {form for e in DP_TABLE.values() for form in e['forms']}
    assert reached == set(T.DP_FORMS)
    for (shape, forms) in T.DP_VARIANT_SHAPES:
        for tag in T.dp_variants():
            assert DP_TABLE[T.dp_name(tag, T.dp_kw(*shape))]['forms'][:len(forms)] == forms
    # the twin works on at most 16 x 64 rows per rank-step and 16 ranks
    assert all(e['kw']['W'] <= 16 and e['kw']['B'] <= 200 for e in DP_TABLE.values())


def test_table_shapes_select_their_forms():
    """Host-side conditions of the forms (that the device then accepts them is asserted on the GPU): the narrow and
    chunk families on shapes of the narrow pass, B <= 64 / 64 < B, the chunked form within 16 ranks; the wide family
    on shapes the narrow pass refuses and the split pass takes, B <= 64, first layer scaled."""
    from omnisafe_amd import _lib

    lib = _lib.load()
    for name, e in DP_TABLE.items():
        kw = e['kw']
        od, ad, B, W = kw['obs_dim'], kw['act_dim'], kw['B'], kw['W']
        narrow = lib.osa_ppo_pass_supported(od, ad, 64) == 1
        forms = set(e['forms'])
        if forms & {'dp-split', 'dp-split-spread'}:
            assert not narrow and B <= 64 and lib.osa_ppo_split_pass_supported(od, ad, 64) == 1, name
            assert kw['w1_scale'] == (64.0 / od) ** 0.5
        elif forms & {'dp-chunked', 'dp-coop-walk'}:
            assert narrow and 64 < B <= 1024 and W <= 16 and forms <= {'dp-chunked', 'dp-coop-walk', 'dp-steps'}, name
            assert W * ((B + 63) // 64) <= 32, name  # peers of the chunked form within the local-placement limit
        else:
            assert narrow and B <= 64 and forms <= {'dp-steps', 'dp-steps-graph', 'dp-coop', 'dp-coop-uncached'}, name


def test_one_rank_is_the_single_rank_step_bit_for_bit():
    case = T.make_case(60, 2, 64, 100, seeded_moments=True, t0=(3, 5, 7), norm_clip=('all', 0.5))
    for k in range(2):
        s, n = T.minibatches(100, 64)[k]
        batch = T.rows(case['data'], case['perm'][s:s + n])
        one = T.step(case['state'], batch, case['hp'], case['lam'], 0)
        dp = T.dp_step(case['state'], [batch], case['hp'], case['lam'], 0)
        for net in T.NETS:
            assert float(one[net]['coef']) < 1.0
            for t in one[net]['grads']:
                assert _same_bits((one[net]['grads'][t] * one[net]['coef']).numpy(), dp[net]['g'][t].numpy())
                for which in ('p', 'm', 'v'):
                    assert _same_bits(one[net][which][t].numpy(), dp[net][which][t].numpy()), (net, t, which)
            for sc in T.SCALARS[net]:
                assert _same_bits(np.float64(one[net][sc]), np.float64(dp[net][sc])), (net, sc)
            assert (dp[net]['t'], dp[net]['step_size'], dp[net]['inv_bc2_sqrt']) == (
                one[net]['t'], one[net]['step_size'], one[net]['inv_bc2_sqrt'])


def test_two_ranks_with_the_same_rows_are_one_rank():
    case = T.make_case(65, 17, 48, 100, norm_clip=(0, 0.5))
    batch = T.rows(case['data'], case['perm'][:48])
    one = T.step(case['state'], batch, case['hp'], case['lam'], 0)
    dp = T.dp_step(case['state'], [batch, batch], case['hp'], case['lam'], 0)
    for net in T.NETS:
        for t in one[net]['grads']:
            for which in ('p', 'm', 'v'):
                assert T.rel_l2(dp[net][which][t].numpy(), one[net][which][t].numpy()) <= 4 * 2.0 ** -52, (net, t, which)
        for sc in T.SCALARS[net]:
            assert T.rel_l2(float(dp[net][sc]), float(one[net][sc])) <= 4 * 2.0 ** -52


def test_layout_is_rank_major_and_ranks_differ(cases):
    """Rank r's minibatches read rows r M .. r M + M - 1 only, each row once per pass; the ranks' first-minibatch
    gradient norms differ by tens of percent (largest / smallest >= 1.2 for every network)."""
    case = cases(T.dp_name('base', T.dp_kw(65, 17, 8, 64, 100)))
    W, M = case['W'], case['M']
    assert case['perm'].shape == (W, M) and case['data']['obs'].shape[0] == W * M
    seen = np.concatenate([np.concatenate(T.dp_minibatch(case, k)) for k in range(2)])
    assert sorted(seen.tolist()) == list(range(W * M))
    for r, idx in enumerate(T.dp_minibatch(case, 1)):
        assert len(idx) == 36 and idx.min() >= r * M and idx.max() < (r + 1) * M
    r0 = T.dp_case_step(case, case['state'], 0)
    for net in T.NETS:
        assert max(r0[net]['gnorms']) >= 1.2 * min(r0[net]['gnorms']), (net, r0[net]['gnorms'])


@pytest.mark.parametrize('name', list(DP_TABLE))
def test_case_reaches_what_it_is_named_for(cases, name):
    case = cases(name)
    info = T.dp_check_coverage(case)
    print(name, info)
    if 'tail' in DP_TABLE[name]:
        rows, empty = DP_TABLE[name]['tail']
        n = T.minibatches(case['M'], case['B'])[-1][1]
        assert (n, T.empty_chunks(case['B'], n)) == (rows, empty)
    res, final = T.dp_run_pass(case, torch.float32)
    for r in res:
        for net in r:
            assert all(bool(torch.isfinite(x).all()) for x in r[net]['g'].values())
            assert all(np.isfinite(float(r[net][sc])) for sc in T.SCALARS[net])
    assert all(bool(torch.isfinite(torch.as_tensor(np.asarray(x))).all()) for w in ('params', 'm', 'v')
               for net in T.case_nets(case) for x in final[w][net].values())


def test_named_tails(cases):
    tails = {name: e['tail'] for name, e in DP_TABLE.items() if 'tail' in e}
    assert {t for t in tails.values()} >= {(65, 0), (44, 1), (100, 2), (128, 0)}, tails
    one_row = cases(T.dp_name('base', T.dp_kw(60, 2, 2, 64, 65)))
    assert T.minibatches(one_row['M'], one_row['B'])[-1][1] == 1


@pytest.mark.parametrize('name', CLIPPED)
def test_table_can_tell_right_from_wrong(cases, name):
    """Every wrong statement of the step differs from the right one by more than the GPU test's whole tolerance,
    K x max(e32, 2^-22) in relative L2, on at least one tensor of the network the case is named for (normclip-all:
    of every network) -- on every minibatch, ragged tail included."""
    case = cases(name)
    e32 = T.load_f32_error(ERR_FILE)[0][name]
    which, arg = case['norm_clip']
    named = [arg] if which == 'straddle' else list(T.case_nets(case))
    for k, (_, n) in enumerate(T.minibatches(case['M'], case['B'])):
        st = T.dp_wrong_statements(case, k)
        assert ('tail-over-B' in st) == (n < case['B'])
        for what, g in st.items():
            if what == 'right':
                continue
            margins = {}
            for net in named:
                margins[net] = max(T.rel_l2(g[net][t].numpy(), st['right'][net][t].numpy())
                                   / (K * max(e32[net][t], T.FLOOR)) for t in g[net])
                print(name, k, what, net, 'distance / tolerance', margins[net])
            if which == 'all' and what == 'tail-over-B':
                # a rank that clips hands on max_grad_norm g_r / |g_r|, which no common factor on g_r changes: with
                # EVERY rank clipped the division by B is invisible wherever the whole gradient carries the factor
                # (the actor, up to its entropy term) and shows only through the critics' L2 term, which does not
                continue_ok = max(margins[net] for net in named if net != 'actor') > 1.0
                assert continue_ok, (k, what, margins)
                continue
            assert all(m > 1.0 for m in margins.values()), (k, what, margins)


def test_earlier_measuring_sticks_keep_their_bytes():
    for fname, want in EARLIER_FILES_SHA256.items():
        with open(os.path.join(HERE, 'golden', fname), 'rb') as fh:
            assert hashlib.sha256(fh.read()).hexdigest() == want, fname


def test_dp_measuring_stick_reproduces(cases):
    """tests/golden/dp_twin_f32_error.json against a fresh measurement, as test_step_twin.py holds the 64-row file:
    within a factor 2 on max(e32, 2^-22), for the worst-of-orders figures (the GPU tests' unit) and the single run."""
    want = T.load_f32_error(ERR_FILE)
    assert sorted(want[0]) == sorted(DP_TABLE)
    for name in DP_TABLE:
        got = T.dp_f32_error(cases(name))
        for which, g, w in zip(('worst', 'single'), got, want):
            assert sorted(g) == sorted(w[name]) == sorted(T.case_nets(cases(name))), name
            for net in g:
                assert sorted(g[net]) == sorted(w[name][net]), (name, net)
                assert T.OUT_BIAS_ROWS in g[net] or net == 'actor'
                for k, e in g[net].items():
                    a, b = max(e, T.FLOOR), max(w[name][net][k], T.FLOOR)
                    assert a <= 2 * b and b <= 2 * a, (which, name, net, k, e, w[name][net][k])


if __name__ == '__main__':  # writes the measuring stick of dp_table()
    torch.set_num_threads(1)
    blob = T.pack_f32_error({nm: T.dp_f32_error(T.make_dp_case(**e['kw'])) for nm, e in DP_TABLE.items()})
    with open(ERR_FILE, 'w') as fh:
        fh.write('{"keys": ' + json.dumps(blob['keys']) + ',\n"blocks": [\n'
                 + ',\n'.join(json.dumps(b) for b in blob['blocks']) + '],\n"cases": {\n'
                 + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in blob['cases'].items()) + '}}\n')
    print(ERR_FILE, os.path.getsize(ERR_FILE), 'bytes', len(blob['blocks']), 'blocks')
