"""The optimiser step beyond one 64-row workgroup per network -- every other form PPOUpdater.run selects on a single
device -- against tests/step_twin.py, with the checks, units and tolerances of tests/test_step_oracle_gpu.py
(imported, not copied: check_structure, check_scalars, the gradient per reference tensor from the zero-moment step,
clip factor, v' within 4 ulp, check_seeded_step, check_adam, check_chain, check_bias_columns; K_GRAD = K_SCALAR = 16
units of max(e32, 2^-22), e32 from tests/golden/step_twin_f32_error.json, nothing measured on the code under test).

  form           selected when                                   code
  per-step       64 < B < 2048, persistent=False                 osa_mb_grad_kernel on ceil(B / 64) blocks +
                                                                 osa_slab_reduce_finalize_kernel (mlp_kernels.hip)
  chunked        64 < B <= 1024, persistent                      osa_ppo_chunked_pass (ppo_pass_kernel.hip, ppo_pass_body.h)
  wide           narrow pass refuses the shape, B <= 64,         osa_ppo_wide_pass (wide_pass_kernel.hip)
                 OSA_WIDE_SPLIT=0
  split          same shapes, default (one XCC per network)      osa_ppo_split_pass, local (wide_split_kernel.hip)
  split-spread   OSA_WIDE_SPLIT=spread                           the same kernel over all XCCs, uncached exchange buffer
  balanced       B >= 2048, plain surrogate                      osa_ppo_part_kernel (part_grad_kernel.hip) + slab reduce
  strided        B >= 2048, OSA_LARGE_BATCH_BALANCED=0           osa_pass_partial_grad (ppo_pass_kernel.hip) + slab reduce

The cases are step_twin.form_table(): per family the shapes and ragged tails at which the form's own machinery is at
work (a second chunk of one row, tails that leave one, two or fifteen chunk workgroups empty, 6 + 1 K blocks on the
helpers, a third helper, an obs_dim that is no multiple of 4, two output tiles, task ranges that cross a network
boundary, a tail that falls to the several-block kernel), and on one shape per family the loss, L2, norm-clip, mask
and Adam variants of the 64-row table.  tests/test_step_twin.py asserts on the CPU that every case reaches its
branches and that the named tails leave the named chunks empty.

How a step is observed: through PPOUpdater.run alone.  Minibatch k of a case is a pass of ONE minibatch -- run() on the
k-th minibatch's rows as a data set of their own (M = n) with the identity permutation, batch_size = B as in the case,
from the state under test -- so the tail of a B-row pass meets the kernels as it does in a pass (n < B rows, empty
chunk workgroups, a several-block or single-block tail after 2048-row steps).  After every run() the test asserts
last_path and that the form did not decline on the device: the chunked and split passes ran with their one-XCC
placement verified (split-spread: not local), and for B >= 2048 the conditions under which the partial-gradient forms
return OSA_EUNSUPPORTED are host-side (shape of the narrow pass, 16-byte aligned rows) and asserted here.  A form that
declines fails the test; nothing skips.

Bias-correction columns 10..15: ppo_pass_body.h (chunked), wide_pass_kernel.hip and wide_split_kernel.hip tabulate
them per step and check_bias_columns runs on these forms; the per-step kernels of mlp_kernels.hip (per-step,
balanced, strided: osa_slab_reduce_finalize_kernel computes the corrections in registers) write no such columns
(column 10 only as P3O's penalty), so there is nothing to check there.

Chains: chunked, wide and split passes are one launch and are compared with the twin's float64 chain; the per-step
forms step by step from the kernel's own state, then run() on the whole pass against its launches bit for bit.

Graph replay: B >= 2048 goes through PPOUpdater._graph_pass (eager, then captured, then replayed).  Every step of
B >= 2048 rows here is run three times from the same state on the same buffers; the three results must be identical
bit for bit, the third must have been a replay, and the comparison with the twin is made on the third.

Measured worst ratios per form, case and tensor: profiles/step_forms_error.md.
"""
import json
import os

import numpy as np
import pytest
import torch

import step_twin as T
import test_step_oracle_gpu as S

pytestmark = pytest.mark.gpu
DEV = S.DEV
FORM_TABLE = T.form_table()
PAIRS = [(name, form) for name, e in FORM_TABLE.items() for form in e['paths']]


@pytest.fixture(scope='module', autouse=True)
def _figures():
    """The figures of THIS module's cases (run one of the two files at a time with OSA_STEP_TWIN_FIGURES)."""
    start = len(S.FIGURES)
    yield
    dst = os.environ.get('OSA_STEP_TWIN_FIGURES')
    if dst:
        with open(dst, 'w') as fh:
            json.dump(S.FIGURES[start:], fh)


class FormHarness(S.Harness):
    """S.Harness with a step launched through PPOUpdater.run on the minibatch's rows."""

    def form(self):
        f = T.FORMS[self.path]
        self._rows = {}
        return f['persistent'], f['last_path'], self.path in ('chunked', 'wide', 'split', 'split-spread'), \
            self.path in ('chunked', 'wide', 'split', 'split-spread')

    def rows(self, k):
        """Minibatch k's rows as a data set of their own (kept: a captured pass bakes the buffers' addresses in)."""
        if k not in self._rows:
            s, n = T.minibatches(self.case['M'], self.case['B'])[k]
            idx = self.perm[s:s + n]
            obs = torch.zeros(n, self.data['obs'].stride(0), device=DEV)  # rows of whole float4s, as the case's
            obs[:, :self.case['obs_dim']] = self.data['obs'][idx]
            d = {key: v[idx].contiguous() for key, v in self.data.items() if key != 'obs'}
            d['obs'] = obs[:, :self.case['obs_dim']]
            old_mean = None if self.upd.ext is None else self.upd._old_mean[idx].contiguous()
            self._rows[k] = (d, torch.arange(n, device=DEV), old_mean)
        return self._rows[k]

    def check_form(self):
        """run() took the form and the device did not decline it."""
        upd = self.upd
        assert upd.last_path == self.last_path, (upd.last_path, self.last_path)
        if self.path == 'chunked':
            ck = upd._chunk
            assert ck.get('verified') and ck.get('local') == 1 and not ck.get('off'), ck
        elif self.path == 'split':
            assert upd._split_xch and upd._split_local and upd._split_verified
        elif self.path == 'split-spread':
            assert upd._split_xch and not upd._split_local
        elif self.path in ('balanced', 'strided'):
            obs = self.data['obs']
            assert upd.lib.osa_ppo_pass_supported(self.case['obs_dim'], self.case['act_dim'], 64) == 1
            assert obs.data_ptr() % 16 == 0 and obs.stride(0) % 4 == 0

    def run_rows(self, d, perm):
        hp = self.case['hp']
        out = self.upd.run(d, self.lam, perms=[perm], actor_lr=hp['lr_actor'], critic_lr=hp['lr_critic'])
        torch.cuda.synchronize()
        self.check_form()
        return out['stats'].cpu().numpy()

    def launch_step(self, k):
        d, ident, old_mean = self.rows(k)
        whole = self.upd._old_mean
        if old_mean is not None:
            self.upd._old_mean = old_mean
        try:
            stats = self.run_rows(d, ident)
        finally:
            self.upd._old_mean = whole
        assert stats.shape[0] == 1
        return stats[0]

    def one_step(self, state, k):
        res = super().one_step(state, k)
        n = T.minibatches(self.case['M'], self.case['B'])[k][1]
        if self.path in ('balanced', 'strided') and n >= 2048:
            # eager, captured + replayed, replayed: the same bits, and what is compared with the twin is the replay
            for _ in range(2):
                again = super().one_step(state, k)
                for which, blk in res[1]['blocks'].items():
                    assert np.array_equal(blk, again[1]['blocks'][which]), (which, 'graph replay against the eager pass')
                assert np.array_equal(res[2], again[2]) and res[1]['t'] == again[1]['t']
            assert self.upd._graphed_pass and self.upd._ug.get('graph') is not None
            res = again
        return res

    def whole_pass(self, state):
        res = super().whole_pass(state)
        self.check_form()
        return res


@pytest.mark.parametrize('name,form', PAIRS)
def test_form_against_the_float64_twin(name, form, monkeypatch):
    for key in ('OSA_WIDE_SPLIT', 'OSA_LARGE_BATCH_BALANCED', 'OSA_CHUNKED_PASS', 'OSA_UPDATE_GRAPH'):
        monkeypatch.delenv(key, raising=False)
    for key, value in T.FORMS[form]['env'].items():
        monkeypatch.setenv(key, value)
    S.check_case(name, form, FormHarness(S.reference(name)['case'], form))
