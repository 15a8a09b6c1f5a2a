"""The optimiser step of GENERAL networks -- the layer-wise path of csrc/general_mlp.hip + csrc/skinny_mlp.h, every
`hidden_sizes` and activation outside the fused [H, H] family -- against tests/step_twin.py, the float64 statement of
the same step, with the checks of tests/test_step_oracle_gpu.py (imported, not copied).

The cases are step_twin.general_table(): the smallest shapes that reach each mechanism of the path -- the skinny step
(B <= 64) with its two ways of fusing the top layer, the clip norm from Gram matrices (gs_gram_norm: a formula of its
own with a cancelling cross term, here set against the gradient the update applies), widths that are no multiple of
4 / 16 / 64, 0 to 7 hidden layers, the five activations, actor and critics of different depth and kind; the tiled step
with its weight-gradient splits, row splits (S = 4, S = 8, a problem with Si < S), loss blocks, and the instantiations
of gm_gemm_kernel the launcher's arithmetic selects.  tests/test_step_twin.py asserts on the CPU, from osa_gmlp_plan,
that every case reaches what it is named for, and lists the instantiations covered.

How a step is observed (as in the 64-row file, never through Adam's division):
  mode 0      PPOUpdater.minibatch from ZERO moments, every minibatch of the pass incl. the ragged tail: the clipped
              gradient is m' / (1 - b1), the clip factor |g_kernel| / the norm column of the statistics row -- on the
              fused skinny step that sets the APPLIED gradient against the Gram-formula norm -- v' = (1 - b2) g^2 to
              4 ulp, the statistics row, p' by check_adam; seeded moments and chains as there.  PPOUpdater.run takes
              this path through the captured pass: the seeded cases (one skinny, one tiled) run it eager, captured +
              replayed and replayed again, demand identical bits and judge the replay; last_path is 'general-per-step'.
  mode 2 / 1  osa_gmlp_minibatch_ext directly: the raw and the clipped gradient in ac.grads against the twin's, per
              reference tensor; parameters, moments and step counters bit-unchanged.
  dp step     mode 1 -> osa_gmlp_adam_apply, the data-parallel step's two halves at world size 1, as a second PATH of
              the same checks (`apply`): from zero moments m' / (1 - b1) is the mode-1 gradient, from seeded moments
              m', v' are the recurrences on it (check_seeded_step), p' by check_adam, counters by check_structure.
  scratch     before every observed launch the whole of ac.gmlp_ws is filled with NaN: a kernel that reads scratch it
              never wrote (padding columns that are 'zero by construction') shows as a NaN or a wrong number.  Padding
              entries of params / m / v / grads stay exactly 0, networks outside the mask keep their bits.

Tolerances: the project's unit max(e32, 2^-22) per reference tensor and scalar with the output-bias extension, e32 from
tests/golden/general_twin_f32_error.json (the float32 twin against the float64 twin: tools/step_twin_report.py
--general-golden, reproduced by tests/test_step_twin.py), K_GRAD = K_SCALAR = 16 of the 64-row file.  Nothing was
measured on the kernels to set a bound.  The clipped gradient of mode 1 is the raw gradient times the clip factor: its
bound is the sum of the two relative bounds, K_GRAD unit(tensor) + K_SCALAR unit(gnorm) where the clip bites.
profiles/general_twin_error.md has the measured ratios.  No element is excluded anywhere.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import step_twin as T
import test_step_oracle_gpu as S

pytestmark = pytest.mark.gpu
DEV = S.DEV
TABLE = T.general_table()
S.CASES.update({_name: _e['kw'] for _name, _e in TABLE.items()})
_E32 = T.load_general_error(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'general_twin_f32_error.json'))
S.E32.update(_E32[0])
S.E32_SINGLE.update(_E32[1])
NAN = float('nan')
# the data-parallel step's two halves: the seeded cases, both ways of finding the norm on the skinny step, a split tiled one
APPLY_CASES = ('sk-seeded', 'tl-B130-tail', 'sk-base', 'sk-a33-normclip-all', 'sk-normclip-reward_critic', 'tl-B300')


@pytest.fixture(scope='module', autouse=True)
def _figures():
    """The figures of THIS module's cases (OSA_STEP_TWIN_FIGURES: one of the twin files per run)."""
    start = len(S.FIGURES)
    yield
    dst = os.environ.get('OSA_STEP_TWIN_FIGURES')
    if dst:
        with open(dst, 'w') as fh:
            json.dump(S.FIGURES[start:], fh)


class GeneralHarness(S.Harness):
    """S.Harness on general networks: a step is PPOUpdater.minibatch (-> osa_gmlp_minibatch_ext, mode 0)."""

    def form(self):
        return False, 'general-per-step', False, False

    def __init__(self, name, path):
        case = S.reference(name)['case']
        super().__init__(case, path)
        assert self.ac.general and self.upd.general
        # one allocation for every call of the case (a captured pass bakes the scratch's address in); the scratch of
        # a skinny step is carved differently and can be the larger one, so every row count of the case is asked for
        for rows in sorted({case['M'], case['B']} | {n for _, n in T.minibatches(case['M'], case['B'])}):
            self.ws = self.ac.gmlp_ws(rows)[0]
        # the process is where the CPU test saw the case: the plan still names the case's features
        assert T.plan_features(T.gmlp_plan(case)) >= set(TABLE[name]['features'])

    def poison(self):
        assert self.ac._gws is self.ws
        self.ws.fill_(NAN)

    def launch_step(self, k):
        s, n = T.minibatches(self.case['M'], self.case['B'])[k]
        stats = torch.zeros(1, S.NSTAT, device=DEV)
        self.poison()
        self.upd.minibatch(self.data, self.perm[s:s + n], n, self.lam, stats[0])
        torch.cuda.synchronize()
        return stats[0].cpu().numpy()

    def whole_pass(self, state):
        self.poison()
        res = super().whole_pass(state)
        if self.case['seeded_moments'] and self.upd.ext is None:
            # eager, captured + replayed, replayed: the same bits; what the caller judges is the replay
            for _ in range(2):
                self.poison()
                again = super().whole_pass(state)
                for which, blk in res[1]['blocks'].items():
                    assert np.array_equal(blk, again[1]['blocks'][which]), (which, 'graph replay against the eager pass')
                assert np.array_equal(res[2], again[2]) and res[1]['t'] == again[1]['t']
            assert self.upd._graphed_pass and self.upd._ug.get('graph') is not None
            res = again
        return res

    # ---- osa_gmlp_minibatch_ext by hand: modes 1 and 2
    def gradient_call(self, k, mode):
        """Minibatch k in `mode` on the state the device holds -> (ac.grads [3][P], statistics row)."""
        upd, lib, ac = self.upd, self._lib, self.ac
        s, n = T.minibatches(self.case['M'], self.case['B'])[k]
        idx = self.perm[s:s + n]
        stats = torch.zeros(1, S.NSTAT, device=DEV)
        ext = None
        if upd.ext is not None:
            upd.ext.old_mean, upd.ext.ld_old_mean = upd._old_mean.data_ptr(), upd._old_mean.stride(0)
            upd.ext.old_log_std = upd._old_log_std.data_ptr()
            ext = C.byref(upd.ext)
        ws, nws = ac.gmlp_ws(n)
        assert ws is self.ws
        self.poison()
        d = self.data
        lib.check(upd.lib.osa_gmlp_minibatch_ext(
            C.byref(ac.desc), lib.ptr(ac.params), lib.ptr(ac.adam_m), lib.ptr(ac.adam_v), lib.ptr(ac.adam_step),
            lib.ptr(ac.grads), lib.ptr(d['obs']), d['obs'].stride(0), lib.ptr(d['act']), d['act'].stride(0),
            lib.ptr(d['logp']), lib.ptr(d['target_value_r']), lib.ptr(d['target_value_c']), lib.ptr(d['adv_r']),
            lib.ptr(d['adv_c']), lib.ptr(idx), n, lib.ptr(self.lam), C.byref(upd.hp), upd.loss_kind, mode, self.mask,
            None, 0.0, lib.ptr(ws), nws, lib.ptr(stats), ext, lib.stream_ptr()), 'osa_gmlp_minibatch_ext')
        torch.cuda.synchronize()
        return ac.grads.cpu().numpy(), stats[0].cpu().numpy()

    def split(self, block, i, net):
        """One network's padded block -> {reference tensor: array}."""
        flat, o, d = block[self.index[i]], 0, {}
        for k, s in T.case_shapes(self.case, net).items():
            n = int(np.prod(s))
            d[k] = flat[o:o + n].reshape(s).astype(np.float64)
            o += n
        return d


class ApplyHarness(GeneralHarness):
    """The data-parallel step at world size 1: mode 1 (clipped gradient into ac.grads), then osa_gmlp_adam_apply."""

    def launch_step(self, k):
        ac, lib, upd = self.ac, self._lib, self.upd
        _, stats = self.gradient_call(k, 1)
        lib.check(upd.lib.osa_gmlp_adam_apply(C.byref(ac.desc), lib.ptr(ac.params), lib.ptr(ac.adam_m), lib.ptr(ac.adam_v),
                                              lib.ptr(ac.adam_step), lib.ptr(ac.grads), C.byref(upd.hp), self.mask,
                                              lib.ptr(ac._gfin), lib.stream_ptr()), 'osa_gmlp_adam_apply')
        torch.cuda.synchronize()
        return stats

    def whole_pass(self, state):
        self.load(state)
        before = self.read()
        stats = [self.launch_step(k) for k in range(len(T.minibatches(self.case['M'], self.case['B'])))]
        return before, self.read(), np.stack(stats)


def _env(monkeypatch, name):
    for key in ('OSA_GMLP_SKINNY', 'OSA_GMLP_NORM_FUSE', 'OSA_UPDATE_GRAPH', 'OSA_FORCE_GENERAL_MLP'):
        monkeypatch.delenv(key, raising=False)
    for key, value in TABLE[name]['env'].items():
        monkeypatch.setenv(key, value)


@pytest.mark.parametrize('name', list(TABLE))
def test_general_step_against_the_float64_twin(name, monkeypatch):
    _env(monkeypatch, name)
    S.check_case(name, 'general', GeneralHarness(name, 'general'))


@pytest.mark.parametrize('name', APPLY_CASES)
def test_gradient_then_adam_apply_against_the_float64_twin(name, monkeypatch):
    _env(monkeypatch, name)
    S.check_case(name, 'apply', ApplyHarness(name, 'apply'))


@pytest.mark.parametrize('name', list(TABLE))
def test_raw_and_clipped_gradients_against_the_float64_twin(name, monkeypatch):
    """Modes 2 and 1 of osa_gmlp_minibatch_ext on the first and the last minibatch of the pass."""
    _env(monkeypatch, name)
    h = GeneralHarness(name, 'general')
    ref = S.reference(name)
    zero, e32 = ref['zero'], S.E32[name]
    nmb = len(T.minibatches(h.case['M'], h.case['B']))
    failures = []
    for k in sorted({0, nmb - 1}):
        r = ref['first'][k]
        for mode in (2, 1):
            h.load(zero['state'])
            sentinel = torch.full_like(h.ac.grads, 0.0)
            for i, net in enumerate(T.NETS):
                if net not in h.nets:
                    sentinel[i, torch.from_numpy(h.index[i]).to(DEV)] = 7.0
            h.ac.grads.copy_(sentinel)
            before = h.read()
            grads, stats = h.gradient_call(k, mode)
            after = h.read()
            for which in ('params', 'm', 'v'):  # a gradient call moves no state
                assert np.array_equal(after['blocks'][which], before['blocks'][which]), (mode, which)
            assert after['t'] == before['t'], (mode, after['t'])
            assert np.isfinite(grads).all() and np.isfinite(stats).all(), (mode, 'NaN: scratch read before it was written')
            kind = f'step{k}/mode{mode}'
            S.check_scalars(name, 'general', kind, r, stats, e32, failures)
            for i, net in enumerate(T.NETS):
                real = np.zeros(grads.shape[1], bool)
                real[h.index[i]] = True
                assert (grads[i][~real] == 0).all(), (mode, net, 'padding of grads moved')
                if net not in h.nets:
                    assert np.array_equal(grads[i], sentinel[i].cpu().numpy()), (mode, net, 'grads outside the mask')
                    continue
                coef = float(r[net]['coef']) if mode == 1 else 1.0
                extra = S.K_SCALAR * S.unit(e32, net, 'gnorm') if coef < 1.0 else 0.0
                for t, got in h.split(grads[i], i, net).items():
                    err = T.rel_l2(got, r[net]['grads'][t].numpy() * coef)
                    u = S.unit(e32, net, t)
                    bound = S.K_GRAD + extra / u
                    # (recorded in units of K_GRAD: a clipped tensor's ratio rescaled by K_GRAD / its own bound)
                    S.record(name, 'general', kind + '/grad', net, t, err / u * S.K_GRAD / bound, S.K_GRAD,
                             err / S.unit(S.E32_SINGLE[name], net, t))
                    if not err <= bound * u:
                        failures.append((kind, net, t, 'gradient rel l2 / max(e32, 2^-22)', err / u, bound))
    assert not failures, failures


def test_masked_extensions_above_256_rows_are_refused_before_any_launch():
    """FOCOPS's trust mask and P3O's penalty are minibatch-level quantities of one 256-row loss block: a general network
    with B > 256 raises when the updater is built, and the library refuses the call without touching the state."""
    from omnisafe_amd import _lib
    from omnisafe_amd.models import ConstraintActorCritic, SurrogateExt
    from omnisafe_amd.spaces import Box
    from omnisafe_amd.update import PPOUpdater

    case = dict(T.GENERAL_TILED, obs_dim=20, act_dim=3)
    ac = ConstraintActorCritic(Box(-np.inf, np.inf, (20,)), Box(-1, 1, (3,)), S.model_cfgs(case), 4, device=DEV)
    for ext in (SurrogateExt(kl_coef=1.0, kl_mask_eta=0.5), SurrogateExt(cost_kappa=2.0)):
        with pytest.raises(NotImplementedError):
            PPOUpdater(ac, batch_size=257, update_iters=1, target_kl=0.02, kl_early_stop=False, ext=ext)
        upd = PPOUpdater(ac, batch_size=256, update_iters=1, target_kl=0.02, kl_early_stop=False, ext=ext)
        n = 257
        z = torch.zeros(n, 20, device=DEV)
        v = torch.zeros(n, device=DEV)
        a = torch.zeros(n, 3, device=DEV)
        ext.old_mean, ext.ld_old_mean, ext.old_log_std = a.data_ptr(), 3, v.data_ptr()
        ws, nws = ac.gmlp_ws(n)
        ws.fill_(NAN)
        ac.adam_step.fill_(5)
        params = ac.params.clone()
        stats = torch.zeros(S.NSTAT, device=DEV)
        rc = upd.lib.osa_gmlp_minibatch_ext(
            C.byref(ac.desc), _lib.ptr(ac.params), _lib.ptr(ac.adam_m), _lib.ptr(ac.adam_v), _lib.ptr(ac.adam_step),
            _lib.ptr(ac.grads), _lib.ptr(z), 20, _lib.ptr(a), 3, _lib.ptr(v), _lib.ptr(v), _lib.ptr(v), _lib.ptr(v),
            _lib.ptr(v), None, n, _lib.ptr(v), C.byref(upd.hp), 1, 0, 7, None, 0.0, _lib.ptr(ws), nws, _lib.ptr(stats),
            C.byref(ext), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0
        assert torch.equal(ac.params, params) and ac.adam_step.tolist() == [5, 5, 5]
        assert bool(torch.isnan(ws).all()) and not bool(ac.adam_m.any())
