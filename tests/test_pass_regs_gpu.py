"""The 64-row pass step against the build before its sign-flip trim, bit for bit, in every mode of the body.

tests/golden/pass_regs_parent.npz holds what the commit BEFORE the trim wrote for the seeded inputs below (written by
tools/pass_regs_fixture.py on that build).  The trim (tanh' and Adam's first moment formed without the v_xor sign flips,
csrc/mlp_device.h: osa_one_minus_sq4, osa_adam_update4_scaled) may not change a rounding, a summation order or a
formula, so parameters, both Adam moments and the statistics rows must come out identical.  The plain small-output
pass runs the new forms; the other modes compile from the same body and must not have moved either.

Cases: obs 60 / act 2, minibatch B = 64, at three sizes
  M = 192  three chained optimiser steps
  M = 150  ragged last minibatch (22 rows)
  M = 64   one step
each on
  clip     osa_ppo_pass, all three networks, max_grad_norm below every step's gradient norm (clip factor < 1)
  noclip   osa_ppo_pass, all three networks, max_grad_norm above every step's gradient norm (clip factor = 1)
           -- both are asserted from the norms in the statistics rows, so both values of the scale ran
  ext      osa_ppo_pass_ext with the KL term and trust mask (actor)
  coop     osa_ppo_dp_pass, two virtual ranks on one device (actor + reward critic), slab tails included
  chunked  osa_ppo_chunked_pass; a chunked step needs B > 64, so B = 128 here (actor + reward critic)
  slabs    osa_ppo_dp_step on the LAST minibatch of the size (gradient-only slabs, then the averaging Adam step)
  nonso    osa_ppo_pass with act 3: the MFMA output layer instead of the small-output one (actor + reward critic)
and clip cases at M = 150 for the other widths of the first layer: obs 12 / act 1 (KB 1), obs 20, 40, 70 (KB 2, 3, 5:
the rewritten forms, as KB 1 and 4) and obs 90 (KB 6: the unchanged forms).

A run writes three arrays of P = 8 448 floats per network: the 63 network rows of the 26 runs would be 6 MB.  The
fixture therefore keeps the statistics rows, step counts and slab tails whole and a SHA-256 digest per network of the
BYTES of params, adam_m and adam_v (and of a gradient slab) -- equal digests are equal bits, stricter than a float
compare (a zero that changed sign fails).  A mismatch names the case, the network and the array.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from test_pass_stall_trim_gpu import NSTAT, net_layout, slab_tails

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURE = 'pass_regs_parent.npz'
SIZES = (192, 150, 64)
CLIP, NOCLIP = 0.02, 100.0  # max_grad_norm below / above the gradient norms of these inputs (asserted per step)

MODES = {
    'clip': dict(entry='plain', act_dim=2, B=64, world=1, nets_mask=7, mgn=CLIP),
    'noclip': dict(entry='plain', act_dim=2, B=64, world=1, nets_mask=7, mgn=NOCLIP),
    'ext': dict(entry='ext', act_dim=2, B=64, world=1, nets_mask=1, mgn=0.5),
    'coop': dict(entry='dp_pass', act_dim=2, B=64, world=2, nets_mask=3, mgn=0.5),
    'chunked': dict(entry='chunked', act_dim=2, B=128, world=1, nets_mask=3, mgn=0.5),
    'slabs': dict(entry='dp_step', act_dim=2, B=64, world=1, nets_mask=7, mgn=0.5),
    'nonso': dict(entry='plain', act_dim=3, B=64, world=1, nets_mask=3, mgn=0.5),
}
CASES = {f'{mode}-{M}': dict(c, obs_dim=60, M=M) for mode, c in MODES.items() for M in SIZES}
CASES['kb1-150'] = dict(MODES['clip'], obs_dim=12, act_dim=1, M=150)
# the other first-layer widths on both sides of the cut-off of the rewritten forms (KB <= 5 run them, KB = 6 does not)
for _kb, _od in ((2, 20), (3, 40), (5, 70), (6, 90)):
    CASES[f'kb{_kb}-150'] = dict(MODES['clip'], obs_dim=_od, M=150)
HASHED = ('params', 'adam_m', 'adam_v')


def make_inputs(name):
    """Seeded host arrays of one case (RandomState streams only): the layout of tests/test_pass_stall_trim_gpu.py."""
    c = CASES[name]
    od, ad, M, W, H = c['obs_dim'], c['act_dim'], c['M'], c['world'], 64
    rs = np.random.RandomState(977 + 31 * od + 7 * ad + M + 101 * W + sum(map(ord, name)))
    L = net_layout(od, ad)
    P, INP = L['P'], L['INP']
    params = np.zeros((3, P), np.float32)
    mask = np.zeros((3, P), bool)  # the real (non-padding) entries
    for net in range(3):
        out = ad if net == 0 else 1
        mask[net, L['W1']:L['b1']].reshape(H, INP)[:, :od] = True
        mask[net, L['b1']:L['b2'] + H] = True  # b1, W2, b2
        mask[net, L['W3']:L['W3'] + out * H] = True
        mask[net, L['b3']:L['b3'] + out] = True
        if net == 0:
            mask[net, L['LS']:L['LS'] + ad] = True
    n = int(mask.sum())
    params[mask] = rs.uniform(-0.2, 0.2, n).astype(np.float32)
    params[0, L['LS']:L['LS'] + ad] = np.linspace(-0.5, 0.3, ad).astype(np.float32)
    adam_m = np.zeros((3, P), np.float32)
    adam_v = np.zeros((3, P), np.float32)
    adam_m[mask] = (1e-3 * rs.randn(n)).astype(np.float32)
    adam_v[mask] = (1e-5 * rs.uniform(0.1, 1.0, n)).astype(np.float32)
    R = W * M
    obs = np.zeros((R, (od + 3) // 4 * 4), np.float32)  # rows of whole float4s (the host pads)
    obs[:, :od] = rs.randn(R, od).astype(np.float32)
    return dict(
        params=params, adam_m=adam_m, adam_v=adam_v, adam_step=np.array([3, 5, 7], np.int32), obs=obs,
        act=(0.5 * rs.randn(R, ad)).astype(np.float32),
        logp=(-1.0 * ad + 0.3 * rs.randn(R)).astype(np.float32),
        tgt_r=rs.randn(R).astype(np.float32), tgt_c=rs.randn(R).astype(np.float32),
        adv_r=rs.randn(R).astype(np.float32), adv_c=rs.randn(R).astype(np.float32),
        perm=np.stack([rs.permutation(M) for _ in range(W)]).astype(np.int64).reshape(-1),
        old_mean=(0.3 * rs.randn(R, ad)).astype(np.float32),
        old_log_std=np.linspace(-0.4, 0.2, ad).astype(np.float32))


def run_case(name):
    """One entry-point call on the case's inputs -> (inputs, the arrays the call wrote), as numpy."""
    import torch

    from omnisafe_amd import _lib
    from omnisafe_amd.models import HParams, SurrogateExt

    c = CASES[name]
    lib = _lib.load(require_gpu=True)
    h = make_inputs(name)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in h.items()}
    od, ad, M, B, W, mask = c['obs_dim'], c['act_dim'], c['M'], c['B'], c['world'], c['nets_mask']
    L = net_layout(od, ad)
    nmb = (M + B - 1) // B
    stats = torch.zeros(nmb, NSTAT, device=DEV)
    lam = torch.tensor([0.3], device=DEV)
    hp = HParams(clip=0.2, entropy_coef=0.01, critic_norm_coef=0.001, max_grad_norm=c['mgn'], lr_actor=3e-4,
                 lr_critic=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-8, use_critic_norm=1,
                 use_max_grad_norm=1, use_cost=1, lr_device=None)
    p = _lib.ptr
    head = (od, ad, 64, p(d['params']), p(d['adam_m']), p(d['adam_v']), p(d['adam_step']), p(d['obs']),
            d['obs'].shape[1], p(d['act']), ad, p(d['logp']), p(d['tgt_r']), p(d['tgt_c']), p(d['adv_r']),
            p(d['adv_c']), p(d['perm']), M, B)
    extra = {}
    if c['entry'] == 'plain':
        rc = lib.osa_ppo_pass(*head, p(lam), C.byref(hp), 0, mask, p(stats), None)
    elif c['entry'] == 'ext':
        ext = SurrogateExt(kl_coef=0.7, kl_mask_eta=0.5, ratio_scale=1.0 / 1.5)
        ext.old_mean, ext.ld_old_mean, ext.old_log_std = d['old_mean'].data_ptr(), ad, d['old_log_std'].data_ptr()
        rc = lib.osa_ppo_pass_ext(*head, p(lam), C.byref(hp), 1, mask, p(stats), C.byref(ext), None)
    elif c['entry'] in ('dp_pass', 'chunked'):
        peers = W if c['entry'] == 'dp_pass' else (B + 63) // 64
        xch = torch.zeros(lib.osa_ppo_dp_pass_ws_floats(od, ad, 64, peers), device=DEV)
        sync = torch.zeros(64, dtype=torch.int32, device=DEV)
        if c['entry'] == 'dp_pass':
            rc = lib.osa_ppo_dp_pass(*head, W, p(lam), C.byref(hp), 0, mask, p(xch), p(sync), p(stats), None)
        else:
            rc = lib.osa_ppo_chunked_pass(*head, p(lam), C.byref(hp), 0, mask, p(xch), p(sync), 0, p(stats), None)
        torch.cuda.synchronize()
        assert int(sync[3]) == 0, 'a cooperating workgroup never arrived'
        extra['tails'] = slab_tails(xch.cpu().numpy(), L, peers)
    else:  # dp_step: the gradient slabs of the last minibatch, then the averaging Adam kernel
        slabs = torch.zeros(lib.osa_ppo_dp_ws_floats(od, ad, 64, W), device=DEV)
        stats = torch.zeros(1, NSTAT, device=DEV)
        rc = lib.osa_ppo_dp_step(*head, W, nmb - 1, p(lam), C.byref(hp), None, 0, mask, p(slabs), p(stats), None)
        torch.cuda.synchronize()
        extra['slabs'] = slabs.cpu().numpy().reshape(3, W, L['P'] + NSTAT)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = {k: d[k].cpu().numpy() for k in HASHED + ('adam_step',)}
    out['stats'] = stats.cpu().numpy()
    out.update(extra)
    return h, out


def rows_of(name):
    return [n for n in range(3) if (CASES[name]['nets_mask'] >> n) & 1]


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def stored(name, out):
    """What the fixture keeps of a case: statistics, step counts and slab tails whole, a digest per network in the case's
    mask of every large array."""
    keep = {'stats': out['stats'], 'adam_step': out['adam_step']}
    if 'tails' in out:
        keep['tails'] = out['tails'][:, rows_of(name)]
    for n in rows_of(name):
        for k in HASHED + (('slabs',) if 'slabs' in out else ()):
            keep[f'{k}{n}'] = digest(out[k][n])
    return keep


def clip_factors_below_one(name, stats):
    """Per network and step: did the step's gradient norm (statistics columns 7, 8, 9) exceed max_grad_norm?"""
    return stats[:, 7:10] + 1e-6 > CASES[name]['mgn']


@pytest.mark.parametrize('name', sorted(CASES))
def test_pass_is_bit_identical_to_the_build_before_the_register_trim(name, golden):
    g = golden(FIXTURE)
    h, out = run_case(name)
    for k in HASHED:
        assert not np.isnan(out[k]).any(), (name, k)
    for k, v in stored(name, out).items():
        want = g[f'{name}/{k}']
        assert v.shape == want.shape and v.dtype == want.dtype, (name, k)
        assert np.array_equal(v, want), (name, k, int((v != want).sum()))
    off = [n for n in range(3) if n not in rows_of(name)]
    for k in HASHED + ('adam_step',):  # networks outside the mask: not a bit of them moves
        assert np.array_equal(out[k][off], h[k][off]), (name, k)
    assert not np.array_equal(out['params'][0], h['params'][0])  # the call did something
    if CASES[name]['entry'] != 'dp_step':  # (the per-step mode counts its steps in osa_ppo_dp_end_pass)
        assert out['adam_step'][0] == h['adam_step'][0] + out['stats'].shape[0]
    mode = name.split('-')[0]
    if mode == 'clip' or mode.startswith('kb'):
        assert clip_factors_below_one(name, out['stats']).all(), out['stats'][:, 7:10]
    if mode == 'noclip':
        assert not clip_factors_below_one(name, out['stats']).any(), out['stats'][:, 7:10]
