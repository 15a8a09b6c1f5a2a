"""The persistent pass kernel against its own earlier build, bit for bit.

tests/golden/pass_trim_parent.npz holds what osa_ppo_pass of the commit BEFORE the instruction trim (select-free L2
term, 32-bit sample indices, dO broadcast on the VALU, two-dimension actor loss of the SO instantiations) wrote for
the seeded inputs below: parameters, both Adam moments, step counters and the
statistics rows.  The trim may change no rounding, no summation order and no formula, so every array must come out
equal (float compare: a zero of either sign is equal, any NaN fails).

Cases -- the smallest that reach every edited line:
  a  obs 60, act 2, B 64, M 232   the SO headline instantiation; 4 steps, the last ragged at 40 rows; PPO clip loss,
                                  critic L2 term and gradient clipping on, non-zero Lagrange multiplier
  b  the same, critic L2 term off, nets_mask = actor only (the critics' blocks must stay untouched)
  c  obs 17, act 6, B 64, M 200   non-SO, KB = 2 (MFMA output layer, six action dimensions, padded rows)
  d  obs 60, act 2, B 128, M 300  MULTI: two 64-row chunks per step, ragged last minibatch

The fixture is written by this file run as a script ON THAT EARLIER BUILD (python tests/test_pass_trim_gpu.py).
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURE = 'pass_trim_parent.npz'

CASES = {
    'a': dict(obs_dim=60, act_dim=2, B=64, M=232, critic_norm=1, nets_mask=7),
    'b': dict(obs_dim=60, act_dim=2, B=64, M=232, critic_norm=0, nets_mask=1),
    'c': dict(obs_dim=17, act_dim=6, B=64, M=200, critic_norm=1, nets_mask=7),
    'd': dict(obs_dim=60, act_dim=2, B=128, M=300, critic_norm=1, nets_mask=7),
}


def net_layout(obs_dim, act_dim, H=64):
    """osa_make_net (csrc/mlp_device.h): offsets of W1 | b1 | W2 | b2 | W3 | b3 | log_std in the padded block."""
    INP, OUTP = (obs_dim + 15) // 16 * 16, (max(act_dim, 1) + 15) // 16 * 16
    o = {'INP': INP, 'OUTP': OUTP, 'W1': 0}
    o['b1'] = o['W1'] + H * INP
    o['W2'] = o['b1'] + H
    o['b2'] = o['W2'] + H * H
    o['W3'] = o['b2'] + H
    o['b3'] = o['W3'] + OUTP * H
    o['LS'] = o['b3'] + OUTP
    o['P'] = o['LS'] + OUTP
    return o


def make_inputs(name):
    """Seeded host arrays of one case: RandomState streams only (no BLAS, nothing machine-dependent)."""
    c = CASES[name]
    od, ad, M, H = c['obs_dim'], c['act_dim'], c['M'], 64
    rs = np.random.RandomState(1234 + 17 * od + ad + M)
    L = net_layout(od, ad)
    P, INP = L['P'], L['INP']
    params = np.zeros((3, P), np.float32)
    mask = np.zeros((3, P), bool)  # the real (non-padding) entries
    for net in range(3):
        out = ad if net == 0 else 1
        w1 = mask[net, L['W1']:L['b1']].reshape(H, INP)
        w1[:, :od] = True
        mask[net, L['b1']:L['b2'] + H] = True  # b1, W2, b2
        mask[net, L['W3']:L['W3'] + out * H] = True
        mask[net, L['b3']:L['b3'] + out] = True
        if net == 0:
            mask[net, L['LS']:L['LS'] + ad] = True
    params[mask] = rs.uniform(-0.2, 0.2, int(mask.sum())).astype(np.float32)
    params[0, L['LS']:L['LS'] + ad] = np.linspace(-0.5, 0.3, ad).astype(np.float32)
    adam_m = np.zeros((3, P), np.float32)
    adam_v = np.zeros((3, P), np.float32)
    adam_m[mask] = (1e-3 * rs.randn(int(mask.sum()))).astype(np.float32)
    adam_v[mask] = (1e-5 * rs.uniform(0.1, 1.0, int(mask.sum()))).astype(np.float32)
    ld_obs = (od + 3) // 4 * 4  # rows of whole float4s (the host pads)
    obs = np.zeros((M, ld_obs), np.float32)
    obs[:, :od] = rs.randn(M, od).astype(np.float32)
    return dict(
        params=params, adam_m=adam_m, adam_v=adam_v, adam_step=np.array([3, 5, 7], np.int32), obs=obs,
        act=(0.5 * rs.randn(M, ad)).astype(np.float32),
        logp=(-1.0 * ad + 0.3 * rs.randn(M)).astype(np.float32),
        tgt_r=rs.randn(M).astype(np.float32), tgt_c=rs.randn(M).astype(np.float32),
        adv_r=rs.randn(M).astype(np.float32), adv_c=rs.randn(M).astype(np.float32),
        perm=rs.permutation(M).astype(np.int64))


def run_case(name):
    """One osa_ppo_pass launch on the case's inputs -> the arrays the launch wrote, as numpy."""
    import torch

    from omnisafe_amd import _lib
    from omnisafe_amd.models import HParams

    c = CASES[name]
    lib = _lib.load(require_gpu=True)
    h = make_inputs(name)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in h.items()}
    nmb = (c['M'] + c['B'] - 1) // c['B']
    stats = torch.zeros(nmb, 16, device=DEV)
    lam = torch.tensor([0.3], device=DEV)
    hp = HParams(clip=0.2, entropy_coef=0.01, critic_norm_coef=0.001, max_grad_norm=0.5, lr_actor=3e-4,
                 lr_critic=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-8, use_critic_norm=c['critic_norm'],
                 use_max_grad_norm=1, use_cost=1, lr_device=None)
    rc = lib.osa_ppo_pass(c['obs_dim'], c['act_dim'], 64, _lib.ptr(d['params']), _lib.ptr(d['adam_m']),
                          _lib.ptr(d['adam_v']), _lib.ptr(d['adam_step']), _lib.ptr(d['obs']), d['obs'].shape[1],
                          _lib.ptr(d['act']), c['act_dim'], _lib.ptr(d['logp']), _lib.ptr(d['tgt_r']),
                          _lib.ptr(d['tgt_c']), _lib.ptr(d['adv_r']), _lib.ptr(d['adv_c']), _lib.ptr(d['perm']),
                          c['M'], c['B'], _lib.ptr(lam), C.byref(hp), 0, c['nets_mask'], _lib.ptr(stats), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = {k: d[k].cpu().numpy() for k in ('params', 'adam_m', 'adam_v', 'adam_step')}
    out['stats'] = stats.cpu().numpy()
    return h, out


def stored(name, out):
    """What the fixture keeps of a case: everything, or (actor-only case) the actor's rows."""
    if CASES[name]['nets_mask'] == 7:
        return out
    return {k: (v if k == 'stats' else v[:1]) for k, v in out.items()}


@pytest.mark.parametrize('name', sorted(CASES))
def test_pass_is_bit_identical_to_the_build_before_the_trim(name, golden):
    g = golden(FIXTURE)
    h, out = run_case(name)
    for k, v in stored(name, out).items():
        want = g[f'{name}/{k}']
        assert v.shape == want.shape and v.dtype == want.dtype, (name, k)
        assert not np.isnan(v).any(), (name, k)
        assert np.array_equal(v, want), (name, k, int((v != want).sum()))
    if CASES[name]['nets_mask'] != 7:  # networks outside the mask: not a bit of them moves
        for k in ('params', 'adam_m', 'adam_v', 'adam_step'):
            assert np.array_equal(out[k][1:], h[k][1:]), (name, k)
    # the launch did something: four optimiser steps moved the actor
    assert not np.array_equal(out['params'][0], h['params'][0])
    assert out['adam_step'][0] == h['adam_step'][0] + out['stats'].shape[0]


if __name__ == '__main__':  # writes the fixture (run on the build the test is to be compared with)
    import sys

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', FIXTURE)
    blob = {}
    for nm in sorted(CASES):
        _, res = run_case(nm)
        assert all(np.isfinite(v).all() for v in res.values()), nm
        for key, val in stored(nm, res).items():
            blob[f'{nm}/{key}'] = val
    np.savez_compressed(dst, **blob)
    print(dst, os.path.getsize(dst), 'bytes')
