"""The other instantiations of the persistent pass body against their own earlier build, bit for bit.

tests/test_pass_trim_gpu.py pins osa_ppo_pass (SO headline, actor only, non-SO KB = 2, MULTI).  The stall trim of the
64-row step (the actor of the plain pass skips the L2 term and the sum of squared parameters nobody reads; the
small-output backward requests its W3 rows together) edits the one body every mode compiles from, so this file pins the
modes that fixture does not reach.  tests/golden/pass_stall_trim_parent.npz holds what the commit BEFORE the trim wrote
for the seeded inputs below; no rounding, summation order or formula may change, so every array must come out equal
(float compare: a zero of either sign is equal, any NaN fails).

Cases -- the smallest that reach the edited lines, one entry-point call each:
  e  osa_ppo_pass_ext      obs 60, act 2, B 64, M 232   EXT: KL term (kl_coef != 0) and trust mask (kl_mask_eta >= 0), whose
                                                        loss keeps the shuffle and its own terms; actor only (the critics of
                                                        an extended pass run the plain body of case a of the other file)
  f  osa_ppo_dp_pass       obs 60, act 2, B 64, M 200   COOP, two virtual ranks on one device: the sum of squared parameters
                                                        must still be published -- the critic's statistics column and the
                                                        tail of every slab, the actor's included
  g  osa_ppo_chunked_pass  obs 60, act 2, B 128, M 300  chunk mode: the L2 term belongs to chunk 0 only
  h  osa_ppo_dp_step       obs 60, act 2, B 64, M 128   gradient-only slabs (DPS), slab[P + 2] included; second minibatch
  i  osa_ppo_pass          obs 27, act 8, B 64, M 200   non-SO (MFMA output layer) with the critic L2 term on

f, g and i run the actor and the reward critic (the cost critic executes the reward critic's code on another target
column), which keeps the fixture under 1 MB; the networks outside a mask must not move.

The fixture is written by this file run as a script ON THAT EARLIER BUILD (OSA_LIB_PATH selects the library, as
tools/ab_pass.sh builds it):  OSA_LIB_PATH=omnisafe_amd/lib/libomnisafe_amd_base.so python tests/test_pass_stall_trim_gpu.py
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIXTURE = 'pass_stall_trim_parent.npz'
NSTAT = 16

CASES = {
    'e': dict(entry='ext', obs_dim=60, act_dim=2, B=64, M=232, world=1, nets_mask=1),
    'f': dict(entry='dp_pass', obs_dim=60, act_dim=2, B=64, M=200, world=2, nets_mask=3),
    'g': dict(entry='chunked', obs_dim=60, act_dim=2, B=128, M=300, world=1, nets_mask=3),
    'h': dict(entry='dp_step', obs_dim=60, act_dim=2, B=64, M=128, world=1, nets_mask=7),
    'i': dict(entry='plain', obs_dim=27, act_dim=8, B=64, M=200, world=1, nets_mask=3),
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
    """Seeded host arrays of one case: RandomState streams only (no BLAS, nothing machine-dependent).  The data
    arrays hold world * M rows (the all-gathered layout of the data-parallel modes), perm one permutation of the
    M local rows per virtual rank."""
    c = CASES[name]
    od, ad, M, W, H = c['obs_dim'], c['act_dim'], c['M'], c['world'], 64
    rs = np.random.RandomState(4321 + 17 * od + ad + M + 101 * W + ord(name))
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
    R = W * M
    ld_obs = (od + 3) // 4 * 4  # rows of whole float4s (the host pads)
    obs = np.zeros((R, ld_obs), np.float32)
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


def slab_tails(xch, L, peers):
    """Tails (statistics, clip factor) of the exchange slabs of a cooperative pass: [2 parities][3][peers][16]."""
    XS = (4 + L['INP'] // 16 + L['OUTP'] // 16) * 1024 + 256 + NSTAT
    body = xch[:2 * 3 * peers * XS].reshape(2, 3, peers, XS)
    return np.ascontiguousarray(body[..., XS - NSTAT:])


def run_case(name):
    """One entry-point call on the case's inputs -> the arrays the call wrote, as numpy."""
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
    hp = HParams(clip=0.2, entropy_coef=0.01, critic_norm_coef=0.001, max_grad_norm=0.5, lr_actor=3e-4,
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
        if c['entry'] == 'dp_pass':  # (spread grid, ordinary memory: no placement protocol)
            rc = lib.osa_ppo_dp_pass(*head, W, p(lam), C.byref(hp), 0, mask, p(xch), p(sync), p(stats), None)
        else:
            rc = lib.osa_ppo_chunked_pass(*head, p(lam), C.byref(hp), 0, mask, p(xch), p(sync), 0, p(stats), None)
        torch.cuda.synchronize()
        assert int(sync[3]) == 0, 'a cooperating workgroup never arrived'
        extra['tails'] = slab_tails(xch.cpu().numpy(), L, peers)
    else:  # dp_step: the gradient slabs of minibatch 1, then the averaging Adam kernel
        slabs = torch.zeros(lib.osa_ppo_dp_ws_floats(od, ad, 64, W), device=DEV)
        stats = torch.zeros(1, NSTAT, device=DEV)
        rc = lib.osa_ppo_dp_step(*head, W, 1, p(lam), C.byref(hp), None, 0, mask, p(slabs), p(stats), None)
        torch.cuda.synchronize()
        extra['slabs'] = slabs.cpu().numpy().reshape(3, W, L['P'] + NSTAT)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = {k: d[k].cpu().numpy() for k in ('params', 'adam_m', 'adam_v', 'adam_step')}
    out['stats'] = stats.cpu().numpy()
    out.update(extra)
    return h, out


def rows_of(name):
    return [n for n in range(3) if (CASES[name]['nets_mask'] >> n) & 1]


def stored(name, out):
    """What the fixture keeps of a case: the rows of the networks in the case's mask."""
    r = rows_of(name)
    keep = {}
    for k, v in out.items():
        if k == 'stats':
            keep[k] = v
        elif k == 'tails':
            keep[k] = v[:, r]
        else:
            keep[k] = v[r]
    return keep


@pytest.mark.parametrize('name', sorted(CASES))
def test_pass_mode_is_bit_identical_to_the_build_before_the_stall_trim(name, golden):
    g = golden(FIXTURE)
    h, out = run_case(name)
    for k, v in stored(name, out).items():
        want = g[f'{name}/{k}']
        assert v.shape == want.shape and v.dtype == want.dtype, (name, k)
        assert not np.isnan(v).any(), (name, k)
        assert np.array_equal(v, want), (name, k, int((v != want).sum()))
    off = [n for n in range(3) if n not in rows_of(name)]
    for k in ('params', 'adam_m', 'adam_v', 'adam_step'):  # networks outside the mask: not a bit of them moves
        assert np.array_equal(out[k][off], h[k][off]), (name, k)
    # the call did something: the actor moved
    assert not np.array_equal(out['params'][0], h['params'][0])
    if CASES[name]['entry'] != 'dp_step':  # (the per-step mode counts its steps in osa_ppo_dp_end_pass)
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
