"""GPU: what surrounds the TD3 / DDPG step (csrc/td3_kernels.hip) -- osa_td3_act against a float64 forward with its
Philox draws restated on the host, osa_td3_draws equal to the host's Philox, osa_td3_store against a numpy ring with the
episode accounting restated in float32 in the kernel's order.  The step itself: test_td3_gpu.py.

Bounds: the forward of osa_td3_act 16 float32 ulps in rel_l2 (test_sac_gpu.py's for the same kind of kernel); every
draw, index, ring row and episode sum exact."""
import functools

import numpy as np
import pytest
import torch
from nav_twin import philox4x32_10, u01
from test_sac_gpu import host_normal
from test_td3_gpu import ACT, GAMMA, LR, POLYAK, rel_l2

pytestmark = pytest.mark.gpu

KEY_IDX, KEY_EPS, KEY_ACT = 0x54443349445831, 0x54443345505331, 0x54443341435431
SEED, OFFSET, SENTINEL = 0x1234ABCD5678, 3, -7.0
ACTORS = {
    'small': (5, 3, [24, 40], 'relu'),       # K below one lane stride of 64, N no multiple of the 4 waves
    'big': (70, 32, [260, 9, 130], 'tanh'),  # K over two strides and a tail, a width above 256, both buffer parities
}


@functools.lru_cache(maxsize=None)
def actor_problem(name, n):
    """Weights, the observations as a column slice of a wider tensor, and the float64 forward."""
    from omnisafe_amd.crr_step import _init_mlp

    D, A, hid, act = ACTORS[name]
    torch.manual_seed(11)
    p = [t.detach() for wb in _init_mlp([D] + hid + [A], 'kaiming_uniform') for t in wb]
    p[-2] *= 4.0  # a head that reaches both ends of the action box under noise
    wide = torch.rand(n, D + 5, generator=torch.Generator().manual_seed(12)) * 2 - 1
    x = wide[:, 2:2 + D].double()
    for l in range(0, len(p), 2):
        x = x @ p[l].double().T + p[l + 1].double()
        x = ACT[act](x) if l + 2 < len(p) else torch.tanh(x)
    return p, wide, x.numpy()


def run_act(name, n, **kw):
    """``act`` of a strided ``obs`` into a column slice of a sentinel-filled tensor; the slice, after the check that
    every other column is untouched."""
    from omnisafe_amd import td3_step

    D, A, hid, act = ACTORS[name]
    p, wide, _ = actor_problem(name, n)
    actor = td3_step.Td3Actor(td3_step.make_desc(D, A, hid, hid, act, 'relu'), 'cuda:0')
    actor.load_state_dict({f'net.{2 * (i // 2)}.{"weight" if i % 2 == 0 else "bias"}': t for i, t in enumerate(p)})
    obs = wide.cuda()[:, 2:2 + D]
    assert obs.stride(0) == D + 5
    box = torch.full((n, A + 3), SENTINEL, device='cuda:0')
    actor.act(obs, out=box[:, 1:1 + A], **kw)
    box = box.cpu().numpy()
    assert np.all(box[:, :1] == SENTINEL) and np.all(box[:, 1 + A:] == SENTINEL)
    return box[:, 1:1 + A]


@pytest.mark.parametrize('n', [9, 1024])
@pytest.mark.parametrize('name', list(ACTORS))
def test_act_matches_the_formula(name, n):
    """Deterministic, noisy and random acting: Philox(seed ^ key, offset, row act_dim + column)."""
    A = ACTORS[name][1]
    a = actor_problem(name, n)[2]
    bound = 16 * 2.0 ** -23
    assert rel_l2(run_act(name, n), a) < bound

    eps, w = host_normal(SEED ^ KEY_ACT, OFFSET, n * A)
    pre = a + 0.8 * eps.astype(np.float64).reshape(n, A)
    want = np.clip(pre, -1.0, 1.0)
    hi, lo = pre > 1.0 + 1e-4, pre < -1.0 - 1e-4  # clamped whatever the float32 rounding
    assert hi.any() and lo.any() and (np.abs(pre) < 1.0 - 1e-4).any()
    got = run_act(name, n, noise=0.8, seed=SEED, offset=OFFSET)
    assert rel_l2(got, want) < bound
    assert np.all(got[hi] == 1.0) and np.all(got[lo] == -1.0)
    assert np.array_equal(got, run_act(name, n, noise=0.8, seed=SEED, offset=OFFSET))
    assert not np.array_equal(got, run_act(name, n, noise=0.8, seed=SEED, offset=OFFSET + 1))

    got = run_act(name, n, random=True, seed=SEED, offset=OFFSET)
    assert np.array_equal(got.ravel(), np.float32(2) * u01(w[:, 0]) - np.float32(1))
    assert not np.array_equal(got, run_act(name, n, random=True, seed=SEED, offset=OFFSET + 1))


def make_step(B=37, A=3, D=5, size=64, nslots=8):
    from omnisafe_amd import td3_step

    return td3_step.Td3Step(td3_step.make_desc(D, A, [8], [8], 'relu', 'relu', B), size=size, gamma=GAMMA,
                            polyak=POLYAK, lr_actor=LR, lr_critic=LR, nslots=nslots)


@pytest.mark.parametrize('pos', [(41, 41), (0, 0), (5, 64)])  # part full; empty: every index 0; full and wrapped
def test_draws_equal_the_host_philox(pos):
    """osa_td3_draws: idx [nslots][B] = (w0 | w1 << 32) fill >> 64 from the idx key, eps [nslots][B][A] from the eps
    key, counter (step, element), step s in slot s % nslots -- 5 steps from step 7 through 8 slots, so the slots wrap."""
    B, A, nslots, first, n = 37, 3, 8, 7, 5
    st = make_step(B, A, nslots=nslots)
    st.idx.fill_(-1)
    st.eps.fill_(SENTINEL)
    st.pos.copy_(torch.tensor(pos))
    st.draw(SEED, first, n)
    fill, seen = pos[1], []
    for k in range(n):
        step, slot = first + k, (first + k) % nslots
        w = philox4x32_10(SEED ^ KEY_IDX, step, np.arange(B))
        want = [((int(a) | (int(b) << 32)) * fill) >> 64 for a, b in zip(w[:, 0], w[:, 1])]
        assert st.idx[slot].tolist() == want
        seen += want
        eps, _ = host_normal(SEED ^ KEY_EPS, step, B * A)
        assert np.array_equal(st.eps[slot].cpu().numpy().reshape(-1), eps)
    assert max(seen) >= 5 if pos == (5, 64) else max(seen) < max(fill, 1)  # below the fill count, not the position
    idle = [s for s in range(nslots) if s not in [(first + k) % nslots for k in range(n)]]
    assert bool((st.idx[idle] == -1).all()) and bool((st.eps[idle] == SENTINEL).all())


def test_store_matches_a_numpy_ring_and_counts_episodes():
    """osa_td3_store over a ring of 512 rows from 3 envs: done = terminated alone, an episode ends on terminated or
    truncated; final_obs replaces next_obs where its mask byte is set, ending row or not, and not at all when it is
    None; every input a column slice of a wider tensor.  Episodes: acc [3][3], out [4][3], count -- 6 finish, two of
    them in one store; float32 sums in the kernel's order, so equality is exact."""
    n, size, D, A, cap = 3, 512, 4, 2, 4
    st = make_step(16, A, D, size=size, nslots=2)
    rng = np.random.default_rng(0)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    want = {k: np.zeros((size, w), np.float32) for k, w in (('obs', D), ('act', A), ('next_obs', D), ('reward', 1),
                                                             ('cost', 1), ('done', 1))}
    dev = lambda x: torch.as_tensor(x).cuda()
    sl = lambda x: dev(np.pad(x, ((0, 0), (1, 2)), constant_values=SENTINEL))[:, 1:1 + x.shape[1]]
    acc, out, count = torch.zeros(n, 3).cuda(), torch.full((cap + 2, 3), SENTINEL).cuda(), torch.zeros(1).long().cuda()
    h_acc, h_out, pos = np.zeros((n, 3), np.float32), [], 0
    #        terminated  truncated  final_mask  final_obs given
    plan = [((0, 0, 0), (0, 0, 0), (0, 0, 0), True),
            ((0, 1, 0), (0, 0, 0), (0, 1, 0), True),    # env 1 terminates
            ((0, 0, 0), (1, 0, 0), (1, 0, 1), True),    # env 0 is truncated: done 0; env 2's mask byte on a running row
            ((0, 0, 0), (0, 0, 0), (0, 0, 0), False),   # no final_obs at all
            ((1, 0, 0), (0, 0, 1), (1, 0, 1), True),    # two episodes end in one store
            ((0, 1, 0), (0, 1, 0), (0, 1, 0), False),   # both flags; the mask is not read without final_obs
            ((0, 0, 1), (0, 0, 0), (0, 0, 1), True)]    # the sixth episode: past cap = 4

    def store(m, term, trunc, mask, with_final, episodes):
        nonlocal pos
        rows = {key: f32(m, v.shape[1]) for key, v in want.items()}
        final = f32(m, D)
        st.store(sl(rows['obs']), sl(rows['act']), dev(rows['reward'][:, 0]), dev(rows['cost'][:, 0]), dev(term),
                 dev(trunc), sl(rows['next_obs']), sl(final) if with_final else None, dev(mask) if with_final else None,
                 episodes)
        rows['done'] = term.astype(np.float32)[:, None]
        if with_final:
            rows['next_obs'][mask != 0] = final[mask != 0]
        for i in range(m):
            for key in want:
                want[key][(pos + i) % size] = rows[key][i]
        pos += m
        return rows

    for term, trunc, mask, with_final in plan:
        term, trunc, mask = (np.array(x, np.uint8) for x in (term, trunc, mask))
        rows = store(n, term, trunc, mask, with_final, (acc, out[:cap], count))
        for i in range(n):  # the envs in order, float32 sums
            h_acc[i] += np.array([rows['reward'][i, 0], rows['cost'][i, 0], 1.0], np.float32)
            if term[i] or trunc[i]:
                h_out.append(h_acc[i].copy())
                h_acc[i] = 0.0
    assert len(h_out) == 6 and int(count) == 6
    assert np.array_equal(out[:cap].cpu().numpy(), np.stack(h_out[:cap]))
    assert bool((out[cap:] == SENTINEL).all())  # rows past cap are unwritten
    assert np.array_equal(acc.cpu().numpy(), h_acc) and np.any(h_acc[:, 2] > 0) and np.any(h_acc[:, 2] == 0)

    def ring_matches(position, fill):
        assert st.pos.tolist() == [position, fill]
        for key, v in want.items():
            assert np.array_equal(st.ring[key].cpu().numpy().reshape(size, -1), v), key

    ring_matches(pos, pos)
    # 300 rows in one launch: past one trip of both loops of the one-workgroup kernel; then n = size, which wraps
    for m in (300, size):
        flags = (rng.random((3, m)) < 0.3).astype(np.uint8)
        store(m, flags[0], flags[1], flags[2], True, None)
        ring_matches(pos % size, min(pos, size))
