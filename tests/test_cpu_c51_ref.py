"""The references of the categorical DQN kernels and the inputs of their GPU tests (host only).

tests/test_gpu_c51_edges.py compares dqn_dist_kernels.hip with c51_td_loop of
tests/c51_ref.py on the inputs of c51_ref.families(), on the bar of
_fp32_as_good_as_torch with c51_td in float32 as the fp32 reference.  Here

  * the two references (torch scatter form, plain-loop gather form) are checked
    against each other in float64 and against what they must satisfy: m sums to
    1, its mean is the Bellman mean where nothing is clamped, the closed-form
    gradients are autograd's, gather equals scatter at integer b too;
  * the inputs are shown to reach what they are meant to reach: both sides of
    both clamps of Tz, a row with every b_j an integer and one with every b_j at
    a half, terminal rows, exact ties of Q(s') on the designated rows and no
    near-tie anywhere else;
  * torch in float32 is shown to stay inside the bar on those inputs, so a
    correct fp32 kernel can meet it;
  * a NaN reward or done gives a NaN row in both references and moves no other
    row.
"""
import math

import numpy as np
import pytest
import torch

from tests import c51_ref as C
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

FAMILIES = C.families()
F64 = torch.float64


def _forms(kw):
    """the (double_q, weighted) pairs the GPU file runs a family with: both of each"""
    return [(1, 1), (0, 0)]


@pytest.mark.parametrize('name', sorted(FAMILIES))
def test_references_agree_and_inputs_hold(name):
    kw = FAMILIES[name]
    c, (A, N, v_min, v_max, gamma) = C.family(**kw), C.params(kw)
    B, ties = kw['B'], C.tie_rows(kw['B'], A)
    assert len(ties) <= 3
    for double_q, weighted in _forms(kw):
        r32, r64, loop = C.refs(kw, double_q, weighted)
        # ---- the two references, float64
        assert np.array_equal(loop['astar'], r64['astar'].numpy())
        # 1e-12 of the tensor's scale where that exceeds 1: q_sel reaches 1000 on the
        # [-1000, 1000] support, where fp64 eps times the scale times N is 1e-11 absolute
        for k in ('q_sel', 'm', 'td', 'dadv', 'stats') + (('dval',) if kw['dueling'] else ()):
            got, want = np.asarray(loop[k]), r64[k].detach().numpy()
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (k, double_q)
        assert (r64['dval'] is None) == (loop['dval'] is None)
        # ---- what m is
        m, tz, b = loop['m'], loop['tz'], loop['b']
        assert np.abs(m.sum(1) - 1.0).max() <= 1e-12
        z = np.array(C._support_list(N, v_min, v_max)[0])
        free = ((tz >= v_min) & (tz <= v_max)).all(1)
        pt = torch.softmax(C.logits(c['t'][0].double(), None if c['t'][1] is None else c['t'][1].double(),
                                    A, N), 2)[torch.arange(B), r64['astar']].numpy()
        bellman = c['rew'].double().numpy() + gamma * (1.0 - c['done'].double().numpy()) * (pt * z).sum(1)
        assert free.sum() >= 2
        assert np.abs((m * z).sum(1) - bellman)[free].max() <= 1e-10
        # ---- the inputs
        assert (tz < v_min).any() and (tz > v_max).any() and ((tz > v_min) & (tz < v_max)).any()
        assert (tz[2] > v_max).any() and (gamma == 0.0 or (tz[2] < v_max).any())
        assert (tz[3] < v_min).any() and (gamma == 0.0 or (tz[3] > v_min).any())
        assert (b[0] == np.round(b[0])).all() and (b[1] - np.floor(b[1]) == 0.5).all()
        done = c['done'].numpy()
        assert (done == 1.0).any() and (done == 0.0).any()
        assert C.gap_ok(loop['q_sel'], skip=ties)
        for row, acts in ties.items():
            q = loop['q_sel'][row]
            assert all(q[a] == q[acts[0]] for a in acts) and loop['astar'][row] == acts[0]
            assert all(q[a] < q[acts[0]] - 1e-4 for a in range(A) if a not in acts)
        # ---- torch in float32 against float64 on the GPU file's bar
        assert torch.equal(r32['astar'], r64['astar'])
        for k in ('m', 'td', 'dadv', 'stats') + (('dval',) if kw['dueling'] else ()):
            _fp32_as_good_as_torch(r32[k].detach(), r32[k].detach(), r64[k].detach())


def test_corner_families_hold_their_corners():
    for name, kw in FAMILIES.items():
        if name.startswith('corner'):
            c = C.family(**kw)
            assert (c['done'] == 0.5).any() and torch.isinf(c['rew']).sum() == 2
            assert torch.isfinite(torch.as_tensor(C.refs(kw, 1, 1)[2]['m'])).all()
    assert {kw['gamma'] for n, kw in FAMILIES.items() if n.startswith('corner')} == set(C.GAMMAS)


@pytest.mark.parametrize('N,v_min,v_max', [(51, -10.0, 10.0), (7, -3.5, 1.25), (2, -1.0, 1.0)])
def test_gather_is_scatter_at_integer_and_half_b(N, v_min, v_max):
    """p' scattered from every exactly representable b = k / 2 (integers: the l == u corner)"""
    D = (v_max - v_min) / (N - 1)
    halves = [k / 2 for k in range(2 * N - 1)
              if (float(np.float32(v_min + k / 2 * D)) - v_min) / D == k / 2]
    assert any(h == int(h) for h in halves) and any(h != int(h) for h in halves)
    B, A = len(halves), 2
    g = torch.Generator().manual_seed(N)
    nets = [(torch.randn(B, A * N, generator=g, dtype=F64), None) for _ in range(2)]
    rew = torch.tensor([v_min + h * D for h in halves], dtype=torch.float32).double()
    args = (nets[0], None, nets[1], torch.zeros(B), rew, torch.ones(B), None, A, N, v_min, v_max, C.GAMMA)
    scatter, gather = C.c51_td(*args), C.c51_td_loop(*args)
    assert (gather['b'] == np.array(halves)[:, None]).all()
    assert np.abs(gather['m'] - scatter['m'].numpy()).max() <= 1e-15
    pt = torch.softmax(nets[1][0].reshape(B, A, N), 2)[torch.arange(B), scatter['astar']].numpy()
    for n, h in enumerate(halves):
        lo, up = int(math.floor(h)), int(math.ceil(h))
        want = np.zeros(N)
        want[lo] += 1.0 if lo == up else 0.5
        want[up] += 0.0 if lo == up else 0.5
        assert np.abs(gather["m"][n] - want * pt[n].sum()).max() <= 1e-14      # two summation orders


@pytest.mark.parametrize('which', ['rew', 'done'])
def test_nan_reward_or_done_is_a_nan_row_in_both_references(which):
    kw = FAMILIES['stage-3x51-d1']
    c, (A, N, v_min, v_max, gamma) = C.family(**kw), C.params(kw)
    col = {k: c[k].clone() for k in ('rew', 'done')}
    col[which][3] = float('nan')
    clean = C.refs(kw, 1, 1)
    args = (c['n'], c['t'], c['act'], col['rew'], col['done'], c['w'], A, N, v_min, v_max, gamma)
    online = tuple(t.double().requires_grad_() for t in c['q'])
    dbl = lambda pr: tuple(t.double() for t in pr)                                      # noqa: E731
    scatter = C.c51_td(online, dbl(args[0]), dbl(args[1]), *args[2:])
    scatter['objective'].backward()
    scatter['dadv'], scatter['dval'] = online[0].grad, online[1].grad
    gather = C.c51_td_loop(c['q'], *args)
    others = [n for n in range(kw['B']) if n != 3]
    for out, ref in ((scatter, clean[1]), (gather, clean[2])):
        for k in ('m', 'td', 'dadv', 'dval'):
            got, want = (np.asarray(t[k].detach() if torch.is_tensor(t[k]) else t[k]) for t in (out, ref))
            assert np.isnan(got[3]).all(), k
            assert np.array_equal(got[others], want[others]), k
        assert np.isnan(np.asarray(out['stats'])).all()
        assert np.array_equal(np.asarray(out['astar']), np.asarray(ref['astar']))


def test_action_index_is_the_kernels_clamp():
    A = 3
    acts = torch.tensor([-1.0, 3.0, 3.5, 1.9, float('nan'), 1e9, 0.0, 2.0, -0.0, 2.999])
    assert C.action_index(acts, A).tolist() == [0, 2, 2, 1, 0, 2, 0, 2, 0, 2]
    kw = FAMILIES['stage-3x51-d0']
    c = C.family(**kw)
    _, N, v_min, v_max, gamma = C.params(kw)
    wild = acts[:kw['B']]
    args = (c['q'], None, c['t'])
    tail = (c['rew'], c['done'], None, A, N, v_min, v_max, gamma)
    for ref in (C.c51_td_loop, lambda *a: C.c51_td(*[tuple(t if t is None else t.double() for t in p)
                                                     if isinstance(p, tuple) else p for p in a])):
        a, b = ref(*args, wild, *tail), ref(*args, C.action_index(wild, A).float(), *tail)
        assert np.array_equal(np.asarray(a['td']), np.asarray(b['td']))
