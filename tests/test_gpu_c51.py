"""Categorical (C51) DQN, the kernels of dqn_dist_kernels.hip through the C ABI
and through DQNLearner / FFQfunc / QAgentBatch, against tests/c51_ref.py in fp64
on the project's bar (_fp32_as_good_as_torch); the reference widens fp32 inputs."""
import copy

import numpy as np
import pytest
import torch

from surreal_amd import _lib as L
from surreal_amd.agent import QAgentBatch
from surreal_amd.config import discrete_env_config
from surreal_amd.dqn import DQNLearner, FFQfunc
from tests import c51_ref as C
from tests import dqn_ref as R
from tests.dp_harness import Group, cut, lockstep, to_dev
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

pytestmark = pytest.mark.gpu
GAMMA, VMIN, VMAX = float(np.float32(0.99)), -10.0, 10.0
F32, F64 = torch.float32, torch.float64
FORMS = [(1, 1), (1, 0), (0, 1), (0, 0)]
SHAPES = [(5, 2, 2), (67, 3, 51), (64, 18, 51), (33, 7, 64), (9, 1, 33)]
CASES = [(s, f, GAMMA) for s in SHAPES for f in FORMS] + [((67, 3, 51), (1, 1), 1.0)]
p = L.ptr
_BITS = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))   # noqa: E731


def _case(B, A, N, dueling, seed):
    """N(0, 1) logits, +100 on every second row; replay-like rows (action, reward,
    done in columns 1, 3, 5) that start with the edges: d = 1; r = +-50; r = 3 D, D / 2"""
    g = torch.Generator().manual_seed(seed)
    c = {}
    for k in 'qnt':
        adv, val = torch.randn(B, A * N, generator=g), torch.randn(B, N, generator=g)
        (val if dueling else adv)[1::2] += 100.0
        c[k] = (adv, val if dueling else None)
    delta = float(np.float32(VMAX - VMIN) / np.float32(N - 1))
    wide = torch.randn(B, 7, generator=g)
    wide[:, 1] = torch.randint(0, A, (B,), generator=g).float()
    wide[:, 5] = (torch.rand(B, generator=g) < 0.2).float()
    wide[0, 5], wide[1, 3], wide[2, 3] = 1.0, 50.0, -50.0
    wide[3, 3], wide[4, 3], wide[3:5, 5] = 3 * delta, 0.5 * delta, 0.0
    c['wide'], c['w'] = wide, 0.3 + 0.7 * torch.rand(B, generator=g)
    return c


def _ref(c, dt, A, N, double_q, w, gamma):
    cv = lambda pr: tuple(None if t is None else t.to(dt) for t in pr)             # noqa: E731
    online = tuple(None if t is None else t.clone().requires_grad_() for t in cv(c['q']))
    wide = c['wide'].to(dt)
    out = C.c51_td(online, cv(c['n']) if double_q else None, cv(c['t']), wide[:, 1], wide[:, 3],
                   wide[:, 5], w, A, N, VMIN, VMAX, gamma)
    out['objective'].backward()
    out['dadv'], out['dval'] = online[0].grad, None if online[1] is None else online[1].grad
    return out


def _launch(name, c, lo, hi, A, N, dueling, double_q, w, gamma, extra=()):
    """rows [lo, hi) of the case through the C ABI (w: None or [B]); every output on the host"""
    B, Bg = hi - lo, extra[0] if extra else hi - lo
    d = lambda t: None if t is None else t[lo:hi].contiguous().to('cuda')              # noqa: E731
    (qa, qv), (na, nv), (ta, tv) = [(d(a), d(v)) for a, v in
                                    (c['q'], c['n'] if double_q else (None, None), c['t'])]
    wide, wd = d(c['wide']), d(w)
    full = lambda shape, v=float('nan'), dt=F32: torch.full(shape, v, dtype=dt, device='cuda')  # noqa: E731
    o = {'dadv': full((B, A * N)), 'dval': full((B, N)), 'td': full((Bg,)), 'm': full((B, N)),
         'astar': full((B,), -1, torch.int32), 'stats': full((2,))}
    part = torch.zeros(int(L.lib().smi_dqn_c51_partials_bytes(B)) // 8, dtype=F64, device='cuda')
    L.call(name, p(qa), A * N, p(na), A * N, p(ta), A * N, p(qv), N, p(nv), N, p(tv), N,
           p(wide[:, 1]), 7, p(wide[:, 3]), 7, p(wide[:, 5]), 7, p(wd), B, *extra, A, N, VMIN, VMAX,
           gamma, dueling, double_q, p(o['dadv']), A * N, p(o['dval']) if dueling else None, N,
           p(o['td']), p(o['m']), p(o['astar']), p(part), 8 * part.numel(), p(o['stats']), L.stream())
    return {k: v.cpu() for k, v in o.items()}


def _close(name, got, ref32, ref64):
    got, ref32, ref64 = (np.asarray(t.detach(), dtype=np.float64) for t in (got, ref32, ref64))
    print(f'{name}: e_gpu {np.abs(got - ref64).max():.3e} e_cpu {np.abs(ref32 - ref64).max():.3e} '
          f'scale {np.abs(ref64).max():.3e}')
    _fp32_as_good_as_torch(got, ref32, ref64)


def _gap_ok(q64):      # the condition on the inputs: no fp64 arg-max within 1e-4 of a tie
    return q64.shape[1] == 1 or float(q64.topk(2, 1).values.diff(dim=1).abs().min()) >= 1e-4


@pytest.mark.parametrize('shape,form,gamma', CASES)
def test_c51_td_against_fp64(shape, form, gamma):
    (B, A, N), (dueling, double_q) = shape, form
    c = _case(B, A, N, dueling, seed=B + A)
    w = c['w'] if (B + dueling + double_q) % 2 else None         # weights on half the cases
    r32, r64 = (_ref(c, dt, A, N, double_q, w, gamma) for dt in (F32, F64))
    assert _gap_ok(r64['q_sel'])
    got = _launch('smi_dqn_c51_td', c, 0, B, A, N, dueling, double_q, w, gamma)
    assert torch.equal(got['astar'].long(), r64['astar'])
    for k in ('m', 'td', 'dadv', 'stats') + (('dval',) if dueling else ()):
        _close(k, got[k], r32[k], r64[k])


@pytest.mark.parametrize('form', FORMS, ids=[f'd{f[0]}q{f[1]}' for f in FORMS])
def test_c51_shards_and_null_weights_have_the_whole_batch_bits(form):
    """statistics as in tests/test_gpu_dqn_dp_kernel.py: three shard values, two fp32 adds and
    the full launch round once each, all positive: at most 3 ulp of the total, held to 4"""
    (dueling, double_q), (Bg, A, N) = form, (48, 3, 51)
    c = _case(Bg, A, N, dueling, seed=11)
    run = lambda name, lo, hi, w, ex=(): _launch(name, c, lo, hi, A, N, *form, w, GAMMA, ex)   # noqa: E731
    full = run('smi_dqn_c51_td', 0, Bg, c['w'])
    td_sum, stats = torch.zeros(Bg), torch.zeros(2)
    for lo, hi in ((0, 16), (16, 32), (32, 48)):
        s = run('smi_dqn_c51_td_shard', lo, hi, c['w'], (Bg, lo))
        for k in ('dadv', 'm') + (('dval',) if dueling else ()):
            assert _BITS(s[k], full[k][lo:hi]), (k, lo)
        assert torch.equal(s['astar'], full['astar'][lo:hi]) and _BITS(s['td'][lo:hi], full['td'][lo:hi])
        assert (torch.cat([s['td'][:lo], s['td'][hi:]]).view(torch.int32) == 0).all()   # +0.0f
        td_sum, stats = td_sum + s['td'], stats + s['stats']
    assert _BITS(td_sum, full['td'])
    want = full['stats'].numpy()
    ulps = np.abs(stats.numpy().astype(np.float64) - want) / np.spacing(want).astype(np.float64)
    assert (want > 0).all() and (ulps <= 4).all()
    ones, null = run('smi_dqn_c51_td', 0, Bg, torch.ones(Bg)), run('smi_dqn_c51_td', 0, Bg, None)
    assert all(_BITS(ones[k], null[k]) for k in ('dadv', 'td', 'stats') + (('dval',) if dueling else ()))


@pytest.mark.parametrize('dueling', [1, 0])
@pytest.mark.parametrize('rows,A,N', [(67, 3, 51), (9, 1, 33), (5, 24, 64)])
def test_c51_q_and_forward(rows, A, N, dueling):
    """a padded leading dimension (the 16-byte staging and its dword tail, 24 x 64
    its second round); FFQfunc.forward against the reference on its own logits"""
    adv, val = _case(rows, A, N, dueling, seed=rows)['q']
    lda = (A * N + 3) // 4 * 4 + 4
    advd = torch.nn.functional.pad(adv, (0, lda - A * N)).to('cuda')
    q = torch.full((rows, A), float('nan'), device='cuda')
    greedy = torch.full((rows,), -1, dtype=torch.int32, device='cuda')
    L.call('smi_dqn_c51_q', p(advd), lda, p(val.to('cuda')) if dueling else None, N, rows, A, N, VMIN,
           VMAX, dueling, p(q), A, p(greedy), L.stream())
    ref = lambda a, v, dt: C.expected_q(a.to(dt), None if v is None else v.to(dt), A, N, VMIN, VMAX)  # noqa: E731
    q64 = ref(adv, val, F64)
    assert _gap_ok(q64)
    _close('q', q.cpu(), ref(adv, val, F32), q64)
    assert torch.equal(greedy.cpu().long(), q64.argmax(1))
    f = FFQfunc(5, A, [16], dueling, 'cuda', torch.Generator().manual_seed(1), atoms=N, v_min=VMIN, v_max=VMAX)
    x = torch.randn(rows, 5, generator=torch.Generator().manual_seed(2)).to('cuda')
    la, lv = (None if t is None else t.cpu() for t in f.logits(x))
    _close('forward', f(x).cpu(), ref(la, lv, F32), ref(la, lv, F64))


D, A, N, B = 5, 3, 51, 32


def _setup(dueling, double_q, world=1, **kw):
    """(config, online twin, target twin, the ranks' learners loaded from the twins; world 0: none)"""
    lc = R.dqn_config(B, [16], bool(dueling), bool(double_q))
    lc.algo.distributional.enabled, lc.algo.gamma = True, GAMMA
    torch.manual_seed(3)
    q, t = C.twin(D, A, N, [16], dueling), C.twin(D, A, N, [16], dueling)
    learners = []
    for r in range(world):
        rc = copy.deepcopy(lc)
        rc.replay.batch_size = B // world
        learners.append(DQNLearner(rc, discrete_env_config(D, A),
                                   dp=Group(world, r) if world > 1 else None, **kw))
        learners[r].q_func.load_state_dict(q.state_dict())
        learners[r].q_target.load_state_dict(t.state_dict())
    return lc, q, t, learners


@pytest.mark.parametrize('form,world', [(f, 1) for f in FORMS] + [((1, 1), 2)])
def test_c51_learn_against_the_fp64_twin(form, world):
    """one learn() (world 2: two ranks in lockstep, one exchange) against the twin's autograd,
    its clip_grad_norm_ + Adam(eps 1e-4) step and the reference's row losses"""
    lc, q, t, learners = _setup(*form, world)
    b = R.dqn_batches(B, D, A, 5, True, steps=1)[0]
    if world == 1:
        learners[0].learn(b)
    else:
        assert lockstep(learners, [cut(to_dev(b), r, B // world) for r in range(world)]) == 1
    learner = learners[0]
    offs = {k: learner.q_func.off(v) for k, v in learner.q_func.named_parameters()}
    image = lambda named: torch.cat([named[k].detach().reshape(-1)                                # noqa: E731
                                     for k in sorted(offs, key=offs.get)])    # the flat layout
    ref = {}
    for dt in (F32, F64):
        qq, tt = copy.deepcopy(q).to(dt), copy.deepcopy(t).to(dt)
        f = lambda k: torch.as_tensor(b[k], dtype=F32).to(dt)                                     # noqa: E731
        with torch.no_grad():
            nxt, tgt = (qq.streams(f('obs_next')) if form[1] else None), tt.streams(f('obs_next'))
        out = C.c51_td(qq.streams(f('obs')), nxt, tgt, f('actions'), f('rewards'), f('dones'), f('weights'),
                       A, N, VMIN, VMAX, GAMMA)
        assert _gap_ok(out['q_sel'])
        out['objective'].backward()
        grad = image({k: v.grad for k, v in qq.named_parameters()})
        torch.nn.utils.clip_grad_norm_(qq.parameters(), lc.algo.grad_norm_clipping)
        torch.optim.Adam(qq.parameters(), lr=lc.algo.lr, eps=1e-4).step()
        ref[dt] = (grad, image(dict(qq.named_parameters())), out['td'])
    for i, got in enumerate((learner.opt['g'], learner.q_func.flat, learner.td_error)):
        _close(('gradient', 'parameters', 'td_error')[i], got.cpu(), ref[F32][i], ref[F64][i])


def test_c51_graph_replay_bit_exact():
    eager, graph = _setup(1, 1)[3][0], _setup(1, 1, use_graph=True)[3][0]
    for it, b in enumerate(R.dqn_batches(B, D, A, 3, True, steps=3)):
        for learner in (eager, graph):
            learner.learn(to_dev(b))
        for a, g in ((eager.q_func.flat, graph.q_func.flat), (eager.td_error, graph.td_error),
                     (eager.stats_buf, graph.stats_buf)):
            assert torch.equal(a, g), it
    assert graph._graph is not None and eager._graph is None


def test_c51_agents_act_on_the_expected_values():
    lc, q, _, _ = _setup(1, 1, world=0)
    agents = QAgentBatch(lc, discrete_env_config(D, A), 8, agent_mode='eval_deterministic')
    agents.q_func.load_state_dict(q.state_dict())
    obs = torch.randn(8, D, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        q64 = C.expected_q(*q.double().streams(obs.double()), A, N, VMIN, VMAX)
    assert _gap_ok(q64)
    assert agents.act(obs.numpy()).tolist() == q64.argmax(1).tolist()
