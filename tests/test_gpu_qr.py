"""Quantile-regression DQN, the kernels of dqn_quant_kernels.hip through the C ABI
and through DQNLearner / FFQfunc / QAgentBatch, against tests/qr_ref.py in fp64
on the project's bar (_fp32_as_good_as_torch); the reference widens fp32 inputs."""
import copy

import numpy as np
import pytest
import torch

from surreal_amd import _lib as L
from surreal_amd.agent import QAgentBatch
from surreal_amd.config import discrete_env_config
from surreal_amd.dqn import DQNLearner, FFQfunc
from tests import dqn_ref as R
from tests import qr_ref as Q
from tests.dp_harness import Group, cut, lockstep, to_dev
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

pytestmark = pytest.mark.gpu
GAMMA = float(np.float32(0.99))
F32, F64 = torch.float32, torch.float64
FORMS = [(1, 1), (1, 0), (0, 1), (0, 0)]
# N = 1; one wave, padded lanes, odd dword tail; full wave, several quads; first row-form
# size (wave 1 holds one quantile); Atari's shape, partial last wave; the A N ceiling
SHAPES = [(5, 2, 1), (9, 3, 51), (33, 7, 64), (6, 3, 65), (5, 18, 200), (3, 16, 256)]
# (shape, form, gamma, kappa, layout); layout: '' contiguous, 'pad' a leading dimension
# rounded up to 4 plus 4 (the 16-byte form and its tail), 'odd' a base 4 bytes off (dwords)
CASES = [(s, f, GAMMA, 1.0, '') for s in SHAPES for f in FORMS] + \
    [(s, (1, 1), g, k, lay) for s in ((9, 3, 51), (5, 18, 200))
     for g, k, lay in ((1.0, 1.0, ''), (GAMMA, 0.25, ''), (GAMMA, 1.0, 'pad'), (GAMMA, 1.0, 'odd'))]
p = L.ptr
_BITS = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))   # noqa: E731


def _case(B, A, N, dueling, seed, dyadic=False):
    """N(0, 1) quantile values (dyadic: multiples of 1/4, rewards a multiple of 1/4 plus 1/64);
    replay-like rows (action, reward, done in columns 1, 3, 5) that start with d = 1, r = +-50"""
    g = torch.Generator().manual_seed(seed)
    grid = (lambda t: (4 * t).round() / 4) if dyadic else (lambda t: t)
    c = {}
    for k in 'qnt':
        adv, val = grid(torch.randn(B, A * N, generator=g)), grid(torch.randn(B, N, generator=g))
        c[k] = (adv, val if dueling else None)
    wide = torch.randn(B, 7, generator=g)
    wide[:, 1] = torch.randint(0, A, (B,), generator=g).float()
    wide[:, 5] = (torch.rand(B, generator=g) < 0.2).float()
    wide[0, 5], wide[1, 3], wide[2, 3] = 1.0, 50.0, -50.0
    if dyadic:
        wide[:, 3] = grid(wide[:, 3]) + 1 / 64
    c['wide'], c['w'] = wide, 0.3 + 0.7 * torch.rand(B, generator=g)
    return c


def _ref(c, dt, A, N, double_q, w, gamma, kappa):
    cv = lambda pr: tuple(None if t is None else t.to(dt) for t in pr)             # noqa: E731
    online = tuple(None if t is None else t.clone().requires_grad_() for t in cv(c['q']))
    wide = c['wide'].to(dt)
    out = Q.qr_td(online, cv(c['n']) if double_q else None, cv(c['t']), wide[:, 1], wide[:, 3],
                  wide[:, 5], w, A, N, kappa, gamma)
    out['objective'].backward()
    out['dadv'], out['dval'] = online[0].grad, None if online[1] is None else online[1].grad
    return out


def _launch(name, c, lo, hi, A, N, dueling, double_q, w, gamma, kappa, extra=(), layout=''):
    """rows [lo, hi) of the case through the C ABI (w: None or [B]); every output on the host"""
    B, Bg = hi - lo, extra[0] if extra else hi - lo
    ld = (A * N + 3) // 4 * 4 + 4 if layout == 'pad' else A * N
    off = 1 if layout == 'odd' else 0

    def slab(t):                 # [B][ld] at `off` floats past a 16-byte aligned base
        buf = torch.full((B * ld + off,), float('nan'), device='cuda')
        view = buf[off:].view(B, ld)
        view[:, :A * N] = t[lo:hi].to('cuda')
        return view
    d = lambda t: None if t is None else t[lo:hi].contiguous().to('cuda')              # noqa: E731
    (qa, qv), (na, nv), (ta, tv) = [(None if a is None else slab(a), d(v)) for a, v in
                                    (c['q'], c['n'] if double_q else (None, None), c['t'])]
    wide, wd = d(c['wide']), d(w)
    full = lambda shape, v=float('nan'), dt=F32: torch.full(shape, v, dtype=dt, device='cuda')  # noqa: E731
    o = {'dadv': full((B, A * N)), 'dval': full((B, N)), 'td': full((Bg,)), 'T': full((B, N)),
         'astar': full((B,), -1, torch.int32), 'stats': full((2,))}
    part = torch.zeros(int(L.lib().smi_dqn_qr_partials_bytes(B)) // 8, dtype=F64, device='cuda')
    L.call(name, p(qa), ld, p(na), ld, p(ta), ld, p(qv), N, p(nv), N, p(tv), N,
           p(wide[:, 1]), 7, p(wide[:, 3]), 7, p(wide[:, 5]), 7, p(wd), B, *extra, A, N, kappa,
           gamma, dueling, double_q, p(o['dadv']), A * N, p(o['dval']) if dueling else None, N,
           p(o['td']), p(o['T']), p(o['astar']), p(part), 8 * part.numel(), p(o['stats']), L.stream())
    return {k: v.cpu() for k, v in o.items()}


def _close(name, got, ref32, ref64):
    got, ref32, ref64 = (np.asarray(t.detach(), dtype=np.float64) for t in (got, ref32, ref64))
    print(f'{name}: e_gpu {np.abs(got - ref64).max():.3e} e_cpu {np.abs(ref32 - ref64).max():.3e} '
          f'scale {np.abs(ref64).max():.3e}')
    _fp32_as_good_as_torch(got, ref32, ref64)


def _gap_ok(q64):      # the condition on the inputs: no fp64 arg-max within 1e-4 of a tie
    return q64.shape[1] == 1 or float(q64.topk(2, 1).values.diff(dim=1).abs().min()) >= 1e-4


def _check_td(c, shape, form, w, gamma, kappa, layout=''):
    (B, A, N), (dueling, double_q) = shape, form
    r32, r64 = (_ref(c, dt, A, N, double_q, w, gamma, kappa) for dt in (F32, F64))
    assert _gap_ok(r64['q_sel'])
    got = _launch('smi_dqn_qr_td', c, 0, B, A, N, dueling, double_q, w, gamma, kappa, layout=layout)
    assert torch.equal(got['astar'].long(), r64['astar'])
    for k in ('T', 'td', 'dadv', 'stats') + (('dval',) if dueling else ()):
        _close(k, got[k], r32[k], r64[k])
    return r64


@pytest.mark.parametrize('shape,form,gamma,kappa,layout', CASES)
def test_qr_td_against_fp64(shape, form, gamma, kappa, layout):
    B, A, N = shape
    c = _case(B, A, N, form[0], seed=B + A)
    w = c['w'] if (B + sum(form) + len(layout)) % 2 else None      # weights on half the cases
    au = _check_td(c, shape, form, w, gamma, kappa, layout)['u'].abs()
    assert (au <= kappa).any() and (au > kappa).any()              # both Huber branches


@pytest.mark.parametrize('shape,form', [((6, 2, 51), (1, 1)), ((5, 4, 65), (1, 0)), ((4, 1, 130), (0, 1))])
def test_qr_pinball_on_a_dyadic_grid(shape, form):
    """kappa = 0: the gradient jumps at u = 0, so every u is exact in fp32 and an odd
    multiple of 1/64 (values on a 1/4 grid, A a power of two, gamma 1/2)"""
    c = _case(*shape, form[0], seed=sum(shape), dyadic=True)
    r64 = _check_td(c, shape, form, c['w'], 0.5, 0.0)
    assert float(r64['u'].abs().min()) >= 1 / 64


@pytest.mark.parametrize('N', [51, 65])
@pytest.mark.parametrize('form', FORMS, ids=[f'd{f[0]}q{f[1]}' for f in FORMS])
def test_qr_shards_and_null_weights_have_the_whole_batch_bits(form, N):
    """statistics as in tests/test_gpu_dqn_dp_kernel.py: three shard values, two fp32 adds and
    the full launch round once each, all positive: at most 3 ulp of the total, held to 4"""
    (dueling, double_q), (Bg, A) = form, (48, 3)
    c = _case(Bg, A, N, dueling, seed=11)
    run = lambda name, lo, hi, w, ex=(): _launch(name, c, lo, hi, A, N, *form, w, GAMMA, 1.0, ex)   # noqa: E731
    full = run('smi_dqn_qr_td', 0, Bg, c['w'])
    td_sum, stats = torch.zeros(Bg), torch.zeros(2)
    for lo, hi in ((0, 16), (16, 32), (32, 48)):
        s = run('smi_dqn_qr_td_shard', lo, hi, c['w'], (Bg, lo))
        for k in ('dadv', 'T') + (('dval',) if dueling else ()):
            assert _BITS(s[k], full[k][lo:hi]), (k, lo)
        assert torch.equal(s['astar'], full['astar'][lo:hi]) and _BITS(s['td'][lo:hi], full['td'][lo:hi])
        assert (torch.cat([s['td'][:lo], s['td'][hi:]]).view(torch.int32) == 0).all()   # +0.0f
        td_sum, stats = td_sum + s['td'], stats + s['stats']
    assert _BITS(td_sum, full['td'])
    want = full['stats'].numpy()
    ulps = np.abs(stats.numpy().astype(np.float64) - want) / np.spacing(want).astype(np.float64)
    assert (want > 0).all() and (ulps <= 4).all()
    ones, null = run('smi_dqn_qr_td', 0, Bg, torch.ones(Bg)), run('smi_dqn_qr_td', 0, Bg, None)
    assert all(_BITS(ones[k], null[k]) for k in ('dadv', 'td', 'stats') + (('dval',) if dueling else ()))


@pytest.mark.parametrize('dueling', [1, 0])
@pytest.mark.parametrize('rows,A,N', [(67, 3, 51), (9, 1, 1), (7, 18, 200), (5, 63, 65)])
def test_qr_q_and_forward(rows, A, N, dueling):
    """a padded leading dimension (the 16-byte staging and its dword tail);
    FFQfunc.forward against the reference on its own head outputs"""
    adv, val = _case(rows, A, N, dueling, seed=rows)['q']
    lda = (A * N + 3) // 4 * 4 + 4
    advd = torch.nn.functional.pad(adv, (0, lda - A * N)).to('cuda')
    q = torch.full((rows, A), float('nan'), device='cuda')
    greedy = torch.full((rows,), -1, dtype=torch.int32, device='cuda')
    L.call('smi_dqn_qr_q', p(advd), lda, p(val.to('cuda')) if dueling else None, N, rows, A, N,
           dueling, p(q), A, p(greedy), L.stream())
    ref = lambda a, v, dt: Q.mean_q(a.to(dt), None if v is None else v.to(dt), A, N)  # noqa: E731
    q64 = ref(adv, val, F64)
    assert _gap_ok(q64)
    _close('q', q.cpu(), ref(adv, val, F32), q64)
    assert torch.equal(greedy.cpu().long(), q64.argmax(1))
    f = FFQfunc(5, A, [16], dueling, 'cuda', torch.Generator().manual_seed(1), quantiles=N)
    x = torch.randn(rows, 5, generator=torch.Generator().manual_seed(2)).to('cuda')
    la, lv = (None if t is None else t.cpu() for t in f.logits(x))
    _close('forward', f(x).cpu(), ref(la, lv, F32), ref(la, lv, F64))


D, A, B = 5, 3, 32


def _setup(N, dueling, double_q, world=1, **kw):
    """(config, online twin, target twin, the ranks' learners loaded from the twins; world 0: none)"""
    lc = R.dqn_config(B, [16], bool(dueling), bool(double_q))
    lc.algo.distributional.update(enabled=True, kind='quantile', atoms=N)
    lc.algo.gamma = GAMMA
    torch.manual_seed(3)
    q, t = Q.twin(D, A, N, [16], dueling), Q.twin(D, A, N, [16], dueling)
    learners = []
    for r in range(world):
        rc = copy.deepcopy(lc)
        rc.replay.batch_size = B // world
        learners.append(DQNLearner(rc, discrete_env_config(D, A),
                                   dp=Group(world, r) if world > 1 else None, **kw))
        learners[r].q_func.load_state_dict(q.state_dict())
        learners[r].q_target.load_state_dict(t.state_dict())
    return lc, q, t, learners


@pytest.mark.parametrize('N', [51, 65])
@pytest.mark.parametrize('form,world', [(f, 1) for f in FORMS] + [((1, 1), 2)])
def test_qr_learn_against_the_fp64_twin(form, world, N):
    """one learn() (world 2: two ranks in lockstep, one exchange) against the twin's autograd,
    its clip_grad_norm_ + Adam(eps 1e-4) step and the reference's row losses"""
    lc, q, t, learners = _setup(N, *form, world)
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
        out = Q.qr_td(qq.streams(f('obs')), nxt, tgt, f('actions'), f('rewards'), f('dones'), f('weights'),
                      A, N, 1.0, GAMMA)
        assert _gap_ok(out['q_sel'])
        out['objective'].backward()
        grad = image({k: v.grad for k, v in qq.named_parameters()})
        torch.nn.utils.clip_grad_norm_(qq.parameters(), lc.algo.grad_norm_clipping)
        torch.optim.Adam(qq.parameters(), lr=lc.algo.lr, eps=1e-4).step()
        ref[dt] = (grad, image(dict(qq.named_parameters())), out['td'])
    for i, got in enumerate((learner.opt['g'], learner.q_func.flat, learner.td_error)):
        _close(('gradient', 'parameters', 'td_error')[i], got.cpu(), ref[F32][i], ref[F64][i])


@pytest.mark.parametrize('N', [51, 65])
def test_qr_graph_replay_bit_exact(N):
    eager, graph = _setup(N, 1, 1)[3][0], _setup(N, 1, 1, use_graph=True)[3][0]
    for it, b in enumerate(R.dqn_batches(B, D, A, 3, True, steps=3)):
        for learner in (eager, graph):
            learner.learn(to_dev(b))
        for a, g in ((eager.q_func.flat, graph.q_func.flat), (eager.td_error, graph.td_error),
                     (eager.stats_buf, graph.stats_buf)):
            assert torch.equal(a, g), it
    assert graph._graph is not None and eager._graph is None


@pytest.mark.parametrize('N', [51, 65])
def test_qr_agents_act_on_the_mean_quantiles(N):
    lc, q, _, _ = _setup(N, 1, 1, world=0)
    agents = QAgentBatch(lc, discrete_env_config(D, A), 8, agent_mode='eval_deterministic')
    agents.q_func.load_state_dict(q.state_dict())
    obs = torch.randn(8, D, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        q64 = Q.mean_q(*q.double().streams(obs.double()), A, N)
    assert _gap_ok(q64)
    assert agents.act(obs.numpy()).tolist() == q64.argmax(1).tolist()
