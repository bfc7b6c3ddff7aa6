"""Implicit quantile DQN, the kernels of dqn_iqn_kernels.hip through the C ABI and
through DQNLearner / FFQfunc / QAgentBatch, against tests/iqn_ref.py in fp64 on
the project's bar (_fp32_as_good_as_torch); the reference widens fp32 inputs."""
import copy

import numpy as np
import pytest
import torch

from surreal_amd import _lib as L
from surreal_amd.agent import QAgentBatch
from surreal_amd.config import discrete_env_config
from surreal_amd.dqn import DQNLearner, FFQfunc
from tests import dqn_ref as R
from tests import iqn_ref as Q
from tests import qconv_ref as QC
from tests.dp_harness import Group, cut, lockstep, to_dev
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

pytestmark = pytest.mark.gpu
GAMMA = float(np.float32(0.99))
F32, F64 = torch.float32, torch.float64
FORMS = [(1, 1), (1, 0), (0, 1), (0, 0)]
p = L.ptr
_BITS = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))   # noqa: E731
_nan = lambda *shape: torch.full(shape, float('nan'), device='cuda')         # noqa: E731


def _close(name, got, ref32, ref64, mag=None):
    got, ref32, ref64 = (np.asarray(t.detach(), dtype=np.float64) for t in (got, ref32, ref64))
    print(f'{name}: e_gpu {np.abs(got - ref64).max():.3e} e_cpu {np.abs(ref32 - ref64).max():.3e} '
          f'scale {np.abs(ref64).max():.3e}')
    _fp32_as_good_as_torch(got, ref32, ref64, mag=mag)


def _gap_ok(q64):      # the condition on the inputs: no fp64 arg-max within 1e-4 of a tie
    return q64.shape[1] == 1 or float(q64.topk(2, 1).values.diff(dim=1).abs().min()) >= 1e-4


def _view(t, layout):
    """t on the device behind a leading dimension rounded up to 4 plus 4 ('pad': 16-byte
    rows) or at a base 4 bytes off ('odd': dwords); NaN around it"""
    rows, cols = t.shape
    ld, off = ((cols + 3) // 4 * 4 + 4, 0) if layout == 'pad' else (cols, 1)
    v = _nan(rows * ld + off)[off:].view(rows, ld)
    v[:, :cols] = t.to('cuda')
    return v, ld


# ------------------------------------------------------------------ embedding
# smallest everything; d no tile multiple, a 16-row tile spans two observations; N not
# dividing a tile, n_cos no multiple of 16, a column tail past one chunk of 128; several
# row tiles per workgroup and a split weight-gradient sum (B N = 4288 > 256 rows)
EMBED = [(3, 1, 8, 4), (5, 8, 40, 64), (9, 7, 130, 12), (67, 64, 256, 64)]


def _embed_case(B, N, d, n_cos):
    """the big shape has too many pre-activations for a seed to keep them all 1e-5 off 0:
    there |bias| >= 0.6 (both signs) against sum_i |w_ji| <= 0.5; the others are N(0, 1)-like"""
    g = torch.Generator().manual_seed(B + d)
    c = {'tau': torch.from_numpy(Q.taus(7, 3, 0, 0, B, N)), 'pre': torch.randn(B, d, generator=g),
         'dZ': torch.randn(B * N, d, generator=g)}
    u = lambda *s: 2 * torch.rand(*s, generator=g) - 1                                   # noqa: E731
    if B * N * d > 100000:
        c['W'], sign = 0.5 * u(d, n_cos) / n_cos, torch.where(u(d) < 0, -1.0, 1.0)
        c['b'] = sign * (0.6 + 0.4 * torch.rand(d, generator=g))
    else:
        c['W'], c['b'] = u(d, n_cos) / n_cos ** 0.5, u(d) / n_cos ** 0.5
    return c


def _embed_ref(c, N, dt):
    pre, W, b = (c[k].clone().to(dt).requires_grad_() for k in ('pre', 'W', 'b'))
    Z, phi = Q.embed(c['tau'].to(dt), torch.relu(pre), W, b, N)
    Z.backward(c['dZ'].to(dt))
    z_pre = torch.cos(np.pi * torch.arange(W.shape[1], dtype=dt) * c['tau'].to(dt)[:, None]) @ W.t() + b
    return {'Z': Z, 'phi': phi, 'dH1': pre.grad, 'dW': W.grad, 'db': b.grad, 'z_pre': z_pre.detach()}


@pytest.mark.parametrize('layout', ['pad', 'odd'])
@pytest.mark.parametrize('B,N,d,n_cos', EMBED)
def test_iqn_embed_against_fp64(B, N, d, n_cos, layout):
    c = _embed_case(B, N, d, n_cos)
    r32, r64 = _embed_ref(c, N, F32), _embed_ref(c, N, F64)
    assert float(r64['z_pre'].abs().min()) >= 1e-5 and (r64['phi'] > 0).any() and (r64['phi'] == 0).any()
    (H1, ldh), (dZ, ldg) = _view(torch.relu(c['pre']), layout), _view(c['dZ'], layout)
    (Z, ldz), (phi, ldp) = _view(torch.zeros(B * N, d), layout), _view(torch.zeros(B * N, d), layout)
    Z.fill_(float('nan')), phi.fill_(float('nan'))
    tau, W, b = c['tau'].to('cuda'), c['W'].to('cuda'), c['b'].to('cuda')
    L.call('smi_iqn_embed_forward', p(tau), p(H1), ldh, B, N, p(W), p(b), n_cos, d, p(Z), ldz, p(phi),
           ldp, L.stream())
    Z2 = _nan(B * N, d)                                   # without phi: the same Z
    L.call('smi_iqn_embed_forward', p(tau), p(H1), ldh, B, N, p(W), p(b), n_cos, d, p(Z2), d, None, 0,
           L.stream())
    assert _BITS(Z2, Z[:, :d].contiguous())
    _close('Z', Z[:, :d].cpu(), r32['Z'], r64['Z'])
    _close('phi', phi[:, :d].cpu(), r32['phi'], r64['phi'])
    need = int(L.lib().smi_iqn_embed_scratch_bytes(B, N, n_cos, d))
    assert (need > 0) == (B * N > 256)
    scratch = _nan(max(need // 4, 1))
    runs = []
    for _ in range(2):               # twice into NaN: written, not accumulated; the same bits
        (dH1, lddh), img = _view(torch.zeros(B, d), layout), _nan(3 + d * n_cos + d)
        dH1.fill_(float('nan'))
        L.call('smi_iqn_embed_backward', p(dZ), ldg, p(tau), p(H1), ldh, p(phi), ldp, B, N, p(img[3:]),
               p(img[3 + d * n_cos:]), n_cos, d, p(dH1), lddh, p(scratch), need, L.stream())
        runs.append((dH1[:, :d].cpu(), img[3:3 + d * n_cos].view(d, n_cos).cpu(), img[3 + d * n_cos:].cpu()))
    assert all(_BITS(a, b) for a, b in zip(*runs))
    mag = float((c['dZ'].double().abs() * torch.relu(c['pre']).double().repeat_interleave(N, 0)).sum(0).max())
    for k, got, m in zip(('dH1', 'dW', 'db'), runs[0], (None, mag, mag)):
        _close(k, got, r32[k], r64[k], mag=m)


# -------------------------------------------------------------------- TD step
# (B, A, N, N'): one sample; padded lanes; N != N', A N' % 4 == 0; full waves; one target
SHAPES = [(5, 2, 1, 1), (9, 3, 8, 8), (6, 18, 8, 32), (4, 5, 64, 64), (7, 64, 64, 1)]
# (shape, form, gamma, kappa, layout); layout '': contiguous, 'pad': a leading dimension of
# A + 3 (the strided staging), 'odd': a base 4 bytes off (contiguous dwords)
CASES = [(s, f, GAMMA, 1.0, '') for s in SHAPES for f in FORMS] + \
    [((9, 3, 8, 8), (1, 1), 1.0, 1.0, ''), ((6, 18, 8, 32), (1, 1), GAMMA, 0.25, ''),
     ((6, 18, 8, 32), (1, 1), GAMMA, 1.0, 'pad'), ((4, 5, 64, 64), (1, 1), GAMMA, 1.0, 'odd')]


def _case(B, A, N, Nt, dueling, seed, dyadic=False):
    """N(0, 1) head outputs (dyadic: multiples of 1/4, rewards a multiple of 1/4 plus 1/64);
    replay-like rows (action, reward, done in columns 1, 3, 5) that start with d = 1, r = +-50"""
    g = torch.Generator().manual_seed(seed)
    grid = (lambda t: (4 * t).round() / 4) if dyadic else (lambda t: t)
    c = {'tau': torch.from_numpy(Q.taus(seed, 1, 0, 0, B, N))}
    for k, n in (('q', N), ('n', Nt), ('t', Nt)):
        adv, val = grid(torch.randn(B * n, A, generator=g)), grid(torch.randn(B * n, generator=g))
        c[k] = (adv, val if dueling else None)
    wide = torch.randn(B, 7, generator=g)
    wide[:, 1] = torch.randint(0, A, (B,), generator=g).float()
    wide[:, 5] = (torch.rand(B, generator=g) < 0.2).float()
    wide[0, 5], wide[1, 3], wide[2, 3] = 1.0, 50.0, -50.0
    if dyadic:
        wide[:, 3] = grid(wide[:, 3]) + 1 / 64
    c['wide'], c['w'] = wide, 0.3 + 0.7 * torch.rand(B, generator=g)
    return c


def _ref(c, dt, A, N, Nt, double_q, w, gamma, kappa):
    cv = lambda pr: tuple(None if t is None else t.to(dt) for t in pr)             # noqa: E731
    online = tuple(None if t is None else t.clone().requires_grad_() for t in cv(c['q']))
    wide = c['wide'].to(dt)
    out = Q.iqn_td(online, cv(c['n']) if double_q else None, cv(c['t']), c['tau'].to(dt), wide[:, 1],
                   wide[:, 3], wide[:, 5], w, A, N, Nt, kappa, gamma)
    out['objective'].backward()
    out['dadv'], out['dval'] = online[0].grad, None if online[1] is None else online[1].grad
    return out


def _launch(name, c, lo, hi, A, N, Nt, dueling, double_q, w, gamma, kappa, extra=(), layout=''):
    """rows [lo, hi) of the case through the C ABI (w: None or [B]); every output on the host"""
    B, Bg = hi - lo, extra[0] if extra else hi - lo
    ld, off = (A + 3, 0) if layout == 'pad' else (A, 1 if layout == 'odd' else 0)

    def slab(t, n):              # [B n][ld] at `off` floats past a 16-byte aligned base
        view = _nan(B * n * ld + off)[off:].view(B * n, ld)
        view[:, :A] = t[lo * n:hi * n].to('cuda')
        return view
    d = lambda t, n=1: None if t is None else t[lo * n:hi * n].contiguous().to('cuda')    # noqa: E731
    (qa, qv), (na, nv), (ta, tv) = [(None if a is None else slab(a, n), d(v, n)) for (a, v), n in
                                    ((c['q'], N), (c['n'] if double_q else (None, None), Nt), (c['t'], Nt))]
    wide, wd = d(c['wide']), d(w)
    o = {'dadv': _nan(B * N, A), 'dval': _nan(B * N), 'td': _nan(Bg), 'T': _nan(B, Nt),
         'astar': torch.full((B,), -1, dtype=torch.int32, device='cuda'), 'stats': _nan(2)}
    part = torch.zeros(int(L.lib().smi_iqn_partials_bytes(B)) // 8, dtype=F64, device='cuda')
    L.call(name, p(qa), ld, p(na), ld, p(ta), ld, p(qv), p(nv), p(tv), p(d(c['tau'], N)),
           p(wide[:, 1]), 7, p(wide[:, 3]), 7, p(wide[:, 5]), 7, p(wd), B, *extra, A, N, Nt, kappa,
           gamma, dueling, double_q, p(o['dadv']), A, p(o['dval']) if dueling else None,
           p(o['td']), p(o['T']), p(o['astar']), p(part), 8 * part.numel(), p(o['stats']), L.stream())
    return {k: v.cpu() for k, v in o.items()}


def _check_td(c, shape, form, w, gamma, kappa, layout=''):
    (B, A, N, Nt), (dueling, double_q) = shape, form
    r32, r64 = (_ref(c, dt, A, N, Nt, double_q, w, gamma, kappa) for dt in (F32, F64))
    assert _gap_ok(r64['q_sel'])
    got = _launch('smi_iqn_td', c, 0, B, A, N, Nt, dueling, double_q, w, gamma, kappa, layout=layout)
    assert torch.equal(got['astar'].long(), r64['astar'])
    for k in ('T', 'td', 'dadv', 'stats') + (('dval',) if dueling else ()):
        _close(k, got[k], r32[k], r64[k])
    return r64


@pytest.mark.parametrize('shape,form,gamma,kappa,layout', CASES)
def test_iqn_td_against_fp64(shape, form, gamma, kappa, layout):
    c = _case(*shape, form[0], seed=sum(shape))
    w = c['w'] if (shape[0] + sum(form) + len(layout)) % 2 else None     # weights on half the cases
    au = _check_td(c, shape, form, w, gamma, kappa, layout)['u'].abs()
    assert (au <= kappa).any() and (au > kappa).any()                    # both Huber branches


@pytest.mark.parametrize('shape,form', [((6, 2, 8, 8), (1, 1)), ((5, 4, 8, 5), (1, 0)), ((4, 1, 64, 3), (0, 1))])
def test_iqn_pinball_on_a_dyadic_grid(shape, form):
    """kappa = 0: the gradient jumps at u = 0, so every u is exact in fp32 and an odd
    multiple of 1/64 (values on a 1/4 grid, A a power of two, gamma 1/2); tau is dyadic too"""
    c = _case(*shape, form[0], seed=sum(shape), dyadic=True)
    r64 = _check_td(c, shape, form, c['w'], 0.5, 0.0)
    assert float(r64['u'].abs().min()) >= 1 / 64


@pytest.mark.parametrize('form', FORMS, ids=[f'd{f[0]}q{f[1]}' for f in FORMS])
def test_iqn_shards_and_null_weights_have_the_whole_batch_bits(form):
    """statistics as in tests/test_gpu_qr.py: three shard values, two fp32 adds and the full
    launch round once each, all positive: at most 3 ulp of the total, held to 4"""
    (dueling, double_q), (Bg, A, N, Nt) = form, (48, 3, 8, 5)
    c = _case(Bg, A, N, Nt, dueling, seed=11)
    run = lambda name, lo, hi, w, ex=(): _launch(name, c, lo, hi, A, N, Nt, *form, w, GAMMA, 1.0, ex)   # noqa: E731
    full = run('smi_iqn_td', 0, Bg, c['w'])
    td_sum, stats = torch.zeros(Bg), torch.zeros(2)
    for lo, hi in ((0, 16), (16, 32), (32, 48)):
        s = run('smi_iqn_td_shard', lo, hi, c['w'], (Bg, lo))
        for k, n in (('dadv', N), ('T', 1)) + ((('dval', N),) if dueling else ()):
            assert _BITS(s[k], full[k][lo * n:hi * n]), (k, lo)
        assert torch.equal(s['astar'], full['astar'][lo:hi]) and _BITS(s['td'][lo:hi], full['td'][lo:hi])
        assert (torch.cat([s['td'][:lo], s['td'][hi:]]).view(torch.int32) == 0).all()   # +0.0f
        td_sum, stats = td_sum + s['td'], stats + s['stats']
    assert _BITS(td_sum, full['td'])
    want = full['stats'].numpy()
    ulps = np.abs(stats.numpy().astype(np.float64) - want) / np.spacing(want).astype(np.float64)
    assert (want > 0).all() and (ulps <= 4).all()
    ones, null = run('smi_iqn_td', 0, Bg, torch.ones(Bg)), run('smi_iqn_td', 0, Bg, None)
    assert all(_BITS(ones[k], null[k]) for k in ('dadv', 'td', 'stats') + (('dval',) if dueling else ()))


@pytest.mark.parametrize('dueling', [1, 0])
@pytest.mark.parametrize('rows,A,K', [(67, 3, 32), (9, 1, 1), (5, 64, 64)])
def test_iqn_q_and_forward(rows, A, K, dueling):
    """a padded leading dimension (the strided staging); FFQfunc.forward against the
    reference on its own head outputs at the fractions its counter draws (step 0)"""
    adv, val = _case(rows, A, K, K, dueling, seed=rows)['q']
    advd, q = _view(adv, 'pad')[0], _nan(rows, A)
    greedy = torch.full((rows,), -1, dtype=torch.int32, device='cuda')
    L.call('smi_iqn_q', p(advd), advd.stride(0), p(val.to('cuda')) if dueling else None, rows, A, K,
           dueling, p(q), A, p(greedy), L.stream())
    ref = lambda a, v, dt: Q.mean_q(a.to(dt), None if v is None else v.to(dt), A, K)  # noqa: E731
    q64 = ref(adv, val, F64)
    assert _gap_ok(q64)
    _close('q', q.cpu(), ref(adv, val, F32), q64)
    assert torch.equal(greedy.cpu().long(), q64.argmax(1))
    f = FFQfunc(5, A, [16], dueling, 'cuda', torch.Generator().manual_seed(1), implicit={'act_atoms': K})
    x = torch.randn(rows, 5, generator=torch.Generator().manual_seed(2)).to('cuda')
    tau = torch.from_numpy(Q.taus(0, 0, 0, 0, rows, K)).to('cuda')
    la, lv = (None if t is None else t.cpu() for t in f.logits(x, tau))
    _close('forward', f(x).cpu(), ref(la, lv, F32), ref(la, lv, F64))


def test_iqn_taus_are_the_numpy_philox_draw():
    step = torch.tensor([5], dtype=torch.int32, device='cuda')

    def draw(sid, row0, rows, N=7, seed=(3 << 32) + 9):
        out = _nan(rows * N)
        L.call('smi_iqn_taus', seed, p(step), sid, row0, rows, N, p(out), L.stream())
        return out.cpu(), torch.from_numpy(Q.taus(seed, 5, sid, row0, rows, N))
    streams = [draw(sid, 0, 300) for sid in range(3)]
    for got, want in streams + [draw(0, (1 << 31) + 5, 3)]:         # a sample index past 2^32
        assert _BITS(got, want) and float(got.min()) > 0 and float(got.max()) < 1
    assert _BITS(draw(0, 100, 50)[0], streams[0][0][700:1050])      # a shard: the slice of the draw
    assert not any(torch.equal(streams[i][0], streams[j][0]) for i, j in ((0, 1), (0, 2), (1, 2)))


# ----------------------------------------------------------- learner and agents
D, A, B, NCOS = 5, 3, 32, 12
PIX = ((1, 6, 6), [[4, 3, 2]])


def _setup(N, Nt, dueling, double_q, world=1, pixel=None, **kw):
    """(config, online twin, target twin, the ranks' learners loaded from the twins; world 0: none)"""
    lc = R.dqn_config(B, [16], bool(dueling), bool(double_q)) if pixel is None else \
        QC.pix_config(B, pixel[1], [16], bool(dueling), bool(double_q))
    lc.algo.distributional.update(enabled=True, kind='implicit', atoms=N, target_atoms=Nt,
                                  act_atoms=16, embed_dim=NCOS)
    lc.algo.gamma = GAMMA
    torch.manual_seed(3)
    q, t = (Q.twin(D, A, [16], dueling, NCOS, pixel) for _ in range(2))
    ec = discrete_env_config(D, A)
    if pixel is not None:
        ec['obs_spec'] = {'pixel': {'camera0': list(pixel[0])}}
    learners = []
    for r in range(world):
        rc = copy.deepcopy(lc)
        rc.replay.batch_size = B // world
        learners.append(DQNLearner(rc, ec, dp=Group(world, r) if world > 1 else None, seed=4, **kw))
        learners[r].q_func.load_state_dict(q.state_dict())
        learners[r].q_target.load_state_dict(t.state_dict())
    return lc, q, t, learners


@pytest.mark.parametrize('form,world,Nt,pixel', [(f, 1, 8, None) for f in FORMS] +
                         [((1, 1), 1, 5, None), ((1, 1), 2, 8, None), ((1, 1), 1, 8, PIX)])
def test_iqn_learn_against_the_fp64_twin(form, world, Nt, pixel):
    """one learn() (world 2: two ranks in lockstep, one exchange) against the twin's autograd
    at the learner's own fractions, its clip_grad_norm_ + Adam(eps 1e-4) step and row losses"""
    N = 8
    lc, q, t, learners = _setup(N, Nt, *form, world, pixel)
    b = R.dqn_batches(B, D, A, 5, True, steps=1)[0] if pixel is None else \
        QC.pix_batches(B, pixel[0], A, 5, True, steps=1)[0]
    if world == 1:
        learners[0].learn(b)
    else:
        assert lockstep(learners, [cut(to_dev(b), r, B // world) for r in range(world)]) == 1
    learner = learners[0]
    tau = {k: None if getattr(learners[0], k) is None else
           torch.cat([getattr(ln, k).cpu() for ln in learners]) for k in ('tau', 'tau_next', 'tau_target')}
    assert _BITS(tau['tau'], torch.from_numpy(Q.taus(4, 0, 0, 0, B, N)))     # the whole batch's draw
    offs = {k: learner.q_func.off(v) for k, v in learner.q_func.named_parameters()}
    assert list(offs)[-2:] == ['fc_tau_layer.weight', 'fc_tau_layer.bias']
    image = lambda named: torch.cat([named[k].detach().reshape(-1)                                # noqa: E731
                                     for k in sorted(offs, key=offs.get)])    # the flat layout
    ref = {}
    for dt in (F32, F64):
        qq, tt = copy.deepcopy(q).to(dt), copy.deepcopy(t).to(dt)
        f = lambda k: torch.as_tensor(b[k]).to(dt)                                                # noqa: E731
        with torch.no_grad():
            nxt = Q.streams(qq, f('obs_next'), tau['tau_next'].to(dt), Nt) if form[1] else None
            tgt = Q.streams(tt, f('obs_next'), tau['tau_target'].to(dt), Nt)
        out = Q.iqn_td(Q.streams(qq, f('obs'), tau['tau'].to(dt), N), nxt, tgt, tau['tau'].to(dt),
                       f('actions'), f('rewards'), f('dones'), f('weights'), A, N, Nt, 1.0, GAMMA)
        assert _gap_ok(out['q_sel'])
        out['objective'].backward()
        grad = image({k: v.grad for k, v in qq.named_parameters()})
        torch.nn.utils.clip_grad_norm_(qq.parameters(), lc.algo.grad_norm_clipping)
        torch.optim.Adam(qq.parameters(), lr=lc.algo.lr, eps=1e-4).step()
        ref[dt] = (grad, image(dict(qq.named_parameters())), out['td'])
    for i, got in enumerate((learner.opt['g'], learner.q_func.flat, learner.td_error)):
        _close(('gradient', 'parameters', 'td_error')[i], got.cpu(), ref[F32][i], ref[F64][i])


def test_iqn_graph_replay_bit_exact():
    eager, graph = _setup(8, 8, 1, 1)[3][0], _setup(8, 8, 1, 1, use_graph=True)[3][0]
    seen = []
    for it, b in enumerate(R.dqn_batches(B, D, A, 3, True, steps=3)):
        for learner in (eager, graph):
            learner.learn(to_dev(b))
        for a, g in ((eager.q_func.flat, graph.q_func.flat), (eager.td_error, graph.td_error),
                     (eager.stats_buf, graph.stats_buf), (eager.tau, graph.tau)):
            assert torch.equal(a, g), it
        seen.append(graph.tau.clone())
    assert graph._graph is not None and eager._graph is None
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_iqn_agents_act_on_the_mean_over_their_fractions():
    lc, q, _, _ = _setup(8, 8, 1, 1, world=0)
    agents = QAgentBatch(lc, discrete_env_config(D, A), 8, agent_mode='eval_deterministic')
    agents.q_func.load_state_dict(q.state_dict())
    obs = torch.randn(8, D, generator=torch.Generator().manual_seed(5))
    acts = agents.act(obs.numpy()).tolist()
    assert agents.tau.numel() == 8 * 16
    with torch.no_grad():
        q64 = Q.mean_q(*Q.streams(q.double(), obs.double(), agents.tau.cpu().double(), 16), A, 16)
    assert _gap_ok(q64)
    assert acts == q64.argmax(1).tolist()
