"""Noisy linear layers: the kernels of noisy_kernels.hip through the C ABI and
through FFQfunc / DQNLearner, against tests/noisy_ref.py in fp64 on the project's
bar (_fp32_as_good_as_torch); the reference widens fp32 inputs."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from surreal_amd import _lib as L
from surreal_amd.agent import QAgentBatch
from surreal_amd.config import discrete_env_config
from surreal_amd.dqn import DQNLearner, FFQfunc, ffq_noisy_layers
from tests import dqn_ref as R
from tests import iqn_ref as IQ
from tests import noisy_ref as NR
from tests import qconv_ref as QC
from tests import qr_ref as QR
from tests.dp_harness import Group, cut, lockstep, to_dev
from tests.ops_ref import adam_ref
from tests.test_gpu_iqn import _BITS, _close, _gap_ok, _nan      # the project's bar, printed
from tests.test_gpu_iqn import _view as _iqn_view

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
p = L.ptr
# '': compact at an aligned base; 'pad' / 'odd': test_gpu_iqn's padded rows / base 4 bytes off
_view = lambda t, layout: _iqn_view(t, layout) if layout else (t.cuda(), t.shape[1])   # noqa: E731


# below one tile (dwords); the exact tile (16-byte loads); one past the tile in M and N with a
# K tail off 4; many K-steps and a tail; a wide head; many rows on a narrow head
SHAPES = [(3, 5, 7), (64, 64, 64), (70, 33, 65), (9, 517, 40), (5, 64, 1000), (130, 100, 6)]
CASES = [(s, relu, '', '') for s in SHAPES for relu in (1, 0)] + \
    [(s, 1, lay, '') for s in ((64, 64, 64), (70, 33, 65)) for lay in ('pad', 'odd')] + \
    [((70, 33, 65), 1, '', 'f0'), ((64, 64, 64), 0, '', 'sig0')]


@pytest.mark.parametrize('shape,relu,layout,special', CASES)
def test_noisy_forward_and_dx_against_fp64(shape, relu, layout, special):
    rows, K, N = shape
    g = torch.Generator().manual_seed(rows * 1000 + K + N)
    rn = lambda *s: torch.randn(*s, generator=g)                              # noqa: E731
    x, wmu, wsig, bmu, bsig = rn(rows, K), rn(N, K) / K ** 0.5, rn(N, K) / K ** 0.5, rn(N), rn(N)
    fi, fo, dy = rn(K), rn(N), rn(rows, N)
    if special == 'f0':
        fi, fo = torch.zeros(K), torch.zeros(N)
    if special == 'sig0':
        wsig = torch.zeros(N, K)
    refs = {}
    for dt in (F32, F64):
        xs = x.to(dt).requires_grad_()
        pre = NR.linear(xs, *(t.to(dt) for t in (wmu, wsig, bmu, bsig, fi, fo)))
        y = torch.relu(pre) if relu else pre
        # dX through THIS layer with the ReLU mask of its input activation x (x > 0)
        dx, = torch.autograd.grad(pre, xs, dy.to(dt))
        refs[dt] = (y.detach(), (dx * (x > 0)).detach() if relu else dx.detach())
    bm, bs, fiv, fov = (t.cuda() for t in (bmu, bsig, fi, fo))
    (xv, ldx), (wm, ldw), (ws, _), (dyv, ldg) = (_view(t, layout) for t in (x, wmu, wsig, dy))
    yv, ldy = _view(torch.zeros(rows, N), layout)
    dxv, lddx = _view(torch.zeros(rows, K), layout)
    yv.fill_(float('nan'))
    dxv.fill_(float('nan'))
    st = L.stream()
    L.call('smi_noisy_forward', p(xv), ldx, rows, K, p(wm), p(ws), ldw, p(bm), p(bs), p(fiv),
           p(fov), N, relu, p(yv), ldy, st)
    L.call('smi_noisy_backward_input', p(dyv), ldg, rows, N, p(wm), p(ws), ldw, K, p(fiv), p(fov),
           p(xv) if relu else None, ldx, p(dxv), lddx, st)
    assert L.lib().smi_last_launch() == b'noisy_gemm_kernel<dx>'
    _close('y', yv[:, :N].cpu(), refs[F32][0], refs[F64][0])
    _close('dx', dxv[:, :K].cpu(), refs[F32][1], refs[F64][1])
    if ldy > N:          # the padding columns stay untouched
        assert bool(torch.isnan(yv[:, N:]).all()) and bool(torch.isnan(dxv[:, K:]).all())


def test_noisy_sigma_grad_bit_equal():
    """three layers, the first at an odd offset (dwords), the third 16-byte able"""
    layers = [(5, 7), (8, 4), (12, 16)]
    g = torch.Generator().manual_seed(5)
    off, tab, fimg = 1, [], []
    for k, n in layers:
        tab.append((off, off + k * n, k, n))
        off += k * n + n
        off += (-off) % 4 if (k, n) == (8, 4) else 0
        fimg.append(torch.randn(k + n, generator=g))
    gmu = torch.randn(off, generator=g)
    f = torch.cat(fimg)
    gsig = _nan(off)
    exp = torch.full((off,), float('nan'))
    for (wo, bo, k, n), fl in zip(tab, fimg):
        fi, fo = fl[:k], fl[k:]
        exp[wo:wo + n * k] = (gmu[wo:wo + n * k].view(n, k) * (fo[:, None] * fi[None, :])).reshape(-1)
        exp[bo:bo + n] = gmu[bo:bo + n] * fo
    nl, t = L.noisy_table(tab)
    gmu_d, f_d = gmu.cuda(), f.cuda()
    L.call('smi_noisy_sigma_grad', p(gmu_d), p(gsig), p(f_d), nl, t, L.stream())
    got = gsig.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(exp))       # nothing outside the layers
    assert _BITS(torch.nan_to_num(got), torch.nan_to_num(exp))


def test_noisy_draw_is_the_numpy_philox_box_muller():
    widths, seed = [(5, 7), (64, 3), (33, 130)], (3 << 32) + 9
    total = sum(k + n for k, n in widths)
    step = torch.tensor([4], dtype=torch.int32, device='cuda')

    def draw(w=widths, sid=1, sd=seed, stp=step):
        n, d = L.noisy_dims(w)
        f, eps = _nan(sum(a + b for a, b in w)), _nan(sum(a + b for a, b in w))
        L.call('smi_noisy_draw', sd, p(stp), sid, n, d, p(f), p(eps), L.stream())
        return f.cpu(), eps.cpu()

    f, eps = draw()
    assert f.numel() == total and bool(torch.isfinite(f).all())
    (_, e32), (_, e64) = (NR.draw(seed, 4, 1, widths, dt) for dt in (np.float32, np.float64))
    _close('eps', eps, torch.from_numpy(e32), torch.from_numpy(e64))
    own = eps.double()
    _close('f', f, (torch.sign(eps) * eps.abs().sqrt()), torch.sign(own) * own.abs().sqrt())
    f2, _ = draw()
    assert _BITS(f, f2)
    for other in (draw(sid=2), draw(sd=seed + 1), draw(stp=step + 1)):
        assert not torch.equal(f, other[0])
    # layer 1's slice with other neighbours
    alt, _ = draw(w=[(9, 2), (64, 3)])
    assert _BITS(alt[11:], f[12:12 + 67])


# ------------------------------------------------------- model, learner, agent
B, D, A, HS = 8, 5, 3, [16, 12]
GAMMA = float(np.float32(0.99))
PIX = ((2, 6, 6), [[4, 3, 2]])             # one conv layer: 4 x 3 x 3 features


def _learners(dueling, double_q, kind=None, pixel=None, world=1, **kw):
    lc = R.dqn_config(B, HS, bool(dueling), bool(double_q)) if pixel is None else \
        QC.pix_config(B, pixel[1], HS, bool(dueling), bool(double_q))
    lc.model.noisy.update(enabled=True, sigma0=0.5)
    lc.algo.gamma = GAMMA
    if kind:
        lc.algo.distributional.update(enabled=True, kind=kind, atoms=4, act_atoms=4, embed_dim=8)
    ec = discrete_env_config(D, A)
    if pixel is not None:
        ec['obs_spec'] = {'pixel': {'camera0': list(pixel[0])}}
    out = []
    for r in range(world):
        rc = copy.deepcopy(lc)
        rc.replay.batch_size = B // world
        out.append(DQNLearner(rc, ec, seed=4, dp=Group(world, r) if world > 1 else None, **kw))
    return lc, out


def _streams(sd, noise, x, dueling, widths=(A, 1), convs=(), tau=None):
    """(adv, val | None) of the noisy twin: sd a state_dict in the dtype of x, noise an image,
    tau the fractions of an implicit model"""
    for i, (_, k, s) in enumerate(convs):
        x = torch.relu(F.conv2d(x / 255.0 if i == 0 else x, sd[f'conv_layers.{i}.weight'],
                                sd[f'conv_layers.{i}.bias'], stride=s, padding=k // 2))
    x = x.flatten(1)
    names = ('fc_action_layers', 'fc_state_layers')[:2 if dueling else 1]
    lay = ffq_noisy_layers(x.shape[1], HS, dueling, widths)
    beg = np.cumsum([0] + [k + n for k, n in lay])

    def lin(h, name, li, rows=slice(None)):
        fi, fo = noise[beg[li]:beg[li] + lay[li][0]], noise[beg[li] + lay[li][0]:beg[li + 1]][rows]
        return NR.linear(h, *(sd[f'{name}.{n}'] for n in ('weight', 'weight_sigma', 'bias', 'bias_sigma')),
                         fi, fo)
    # the stacked first layer: stream s owns rows [s h1, (s + 1) h1) of layer 0's f_out
    H1 = torch.cat([torch.relu(lin(x, f'{nm}.0', 0, slice(s * HS[0], (s + 1) * HS[0])))
                    for s, nm in enumerate(names)], 1)
    if tau is not None:
        H1 = IQ.embed(tau, H1, sd['fc_tau_layer.weight'], sd['fc_tau_layer.bias'],
                      tau.numel() // x.shape[0])[0]
    outs = []
    for s, (nm, h) in enumerate(zip(names, H1.chunk(len(names), 1))):
        for k in range(1, len(HS) + 1):
            h = lin(h, f'{nm}.{k}', s * len(HS) + k)
            h = torch.relu(h) if k < len(HS) else h
        outs.append(h)
    return outs[0], (outs[1] if dueling else None)


def _q(av):
    return av[0] if av[1] is None else (av[0] - av[0].mean(1, keepdim=True)) + av[1]


def _scalar_td(online, nxt, target, actions, rewards, dones, w):
    with torch.no_grad():
        q_sel = _q(nxt or target)
        y = rewards + GAMMA * ((1 - dones) * _q(target).gather(1, q_sel.argmax(1, keepdim=True)))
    td = _q(online).gather(1, actions.long()) - y
    loss = (w * R.huber(td)).mean()
    return {'q_sel': q_sel, 'td': td.detach().reshape(-1), 'objective': loss,
            'stats': torch.stack([loss.detach(), td.detach().abs().mean()])}


CASES_E2E = [(f, None, None, 1) for f in ((1, 1), (1, 0), (0, 1), (0, 0))] + \
    [((1, 1), 'quantile', None, 1), ((1, 1), 'implicit', None, 1), ((1, 1), None, PIX, 1),
     ((1, 1), None, None, 2)]


@pytest.mark.parametrize('form,kind,pixel,world', CASES_E2E)
def test_noisy_learn_against_the_fp64_twin(form, kind, pixel, world):
    """one learn() (world 2: two ranks in lockstep, one exchange) against autograd through the
    materialised noisy weights at the learner's own noise images (and fractions), then
    clip_grad_norm_ over mu and sigma and Adam(eps 1e-4)"""
    dueling, double_q = form
    lc, learners = _learners(*form, kind, pixel, world)
    learner = learners[0]
    q = learner.q_func
    for ln in learners:                      # the target differs from the online net
        with torch.no_grad():
            ln.q_target.flat.add_(0.05 * torch.randn(q.flat.shape, generator=torch.Generator().manual_seed(1)).cuda())
    sd0 = {k: v.cpu() for k, v in q.state_dict().items()}
    sdt = {k: v.cpu() for k, v in learner.q_target.state_dict().items()}
    flat0 = q.flat.cpu().clone()
    offs = {k: q.off(v) for k, v in q.named_parameters()}
    fc = [k for k in offs if k.startswith(('fc_action', 'fc_state'))]
    assert list(sd0) == list(offs) + [k + '_sigma' for k in fc]          # sigma after every other name
    offs.update({k + '_sigma': offs[k] + q.sig_shift for k in fc})
    ns = min(offs[k + '_sigma'] for k in fc)        # the sigma image starts where everything else ends
    assert ns == max(offs[k] + sd0[k].numel() for k in list(sd0)[:-len(fc)])
    assert all(bool((sd0[f'fc_action_layers.{k}.{n}_sigma'] == np.float32(0.5 / i ** 0.5)).all())
               for k, i in enumerate([q.dims[0]] + HS) for n in ('weight', 'bias'))
    b = R.dqn_batches(B, D, A, 5, True, steps=1)[0] if pixel is None else \
        QC.pix_batches(B, pixel[0], A, 5, True, steps=1)[0]
    if world == 1:
        learner.learn(b)
    else:
        assert lockstep(learners, [cut(to_dev(b), r, B // world) for r in range(world)]) == 1
    keys = ('noise', 'noise_next', 'noise_target', 'tau', 'tau_next', 'tau_target')
    assert all(_BITS(getattr(learners[-1], k), getattr(learner, k)) for k in keys[:3] if getattr(learner, k) is not None)
    assert all(_BITS(ln.q_func.flat, q.flat) and _BITS(ln.td_error, learner.td_error) for ln in learners)
    z = {k: None if getattr(learner, k) is None else getattr(learner, k).cpu() for k in keys}
    assert (z['noise_next'] is not None) == bool(double_q) and (z['tau'] is not None) == (kind == 'implicit')
    N = 4 if kind == 'quantile' else 1
    ref = {}
    for dt in (F32, F64):
        f = lambda k: torch.as_tensor(b[k]).to(dt).reshape(B, *((-1,) if b[k].ndim < 3 else b[k].shape[1:]))   # noqa: E731
        sd = {k: v.to(dt).clone().requires_grad_() for k, v in sd0.items()}
        tt = {k: v.to(dt) for k, v in sdt.items()}
        net = lambda w, nz, x, tau: _streams(w, z[nz].to(dt), f(x), dueling, (A * N, N),   # noqa: E731
                                             pixel[1] if pixel else (), None if z[tau] is None else z[tau].to(dt))
        with torch.no_grad():
            nxt = net(sd, 'noise_next', 'obs_next', 'tau_next') if double_q else None
            tgt = net(tt, 'noise_target', 'obs_next', 'tau_target')
        heads = (net(sd, 'noise', 'obs', 'tau'), nxt, tgt)
        rest = (f('actions'), f('rewards'), f('dones'), f('weights'))
        out = _scalar_td(*heads, *rest) if kind is None else \
            QR.qr_td(*heads, *rest, A, 4, 1.0, GAMMA) if kind == 'quantile' else \
            IQ.iqn_td(*heads, z['tau'].to(dt), *rest, A, 4, 4, 1.0, GAMMA)
        assert _gap_ok(out['q_sel'])
        out['objective'].backward()
        g = torch.zeros(flat0.numel(), dtype=dt)
        for k, o in offs.items():
            g[o:o + sd[k].numel()] = sd[k].grad.reshape(-1)
        p1 = adam_ref(flat0, g, torch.zeros_like(g), torch.zeros_like(g), 1, lc.algo.lr, 0.9, 0.999,
                      1e-4, 0.0, float(lc.algo.grad_norm_clipping), 0.0)[0]
        ref[dt] = (out['td'], g, p1, out['stats'])
    g = learner.opt['g'].cpu()
    assert float(ref[F64][1][ns:].abs().max()) > 0
    _close('td_error', learner.td_error.cpu(), ref[F32][0], ref[F64][0])
    _close('gradient mu', g[:ns], ref[F32][1][:ns], ref[F64][1][:ns])
    _close('gradient sigma', g[ns:], ref[F32][1][ns:], ref[F64][1][ns:])
    _close('parameters', q.flat.cpu(), ref[F32][2], ref[F64][2])
    _close('stats', learner.stats_buf.cpu(), ref[F32][3], ref[F64][3])


def test_noisy_graph_replay_bit_exact():
    eager, graph = _learners(1, 1)[1][0], _learners(1, 1, use_graph=True)[1][0]
    seen = []
    for it, b in enumerate(R.dqn_batches(B, D, A, 3, True, steps=3)):
        for learner in (eager, graph):
            learner.learn(to_dev(b))
        for a, g in ((eager.q_func.flat, graph.q_func.flat), (eager.td_error, graph.td_error),
                     (eager.stats_buf, graph.stats_buf), (eager.noise, graph.noise)):
            assert torch.equal(a, g), it
        seen.append(graph.noise.clone())
    assert graph._graph is not None and eager._graph is None
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


def test_noisy_state_dict_round_trip_and_eval_forward():
    a, fresh = _learners(1, 1)[1][0], _learners(1, 1)[1][0]
    a.learn(R.dqn_batches(B, D, A, 5, True, steps=1)[0])          # moves mu and sigma
    sd = a.q_func.state_dict()
    assert not torch.equal(a.q_func.flat, fresh.q_func.flat)
    fresh.q_func.load_state_dict({k: v.cpu() for k, v in sd.items()})
    assert list(fresh.q_func.state_dict()) == list(sd) and _BITS(fresh.q_func.flat, a.q_func.flat)
    assert list(sd)[-2:] == ['fc_state_layers.2.weight_sigma', 'fc_state_layers.2.bias_sigma']
    # eval(): the mu parameters through the plain layers, bit for bit
    plain = FFQfunc(D, A, HS, True, 'cuda')
    plain.load_state_dict({k: v for k, v in sd.items() if not k.endswith('_sigma')})
    x = torch.randn(9, D, generator=torch.Generator().manual_seed(2)).cuda()
    assert _BITS(a.q_func.eval()(x), plain(x))
    assert not torch.equal(a.q_func.train()(x), plain(x)) and a.q_func.noise is not None


def test_noisy_agents_are_greedy_on_the_noisy_net():
    import random
    lc, (learner,) = _learners(1, 1)
    sd = {k: v.cpu() for k, v in learner.q_func.state_dict().items()}
    obs = torch.randn(8, D, generator=torch.Generator().manual_seed(5))
    agents = QAgentBatch(lc, discrete_env_config(D, A), 8, agent_mode='training')
    agents.load_module_dict({'q_func': learner.q_func})
    state = random.getstate()
    acts = agents.act(obs.numpy()).tolist()
    assert random.getstate() == state and agents.T.tolist() == [1] * 8
    sd64 = {k: v.double() for k, v in sd.items()}
    q64 = _q(_streams(sd64, agents.noise.cpu().double(), obs.double(), True))
    assert _gap_ok(q64)
    assert acts == q64.argmax(1).tolist()
    first = agents.noise.clone()
    agents.act(obs.numpy())
    assert not torch.equal(first, agents.noise)
    det = QAgentBatch(lc, discrete_env_config(D, A), 8, agent_mode='eval_deterministic')
    det.load_module_dict({'q_func': learner.q_func})
    mu64 = _q(_streams(sd64, torch.zeros_like(first).cpu().double(), obs.double(), True))
    assert _gap_ok(mu64)
    assert det.act(obs.numpy()).tolist() == mu64.argmax(1).tolist() and det.noise is None
