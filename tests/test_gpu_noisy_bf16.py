"""The bf16 noisy layers (surreal_amd/csrc/noisy_bf16_kernels.hip,
smi_noisy_forward_bf16 / smi_noisy_backward_input_bf16) and model.noisy.dtype.

A shape is the GEMM's (M, K, N): the forward runs in_dim K -> out_dim N, the
input gradient out_dim K -> in_dim N; ks [K] scales the sigma chain's row
operand, ns [N] the sigma sums.  Layer parity is the fp32 dense layers' bar
(_fp32_as_good_as_torch) on operands that are exact in bf16 with noise from
+-{0.5, 1, 2} (the product with it is exact too); the rounding is held to fp64
over operands rounded on the host as the header specifies, bf16(fp32(a * ks)),
on the same bar, after asserting that rounding a first misses that bar."""
import pytest
import torch

from surreal_amd import _lib as L
from surreal_amd.agent import QAgentBatch
from surreal_amd.config import discrete_env_config
from surreal_amd.dqn import DQNLearner, _QNet
from tests import dqn_ref as R
from tests import qconv_ref as Q
from tests import test_gpu_noisy as T
from tests import views as V
from tests.dp_harness import to_dev
from tests.ops_ref import adam_ref
from tests.test_gpu_conv2d import E_ARG, NAN
from tests.test_gpu_conv2d_bf16 import _bf16, _deviation
from tests.test_gpu_ddpg import _fp32_as_good_as_torch
from tests.test_gpu_linear_views import ACT, _In, _last, _Out, _weights

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SPLIT = (24, 800, 48)               # 1 tile, 13 chunks: 5 slabs of 3 chunks, the last of 32
ENTRY = {'fwd': 'smi_noisy_forward_bf16', 'dx': 'smi_noisy_backward_input_bf16'}


def setup_module(m):
    L.ensure_workspace(DEV)


def _operands(shape, d, seed=0, exact=False):
    """a [M][K], W_mu and W_sig (fwd [N][K], dx [K][N]), ks [K], ns [N], b_mu, b_sig [N], mask [M][N]"""
    M, K, N = shape
    g = torch.Generator().manual_seed(M * 131 + K * 17 + N + seed)
    a = torch.randn(M, K, generator=g)
    Wm, bm = _weights(g, *((N, K) if d == 'fwd' else (K, N)))
    Ws, bs = _weights(g, *((N, K) if d == 'fwd' else (K, N)))
    ks, ns = torch.randn(K, generator=g), torch.randn(N, generator=g)
    if exact:
        a, Wm, Ws = _bf16(a), _bf16(Wm), _bf16(Ws)
        pick = lambda n: torch.tensor([.5, 1., 2., -.5, -1., -2.])[torch.randint(0, 6, (n,), generator=g)]  # noqa: E731
        ks, ns = pick(K), pick(N)
    return a, Wm, Ws, ks, ns, torch.randn(N, generator=g), torch.randn(N, generator=g), V.relu_mask(M, N, g)


def _run(d, ops, act=0, masked=False, view='tight', wviews=None, check=True):
    a, Wm, Ws, ks, ns, bm, bs, mask = ops
    (M, K), N = a.shape, ns.numel()
    ao, wm, ws = _In(a, view), _In(Wm, (wviews or (view,) * 2)[0]), _In(Ws, (wviews or (view,) * 2)[1])
    fk, fn, out = _In(ks, 'tight' if view == 'tight' else 'off1'), _In(ns, 'off1'), _Out(M, N, view)
    assert wm.ld == ws.ld
    if d == 'fwd':
        b1, b2 = (_In(bm, view), _In(bs, view)) if act else (None, None)      # act 0: NULL biases
        L.call(ENTRY[d], ao.ptr, ao.ld, M, K, wm.ptr, ws.ptr, wm.ld, b1 and b1.ptr, b2 and b2.ptr,
               fk.ptr, fn.ptr, N, act, out.ptr, out.ld, L.stream())
    else:
        mo = _In(mask, 'wide3') if masked else None
        L.call(ENTRY[d], ao.ptr, ao.ld, M, K, wm.ptr, ws.ptr, wm.ld, N, fn.ptr, fk.ptr,
               mo and mo.ptr, mo.ld if mo else 0, out.ptr, out.ld, L.stream())
    form = 'noisy_bf16_kernel<%s,%d>' % (d, 16 if N <= 16 else 64)
    assert _last() == ('noisy_bf16_reduce_kernel<%s>' % form if (M, K, N) == SPLIT else form)
    if check:
        return out.check()
    V.assert_untouched(out.buf, M, N, out.ld, out.off)
    return V.read_out(out.buf, M, N, out.ld, out.off)


def _refs(d, ops, act, masked, a, a_sig, Wm, Ws):
    """the header's formula on the given (rounded or not) operands, in fp32 and in fp64"""
    def formula(a, a_sig, Wm, Ws, ns, bm, bs):
        if d == 'fwd':
            return ACT[act]((a @ Wm.t() + bm) + ns * (a_sig @ Ws.t() + bs))
        return (a @ Wm + ns * (a_sig @ Ws)) * ((ops[7] > 0) if masked else 1)
    bm, bs = (ops[5], ops[6]) if act else (torch.zeros_like(ops[5]),) * 2      # act 0 runs with NULL biases
    return [formula(*(t.to(dt) for t in (a, a_sig, Wm, Ws, ops[4], bm, bs))) for dt in (torch.float32, torch.float64)]


# (shape, act (fwd) = masked (dx), view, (W_mu view, W_sig view) | None): 'off1wide3' is dword loads
# everywhere; ('tight', 'off1') / ('off1', 'tight') put one of the two weight images one float off
CASES = [((1, 1, 1), 0, 'tight', None), ((5, 17, 6), 1, 'off1wide3', None), ((5, 17, 6), 2, 'tight', None),
         ((16, 64, 64), 1, 'tight', ('tight', 'off1')), ((16, 64, 64), 0, 'off1wide3', None),
         ((67, 130, 70), 2, 'off1wide3', None), ((67, 130, 70), 1, 'tight', None),
         ((130, 64, 16), 0, 'tight', ('off1', 'tight')), ((130, 64, 16), 1, 'off1wide3', None),
         (SPLIT, 1, 'tight', ('off1', 'tight')), (SPLIT, 2, 'off1wide3', None), (SPLIT, 0, 'tight', None)]


@pytest.mark.parametrize('d', ['fwd', 'dx'])
@pytest.mark.parametrize('shape,act,view,wviews', CASES,
                         ids=['%dx%dx%d-%d-%s%s' % (*c[0], c[1], c[2], '-' + '.'.join(c[3]) if c[3] else '')
                              for c in CASES])
def test_parity_on_bf16_exact_operands(d, shape, act, view, wviews):
    ops = _operands(shape, d, exact=True)
    a, Wm, Ws, ks = ops[:4]
    got = _run(d, ops, act, bool(act), view, wviews)
    r32, r64 = _refs(d, ops, act, bool(act), a, a * ks, Wm, Ws)
    if d == 'dx' and act:
        assert bool((got[~(ops[7] > 0)] == 0).all()) and not bool(torch.signbit(got[~(ops[7] > 0)]).any())
    _fp32_as_good_as_torch(got, r32, r64)


@pytest.mark.parametrize('d', ['fwd', 'dx'])
@pytest.mark.parametrize('shape', [(67, 130, 70), SPLIT], ids=['edges', 'split'])
def test_staging_rounds_the_fp32_product_once(d, shape):
    """generic operands and noise against fp64 over bf16(a), bf16(fp32(a * ks)), bf16(W); rounding a
    before the multiply misses the bar (asserted before the GPU call); then a NaN and an infinity
    in two rows of the row operand: exactly those output rows are non-finite"""
    ops = _operands(shape, d, seed=7)
    a, Wm, Ws, ks = ops[:4]
    r32, r64 = _refs(d, ops, 0, False, _bf16(a), _bf16(a * ks), _bf16(Wm), _bf16(Ws))
    wrong = _refs(d, ops, 0, False, _bf16(a), _bf16(a) * ks, _bf16(Wm), _bf16(Ws))[0]
    with pytest.raises(AssertionError):
        _fp32_as_good_as_torch(wrong, r32, r64)
    _fp32_as_good_as_torch(_run(d, ops, view='off1wide3'), r32, r64)
    bad = a.clone()
    bad[3 % shape[0], 5] = NAN
    bad[-1, 2] = float('inf')
    finite = torch.isfinite(_run(d, (bad,) + ops[1:], view='off1wide3', check=False))
    want = torch.ones_like(finite)
    want[3 % shape[0]] = want[-1] = False
    assert torch.equal(finite, want)


@pytest.mark.parametrize('d', ['fwd', 'dx'])
def test_split_call_twice_is_bit_identical(d):
    ops = _operands(SPLIT, d, seed=3)
    assert torch.equal(_run(d, ops, 2, True).view(torch.int32), _run(d, ops, 2, True).view(torch.int32))


@pytest.mark.parametrize('d', ['fwd', 'dx'])
def test_argument_errors_leave_the_output_untouched(d):
    """the fp32 entry's refusals: same code, nothing written"""
    lib, P, st = L.lib(), L.ptr, L.stream()
    M, K, N = 5, 17, 6
    a, Wm, Ws, ks, ns, bm, bs, mask = (t.to(DEV) for t in _operands((M, K, N), d))
    out = torch.full((M, N), NAN, device=DEV)

    def call(sfx, a=a, Wm=Wm, Ws=Ws, ks=ks, ns=ns, out=out, rows=M, lda=K, ldw=Wm.shape[1], ldo=N, ldm=N,
             act=1):
        if d == 'fwd':
            return getattr(lib, 'smi_noisy_forward' + sfx)(
                P(a), lda, rows, K, P(Wm), P(Ws), ldw, P(bm), P(bs), P(ks), P(ns), N, act, P(out), ldo, st)
        return getattr(lib, 'smi_noisy_backward_input' + sfx)(
            P(a), lda, rows, K, P(Wm), P(Ws), ldw, N, P(ns), P(ks), P(mask), ldm, P(out), ldo, st)
    bad = [dict(a=None), dict(Wm=None), dict(Ws=None), dict(ks=None), dict(ns=None), dict(out=None),
           dict(rows=0), dict(lda=K - 1), dict(ldw=Wm.shape[1] - 1), dict(ldo=N - 1),
           dict(act=3) if d == 'fwd' else dict(ldm=N - 1)]
    for kw in bad:
        assert call('_bf16', **kw) == call('', **kw) == E_ARG, kw
        assert lib.smi_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call('_bf16') == 0                            # and the same operands do run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------ model, learner, agent
MARGIN = 1e-3


def _rounded(all_):
    """noisy_ref.linear rounding where the kernels round (all_: the weight gradient's dy and x too;
    db from the unrounded dy, the sigma gradients as smi_noisy_sigma_grad forms them)"""
    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, wmu, wsig, bmu, bsig, fi, fo):
            ctx.save_for_backward(x, wmu, wsig, fi, fo)
            return (_bf16(x) @ _bf16(wmu).t() + bmu) + fo * (_bf16(x * fi) @ _bf16(wsig).t() + bsig)

        @staticmethod
        def backward(ctx, dy):
            x, wmu, wsig, fi, fo = ctx.saved_tensors
            dw = (_bf16(dy).t() @ _bf16(x)) if all_ else dy.t() @ x
            return (_bf16(dy) @ _bf16(wmu) + fi * (_bf16(dy * fo) @ _bf16(wsig)), dw,
                    dw * torch.outer(fo, fi), dy.sum(0), dy.sum(0) * fo, None, None)
    return Fn.apply


def _config(kind, pixel, dtype):
    lc = T.QC.pix_config(T.B, pixel[1], T.HS) if pixel else R.dqn_config(T.B, T.HS)
    lc.model.noisy.update(enabled=True, sigma0=0.5, **({'dtype': dtype} if dtype else {}))
    lc.algo.gamma, lc.algo.target_network_update_freq = T.GAMMA, 10 ** 6
    if kind:
        lc.algo.distributional.update(enabled=True, kind=kind, atoms=4, act_atoms=4, embed_dim=8)
    ec = discrete_env_config(T.D, T.A)
    if pixel:
        ec['obs_spec'] = {'pixel': {'camera0': list(pixel[0])}}
    return lc, ec


def _learner(lc, ec, **kw):
    ln = DQNLearner(lc, ec, seed=4, **kw)
    with torch.no_grad():                    # the target differs from the online net
        ln.q_target.flat.add_(0.05 * torch.randn(ln.q_target.flat.shape,
                                                 generator=torch.Generator().manual_seed(1)).cuda())
    return ln


def _draws(ln, steps):
    """the noise images (and fractions) learn() will draw at Adam steps 0 .. steps - 1"""
    net, out = _QNet(ln.q_func, {}), []
    for s in range(steps):
        st = torch.tensor([s], dtype=torch.int32, device=DEV)
        z = {n: net.draw(ln._noise_seed, st, i, n).cpu() for i, n in enumerate(KEYS[:3])}
        if ln.implicit:
            z.update({n: net.taus(ln._tau_seed, st, i, 0, T.B, ln.implicit['target_atoms' if i else 'atoms'],
                                  n).cpu() for i, n in enumerate(KEYS[3:])})
        out.append(z)
    return out


KEYS = ('noise', 'noise_next', 'noise_target', 'tau', 'tau_next', 'tau_target')


def _twin(ln, lc, kind, pixel, batches, draws):
    """test_gpu_noisy's fp64 twin over the steps with Adam: ({flat, td_error}, smallest arg-max margin)"""
    q, B, A = ln.q_func, T.B, T.A
    sd0 = {k: v.cpu() for k, v in q.state_dict().items()}
    offs = {k: q.off(v) for k, v in q.named_parameters()}
    offs.update({k + '_sigma': o + q.sig_shift for k, o in list(offs.items()) if k.startswith(('fc_action', 'fc_state'))})
    cut = lambda flat: {k: flat[o:o + sd0[k].numel()].view_as(sd0[k]).clone() for k, o in offs.items()}   # noqa: E731
    p, tt, margin = q.flat.cpu().double(), cut(ln.q_target.flat.cpu().double()), float('inf')
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t, (b, z) in enumerate(zip(batches, draws), 1):
        f = lambda k: torch.as_tensor(b[k]).double().reshape(B, *((-1,) if b[k].ndim < 3 else b[k].shape[1:]))   # noqa: E731
        sd = {k: w.requires_grad_() for k, w in cut(p).items()}
        net = lambda w, nz, x, tau: T._streams(w, z[nz].double(), f(x), True, (A, 1), pixel[1] if pixel else (),   # noqa: E731
                                               z[tau].double() if tau in z else None)
        with torch.no_grad():
            nxt, tgt = net(sd, 'noise_next', 'obs_next', 'tau_next'), net(tt, 'noise_target', 'obs_next', 'tau_target')
        heads, rest = (net(sd, 'noise', 'obs', 'tau'), nxt, tgt), (f('actions'), f('rewards'), f('dones'), f('weights'))
        out = T._scalar_td(*heads, *rest) if kind is None else \
            T.IQ.iqn_td(*heads, z['tau'].double(), *rest, A, 4, 4, 1.0, T.GAMMA)
        top = out['q_sel'].topk(2, 1)[0]
        margin = min(margin, float((top[:, 0] - top[:, 1]).min() / out['q_sel'].abs().max()))
        out['objective'].backward()
        g = torch.zeros_like(p)
        for k, o in offs.items():
            g[o:o + sd[k].numel()] = sd[k].grad.reshape(-1)
        p, m, v = adam_ref(p, g, m, v, t, lc.algo.lr, 0.9, 0.999, 1e-4, 0.0, float(lc.algo.grad_norm_clipping), 0.0)[:3]
    return {'flat': p, 'td_error': out['td']}, margin


@pytest.mark.parametrize('kind,pixel,dtype', [(None, None, 'bf16'), ('implicit', None, 'bf16_all'),
                                              (None, T.PIX, 'bf16')], ids=['lowdim', 'implicit-all', 'pix'])
def test_learn_and_graph_replay_with_bf16_noisy_layers(kind, pixel, dtype, monkeypatch):
    """PIX_STEPS steps of dueling double-Q against the fp64 twin that rounds where the kernels
    round, at the learner's own noise images; bar d / 4, d the twin's distance from the plain
    fp64 twin, both computed here on the CPU and printed.  Measured on one MI355X: lowdim d =
    6.6e-4, learner 8.9e-8; implicit-all d = 1.2e-3, learner 8.3e-8; pix d = 1.2e-3, learner 9.6e-8"""
    lc, ec = _config(kind, pixel, dtype)
    eager, graph = _learner(lc, ec), _learner(lc, ec, use_graph=True)
    assert eager.q_func.noisy_dtype == eager.q_target.noisy_dtype == dtype
    batches = R.dqn_batches(T.B, T.D, T.A, 5, True, steps=Q.PIX_STEPS) if pixel is None else \
        Q.pix_batches(T.B, pixel[0], T.A, 5, True, steps=Q.PIX_STEPS)
    draws = _draws(eager, len(batches))
    plain = _twin(eager, lc, kind, pixel, batches, draws)[0]
    monkeypatch.setattr(T.NR, 'linear', _rounded(dtype == 'bf16_all'))
    rounding, margin = _twin(eager, lc, kind, pixel, batches, draws)
    assert margin >= MARGIN, f'arg-max margin {margin:.2e}: choose another seed'
    d = _deviation(plain, rounding)
    for b in batches:                                    # replayed steps against eager ones
        eager.learn(to_dev(b))
        graph.learn(to_dev(b))
        assert all(torch.equal(getattr(eager, k).flat, getattr(graph, k).flat) for k in ('q_func', 'q_target'))
        assert torch.equal(eager.td_error, graph.td_error) and torch.equal(eager.stats_buf, graph.stats_buf)
    assert graph._graph is not None
    assert all(torch.equal(getattr(eager, k).cpu(), z) for k, z in draws[-1].items())
    got = _deviation({'flat': eager.q_func.flat, 'td_error': eager.td_error}, rounding)
    print(f'd = {d:.3e}, learner within {got:.3e} of the rounding reference (bar d / 4)')
    assert 0 < got <= d / 4


def test_fp32_value_is_the_model_without_the_key():
    a, b = _learner(*_config(None, None, 'fp32')), _learner(*_config(None, None, None))
    for ln in (a, b):
        ln.learn(to_dev(R.dqn_batches(T.B, T.D, T.A, 5, True, steps=1)[0]))
    assert torch.equal(a.q_func.flat, b.q_func.flat) and torch.equal(a.td_error, b.td_error)


def test_training_agents_are_greedy_on_the_rounding_reference(monkeypatch):
    lc, ec = _config(None, None, 'bf16')
    ln = _learner(lc, ec)
    agents = QAgentBatch(lc, ec, 8, agent_mode='training')
    agents.load_module_dict({'q_func': ln.q_func})
    assert agents.q_func.noisy_dtype == 'bf16'
    obs = torch.randn(8, T.D, generator=torch.Generator().manual_seed(5))
    acts = agents.act(obs.numpy()).tolist()
    monkeypatch.setattr(T.NR, 'linear', _rounded(False))
    sd64 = {k: v.cpu().double() for k, v in ln.q_func.state_dict().items()}
    q64 = T._q(T._streams(sd64, agents.noise.cpu().double(), obs.double(), True))
    top = q64.topk(2, 1)[0]
    sure = ((top[:, 0] - top[:, 1]) / q64.abs().max() >= MARGIN).tolist()
    assert any(sure) and all(a == r for a, r, k in zip(acts, q64.argmax(1).tolist(), sure) if k)
