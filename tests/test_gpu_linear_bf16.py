"""The bf16 dense layers (surreal_amd/csrc/linear_bf16_kernels.hip,
smi_linear_forward_bf16 / smi_linear_backward_input_bf16) and model.fc_dtype =
'bf16'.

A shape is the GEMM's (M, K, N): M rows, a reduction of K, N output columns,
so the forward runs in_dim K -> out_dim N and the input gradient out_dim K ->
in_dim N.  Layer parity is the fp32 dense layers' bar (_fp32_as_good_as_torch,
slack 1e-6) on operands that are exact in bf16: the kernel then computes the
sums torch fp32 computes.  The rounding itself is held to fp64 over operands
rounded on the host, on the same bar.

The learner is held to a reference that rounds where the kernels round
(_Rounding, fp64: x and W in a forward, dy and W in an input gradient, nothing
in the weight and bias gradients).  Its bar is d / 4, d the largest scaled
deviation between that reference and the plain fp64 one after the same steps
(the rule of the bf16 convolutions: a boundary flip moves one term by one bf16
ulp, a missing or misplaced rounding lands at ~d).  Both references are
computed here, on the CPU: d is 9.6e-3 at the low-dimensional case and 2.6e-3
at pix_small; the learner on one MI355X lies 1.1e-7 and 1.4e-7 from the
rounding reference.  Over all steps the rounding reference's smallest margin
between the best and the second-best action value where double-Q takes its
arg-max is at least MARGIN of the value scale (asserted on the CPU, before the
GPU runs), so no flipped arg-max hides in or fakes a failure."""
import copy
import functools

import pytest
import torch

from surreal_amd import _lib as L
from surreal_amd.config import discrete_env_config, discrete_pixel_env_config
from surreal_amd.dqn import DQNLearner, FFQfunc
from tests import dqn_ref as R
from tests import qconv_ref as Q
from tests import views as V
from tests.test_gpu_conv2d import E_ARG, NAN
from tests.test_gpu_conv2d_bf16 import _bf16, _deviation
from tests.test_gpu_ddpg import _fp32_as_good_as_torch
from tests.test_gpu_linear_views import ACT, RED, _In, _last, _Out, _weights

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SPLIT = (24, 800, 48)               # 1 tile, 13 chunks: 5 slabs of 3 chunks, the last of 32


def setup_module(m):
    L.ensure_workspace(DEV)


def _form(direction, shape):
    name = 'linear_bf16_kernel<%s,%d>' % (direction, 16 if shape[2] <= 16 else 64)
    return RED % name if shape == SPLIT else name


def _forward(x, W, b, act, view, check=True):
    (M, K), N = x.shape, W.shape[0]
    xo, wo, bo = _In(x, view), _In(W, view), (None if b is None else _In(b, view))
    y = _Out(M, N, view)
    L.call('smi_linear_forward_bf16', xo.ptr, xo.ld, M, K, wo.ptr, wo.ld, bo.ptr if bo else None, N,
           act, y.ptr, y.ld, L.stream())
    assert _last() == _form('fwd', (M, K, N))
    if check:
        return y.check()
    V.assert_untouched(y.buf, M, N, y.ld, y.off)
    return V.read_out(y.buf, M, N, y.ld, y.off)


def _backward(dy, W, mask, view, check=True):
    (M, K), N = dy.shape, W.shape[1]
    dyo, wo = _In(dy, view), _In(W, view)
    mo = None if mask is None else _In(mask, 'wide3')              # ldm > in_dim
    dx = _Out(M, N, view)
    L.call('smi_linear_backward_input_bf16', dyo.ptr, dyo.ld, M, K, wo.ptr, wo.ld, N,
           mo.ptr if mo else None, mo.ld if mo else 0, dx.ptr, dx.ld, L.stream())
    assert _last() == _form('dx', (M, K, N))
    if check:
        return dx.check()
    V.assert_untouched(dx.buf, M, N, dx.ld, dx.off)
    return V.read_out(dx.buf, M, N, dx.ld, dx.off)


def _operands(shape, direction, seed=0):
    """fwd: x [M][K], W [N][K], b [N]; dx: dy [M][K], W [K][N], mask [M][N]"""
    M, K, N = shape
    g = torch.Generator().manual_seed(M * 131 + K * 17 + N + seed)
    a = torch.randn(M, K, generator=g)
    if direction == 'fwd':
        W, b = _weights(g, N, K)
        return a, W, b
    return a, _weights(g, K, N)[0], V.relu_mask(M, N, g)


# (shape, act, bias, view); 'off1wide3': every leading dimension 3 wider and every
# base one float off 16 bytes (dword loads), 'wide4': strided and still 16-byte
FWD_CASES = [((1, 1, 1), 0, True, 'tight'), ((5, 17, 6), 1, True, 'off1wide3'),
             ((5, 17, 6), 2, False, 'tight'), ((16, 64, 64), 0, False, 'tight'),
             ((16, 64, 64), 1, True, 'off1wide3'), ((67, 130, 70), 2, True, 'off1wide3'),
             ((67, 130, 70), 1, False, 'tight'), ((130, 64, 16), 0, True, 'tight'),
             ((130, 64, 16), 2, True, 'off1wide3'), (SPLIT, 1, True, 'tight'),
             (SPLIT, 2, False, 'off1wide3'), (SPLIT, 0, True, 'wide4')]


@pytest.mark.parametrize('shape,act,bias,view', FWD_CASES,
                         ids=['%dx%dx%d-act%d%s-%s' % (*c[0], c[1], '' if c[2] else '-nob', c[3])
                              for c in FWD_CASES])
def test_forward_on_bf16_exact_operands(shape, act, bias, view):
    x, W, b = _operands(shape, 'fwd')
    x, W, b = _bf16(x), _bf16(W), (b if bias else None)
    got = _forward(x, W, b, act, view)
    z32 = x @ W.t() + (b if bias else 0)
    z64 = x.double() @ W.double().t() + (b.double() if bias else 0)
    _fp32_as_good_as_torch(got, ACT[act](z32), ACT[act](z64))


# (shape, masked, view)
DX_CASES = [((1, 1, 1), False, 'tight'), ((5, 17, 6), True, 'off1wide3'), ((5, 17, 6), False, 'tight'),
            ((16, 64, 64), True, 'tight'), ((16, 64, 64), False, 'wide4'),
            ((67, 130, 70), True, 'off1wide3'), ((67, 130, 70), False, 'tight'),
            ((130, 64, 16), True, 'tight'), ((130, 64, 16), True, 'off1wide3'), (SPLIT, True, 'tight'),
            (SPLIT, False, 'off1wide3'), (SPLIT, True, 'wide4')]


@pytest.mark.parametrize('shape,masked,view', DX_CASES,
                         ids=['%dx%dx%d%s-%s' % (*c[0], '-mask' if c[1] else '', c[2]) for c in DX_CASES])
def test_backward_input_on_bf16_exact_operands(shape, masked, view):
    dy, W, mask = _operands(shape, 'dx')
    dy, W = _bf16(dy), _bf16(W)
    got = _backward(dy, W, mask if masked else None, view)
    keep = (mask > 0) if masked else torch.ones_like(mask, dtype=torch.bool)
    assert bool((got[~keep] == 0).all())                  # exact and negative zeros do not pass
    _fp32_as_good_as_torch(got, (dy @ W) * keep, (dy.double() @ W.double()) * keep)


@pytest.mark.parametrize('direction', ['fwd', 'dx'])
@pytest.mark.parametrize('shape', [(67, 130, 70), SPLIT], ids=['edges', 'split'])
def test_staging_rounds_to_nearest_even(direction, shape):
    """generic fp32 operands against fp64 over the operands rounded on the host;
    then a NaN and an infinity in two rows of the row operand: exactly those
    output rows are non-finite"""
    a, W, third = _operands(shape, direction, seed=7)
    assert not torch.equal(_bf16(a), a) and not torch.equal(_bf16(W), W)
    run = (lambda t, check=True: _forward(t, W, None, 0, 'off1wide3', check)) if direction == 'fwd' \
        else (lambda t, check=True: _backward(t, W, None, 'off1wide3', check))
    ra, rW = _bf16(a), _bf16(W)
    r32, r64 = (ra @ rW.t(), ra.double() @ rW.double().t()) if direction == 'fwd' \
        else (ra @ rW, ra.double() @ rW.double())
    _fp32_as_good_as_torch(run(a), r32, r64)
    bad = a.clone()
    bad[3 % shape[0], 5] = NAN
    bad[-1, 2] = float('inf')
    finite = torch.isfinite(run(bad, check=False))
    want = torch.ones_like(finite)
    want[3 % shape[0]] = want[-1] = False
    assert torch.equal(finite, want)


@pytest.mark.parametrize('direction', ['fwd', 'dx'])
def test_split_call_twice_is_bit_identical(direction):
    a, W, third = _operands(SPLIT, direction, seed=3)
    run = (lambda: _forward(a, W, third, 2, 'tight')) if direction == 'fwd' \
        else (lambda: _backward(a, W, third, 'tight'))
    assert torch.equal(run().view(torch.int32), run().view(torch.int32))


@pytest.mark.parametrize('entry', ['forward', 'backward_input'])
def test_argument_errors_leave_the_output_untouched(entry):
    """the fp32 entry's refusals: same code, nothing written"""
    lib, P, st = L.lib(), L.ptr, L.stream()
    M, K, N = 5, 17, 6
    a, W, third = (t.to(DEV) for t in _operands((M, K, N), 'fwd' if entry == 'forward' else 'dx'))
    out = torch.full((M, N), NAN, device=DEV)

    def call(sfx, a=a, W=W, out=out, rows=M, lda=K, ldw=W.shape[1], ldo=N, ldm=N, act=1):
        if entry == 'forward':
            return getattr(lib, 'smi_linear_forward' + sfx)(
                P(a), lda, rows, K, P(W), ldw, P(third), N, act, P(out), ldo, st)
        return getattr(lib, 'smi_linear_backward_input' + sfx)(
            P(a), lda, rows, K, P(W), ldw, N, P(third), ldm, P(out), ldo, st)
    bad = [dict(a=None), dict(W=None), dict(out=None), dict(rows=-1), dict(lda=K - 1),
           dict(ldw=W.shape[1] - 1), dict(ldo=N - 1)]
    bad.append(dict(act=3) if entry == 'forward' else dict(ldm=N - 1))
    for kw in bad:
        assert call('_bf16', **kw) == call('', **kw) == E_ARG, kw
        assert lib.smi_last_error()
    assert call('_bf16', rows=0) == call('', rows=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call('_bf16') == 0                            # and the same operands do run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------ model and learner
MARGIN = 1e-3


class _RoundedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return _bf16(x) @ _bf16(w).t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return _bf16(dy) @ _bf16(w), dy.t() @ x, dy.sum(0)


class _Rounding(object):
    """mixed into FFQfuncRef / QConvRef: every FC layer rounds what the kernels round"""

    def _stream(self, layers, x):
        for k, lin in enumerate(layers):
            z = _RoundedLinear.apply(x, lin.weight, lin.bias)
            x = torch.relu(z) if k < len(layers) - 1 else z
        return x


def _ref_run(ref, init, batches, rounding):
    """(state_dict + td_error + q of the first batch after every step, smallest
    scaled arg-max margin) of a reference learner over the batches"""
    ref.load(init)
    if rounding:
        for net in (ref.q_func, ref.q_target):
            net.__class__ = type('Rounding', (_Rounding, type(net)), {})
    margin = float('inf')
    for b in batches:
        td = ref.optimize(b['obs'], b['actions'], b['rewards'], b['obs_next'], b['dones'],
                          b.get('weights'))[1]
        top = ref.last['scanned'].topk(2, dim=1)[0]
        margin = min(margin, float((top[:, 0] - top[:, 1]).min() / ref.last['scanned'].abs().max()))
    with torch.no_grad():
        q = ref.q_func(torch.as_tensor(batches[0]['obs']).to(ref.dtype))
    return dict(ref.q_func.state_dict(), td_error=td, q=q), margin


@functools.lru_cache(None)
def _case(name):
    """(config, env config, init, batches, the rounding reference's result, d)"""
    if name == 'lowdim':
        D, A, seed = 5, 3, 0
        lc = R.dqn_config(24, [32, 32], True, True)
        ec, init = discrete_env_config(D, A), R.make_init(lc, D, A, seed)
        batches = R.dqn_batches(24, D, A, seed, True, steps=Q.PIX_STEPS)
        mk = lambda: R.DQNLearnerRef(lc, D, A, torch.float64)                  # noqa: E731
    else:
        lc, shape, A, init, batches = Q.pix_case(name)
        ec = discrete_pixel_env_config(shape, A)
        mk = lambda: Q.PixLearnerRef(lc, shape, A, torch.float64)              # noqa: E731
    rounding, margin = _ref_run(mk(), init, batches, True)
    assert margin >= MARGIN, f'{name}: arg-max margin {margin:.2e}: choose another seed'
    d = _deviation(_ref_run(mk(), init, batches, False)[0], rounding)
    return lc, ec, init, batches, rounding, d


def _learner(lc, ec, init, **kw):
    learner = DQNLearner(lc, ec, **kw)
    learner.q_func.load_state_dict(init['q_func'])
    learner.q_target.load_state_dict(init['q_target'])
    return learner


def _dev(b):
    return {k: torch.as_tensor(v).to(DEV) if torch.as_tensor(v).dtype == torch.uint8
            else torch.as_tensor(v, dtype=torch.float32).to(DEV) for k, v in b.items()}


def _bits_equal(a, b):
    return all(torch.equal(getattr(a, n).flat, getattr(b, n).flat) for n in ('q_func', 'q_target')) \
        and torch.equal(a.td_error, b.td_error) and torch.equal(a.stats_buf, b.stats_buf)


@pytest.mark.parametrize('name', ['lowdim', 'pix_small'])
def test_learn_forward_and_graph_replay_with_bf16_fc(name):
    """PIX_STEPS eager steps against the rounding reference (d measured: 9.6e-3
    at lowdim, 2.6e-3 at pix_small; the learner 1.1e-7 and 1.4e-7 on one
    MI355X), forward() after them, every step against its graph replay"""
    lc, ec, init, batches, rounding, d = _case(name)
    lc = copy.deepcopy(lc)
    lc.model.fc_dtype = 'bf16'
    eager, graph = _learner(lc, ec, init), _learner(lc, ec, init, use_graph=True)
    assert isinstance(eager.q_func, FFQfunc) and eager.q_func.fc_dtype == eager.q_target.fc_dtype == 'bf16'
    for b in batches:                                    # replayed steps against eager ones
        eager.learn(_dev(b))
        graph.learn(_dev(b))
        assert _bits_equal(eager, graph)
    assert graph._graph is not None
    q = eager.q_func(_dev(batches[0])['obs'])
    got = _deviation(dict(eager.q_func.state_dict(), td_error=eager.td_error, q=q), rounding)
    print(f'{name}: d = {d:.3e}, learner within {got:.3e} of the rounding reference (bar d / 4)')
    assert 0 < got <= d / 4
    # 'fp32' is the model without the key, bit for bit
    lc32, lc0 = copy.deepcopy(lc), copy.deepcopy(lc)
    lc32.model.fc_dtype = 'fp32'
    del lc0['model']['fc_dtype']
    a, b = _learner(lc32, ec, init), _learner(lc0, ec, init)
    a.learn(_dev(batches[0]))
    b.learn(_dev(batches[0]))
    torch.cuda.synchronize()
    assert _bits_equal(a, b)
