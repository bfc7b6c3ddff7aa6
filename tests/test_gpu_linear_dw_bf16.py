"""smi_linear_backward_weight_bf16 and model.fc_dtype = 'bf16_all'.  A shape is
(rows, out, in).  Layers: the fp32 weight gradient's bar (_fp32_as_good_as_torch,
slack 1e-6, on the scale of the magnitudes summed), db over the UNROUNDED dy.
The learner is held to R_all: test_gpu_linear_bf16._Rounding (R_bf16) that also
rounds dy and x in the weight gradient; d_w is the deviation between the two,
where a learner that does not round there lands, the bar d_w / 4.  On the CPU d_w
is 1.3e-3 (lowdim) and 1.8e-3 (pix_small); one MI355X lies 1.1e-7 and 3.4e-6 from R_all."""
import copy
import ctypes

import pytest
import torch

from surreal_amd import _lib as L
from tests import dqn_ref as R
from tests import qconv_ref as Q
from tests import test_gpu_linear_bf16 as B
from tests import views as V
from tests.test_gpu_conv2d import E_ARG, NAN
from tests.test_gpu_conv2d_bf16 import _bf16, _deviation
from tests.test_gpu_ddpg import _fp32_as_good_as_torch
from tests.test_gpu_linear_views import RED, _In, _last, _Out

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SPLIT = (800, 48, 24)               # 1 tile, 13 chunks: 5 slabs of 3 chunks, the last of 32 rows
EDGES = (67, 70, 130)               # edge tiles in both directions and a row tail
CASES = [((1, 1, 1), 'tight'), ((5, 6, 17), 'off1wide3'), ((64, 64, 64), 'tight'), (EDGES, 'tight'),
         (EDGES, 'off1wide3'), ((130, 16, 64), 'tight'), (SPLIT, 'tight')]


def _operands(shape, seed=0):
    rows, n, k = shape
    g = torch.Generator().manual_seed(rows * 131 + n * 17 + k + seed)
    return torch.randn(rows, n, generator=g), torch.randn(rows, k, generator=g), g


def _run(dy, x, view, init=None, with_db=True):
    """(dW, db | None) of one call; init = (dW0, db0): accumulate into them"""
    L.ensure_workspace(DEV)
    (rows, n), k = dy.shape, x.shape[1]
    dyo, xo = _In(dy, view), _In(x, view)
    dw = _Out(n, k, view, init=init[0] if init else None)
    db = _Out(1, n, view, init=init[1] if init and with_db else None)
    L.call('smi_linear_backward_weight_bf16', dyo.ptr, dyo.ld, rows, n, xo.ptr, xo.ld, k, dw.ptr,
           dw.ld, db.ptr if with_db else None, 1 if init else 0, L.stream())
    name = 'linear_bf16_kernel<dw,%d>' % (16 if n <= 16 else 64)
    assert _last() == (RED % name if (rows, n, k) == SPLIT else name)
    V.assert_untouched(dw.buf, n, k, dw.ld, dw.off)
    V.assert_untouched(db.buf, 1, n if with_db else 0, db.ld, db.off)
    return V.read_out(dw.buf, n, k, dw.ld, dw.off), \
        (V.read_out(db.buf, 1, n, db.ld, db.off)[0] if with_db else None)


def _check(got, dyr, xr, dy, init=None):
    """dW against the sums over (dyr, xr), db against the sum of dy (a NaN fails either)"""
    w0, b0 = init or (torch.zeros(dyr.shape[1], xr.shape[1]), torch.zeros(dyr.shape[1]))
    mw = float((dyr.abs().t() @ xr.abs()).max() + w0.abs().max())
    _fp32_as_good_as_torch(got[0], w0 + dyr.t() @ xr, w0.double() + dyr.double().t() @ xr.double(),
                           1e-6, mw)
    if got[1] is not None:
        mb = float(dy.abs().sum(0).max() + b0.abs().max())
        _fp32_as_good_as_torch(got[1], b0 + dy.sum(0), b0.double() + dy.double().sum(0), 1e-6, mb)


@pytest.mark.parametrize('shape,view', CASES, ids=['%dx%dx%d-%s' % (*c[0], c[1]) for c in CASES])
def test_weight_gradient_on_bf16_exact_operands(shape, view):
    dy, x, g = _operands(shape)
    dy, x = _bf16(dy), _bf16(x)
    _check(_run(dy, x, view), dy, x, dy)
    if shape == SPLIT:
        plan, ws = (ctypes.c_int * 5)(), L.lib().smi_workspace_bytes() // 4
        assert L.lib().smi_diag_linear_bf16_dw_plan(48, 24, 800, ws, plan) == 5
        assert list(plan) == [64, 1, 1, 5, 192]
    if shape in (EDGES, SPLIT) and view == 'tight':     # accumulate: unsplit epilogue, reducer
        init = (torch.randn(shape[1], shape[2], generator=g), torch.randn(shape[1], generator=g))
        _check(_run(dy, x, view, init=init), dy, x, dy, init)
    if shape == EDGES:
        _check(_run(dy, x, view, with_db=False), dy, x, dy)


@pytest.mark.parametrize('shape', [EDGES, SPLIT], ids=['edges', 'split'])
def test_staging_rounds_both_operands_and_db_reads_the_unrounded_dy(shape):
    dy, x, _ = _operands(shape, seed=7)
    rdy, rx = _bf16(dy), _bf16(x)
    assert not torch.equal(rdy, dy) and not torch.equal(rx, x)
    # a db summed from rounded values misses the bar's outer bound (1e-5 of the scale) twice over
    mb = float(dy.abs().sum(0).max())
    assert float((rdy.double().sum(0) - dy.double().sum(0)).abs().max()) > 2e-5 * mb
    first = _run(dy, x, 'off1wide3')
    _check(first, rdy, rx, dy)
    if shape == SPLIT:                                   # no atomics: the same bits again
        assert all(torch.equal(s.view(torch.int32), t.view(torch.int32))
                   for s, t in zip(first, _run(dy, x, 'off1wide3')))
    # a NaN and an infinity in dy: exactly their columns' rows of dW and entries of db
    dy[3, 2], dy[-1, 5] = NAN, float('inf')
    dw, db = _run(dy, x, 'off1wide3')
    want = ~torch.isin(torch.arange(shape[1]), torch.tensor([2, 5]))
    assert torch.equal(torch.isfinite(db), want)
    assert torch.equal(torch.isfinite(dw), want[:, None].expand(-1, shape[2]))


def test_argument_errors_leave_the_outputs_untouched():
    """the fp32 entry's refusals: same code, nothing written"""
    lib, P, st = L.lib(), L.ptr, L.stream()
    rows, n, k = 5, 6, 17
    dy, x = (t.to(DEV) for t in _operands((rows, n, k))[:2])
    dw, db = torch.full((n, k), NAN, device=DEV), torch.full((n,), NAN, device=DEV)

    def call(sfx, dy=dy, x=x, dw=dw, rows=rows, n=n, k=k, ldg=n, ldx=k, lddw=k):
        return getattr(lib, 'smi_linear_backward_weight' + sfx)(
            P(dy), ldg, rows, n, P(x), ldx, k, P(dw), lddw, P(db), 0, st)
    for kw in (dict(dy=None), dict(x=None), dict(dw=None), dict(rows=-1), dict(n=0), dict(k=0),
               dict(ldg=n - 1), dict(ldx=k - 1), dict(lddw=k - 1)):
        assert call('_bf16', **kw) == call('', **kw) == E_ARG and lib.smi_last_error(), kw
    assert call('_bf16', rows=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())
    assert call('_bf16') == 0                            # and the same operands do run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())


class _RoundedAllLinear(B._RoundedLinear):
    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return _bf16(dy) @ _bf16(w), _bf16(dy).t() @ _bf16(x), dy.sum(0)


@pytest.mark.parametrize('name', ['lowdim', 'pix_small'])
def test_learn_forward_and_graph_replay_with_bf16_all(name, monkeypatch):
    """PIX_STEPS eager steps against R_all (bar d_w / 4), every step against its
    graph replay, and the forward against a 'bf16' model with the same weights"""
    lc, ec, init, batches, r_bf16, _ = B._case(name)
    ref = R.DQNLearnerRef(lc, 5, 3, torch.float64) if name == 'lowdim' \
        else Q.PixLearnerRef(lc, Q.pix_case(name)[1], Q.pix_case(name)[2], torch.float64)
    with monkeypatch.context() as mp:                    # R_all: _Rounding over the layer above
        mp.setattr(B, '_RoundedLinear', _RoundedAllLinear)
        r_all, margin = B._ref_run(ref, init, batches, True)        # on the CPU, before any GPU call
    assert margin >= B.MARGIN, f'{name}: arg-max margin {margin:.2e}: choose another seed'
    d_w = _deviation(r_bf16, r_all)
    lc, lc16 = copy.deepcopy(lc), copy.deepcopy(lc)
    lc.model.fc_dtype, lc16.model.fc_dtype = 'bf16_all', 'bf16'
    eager, graph = B._learner(lc, ec, init), B._learner(lc, ec, init, use_graph=True)
    for b in batches:
        eager.learn(B._dev(b))
        graph.learn(B._dev(b))
        assert B._bits_equal(eager, graph)
    assert graph._graph is not None
    obs = B._dev(batches[0])['obs']
    q = eager.q_func(obs)
    got = _deviation(dict(eager.q_func.state_dict(), td_error=eager.td_error, q=q), r_all)
    print(f'{name}: d_w = {d_w:.3e}, learner within {got:.3e} of R_all (bar d_w / 4)')
    assert 0 < got <= d_w / 4
    other = B._learner(lc16, ec, init)
    other.q_func.load_state_dict(eager.q_func.state_dict())
    assert torch.equal(other.q_func(obs), q)
