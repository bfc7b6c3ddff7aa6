"""Fitted edge tiles of the grouped weight-gradient launch (gemm_dwd_group_kernel,
dw_plan): every tile class the 4-wave dispatch reaches, through
smi_dw_group_begin / smi_linear_backward_weight / smi_dw_group_flush at 1100
rows (above the 512-row short-batch kernel).  out_dim 8 / 72 / 90 / 108 / 128
gives an M edge alone, M edges of 1, 2 and 3 sixteen-wide sub-tiles and none;
in_dim 78 / 90 / 100 / 127 (+ the bias column) gives N edges of 1, 2, 3 and 4.
Each result is held to the bar of the existing dW cases (test_gpu_ddpg.py:
fp32 torch against the fp64 product), with and without db, plain then
accumulating, into NaN-filled outputs, and smi_last_launch() must name the
tile classes the case was written for."""
import pytest
import torch

from surreal_amd import _lib as L
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
ROWS = 1100


def setup_module(m):
    L.ensure_workspace(DEV)


def _last():
    return L.lib().smi_last_launch().decode()


def _classes(out_dim, in_dim, db, x_aligned=True):
    """the tile classes of one GEMM's rectangles in entry order (interior, M
    edge, N edge, corner), spelled as smi_last_launch does."""
    M, N = out_dim, in_dim + (1 if db else 0)
    va = out_dim % 4 == 0 and out_dim >= 4                # dY rows of 16-byte runs
    vb = x_aligned and in_dim % 4 == 0 and in_dim >= 4
    Mf, Me, Nf, Ne = M // 64 * 64, M % 64, N // 64 * 64, N % 64
    mte = -(-Me // 16)
    nte = 0
    if Ne:
        R = Ne - (1 if db else 0)
        nte = min(4, max(1, -(-R // 15)) if db else -(-R // 16))
        if nte in (2, 3) and not x_aligned:
            nte = 4
        if mte == 1 and not vb:      # a 16-wide tail keeps the loop (and chain restarts) of its padded tiles
            nte = 4
    a = lambda mt: f'{mt}{("v" if va else "s") if mt == 4 else ""}'
    b = lambda nt: f'{nt}{("v" if vb else "s") if nt == 4 else ""}'
    out = []
    if Mf and Nf:
        out.append(f'{a(4)}x{b(4)}')
    if Me and Nf:
        out.append(f'{a(mte)}x{b(4)}')
    if Mf and Ne:
        out.append(f'{a(4)}x{b(nte)}')
    if Me and Ne:
        out.append(f'{a(mte)}x{b(nte)}')
    return out


def _form(classes):
    seen = []
    for c in classes:
        if c not in seen:
            seen.append(c)
    return f'gemm_group_reduce_kernel<gemm_dwd_group_kernel<{",".join(seen)}>>'


def _case(out_dim, in_dim, seed, x_off=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ROWS, in_dim, generator=g)
    dy = torch.randn(ROWS, out_dim, generator=g)
    xbuf = torch.empty(ROWS * in_dim + 4, device=DEV)
    xd = xbuf[x_off:x_off + ROWS * in_dim].view(ROWS, in_dim)
    xd.copy_(x)
    return x, dy, xd, dy.to(DEV)


def _check(items, st):
    """items: [(out_dim, in_dim, db, x, dy, xd, dyd)] as ONE group, plain then accumulating."""
    outs = [(torch.full((o, i), NAN, device=DEV), torch.full((o,), NAN, device=DEV))
            for o, i, *_ in items]
    for acc in (0, 1):
        L.call('smi_dw_group_begin')
        for (o, i, db, x, dy, xd, dyd), (dw, dbv) in zip(items, outs):
            L.call('smi_linear_backward_weight', L.ptr(dyd), o, ROWS, o, L.ptr(xd), i, i, L.ptr(dw), i,
                   L.ptr(dbv) if db else None, acc, st)
        L.call('smi_dw_group_flush', st)
        f = 1 + acc
        for (o, i, db, x, dy, xd, dyd), (dw, dbv) in zip(items, outs):
            mw = float((dy.abs().t() @ x.abs()).max())
            _fp32_as_good_as_torch(dw.cpu(), f * (dy.t() @ x), f * (dy.double().t() @ x.double()), 1e-6,
                                   f * mw)
            if db:
                mb = float(dy.abs().sum(0).max())
                _fp32_as_good_as_torch(dbv.cpu(), f * dy.sum(0), f * dy.double().sum(0), 1e-6, f * mb)
            else:
                assert torch.isnan(dbv).all()             # never touched


@pytest.mark.parametrize('in_dim', [78, 90, 100, 127])
@pytest.mark.parametrize('out_dim', [8, 72, 90, 108, 128])
def test_dw_fit_classes(out_dim, in_dim):
    st = L.stream()
    x, dy, xd, dyd = _case(out_dim, in_dim, 1000 * out_dim + in_dim)
    for db in (1, 0):
        _check([(out_dim, in_dim, db, x, dy, xd, dyd)], st)
        assert _last() == _form(_classes(out_dim, in_dim, db))


def test_dw_fit_tail_on_two_wide_edge():
    """a 16-wide M tail over a 2-sub-tile N edge (class 1x2; in the learner the
    LSTM's [x | h] gradient): in_dim 88 has 16-byte X rows, which the matrix's
    2-wide case (in_dim 90) has not."""
    st = L.stream()
    x, dy, xd, dyd = _case(72, 88, 9)
    _check([(72, 88, 1, x, dy, xd, dyd)], st)
    assert _classes(72, 88, 1) == ['4vx4v', '1x4v', '4vx2', '1x2']
    assert _last() == _form(_classes(72, 88, 1))


def test_dw_fit_c3_group():
    """the four GEMMs of a C3 backward phase in one group: 14 entries (the 142
    unpadded X columns of the last one rule out 16-byte loads, so its tail and
    with it its N edge stay 4 wide)."""
    st = L.stream()
    shapes = [(8, 200), (200, 300), (300, 100), (400, 142)]
    items, classes = [], []
    for k, (o, i) in enumerate(shapes):
        x, dy, xd, dyd = _case(o, i, 77 + k)
        items.append((o, i, 1, x, dy, xd, dyd))
        classes += _classes(o, i, 1)
    assert len(classes) == 14
    _check(items, st)
    assert _last() == _form(classes)
    assert _last() == ('gemm_group_reduce_kernel<gemm_dwd_group_kernel<'
                       '1x4v,1x1,4vx4v,4vx3,1x3,3x4v,3x3,4vx4s,1x4s>>')


def test_dw_fit_unaligned_operand_is_padded():
    """X one float off 16-byte alignment: no 16-byte and no 2- / 3-wide loads of
    it, so its N edge runs as padded 4-wide tiles on per-column loads (the M
    edge, loaded from the aligned dY, stays fitted)."""
    st = L.stream()
    x, dy, xd, dyd = _case(90, 100, 5, x_off=1)
    assert xd.data_ptr() % 16 == 4
    _check([(90, 100, 1, x, dy, xd, dyd)], st)
    assert _classes(90, 100, 1, x_aligned=False) == ['4sx4s', '2x4s', '4sx4s', '2x4s']
    assert _last() == _form(['4sx4s', '2x4s'])


def test_dw_fit_learner_two_source_and_bptt_shared():
    """The LSTM's two-source [x_t | h_{t-1}] gradient and the launch the heads'
    gradients share with the BPTT are reachable only through the learner: one
    learn at the smallest RNN batch whose grouped launch is not the short-batch
    kernel (E * B = 21 * 32 = 672 rows > 512), C3 layer sizes, on the bars of
    test_gpu_rnn.py's learns."""
    from tests.test_gpu_rnn import _run_rnn
    _run_rnn('adapt', B=32, T=25, H=5, D=42, A=8, Hd=100, hidden=(300, 200), iters=1)
