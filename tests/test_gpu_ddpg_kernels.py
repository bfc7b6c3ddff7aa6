"""Direct tests of ddpg_kernels.hip: the elementwise, reduction and copy kernels
that the suite otherwise reaches only through learn() at one shape (which never
enters their grid-stride loops: grid caps of 2048, 256 and 64 workgroups).

References are fp64 numpy / torch.  Every bar is derived from the fp32
expression the kernel evaluates (u = 2^-24, one rounding), not measured from
it; operands are views with poison and canaries (tests/views.py) wherever the
call takes a leading dimension or a stride.

Buffers stay under 2.5 MB: the 87382 x 7 tanh_backward / copy_cols shape
(611674 elements, more than 2048 * 256) therefore runs at ld = cols with only
the bases offset, the strided views at 70 rows; LayerNorm takes n = 1024 at 3
rows and the 1025- / 2050-row shapes at n <= 65.
"""
import ctypes

import numpy as np
import pytest
import torch

from surreal_amd import _lib as L
from tests import views as V
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
E_ARG, E_NOFIT = -1, -2


def setup_module(m):
    L.ensure_workspace(DEV)             # layernorm_backward's block partials


def _st():
    return L.stream()


def _last():
    return L.lib().smi_last_launch().decode()


def _bits(t):
    return t.contiguous().view(torch.int32)


# --------------------------------------------- tanh_backward / copy_cols
# (rows, cols, (ldg - cols, off), (ldy - cols, off), (ldz - cols, off))
ELT_SHAPES = [(70, 1, (1, 0), (2, 1), (3, 1)),
              (70, 6, (1, 1), (2, 0), (3, 1)),
              (70, 7, (3, 1), (1, 0), (2, 0)),
              (87382, 7, (0, 0), (0, 1), (0, 1))]


@pytest.mark.parametrize('rows,cols,vg,vy,vz', ELT_SHAPES, ids=[f'{c[0]}x{c[1]}' for c in ELT_SHAPES])
def test_tanh_backward(rows, cols, vg, vy, vz):
    """dz = dy (1 - y^2): roundings of y*y (<= u), of 1 - y*y (<= u) and of the
    product (<= u |dz|), so |got - ref| <= 3 u |dy|; the bar is 4 u |dy| = 2^-22 |dy|."""
    g = torch.Generator().manual_seed(rows + cols)
    dy = torch.randn(rows, cols, generator=g)
    y = torch.tanh(2 * torch.randn(rows, cols, generator=g))
    flat = y.view(-1)
    for i, v in enumerate((1.0, -1.0, 0.0, -0.0)):      # saturated and dead units
        flat[i::17][:max(1, flat.numel() // 40)] = v
    gp, gbuf = V.make_in(dy, cols + vg[0], vg[1], DEV)
    yp, ybuf = V.make_in(y, cols + vy[0], vy[1], DEV)
    zp, zbuf = V.make_out(rows, cols, cols + vz[0], vz[1], device=DEV)
    L.call('smi_tanh_backward', gp, cols + vg[0], yp, cols + vy[0], rows, cols, zp, cols + vz[0], _st())
    assert _last() == 'tanh_backward_kernel'
    got = V.check_out(zbuf, rows, cols, cols + vz[0], vz[1]).double()
    ref = dy.double() * (1 - y.double() ** 2)
    err = (got - ref).abs()
    assert bool((err <= 2.0 ** -22 * dy.double().abs()).all()), float((err / dy.double().abs()).max())
    assert bool((got[y.abs() == 1] == 0).all())


@pytest.mark.parametrize('rows,cols,vs,_,vd', ELT_SHAPES, ids=[f'{c[0]}x{c[1]}' for c in ELT_SHAPES])
def test_copy_cols(rows, cols, vs, _, vd):
    """bit-identical to the source, -0.0 and NaN payloads included."""
    g = torch.Generator().manual_seed(rows * 3 + cols)
    src = torch.randn(rows, cols, generator=g)
    sb = _bits(src).view(-1)
    for i, v in enumerate((-0x80000000, 0x7fc01234, -0x3fffff, 0x7f800001, 0x00000001)):
        sb[i::13][:max(1, sb.numel() // 50)] = v        # -0.0, quiet / negative / signalling NaN, denormal
    sp, sbuf = V.make_in(src, cols + vs[0], vs[1], DEV)
    dp, dbuf = V.make_out(rows, cols, cols + vd[0], vd[1], device=DEV)
    L.call('smi_copy_cols', sp, cols + vs[0], rows, cols, dp, cols + vd[0], _st())
    assert _last() == 'copy_cols_kernel'
    V.assert_untouched(dbuf, rows, cols, cols + vd[0], vd[1])
    on_dev = _bits(V.read_out(sbuf, rows, cols, cols + vs[0], vs[1]))
    assert torch.equal(on_dev, _bits(src))              # the upload kept the payloads
    assert torch.equal(_bits(V.read_out(dbuf, rows, cols, cols + vd[0], vd[1])), on_dev)


# ------------------------------------------------------------ soft_update
@pytest.mark.parametrize('tau', [1e-3, 0.0, 1.0])
@pytest.mark.parametrize('n', [1, 255, 257, 524288 + 257])
def test_soft_update(n, tau):
    """t <- tau s + (1 - tau) t in fp32: 1 - tau (<= u), two products and the
    sum, <= 3 u (|tau s| + |(1 - tau) t|); the bar is 2^-22 of it.  tau = 1
    gives src and tau = 0 the old target exactly.  524288 + 257 elements are
    more than the grid's 2048 * 256."""
    g = torch.Generator().manual_seed(n)
    s, t = torch.randn(n, generator=g), torch.randn(n, generator=g)
    sp, sbuf = V.make_in(s, n, 1, DEV)
    tp, tbuf = V.make_out(1, n, n, 1, init=t, device=DEV)
    L.call('smi_soft_update', tp, sp, n, tau, _st())
    assert _last() == 'soft_update_kernel'
    got = V.check_out(tbuf, 1, n, n, 1)[0]
    if tau == 1.0:
        assert torch.equal(got, s)
    elif tau == 0.0:
        assert torch.equal(got, t)
    else:
        tf = float(np.float32(tau))
        a, b = tf * s.double(), (1 - tf) * t.double()
        assert bool(((got.double() - (a + b)).abs() <= 2.0 ** -22 * (a.abs() + b.abs())).all())


# ------------------------------------------------------------ loss pieces
def _col(q, stride, off):
    """q [n] as column 0 of a poisoned [n][stride] buffer."""
    return V.make_in(q.view(-1, 1), stride, off, DEV)


@pytest.mark.parametrize('with_loss', [1, 0])
@pytest.mark.parametrize('qs', [1, 3])
@pytest.mark.parametrize('n', [1, 1000])
def test_mse_grad_strided(n, qs, with_loss):
    """smi_mse_grad and smi_mse_grad_weighted on q as a column of a wider
    buffer, with and without the loss output, on the bars of
    test_gpu_per.py::test_mse_grad_weighted (td exact; dq and loss
    _fp32_as_good_as_torch)."""
    g = torch.Generator().manual_seed(n * 5 + qs)
    q, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    w = torch.rand(n, generator=g) + 0.01
    qp, qbuf = _col(q, qs, 1)
    yd, wd = y.to(DEV), w.to(DEV)
    q64, y64, w64 = q.double(), y.double(), w.double()

    def outs():
        return (V.make_out(1, n, n, 1, device=DEV), V.make_out(1, 1, 1, 1, device=DEV),
                V.make_out(1, n, n, 1, device=DEV))
    (dqp, dqb), (lp, lb), (tdp, tdb) = outs()
    L.call('smi_mse_grad', qp, qs, L.ptr(yd), n, dqp, lp if with_loss else None, _st())
    assert _last() == 'mse_grad_kernel'
    base = V.check_out(dqb, 1, n, n, 1)[0]
    _fp32_as_good_as_torch(base, 2 * (q - y) / n, 2 * (q64 - y64) / n)
    if with_loss:
        _fp32_as_good_as_torch(V.check_out(lb, 1, 1, 1, 1)[0], ((q - y) ** 2).mean().view(1),
                               ((q64 - y64) ** 2).mean().view(1))
    else:
        V.assert_untouched(lb, 1, 0, 1, 1)
    (dqp, dqb), (lp, lb), (tdp, tdb) = outs()
    L.call('smi_mse_grad_weighted', qp, qs, L.ptr(yd), L.ptr(wd), n, dqp, lp if with_loss else None, tdp,
           _st())
    assert _last() == 'mse_grad_weighted_kernel'
    assert torch.equal(V.check_out(tdb, 1, n, n, 1)[0], q - y)
    _fp32_as_good_as_torch(V.check_out(dqb, 1, n, n, 1)[0], (2 * (q - y) / n) * w,
                           (2 * (q64 - y64) / n) * w64)
    if with_loss:
        _fp32_as_good_as_torch(V.check_out(lb, 1, 1, 1, 1)[0], (w * (q - y) ** 2).mean().view(1),
                               (w64 * (q64 - y64) ** 2).mean().view(1))
    else:
        V.assert_untouched(lb, 1, 0, 1, 1)
    # w = NULL with td: the weighted kernel, mse_grad's bits
    (dqp, dqb), (lp, lb), (tdp, tdb) = outs()
    L.call('smi_mse_grad_weighted', qp, qs, L.ptr(yd), None, n, dqp, None, tdp, _st())
    assert torch.equal(V.check_out(dqb, 1, n, n, 1)[0], base)
    assert torch.equal(V.check_out(tdb, 1, n, n, 1)[0], q - y)


@pytest.mark.parametrize('with_loss', [1, 0])
@pytest.mark.parametrize('qs', [1, 3])
@pytest.mark.parametrize('n', [1, 1000])
def test_neg_mean_grad_strided(n, qs, with_loss):
    """dq = float32(-1 / float32(n)) exactly; loss = -mean(q) summed in fp64
    and rounded once: within 2 u mean|q|."""
    g = torch.Generator().manual_seed(n * 7 + qs)
    q = torch.randn(n, generator=g)
    qp, qbuf = _col(q, qs, 1)
    dqp, dqb = V.make_out(1, n, n, 1, device=DEV)
    lp, lb = V.make_out(1, 1, 1, 1, device=DEV)
    L.call('smi_neg_mean_grad', qp, qs, n, dqp, lp if with_loss else None, _st())
    assert _last() == 'neg_mean_grad_kernel'
    want = np.float32(-1.0) / np.float32(n)
    assert torch.equal(V.check_out(dqb, 1, n, n, 1)[0], torch.full((n,), float(want)))
    if with_loss:
        got = float(V.check_out(lb, 1, 1, 1, 1)[0])
        assert abs(got + float(q.double().mean())) <= 2.0 ** -23 * float(q.double().abs().mean())
    else:
        V.assert_untouched(lb, 1, 0, 1, 1)


@pytest.mark.parametrize('n', [1, 300, 1000])
@pytest.mark.parametrize('A', [1, 6, 17])
def test_ddpg_stats(A, n):
    """stats = mean ||a||, mean r, mean y, mean q.  Per row the norm is A
    fp32 products and adds and a square root, relative error <= (A + 1) u / 2 +
    u, the sums run in fp64 and the mean is rounded once: (A + 2) u mean||a||
    covers stat 0, 2 u mean|x| the others."""
    g = torch.Generator().manual_seed(A * 1000 + n)
    a = torch.tanh(torch.randn(n, A, generator=g))
    r, y, q = (torch.randn(n, generator=g) for _ in range(3))
    ap, abuf = V.make_in(a, A + 3, 1, DEV)
    yd = y.to(DEV)
    ref = [float(a.double().norm(dim=1).mean()), float(r.double().mean()), float(y.double().mean()),
           float(q.double().mean())]
    mag = [ref[0]] + [float(t.double().abs().mean()) for t in (r, y, q)]
    bar = [(A + 2) * U * mag[0]] + [2 * U * m for m in mag[1:]]
    for rs, qs in ((1, 1), (2, 1), (1, 2), (2, 2)):
        rp, rbuf = _col(r, rs, 1)
        qp, qbuf = _col(q, qs, 0)
        sp, sbuf = V.make_out(1, 4, 4, 1, device=DEV)
        L.call('smi_ddpg_stats', ap, A + 3, A, rp, rs, L.ptr(yd), qp, qs, n, sp, _st())
        assert _last() == 'ddpg_stats_kernel'
        got = V.check_out(sbuf, 1, 4, 4, 1)[0].double()
        for i in range(4):
            assert abs(float(got[i]) - ref[i]) <= bar[i], (i, rs, qs, float(got[i]), ref[i], bar[i])


# -------------------------------------------------------------- LayerNorm
LN_SHAPES = [(r, n) for r in (3, 1025, 2050) for n in (1, 63, 64, 65)] + [(3, 1024)]


@pytest.mark.parametrize('relu', [1, 0])
@pytest.mark.parametrize('rows,n', LN_SHAPES, ids=[f'{r}x{n}' for r, n in LN_SHAPES])
def test_layernorm_views(rows, n, relu):
    """smi_layernorm_forward / _backward with every leading dimension different
    from n, relu_input 0 and 1, a constant row (variance 0) and an all-zero row,
    more than 1024 rows (the backward's 256 blocks x 4 waves iterate, the last
    block ragged), on the bar of test_layernorm_kernels_vs_torch: twice the
    error of torch's fp32 CPU layer_norm against fp64 autograd + 1e-6 of the
    scale, the scale of dgamma / dbeta the largest sum of |terms|."""
    g = torch.Generator().manual_seed(rows * 7 + n + relu)
    z = torch.randn(rows, n, generator=g, dtype=torch.float64)
    x = torch.relu(z) if relu else z.clone()
    x[0] = 0.5                                          # exact mean in fp32: variance exactly 0
    x[rows - 1] = 0.0                                   # a dead row
    x = x.float().double()
    gamma = 1 + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    dy = torch.randn(rows, n, generator=g, dtype=torch.float64)
    gamma, beta, dy = (t.float().double() for t in (gamma, beta, dy))

    def ref(dtype):
        xx = x.to(dtype).clone().requires_grad_(True)
        gg, bb = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
        y = torch.nn.functional.layer_norm(xx, (n,), gg, bb, 1e-5)
        y.backward(dy.to(dtype))
        dx = xx.grad * (x > 0).to(dtype) if relu else xx.grad
        return [t.detach().double() for t in (y, dx, gg.grad, bb.grad)]
    r64, r32 = ref(torch.float64), ref(torch.float32)
    xhat = (x - x.mean(1, keepdim=True)) / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
    scales = [float(r64[0].abs().max()), float(r64[1].abs().max()),
              float((dy * xhat).abs().sum(0).max()), float(dy.abs().sum(0).max())]
    ldx, ldy, ldg, lddx = n + 3, n + 1, n + 2, n + 4
    xp, xbuf = V.make_in(x.float(), ldx, 1, DEV)
    gp, gbuf = V.make_in(dy.float(), ldg, 0, DEV)
    gd, bd = gamma.float().to(DEV), beta.float().to(DEV)
    yp, ybuf = V.make_out(rows, n, ldy, 1, device=DEV)
    dxp, dxbuf = V.make_out(rows, n, lddx, 1, device=DEV)
    outs = {k: V.make_out(1, w, w, 1, device=DEV) for k, w in (('mu', rows), ('rs', rows), ('dg', n), ('db', n))}
    st = _st()
    L.call('smi_layernorm_forward', xp, ldx, rows, n, L.ptr(gd), L.ptr(bd), 1e-5, yp, ldy, outs['mu'][0],
           outs['rs'][0], st)
    assert _last() == 'layernorm_fwd_kernel'
    L.call('smi_layernorm_backward', gp, ldg, xp, ldx, outs['mu'][0], outs['rs'][0], L.ptr(gd), rows, n, relu,
           dxp, lddx, outs['dg'][0], outs['db'][0], st)
    assert _last() == 'layernorm_param_grad_kernel'
    got = [V.check_out(ybuf, rows, n, ldy, 1), V.check_out(dxbuf, rows, n, lddx, 1),
           V.check_out(outs['dg'][1], 1, n, n, 1)[0], V.check_out(outs['db'][1], 1, n, n, 1)[0]]
    for name, gt, a, b, scale in zip(('y', 'dx', 'dgamma', 'dbeta'), got, r32, r64, scales):
        e_gpu, e_cpu = float((gt.double() - b).abs().max()), float((a - b).abs().max())
        assert e_gpu <= 2 * e_cpu + 1e-6 * scale, (name, e_gpu, e_cpu, scale)
    mu = V.check_out(outs['mu'][1], 1, rows, rows, 1)[0]
    rs = V.check_out(outs['rs'][1], 1, rows, rows, 1)[0]
    assert torch.allclose(mu.double(), x.mean(1), rtol=1e-5, atol=1e-6)
    assert float(mu[0]) == 0.5 and float(mu[rows - 1]) == 0.0
    assert float(rs[0]) == float(rs[rows - 1]) and abs(float(rs[0]) - 1e-5 ** -0.5) <= 4 * U * 1e-5 ** -0.5


def test_layernorm_argument_errors():
    """n = 1025 and every leading dimension below n: SMI_E_ARG, nothing written."""
    rows = 3
    lib, st = L.lib(), _st()
    for n, lds in ((1025, (1025,) * 5), (8, (7, 8, 8, 8, 8)), (8, (8, 7, 8, 8, 8)), (8, (8, 8, 7, 8, 8)),
                   (8, (8, 8, 8, 7, 8)), (8, (8, 8, 8, 8, 7))):
        ldx, ldy, ldg, ldxb, lddx = lds
        big = max(n, 8)
        x = torch.randn(rows, big, device=DEV)
        gam = torch.ones(big, device=DEV)
        mu, rs = torch.zeros(rows, device=DEV), torch.ones(rows, device=DEV)
        yp, ybuf = V.make_out(rows, big, big, 0, device=DEV)
        dxp, dxbuf = V.make_out(rows, big, big, 0, device=DEV)
        dgp, dgbuf = V.make_out(1, big, big, 0, device=DEV)
        dbp, dbbuf = V.make_out(1, big, big, 0, device=DEV)
        mp, mbuf = V.make_out(1, rows, rows, 0, device=DEV)
        rp, rbuf = V.make_out(1, rows, rows, 0, device=DEV)
        fwd_bad = n > 1024 or ldx < n or ldy < n
        rc = lib.smi_layernorm_forward(L.ptr(x), ldx, rows, n, L.ptr(gam), L.ptr(gam), 1e-5, yp, ldy, mp, rp, st)
        assert rc == (E_ARG if fwd_bad else 0), (n, lds)
        if fwd_bad:
            for b in (ybuf, mbuf, rbuf):
                assert bool(torch.isnan(b).all())
        bwd_bad = n > 1024 or ldg < n or ldxb < n or lddx < n
        rc = lib.smi_layernorm_backward(L.ptr(x), ldg, L.ptr(x), ldxb, L.ptr(mu), L.ptr(rs), L.ptr(gam), rows, n,
                                        1, dxp, lddx, dgp, dbp, st)
        assert rc == (E_ARG if bwd_bad else 0), (n, lds)
        if bwd_bad:
            for b in (dxbuf, dgbuf, dbbuf):
                assert bool(torch.isnan(b).all())


# ------------------------------------------------- mlp3_forward_stacked
def _stacked(g, n, dims, gap):
    """n parameter sets [W1 b1 W2 b2 W3 b3] pstride apart, NaN between them."""
    din, h1, h2, out = dims
    shapes = [(h1, din), (h1,), (h2, h1), (h2,), (out, h2), (out,)]
    offs, o = [], 0
    for s in shapes:
        offs.append(o)
        o += int(np.prod(s))
    pstride = o + gap
    P = torch.full((n * pstride + 1,), float('nan'))
    sets = []
    for i in range(n):
        ps = []
        for j, (s, off) in enumerate(zip(shapes, offs)):
            fan = s[1] if len(s) == 2 else shapes[j - 1][1]
            t = (2 * torch.rand(*s, generator=g) - 1) / fan ** 0.5
            P[1 + i * pstride + off:1 + i * pstride + off + t.numel()] = t.reshape(-1)
            ps.append(t)
        sets.append(ps)
    return P, pstride, offs, sets


@pytest.mark.parametrize('out_act', [0, 1, 2])
@pytest.mark.parametrize('dims', [(1, 1, 1, 1), (17, 300, 200, 6), (65, 64, 1024, 1)],
                         ids=lambda d: 'x'.join(map(str, d)))
@pytest.mark.parametrize('n', [1, 5])
def test_mlp3_forward_stacked(n, dims, out_act):
    """row i of x through parameter set i, against per-agent MLPs in fp64 on
    the GEMM bar; ldx / ldy wider than the widths, the sets pstride apart (and
    4-byte aligned only) with NaN between them."""
    din, h1, h2, out = dims
    g = torch.Generator().manual_seed(n * 100 + sum(dims) + out_act)
    P, pstride, offs, sets = _stacked(g, n, dims, gap=5)
    x = torch.randn(n, din, generator=g)
    Pd = P.to(DEV)
    xp, xbuf = V.make_in(x, din + 3, 1, DEV)
    yp, ybuf = V.make_out(n, out, out + 2, 1, device=DEV)
    o6 = (ctypes.c_int64 * 6)(*offs)
    L.call('smi_mlp3_forward_stacked', ctypes.c_void_p(Pd.data_ptr() + 4), pstride, o6, din, h1, h2, out,
           out_act, xp, din + 3, n, yp, out + 2, _st())
    assert _last() == 'mlp3_stacked_kernel'
    got = V.check_out(ybuf, n, out, out + 2, 1)
    act = {0: lambda t: t, 1: torch.relu, 2: torch.tanh}[out_act]

    def ref(dt):
        rows = []
        for i, (W1, b1, W2, b2, W3, b3) in enumerate(sets):
            h = torch.relu(W1.to(dt) @ x[i].to(dt) + b1.to(dt))
            h = torch.relu(W2.to(dt) @ h + b2.to(dt))
            rows.append(act(W3.to(dt) @ h + b3.to(dt)))
        return torch.stack(rows)
    _fp32_as_good_as_torch(got, ref(torch.float32), ref(torch.float64))


@pytest.mark.parametrize('which', range(4))
def test_mlp3_forward_stacked_width_limit(which):
    """a width of 1025 anywhere: SMI_E_NOFIT, y untouched."""
    dims = [4, 4, 4, 4]
    dims[which] = 1025
    P = torch.zeros(4 * 1025 + 1025 + 64, device=DEV)
    x = torch.zeros(2, 1025, device=DEV)
    yp, ybuf = V.make_out(2, 1025, 1025, 0, device=DEV)
    o6 = (ctypes.c_int64 * 6)(0, 0, 0, 0, 0, 0)
    rc = L.lib().smi_mlp3_forward_stacked(L.ptr(P), 0, o6, dims[0], dims[1], dims[2], dims[3], 0, L.ptr(x),
                                          1025, 2, yp, 1025, _st())
    assert rc == E_NOFIT
    assert bool(torch.isnan(ybuf).all())


# ------------------------------------------------------------------ copies
SIZES = [20, 0, 4, 12, 16, 36, 1024 + 8, 16 * 256 + 4]
BIG = 262144 + 20                  # 16385 16-byte units: more than 64 workgroups x 256 threads


def _gather_case(count, g):
    sizes = [SIZES[i % len(SIZES)] for i in range(count)]
    if count >= 16:
        sizes[count - 1] = BIG                             # (the last launch's widest segment)
        sizes[3] = BIG if count == 33 else sizes[3]        # and one inside a full 16-segment launch
    srcs = [torch.randint(0, 256, (max(s, 1),), generator=g, dtype=torch.uint8).to(DEV) for s in sizes]
    offs, o = [], 16
    for s in sizes:
        offs.append(o)
        o = (o + s + 15) // 16 * 16 + 16                   # a canary gap of >= 16 bytes
    return sizes, srcs, offs, o


@pytest.mark.parametrize('count', [1, 16, 17, 33])
def test_copy_gather(count):
    g = torch.Generator().manual_seed(count)
    sizes, srcs, offs, total = _gather_case(count, g)
    dst = torch.full((total,), 0xA5, dtype=torch.uint8, device=DEV)
    ps = (ctypes.c_void_p * count)(*[s.data_ptr() for s in srcs])
    po = (ctypes.c_int64 * count)(*offs)
    pn = (ctypes.c_int64 * count)(*sizes)
    L.call('smi_copy_gather', ctypes.c_void_p(dst.data_ptr()), ps, po, pn, count, _st())
    assert _last() == 'copy_gather_kernel'
    want = torch.full((total,), 0xA5, dtype=torch.uint8)
    for s, t, o in zip(sizes, srcs, offs):
        want[o:o + s] = t.cpu()[:s]
    assert torch.equal(dst.cpu(), want)


@pytest.mark.parametrize('bad', ['nbytes', 'offset', 'source'])
def test_copy_gather_argument_errors(bad):
    src = torch.arange(64, dtype=torch.uint8, device=DEV)
    dst = torch.full((128,), 0xA5, dtype=torch.uint8, device=DEV)
    sizes = [16, 6 if bad == 'nbytes' else 8]
    offs = [0, 36 if bad == 'offset' else 32]
    ptrs = [src.data_ptr(), src.data_ptr() + (20 if bad == 'source' else 32)]
    rc = L.lib().smi_copy_gather(ctypes.c_void_p(dst.data_ptr()), (ctypes.c_void_p * 2)(*ptrs),
                                 (ctypes.c_int64 * 2)(*offs), (ctypes.c_int64 * 2)(*sizes), 2, _st())
    assert rc == E_ARG
    assert bool((dst.cpu() == 0xA5).all())


@pytest.mark.parametrize('nbytes', [16, (1 << 20) + 16])
def test_copy_to_host(nbytes):
    """into a pinned tensor; 1 MiB + 16 bytes are 65537 16-byte units, more
    than 256 workgroups x 256 threads."""
    g = torch.Generator().manual_seed(nbytes)
    src = torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8)
    sd = src.to(DEV)
    host = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8).pin_memory()
    L.call('smi_copy_to_host', ctypes.c_void_p(host.data_ptr()), ctypes.c_void_p(sd.data_ptr()), nbytes, _st())
    assert _last() == 'copy_bytes16_kernel'
    torch.cuda.synchronize()
    assert torch.equal(host[:nbytes], src)
    assert bool((host[nbytes:] == 0xA5).all())


def test_copy_to_host_pageable_destination():
    """a pageable destination is refused, and the refusal does not surface as
    the next launch's error."""
    sd = torch.arange(64, dtype=torch.uint8, device=DEV)
    host = torch.full((64,), 0xA5, dtype=torch.uint8)
    assert host.data_ptr() % 16 == 0 and not host.is_pinned()
    rc = L.lib().smi_copy_to_host(ctypes.c_void_p(host.data_ptr()), ctypes.c_void_p(sd.data_ptr()), 64, _st())
    assert rc == E_ARG and b'pinned' in L.lib().smi_last_error()
    assert bool((host == 0xA5).all())
    for nb, ptr_off in ((24, 0), (32, 4)):                 # not a multiple of 16; a misaligned source
        pinned = torch.full((64,), 0xA5, dtype=torch.uint8).pin_memory()
        rc = L.lib().smi_copy_to_host(ctypes.c_void_p(pinned.data_ptr()),
                                      ctypes.c_void_p(sd.data_ptr() + ptr_off), nb, _st())
        assert rc == E_ARG
    t = torch.ones(4, device=DEV)
    s = torch.zeros(4, device=DEV)
    L.call('smi_soft_update', L.ptr(t), L.ptr(s), 4, 0.5, _st())
    assert torch.equal(t.cpu(), torch.full((4,), 0.5))
