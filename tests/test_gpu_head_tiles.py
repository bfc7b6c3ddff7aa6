"""The fused head chains' tile -> wave map (head_kernels.hip): in the
two-row-tile forms a wave runs exactly the output tiles it owns (a k loop
unrolled for that count, chosen by one branch per layer), so a wrong count, a
tile computed by no wave or by two, a chunk counted twice or an epilogue that
follows another map than the k loop all show here.  Through smi_head_forward /
smi_head_backward_input against torch fp64, with the bars of
tests/test_gpu_head_two_tiles.py (test_gpu_ddpg._fp32_as_good_as_torch: within
2x torch-CPU fp32's own error against fp64 and 1e-5 of the tensor's scale).

* Tile counts: the widths 16, 80, 96, 112, 128 (1, 5, 6, 7, 8 tiles: every
  remainder mod 4 over the four waves) for h1, h2 and the dX width in turn,
  plus 300 x 200 (19 and 13 tiles), plus 160 for h1 and the dX width (10 tiles
  on 5 slots: waves of 3 and 2 tiles, the 2-tile waves run the 3-tile body
  with one clamped slot, hc_run's only path that still has one); out in {1, 3,
  8, 16}; K0 in {4, 20, 64, 100} (one chunk that is mostly padding, a ragged
  last chunk, no padding) and 132 / 164 (the input wide enough for 112, 128
  and 160 dX columns); each in the one-row-tile form (37 rows) and the
  two-row-tile form (16411 rows: from 16384 rows on, here with a part-filled
  last workgroup).
* Padding: X with ldx > K0 and NaN in the padding columns, dX with dx0 > 0 and
  lddx > dxn, a ragged last row block: the results equal the compact run's bit
  for bit and nothing lands outside the dX columns.
* Block invariance: inputs that repeat with the row block's period give every
  workgroup the same problem, so every block's outputs must equal block 0's
  bit for bit.  The kernels' tile -> wave map is the same in every workgroup
  today; a map that depended on the workgroup index (one rotated by
  (index >> 8) & 3 or (index >> 3) & 3 was measured and not kept) must give
  the same bits, and the 1023 / 1024 workgroups run here take every value of
  both."""
import pytest
import torch

from surreal_amd import _lib as L
from tests.test_gpu_ddpg import _fp32_as_good_as_torch
from tests.test_gpu_head import _flat

pytestmark = pytest.mark.gpu

# (din = K0, dx0, dxn, h1, h2, out)
SHAPES = [
    (4, 0, 4, 16, 80, 1),
    (20, 4, 16, 80, 96, 3),
    (64, 0, 64, 96, 112, 8),
    (100, 20, 80, 112, 128, 16),
    (100, 4, 96, 128, 16, 8),
    (132, 20, 112, 96, 80, 1),
    (132, 4, 128, 80, 16, 16),
    (100, 0, 100, 300, 200, 8),
    (164, 4, 160, 160, 144, 3),
]
ONE_TILE_ROWS, TWO_TILE_ROWS = 37, 16411


def _weights(din, h1, h2, out, seed):
    torch.manual_seed(seed)
    lins = [torch.nn.Linear(din, h1), torch.nn.Linear(h1, h2), torch.nn.Linear(h2, out)]
    return [t for l in lins for t in (l.weight.detach(), l.bias.detach())]


def _run(P, x, ldx, rows, din, h1, h2, out, tanh_out, dz, dx0, dxn, lddx=None, dx_fill=float('nan')):
    """Both chains on the GPU.  x: device tensor [rows][ldx]; returns HA1, HA2,
    Y, dH2, dH1 and the dX buffer [rows][lddx]."""
    lddx = dxn if lddx is None else lddx
    ha1 = torch.full((rows, h1), float('nan'), device='cuda')
    ha2 = torch.full((rows, h2), float('nan'), device='cuda')
    y = torch.full((rows, out), float('nan'), device='cuda')
    wT = torch.empty(din * h1 + h1 * h2, device='cuda')
    st = L.stream()
    L.call('smi_head_forward', L.ptr(P), din, h1, h2, out, tanh_out, L.ptr(x), ldx, rows,
           L.ptr(ha1), L.ptr(ha2), L.ptr(y), L.ptr(wT), st)
    dh2 = torch.full((rows, h2), float('nan'), device='cuda')
    dh1 = torch.full((rows, h1), float('nan'), device='cuda')
    dx = torch.full((rows, lddx), dx_fill, device='cuda')
    L.call('smi_head_backward_input', L.ptr(P), din, h1, h2, out, L.ptr(wT), L.ptr(dz), rows,
           L.ptr(ha1), L.ptr(ha2), L.ptr(dh2), L.ptr(dh1), dx0, dxn, L.ptr(dx), lddx, None, 0, st)
    torch.cuda.synchronize()
    return ha1, ha2, y, dh2, dh1, dx


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('rows', [ONE_TILE_ROWS, TWO_TILE_ROWS])
@pytest.mark.parametrize('din,dx0,dxn,h1,h2,out', SHAPES)
def test_tile_counts_vs_torch(din, dx0, dxn, h1, h2, out, rows):
    W1, b1, W2, b2, W3, b3 = _weights(din, h1, h2, out, 11 * din + h1 + h2)
    g = torch.Generator().manual_seed(rows + din + h2)
    x = torch.randn(rows, din, generator=g)
    dz = torch.randn(rows, out, generator=g)
    tanh_out = out % 2
    P = _flat(W1, b1, W2, b2, W3, b3).cuda()
    ha1, ha2, y, dh2, dh1, dx = _run(P, x.cuda(), din, rows, din, h1, h2, out, tanh_out, dz.cuda(),
                                     dx0, dxn)

    def fwd(dt):
        a1 = torch.relu(x.to(dt) @ W1.to(dt).t() + b1.to(dt))
        a2 = torch.relu(a1 @ W2.to(dt).t() + b2.to(dt))
        z = a2 @ W3.to(dt).t() + b3.to(dt)
        return a1, a2, torch.tanh(z) if tanh_out else z
    for got, e32, e64 in zip((ha1, ha2, y), fwd(torch.float32), fwd(torch.float64)):
        _fp32_as_good_as_torch(got.cpu(), e32, e64)
    m1, m2 = (ha1 > 0).cpu(), (ha2 > 0).cpu()      # the GPU's own ReLU masks

    def bwd(dt):
        d2 = (dz.to(dt) @ W3.to(dt)) * m2
        d1 = (d2 @ W2.to(dt)) * m1
        return d2, d1, d1 @ W1.to(dt)[:, dx0:dx0 + dxn]
    for got, e32, e64 in zip((dh2, dh1, dx), bwd(torch.float32), bwd(torch.float64)):
        _fp32_as_good_as_torch(got.cpu(), e32, e64)


@pytest.mark.parametrize('rows', [ONE_TILE_ROWS, TWO_TILE_ROWS])
@pytest.mark.parametrize('din,dx0,dxn,h1,h2,out', [(20, 4, 16, 80, 96, 3), (100, 20, 80, 300, 200, 8),
                                                    (4, 0, 4, 16, 80, 1)])
def test_padding_columns_never_read(din, dx0, dxn, h1, h2, out, rows):
    P = _flat(*_weights(din, h1, h2, out, 5 * din + h1)).cuda()
    g = torch.Generator().manual_seed(rows + din)
    x = torch.randn(rows, din, generator=g).cuda()
    dz = torch.randn(rows, out, generator=g).cuda()
    ref = _run(P, x, din, rows, din, h1, h2, out, 1, dz, dx0, dxn)
    for t in ref:
        assert bool(torch.isfinite(t).all())
    # the same rows inside a wider matrix, NaN beside them; dX into the middle
    # columns' width of a wider matrix filled with a sentinel
    ldx, lddx = din + 12, dxn + 8
    xw = torch.full((rows, ldx), float('nan'), device='cuda')
    xw[:, :din] = x
    got = _run(P, xw, ldx, rows, din, h1, h2, out, 1, dz, dx0, dxn, lddx=lddx, dx_fill=-7.0)
    for a, b in zip(got[:5], ref[:5]):
        assert bool(torch.isfinite(a).all())
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(got[5][:, :dxn]), _bits(ref[5]))
    assert bool((got[5][:, dxn:] == -7.0).all())


def _periodic_run(rows, period):
    """The C3 head (100 -> 300 -> 200 -> 8, dX over 96 columns from column 4)
    over `rows` rows that repeat with `period`: outputs on the device, and the
    inputs of the first period."""
    din, h1, h2, out, dx0, dxn = 100, 300, 200, 8, 4, 96
    P = _flat(*_weights(din, h1, h2, out, 3)).cuda()
    g = torch.Generator().manual_seed(period)
    x0 = torch.randn(period, din, generator=g).cuda()
    dz0 = torch.randn(period, out, generator=g).cuda()
    reps = rows // period
    assert reps * period == rows
    outs = _run(P, x0.repeat(reps, 1), din, rows, din, h1, h2, out, 1, dz0.repeat(reps, 1), dx0, dxn)
    return P, x0, dz0, outs, (din, h1, h2, out, dx0, dxn)


@pytest.fixture(scope='module')
def periodic():
    """One run per (rows, period), shared by the tests below, freed with the module."""
    cache = {}

    def get(rows, period):
        if (rows, period) not in cache:
            cache[(rows, period)] = _periodic_run(rows, period)
        return cache[(rows, period)]
    yield get
    cache.clear()


# 1023 workgroups of 16 rows (the one-row-tile form ends below 16384 rows) and
# 1024 of 32 rows: the workgroup indices 0 .. 1022 / 1023 take every value of
# (index >> 8) & 3 and of (index >> 3) & 3
@pytest.mark.parametrize('rows,period', [(1023 * 16, 16), (1024 * 32, 32)])
def test_every_block_equals_block_zero_bitwise(periodic, rows, period):
    _, _, _, outs, _ = periodic(rows, period)
    for t in outs:
        assert bool(torch.isfinite(t).all())
        b = _bits(t).view(rows // period, period, -1)
        same = (b == b[:1]).all(dim=2).all(dim=1)
        assert bool(same.all()), f'blocks differing from block 0: {(~same).nonzero().flatten()[:8].tolist()}'


def test_two_tile_rows_equal_one_tile_rows_bitwise(periodic):
    """The first 32 rows of the two-row-tile run against the same rows run
    alone (32 rows: two workgroups of the one-row-tile form)."""
    P, x0, dz0, outs, (din, h1, h2, out, dx0, dxn) = periodic(1024 * 32, 32)
    alone = _run(P, x0, din, 32, din, h1, h2, out, 1, dz0, dx0, dxn)
    for a, b in zip(alone, outs):
        assert torch.equal(_bits(a), _bits(b[:32]))
