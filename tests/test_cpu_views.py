"""The view checker checked (tests/views.py), without a GPU.

tests/test_gpu_linear_views.py and tests/test_gpu_ddpg_kernels.py trust three
checks: the canaries around every output (assert_untouched), no NaN in a data
region (the poison around every input), and parity with the fp64 reference on
the GEMM bar (_fp32_as_good_as_torch).  Here the same checks run on CPU
tensors against small torch emulations of a dense-layer kernel: the correct
one passes under every view variant, and each fault the views were built to
expose fails the check that is meant to see it:

  spill4       a 4-wide store that runs one float past a column block
  ld_is_width  a row written at ld = width into a wider output
  mul_valid    a sum that multiplies the padding by 0 where it should select
               it away (0 * NaN = NaN)
  mask_ge      the ReLU mask applied as >= 0 (exact and negative zeros pass)
  cat_lds      a forward_cat that copies s with lds = s_cols
"""
import pytest
import torch

from tests import views as V
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

ROWS, K, N, SC = 9, 5, 7, 3         # N % 4 == 3: a 4-wide store spills exactly one float


def _flat(buf, r, ld, off, c0, n):
    return buf[off + r * ld + c0: off + r * ld + c0 + n]


def emu_forward(x, w, b, y, fault=None):
    """y = relu(x w^T + b) over (buffer, rows, cols, ld, off) operands."""
    xb, rows, k, ldx, offx = x
    wv, bv = V._region(*w), V._region(*b)[0]
    if fault == 'mul_valid':
        k4 = (k + 3) // 4 * 4                       # whole 4-wide loads of the row, then * [k < K]
        assert ldx >= k4
        raw = V._region(xb, rows, k4, ldx, offx)
        valid = (torch.arange(k4) < k).float()
        xv = raw * valid                            # NaN * 0 in the padding columns
        wv = torch.cat([wv, torch.zeros(wv.shape[0], k4 - k)], 1)
    else:
        xv = V._region(*x)
    res = torch.relu(xv @ wv.t() + bv)
    yb, _, n, ldy, offy = y
    if fault == 'ld_is_width':
        ldy = n
    for r in range(rows):
        if fault == 'spill4':
            for c0 in range(0, n, 4):
                v = torch.zeros(4)
                v[:min(4, n - c0)] = res[r, c0:c0 + 4]
                _flat(yb, r, ldy, offy, c0, 4).copy_(v)
        else:
            _flat(yb, r, ldy, offy, 0, n).copy_(res[r])


def emu_dx(dy, w, mask, dx, fault=None):
    """dx = (dy w) * [mask > 0]."""
    m = V._region(*mask)
    keep = (m >= 0) if fault == 'mask_ge' else (m > 0)
    V._region(*dx).copy_((V._region(*dy) @ V._region(*w)) * keep)


def emu_cat(s, y, n, fault=None):
    """y[:, n : n + s_cols] = s."""
    sb, rows, sc, lds, offs = s
    if fault == 'cat_lds':
        lds = sc
    yb, _, _, ldy, offy = y
    for r in range(rows):
        _flat(yb, r, ldy, offy, n, sc).copy_(_flat(sb, r, lds, offs, 0, sc))


def _operands(view, seed=3):
    g = torch.Generator().manual_seed(seed)
    t = {'x': torch.randn(ROWS, K, generator=g), 'w': torch.randn(N, K, generator=g),
         'b': torch.randn(N, generator=g), 'dy': torch.randn(ROWS, N, generator=g),
         's': torch.randn(ROWS, SC, generator=g), 'mask': V.relu_mask(ROWS, K, g)}
    ops = {}
    for name, v in t.items():
        rows, cols = (1, v.numel()) if v.dim() == 1 else v.shape
        ld, off = V.layout(view, cols)
        ops[name] = (V.make_in(v, ld, off)[1], rows, cols, ld, off)
    return t, ops


def _out(view, rows, cols):
    ld, off = V.layout(view, cols)
    return (V.make_out(rows, cols, ld, off)[1], rows, cols, ld, off)


def _run(view, fault=None):
    """one forward (+ cat) and one input gradient under `view`, checked as the
    GPU tests check them."""
    t, o = _operands(view)
    y = _out(view, ROWS, N + SC)                    # [ relu(x w^T + b) | s ]
    ygemm = (y[0], ROWS, N, y[3], y[4])
    emu_cat(o['s'], y, N, fault)                    # (first: a spill of the GEMM block lands in s)
    emu_forward(o['x'], o['w'], o['b'], ygemm, fault)
    got = V.check_out(*y)
    ref32 = torch.relu(t['x'] @ t['w'].t() + t['b'])
    ref64 = torch.relu(t['x'].double() @ t['w'].double().t() + t['b'].double())
    _fp32_as_good_as_torch(got[:, :N], ref32, ref64)
    assert torch.equal(got[:, N:], t['s'])
    dx = _out(view, ROWS, K)
    emu_dx(o['dy'], o['w'], o['mask'], dx, fault)
    got = V.check_out(*dx)
    keep = t['mask'] > 0
    _fp32_as_good_as_torch(got, (t['dy'] @ t['w']) * keep, (t['dy'].double() @ t['w'].double()) * keep)


@pytest.mark.parametrize('view', list(V.VIEWS))
def test_correct_emulation_passes(view):
    _run(view)


# the narrowest view under which each fault is visible at all, and the others
@pytest.mark.parametrize('fault,view', [('spill4', 'wide4'), ('spill4', 'wide3'), ('spill4', 'off1wide3'),
                                        ('ld_is_width', 'wide3'), ('ld_is_width', 'wide4'),
                                        ('mul_valid', 'wide3'), ('mul_valid', 'wide4'),
                                        ('mul_valid', 'off1wide3'),
                                        ('mask_ge', 'tight'), ('mask_ge', 'off1wide3'),
                                        ('cat_lds', 'wide3'), ('cat_lds', 'wide4')])
def test_fault_is_caught(fault, view):
    with pytest.raises(AssertionError):
        _run(view, fault)


def test_each_fault_trips_the_check_meant_for_it():
    """spill4 and ld_is_width break canaries; mul_valid puts a NaN into the
    data; mask_ge leaves both intact and misses parity; cat_lds leaves both
    intact and misses the exact copy."""
    t, o = _operands('wide3')
    for fault in ('spill4', 'ld_is_width'):
        y = _out('wide3', ROWS, N)
        emu_forward(o['x'], o['w'], o['b'], y, fault)
        with pytest.raises(AssertionError, match='outside the data region'):
            V.assert_untouched(*y)
    y = _out('wide3', ROWS, N)
    emu_forward(o['x'], o['w'], o['b'], y, 'mul_valid')
    V.assert_untouched(*y)
    with pytest.raises(AssertionError, match='NaN in the data region'):
        V.check_out(*y)
    dx = _out('wide3', ROWS, K)
    emu_dx(o['dy'], o['w'], o['mask'], dx, 'mask_ge')
    got = V.check_out(*dx)
    keep = t['mask'] > 0
    with pytest.raises(AssertionError):
        _fp32_as_good_as_torch(got, (t['dy'] @ t['w']) * keep, (t['dy'].double() @ t['w'].double()) * keep)
    y = _out('wide3', ROWS, N + SC)
    V._region(y[0], ROWS, N, y[3], y[4]).fill_(0.0)
    emu_cat(o['s'], y, N, 'cat_lds')
    V.assert_untouched(*y)
    assert not torch.equal(V.read_out(*y)[:, N:], t['s'])


def test_canary_sees_a_nan_written_over_a_nan():
    """the canaries are compared as bit patterns: a NaN of another payload
    written into the padding is a write."""
    ptr, buf = V.make_out(3, 5, 8, 1)
    V.assert_untouched(buf, 3, 5, 8, 1)
    buf.view(torch.int32)[1 + 8 + 6] = 0x7fc00001
    with pytest.raises(AssertionError, match='outside the data region'):
        V.assert_untouched(buf, 3, 5, 8, 1)
    ptr, buf = V.make_out(3, 5, 8, 1)
    buf[0] = 0.0                                     # the float before an off1 view
    with pytest.raises(AssertionError):
        V.assert_untouched(buf, 3, 5, 8, 1)


def test_views_and_mask():
    g = torch.Generator().manual_seed(1)
    t = torch.randn(4, 6, generator=g)
    for name, (pad, off) in V.VIEWS.items():
        ld, o = V.layout(name, 6)
        assert (ld, o) == (6 + pad, off)
        ptr, buf = V.make_in(t, ld, o)
        assert buf.numel() == o + 4 * ld + V.TAIL and ptr.value == buf.data_ptr() + 4 * o
        assert torch.equal(V.read_out(buf, 4, 6, ld, o), t)
        V.assert_untouched(buf, 4, 6, ld, o)
        assert int(torch.isnan(buf).sum()) == buf.numel() - 24
    init = torch.randn(4, 6, generator=g)
    ptr, buf = V.make_out(4, 6, 9, 1, init=init)
    assert torch.equal(V.check_out(buf, 4, 6, 9, 1), init)
    m = V.relu_mask(64, 33, g)
    zeros = int((m == 0).sum())
    assert 0.4 * m.numel() < zeros < 0.6 * m.numel()
    assert int(torch.signbit(m).sum()) >= 1 and bool((m >= 0).all()) and int((m > 0).sum()) > 0
