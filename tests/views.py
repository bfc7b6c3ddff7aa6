"""Operand views with poison and canaries (test infrastructure only).

The learner hands the dense-layer and elementwise kernels column blocks of
wider buffers: a leading dimension larger than the width, a base pointer that
is 4-byte aligned only, neighbouring columns that must survive the call.  The
helpers here build such operands inside one flat buffer

    [ off floats | rows x ld floats, the first `cols` of each row are data | 64 floats ]

with every float outside the data region a NaN:

  * an input's padding that leaks into a result shows up as a NaN in it (a sum
    that multiplies the padding by 0 where it should select it away gives
    0 * NaN = NaN);
  * an output's padding is a canary: assert_untouched compares its int32 bit
    pattern with the fill value's, so a store past a column block, or a row
    written at the wrong stride, is seen even where it writes a NaN;
  * the 64-float tail keeps a small over-read or over-write inside the
    allocation.

tests/test_cpu_views.py runs these checks against torch emulations of a correct
kernel and of the faults they are meant to catch.
"""
import ctypes

import torch

NAN = float('nan')
TAIL = 64

# name -> (ld - width, off)
VIEWS = {'tight': (0, 0), 'wide4': (4, 0), 'wide3': (3, 0), 'off1': (0, 1), 'off1wide3': (3, 1)}


def layout(name, width):
    """(ld, off) of the named view variant for an operand `width` floats wide."""
    pad, off = VIEWS[name]
    return width + pad, off


def _ptr(buf, off):
    return ctypes.c_void_p(buf.data_ptr() + 4 * off)


def _region(buf, rows, cols, ld, off):
    return buf[off:off + rows * ld].view(rows, ld)[:, :cols]


def make_in(t, ld, off, device=None):
    """t ([rows][cols], or 1-D as one row) inside a NaN-filled buffer of
    off + rows * ld + 64 floats on `device` (default: t's).  Returns (pointer to
    the view's first element, buffer)."""
    t2 = t.reshape(1, -1) if t.dim() == 1 else t
    rows, cols = t2.shape
    assert ld >= cols and off >= 0
    buf = torch.full((off + rows * ld + TAIL,), NAN, dtype=torch.float32,
                     device=device if device is not None else t.device)
    _region(buf, rows, cols, ld, off).copy_(t2)
    return _ptr(buf, off), buf


def make_out(rows, cols, ld, off, init=None, device='cpu'):
    """the layout of make_in with every float NaN; `init` ([rows][cols]:
    accumulating calls) fills the data region.  Returns (pointer, buffer)."""
    assert ld >= cols and off >= 0
    buf = torch.full((off + rows * ld + TAIL,), NAN, dtype=torch.float32, device=device)
    if init is not None:
        _region(buf, rows, cols, ld, off).copy_(init.reshape(rows, cols))
    return _ptr(buf, off), buf


def read_out(buf, rows, cols, ld, off):
    """the data region, as a contiguous CPU tensor."""
    return _region(buf, rows, cols, ld, off).detach().cpu().clone()


def assert_untouched(buf, rows, cols, ld, off, fill=NAN):
    """every float outside the data region still holds `fill`, bit for bit."""
    bits = buf.detach().cpu().view(torch.int32)
    want = int(torch.tensor([fill], dtype=torch.float32).view(torch.int32))
    outside = torch.ones(bits.numel(), dtype=torch.bool)
    _region(outside, rows, cols, ld, off).fill_(False)
    bad = torch.nonzero(outside & (bits != want)).flatten()
    assert bad.numel() == 0, (f'{bad.numel()} floats outside the data region were written, first at '
                              f'buffer index {int(bad[0])} (off {off}, ld {ld}, {rows} x {cols})')


def check_out(buf, rows, cols, ld, off, fill=NAN):
    """canaries intact and no NaN in the data region; returns the data."""
    assert_untouched(buf, rows, cols, ld, off, fill)
    data = read_out(buf, rows, cols, ld, off)
    nans = int(torch.isnan(data).sum())
    assert nans == 0, f'{nans} NaN in the data region ({rows} x {cols})'
    return data


def relu_mask(rows, cols, g):
    """a ReLU output as the mask of an input gradient: about half exact +0.0,
    a few -0.0 (neither passes `> 0`; both pass `>= 0`)."""
    m = torch.relu(torch.randn(rows, cols, generator=g))
    flat = m.view(-1)
    n = flat.numel()
    idx = torch.randperm(n, generator=g)[:max(1, min(8, n // 4))]
    flat[idx] = -0.0
    return m
