"""The general convolution layer (surreal_amd/csrc/conv_kernels.hip) through the
C ABI against torch on the CPU: tests/qconv_ref.py holds the cases, the bars
and the checker (tests/test_cpu_qconv_ref.py shows what that checker catches).

Operands are views inside NaN-filled buffers (tests/views.py): inputs carry NaN
before and after the data, outputs are canaried, the weight-gradient scratch is
NaN.  At n = 5 every float pointer is 4-byte aligned only and the uint8 image
starts at an odd address (the element-load paths); at n = 1 everything is
16-byte aligned (the 16-byte weight loads where cin k k % 4 == 0)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from surreal_amd import _lib as L
from tests import qconv_ref as Q
from tests import views as V

pytestmark = pytest.mark.gpu
DEV = 'cuda'
E_ARG = -1
NAN = float('nan')


def _in(t, off):
    if t.dtype == torch.uint8:
        buf = torch.full((t.numel() + 2 * 16 + off,), 0xAB, dtype=torch.uint8, device=DEV)
        buf[16 + off:16 + off + t.numel()].copy_(t.reshape(-1))
        return ctypes.c_void_p(buf.data_ptr() + 16 + off), buf
    return V.make_in(t.reshape(-1).float(), t.numel(), off, device=DEV)


def _scratch(n, geom):
    nbytes = int(L.lib().smi_conv2d_scratch_bytes(n, *geom))
    assert nbytes >= 0
    return torch.full((nbytes // 4 + 8,), NAN, device=DEV), nbytes


class GpuLayer(object):
    """the impl interface of qconv_ref.check_layer over the C ABI"""

    def __init__(self, off):
        self.off = off

    def forward(self, c, div255, act=1):
        cin, H, W, cout, k, s, p = c.geom
        px, bx = _in(c.x, self.off)
        pw, bw = _in(c.w, self.off)
        pb, bb = _in(c.b, self.off)
        ny = c.n * cout * c.ho * c.wo
        py, by = V.make_out(1, ny, ny, self.off, device=DEV)
        L.call('smi_conv2d_forward', px, int(c.u8), int(div255), c.n, cin, H, W, pw, pb, cout, k, s, p,
               act, py, L.stream())
        return V.check_out(by, 1, ny, ny, self.off).reshape(c.n, cout, c.ho, c.wo)

    def backward_input(self, c, dz):
        cin, H, W, cout, k, s, p = c.geom
        pdy, b1 = _in(dz, self.off)
        pw, b2 = _in(c.w, self.off)
        pm, b3 = _in(c.mask, self.off)
        nx = c.n * cin * H * W
        pdx, bdx = V.make_out(1, nx, nx, self.off, device=DEV)
        L.call('smi_conv2d_backward_input', pdy, c.n, cin, H, W, pw, cout, k, s, p, pm, pdx, L.stream())
        return V.check_out(bdx, 1, nx, nx, self.off).reshape(c.n, cin, H, W)

    def backward_weight(self, c, dz, div255, raw=False):
        cin, H, W, cout, k, s, p = c.geom
        pdy, b1 = _in(dz, self.off)
        px, b2 = _in(c.x, self.off)
        nw = cout * cin * k * k
        # one gradient image [dw | 3 floats that must survive | db]
        pg, bg = V.make_out(1, nw + 3 + cout, nw + 3 + cout, self.off, device=DEV)
        scratch, nbytes = _scratch(c.n, c.geom)
        pdb = ctypes.c_void_p(pg.value + 4 * (nw + 3))
        L.call('smi_conv2d_backward_weight', pdy, px, int(c.u8), int(div255), c.n, cin, H, W, cout,
               k, s, p, pg, pdb, L.ptr(scratch), nbytes, L.stream())
        torch.cuda.synchronize()
        V.assert_untouched(bg, 1, nw + 3 + cout, nw + 3 + cout, self.off)
        img = V.read_out(bg, 1, nw + 3 + cout, nw + 3 + cout, self.off).reshape(-1)
        assert bool(torch.isnan(img[nw:nw + 3]).all()), 'floats between dw and db were written'
        if raw:
            return img
        return img[:nw].reshape(cout, cin, k, k), img[nw + 3:]


def _cases():
    for name in Q.GEOMS:
        for n in Q.NS:
            for div in ((False, True) if Q.GEOMS[name][5] else (False,)):
                yield pytest.param(name, n, div, id=f'{name}-n{n}' + ('-div255' if div else ''))


@pytest.mark.parametrize('name,n,div255', list(_cases()))
def test_layer_against_torch(name, n, div255):
    Q.check_layer(GpuLayer(off=0 if n == 1 else 1), Q.LayerCase(name, n), div255)


def test_more_images_than_resident_workgroups():
    """k1_7x4x4 at 10000 images is 2500 forward and input-gradient tiles; 256 CUs
    hold at most 9 workgroups of 17 KiB LDS each, so workgroups loop"""
    Q.check_layer(GpuLayer(off=1), Q.LayerCase('k1_7x4x4', 10000))


def test_weight_gradient_twice_is_bit_identical():
    c = Q.LayerCase('tiles_64x12x12', 5)
    dz = c.dy * (c.dy > 0.3)
    a = GpuLayer(1).backward_weight(c, dz, False, raw=True)
    b = GpuLayer(1).backward_weight(c, dz, False, raw=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_atari_chain_forward_and_backward():
    """4x84x84 -> 32@8/4 -> 64@4/2 -> 64@3/1 (SAME padding) at n = 4, composed:
    each layer reads the previous kernel's output; the backward runs on the
    masks of that forward"""
    n = 4
    layers, shape = Q.conv_shapes((4, 84, 84), Q.NATURE)
    assert shape == (64, 12, 12)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 256, (n, 4, 84, 84), generator=g, dtype=torch.uint8)
    ws = [torch.randn(co, ci, k, k, generator=g) / float(np.sqrt(ci * k * k))
          for ci, _, _, co, k, _, _ in layers]
    bs = [0.1 * torch.randn(l[3], generator=g) for l in layers]
    dyl = torch.randn(n, 64, 12, 12, generator=g)
    st = L.stream()
    acts = [x.to(DEV)]
    wd, bd = [w.to(DEV) for w in ws], [b.to(DEV) for b in bs]
    for i, (ci, H, W, co, k, s, p) in enumerate(layers):
        ho, wo = Q.out_hw(H, W, k, s, p)
        y = torch.full((n, co, ho, wo), NAN, device=DEV)
        L.call('smi_conv2d_forward', L.ptr(acts[-1]), int(i == 0), int(i == 0), n, ci, H, W,
               L.ptr(wd[i]), L.ptr(bd[i]), co, k, s, p, 1, L.ptr(y), st)
        acts.append(y)
    # torch forward, fp32 and fp64
    refs = {}
    for dt in (torch.float32, torch.float64):
        a = [x.to(dt) / 255.0]
        for i, (ci, H, W, co, k, s, p) in enumerate(layers):
            a.append(torch.relu(F.conv2d(a[-1], ws[i].to(dt), bs[i].to(dt), stride=s, padding=p)))
        refs[dt] = a
    for i in range(1, 4):
        Q.fp32_as_good_as_torch(acts[i].cpu(), refs[torch.float32][i], refs[torch.float64][i],
                                Q.FWD_SLACK)
    # backward, on the device
    masks = [(a > 0).cpu() for a in acts[1:]]
    dz = (dyl * masks[2]).to(DEV)
    got = [None] * 3
    for i in (2, 1, 0):
        ci, H, W, co, k, s, p = layers[i]
        dw, db = torch.full_like(wd[i], NAN), torch.full_like(bd[i], NAN)
        scratch, nbytes = _scratch(n, layers[i])
        L.call('smi_conv2d_backward_weight', L.ptr(dz), L.ptr(acts[i]), int(i == 0), int(i == 0), n,
               ci, H, W, co, k, s, p, L.ptr(dw), L.ptr(db), L.ptr(scratch), nbytes, st)
        got[i] = (dw.cpu(), db.cpu())
        if i:
            dx = torch.full_like(acts[i], NAN)
            L.call('smi_conv2d_backward_input', L.ptr(dz), n, ci, H, W, L.ptr(wd[i]), co, k, s, p,
                   L.ptr(acts[i]), L.ptr(dx), st)
            dz = dx
    # torch backward with the device's masks, layer by layer
    want = {}
    for dt in (torch.float32, torch.float64):
        a, out = refs[dt], [None] * 3
        d = dyl.to(dt) * masks[2]
        for i in (2, 1, 0):
            ci, H, W, co, k, s, p = layers[i]
            xi = a[i].detach().clone().requires_grad_(True)
            w, b = ws[i].to(dt).requires_grad_(True), bs[i].to(dt).requires_grad_(True)
            gx, gw, gb = torch.autograd.grad(F.conv2d(xi, w, b, stride=s, padding=p), (xi, w, b), d)
            out[i] = (gw, gb, float((d.abs().double().sum(dim=(0, 2, 3))).max()))
            if i:
                d = gx * masks[i - 1]
        want[dt] = out
    for i in range(3):
        w32, w64 = want[torch.float32][i], want[torch.float64][i]
        # (mag of dw: |dz| summed times the largest activation bounds every sum of |terms|)
        amax = float(refs[torch.float64][i].abs().max())
        Q.fp32_as_good_as_torch(got[i][0], w32[0], w64[0], Q.GRAD_SLACK, w64[2] * amax)
        Q.fp32_as_good_as_torch(got[i][1], w32[1], w64[1], Q.GRAD_SLACK, w64[2])


def test_argument_errors_leave_the_outputs_untouched():
    lib = L.lib()
    c = Q.LayerCase('halo_2x5x7', 2)
    cin, H, W, cout, k, s, p = c.geom
    x, w, b, dy = c.x.to(DEV), c.w.to(DEV), c.b.to(DEV), c.dy.to(DEV)
    y = torch.full((2, cout, c.ho, c.wo), NAN, device=DEV)
    dx = torch.full((2, cin, H, W), NAN, device=DEV)
    dw, db = torch.full_like(w, NAN), torch.full_like(b, NAN)
    scratch, nbytes = _scratch(2, c.geom)
    st = L.stream()
    P = L.ptr

    def fwd(cin=cin, H=H, W=W, cout=cout, k=k, s=s, p=p, x=x, w=w, b=b, y=y, act=1, n=2):
        return lib.smi_conv2d_forward(P(x), 0, 0, n, cin, H, W, P(w), P(b), cout, k, s, p, act, P(y), st)

    def bwi(cin=cin, cout=cout, k=k, s=s, p=p, dy=dy, w=w, dx=dx, n=2):
        return lib.smi_conv2d_backward_input(P(dy), n, cin, H, W, P(w), cout, k, s, p, None, P(dx), st)

    def bww(cin=cin, cout=cout, k=k, s=s, p=p, dy=dy, x=x, dw=dw, db=db, scratch=scratch,
            nbytes=nbytes, n=2):
        return lib.smi_conv2d_backward_weight(P(dy), P(x), 0, 0, n, cin, H, W, cout, k, s, p, P(dw),
                                              P(db), P(scratch), nbytes, st)
    bad = [dict(k=9), dict(k=0), dict(s=0), dict(s=4), dict(k=8, s=5, p=3), dict(p=3), dict(p=-1),
           dict(cin=129), dict(cin=0), dict(cout=129), dict(cout=0), dict(n=-1)]
    for kw in bad:
        assert fwd(**kw) == E_ARG, kw
        assert lib.smi_last_error()
        assert bwi(**kw) == E_ARG, kw
        assert bww(**kw) == E_ARG, kw
    assert fwd(H=1, W=1, k=8, s=1, p=0) == E_ARG              # Ho < 1
    assert fwd(act=2) == E_ARG
    for kw in (dict(x=None), dict(w=None), dict(b=None), dict(y=None)):
        assert fwd(**kw) == E_ARG, kw
    for kw in (dict(dy=None), dict(w=None), dict(dx=None)):
        assert bwi(**kw) == E_ARG, kw
    for kw in (dict(dy=None), dict(x=None), dict(dw=None), dict(db=None), dict(scratch=None),
               dict(nbytes=nbytes - 4)):
        assert bww(**kw) == E_ARG, kw
    assert b'scratch' in lib.smi_last_error()
    ho, wo = ctypes.c_int(-7), ctypes.c_int(-7)
    assert lib.smi_conv2d_out_hw(84, 84, 9, 4, 4, ctypes.byref(ho), ctypes.byref(wo)) == E_ARG
    assert (ho.value, wo.value) == (-7, -7)
    assert lib.smi_conv2d_out_hw(84, 84, 8, 4, 4, ctypes.byref(ho), ctypes.byref(wo)) == 0
    assert (ho.value, wo.value) == (22, 22)
    assert lib.smi_conv2d_out_hw(9, 11, 4, 2, 2, ctypes.byref(ho), ctypes.byref(wo)) == 0
    assert (ho.value, wo.value) == (5, 6)
    assert lib.smi_conv2d_scratch_bytes(2, cin, H, W, cout, 9, s, p) == -1
    # n == 0: SMI_OK, nothing launched
    assert fwd(n=0) == 0 and bwi(n=0) == 0 and bww(n=0) == 0
    assert lib.smi_conv2d_scratch_bytes(0, cin, H, W, cout, k, s, p) == 0
    torch.cuda.synchronize()
    for t in (y, dx, dw, db, scratch):
        assert bool(torch.isnan(t).all())
    # and the same operands do run
    assert fwd() == 0 and bwi() == 0 and bww() == 0
    torch.cuda.synchronize()
    for t in (y, dx, dw, db):
        assert bool(torch.isfinite(t).all())
