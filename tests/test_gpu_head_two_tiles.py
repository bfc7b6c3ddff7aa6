"""The two-row-tile forms of the fused head chains (head_kernels.hip, rows >=
16384: 32 rows per workgroup) through the C ABI against torch, at the smallest
shapes that reach them and can break the forward's shared LDS carve
(head_plan, smi_shapes.hpp: X, HA1 and HA2 take turns in one region):
whole workgroups at the C3 widths; a ragged last workgroup whose second row
tile is part full; an input wider than HA1 and an HA2 wider than HA1 (the
region is sized by the widest, the last workgroup holds one row); every K not
a multiple of 16 (each tile's zero padding lands on a wider predecessor); and
the widest shapes the chains take.  Bar as tests/test_gpu_head.py: within 2x
torch-CPU fp32's own error against fp64 and 1e-5 of the tensor's scale
(test_gpu_ddpg._fp32_as_good_as_torch); the W1^T / W2^T side job exact."""
import pytest
import torch

from surreal_amd import _lib as L
from tests.test_gpu_ddpg import _fp32_as_good_as_torch
from tests.test_gpu_head import _flat

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('rows,din,h1,h2,out,tanh_out', [
    (16384, 100, 300, 200, 8, 1), (16411, 100, 300, 200, 1, 0), (16385, 64, 32, 64, 6, 0),
    (16400, 20, 36, 28, 3, 0), (16384, 320, 512, 512, 16, 0)])
def test_two_tile_head_forward_backward_vs_torch(rows, din, h1, h2, out, tanh_out):
    g = torch.Generator().manual_seed(rows + din + h1)
    torch.manual_seed(rows + 7 * din + h2)
    lins = [torch.nn.Linear(din, h1), torch.nn.Linear(h1, h2), torch.nn.Linear(h2, out)]
    (W1, b1), (W2, b2), (W3, b3) = ((l.weight.detach(), l.bias.detach()) for l in lins)
    x = torch.randn(rows, din, generator=g)
    dz = torch.randn(rows, out, generator=g)
    P = _flat(W1, b1, W2, b2, W3, b3).cuda()
    xd, dzd = x.cuda(), dz.cuda()
    ha1 = torch.full((rows, h1), float('nan'), device='cuda')
    ha2 = torch.full((rows, h2), float('nan'), device='cuda')
    y = torch.full((rows, out), float('nan'), device='cuda')
    wT = torch.empty(din * h1 + h1 * h2, device='cuda')
    st = L.stream()
    L.call('smi_head_forward', L.ptr(P), din, h1, h2, out, tanh_out, L.ptr(xd), din, rows,
           L.ptr(ha1), L.ptr(ha2), L.ptr(y), L.ptr(wT), st)
    torch.cuda.synchronize()
    # the transposes the backward reads
    assert torch.equal(wT[:din * h1].view(din, h1).cpu(), W1.t())
    assert torch.equal(wT[din * h1:].view(h1, h2).cpu(), W2.t())

    def fwd(dt):
        a1 = torch.relu(x.to(dt) @ W1.to(dt).t() + b1.to(dt))
        a2 = torch.relu(a1 @ W2.to(dt).t() + b2.to(dt))
        z = a2 @ W3.to(dt).t() + b3.to(dt)
        return a1, a2, torch.tanh(z) if tanh_out else z
    r32, r64 = fwd(torch.float32), fwd(torch.float64)
    for got, e32, e64 in zip((ha1, ha2, y), r32, r64):
        _fp32_as_good_as_torch(got.cpu(), e32, e64)
    # backward from dz with the GPU's masks, dX over columns [2, 2 + dxn)
    m1, m2 = (ha1 > 0).cpu(), (ha2 > 0).cpu()
    dx0 = 2 if din > 8 else 0
    dxn = din - dx0
    dh2 = torch.full((rows, h2), float('nan'), device='cuda')
    dh1 = torch.full((rows, h1), float('nan'), device='cuda')
    dx = torch.full((rows, dxn), float('nan'), device='cuda')
    L.call('smi_head_backward_input', L.ptr(P), din, h1, h2, out, L.ptr(wT), L.ptr(dzd), rows,
           L.ptr(ha1), L.ptr(ha2), L.ptr(dh2), L.ptr(dh1), dx0, dxn, L.ptr(dx), dxn, None, 0, st)

    def bwd(dt):
        d2 = (dz.to(dt) @ W3.to(dt)) * m2
        d1 = (d2 @ W2.to(dt)) * m1
        return d2, d1, d1 @ W1.to(dt)[:, dx0:dx0 + dxn]
    b32, b64 = bwd(torch.float32), bwd(torch.float64)
    for got, e32, e64 in zip((dh2, dh1, dx), b32, b64):
        _fp32_as_good_as_torch(got.cpu(), e32, e64)
    # with a mask on dX (the MLP policy's CNN-feature columns)
    mask = torch.randn(rows, dxn, generator=g).cuda()
    dx.fill_(float('nan'))
    L.call('smi_head_backward_input', L.ptr(P), din, h1, h2, out, L.ptr(wT), L.ptr(dzd), rows,
           L.ptr(ha1), L.ptr(ha2), L.ptr(dh2), L.ptr(dh1), dx0, dxn, L.ptr(dx), dxn, L.ptr(mask),
           dxn, st)
    mk = (mask > 0).cpu()
    _fp32_as_good_as_torch(dx.cpu(), b32[2] * mk, b64[2] * mk)
