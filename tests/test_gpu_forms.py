"""Direct parity of the kernel forms the host dispatch reaches in a default
build, one small shape per template instantiation of the LSTM, head, GEMM and
GAE launchers ("Dispatch coverage", lists what selects each).

Every case calls the C ABI the way the sibling tests do, asserts that
smi_last_launch() names the instantiation the case was written for (a later
re-tuning of the dispatch turns the case red instead of silently testing
another form), and compares every output with torch on the CPU in fp64 on the
siblings' bars: LSTM h / c 2e-6 and the weight gradients assembled from dgates
4e-6 (test_gpu_rnn.py), heads and GEMMs 1e-6 with the row-sum magnitude for
the weight gradients (test_gpu_head.py, test_gpu_ddpg.py), GAE RTOL against
oracle.ppo_ref.gae_and_return (test_gpu_ops.py).

Batches are a handful of segments or CUs + 1 (the device's CU count decides
between the one-segment-per-workgroup K-split forms and the 4-segment MFMA
forms), sequences 2-4 steps, sizes ragged."""
import ctypes

import pytest
import torch

from oracle import ppo_ref as R
from surreal_amd import _lib as L
from tests.helpers import lstm_flat, max_rel_err
from tests.test_gpu_ddpg import _fp32_as_good_as_torch
from tests.test_gpu_ops import RTOL

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


def setup_module(m):
    L.ensure_workspace(DEV)       # split-K partials


def _last():
    return L.lib().smi_last_launch().decode()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------- LSTM
def _q(kq, xq, w, xm=False):
    """lstm_fwd_q_kernel: the K-split form at one segment per workgroup."""
    return f'lstm_fwd_q_kernel<{kq},{xq},{"xm" if xm else "xv"},w{w}{",a4" if xm else ""}>'


def _r4(kp, kx, vf):
    return f'lstm_fwd_r4_kernel<{kp},{kx}{",vf" if vf else ""}>'


def _bq(br):
    return f'lstm_bwd_q_kernel<{br}>'


def _bv(kp):
    return f'lstm_bwd_v_kernel<1,{kp}>'


def _br4(kw):
    return f'lstm_bwd_r4_kernel<{kw}>'


def _padded(x2d, pad):
    """rows of x2d in a buffer of row stride cols + pad, the padding NaN."""
    rows, cols = x2d.shape
    buf = torch.full((rows, cols + pad), NAN)
    buf[:, :cols] = x2d
    return buf.to(DEV)


def _lstm_check(B, S, D, H, pad, f_fwd, f_fwdx, f_bwd, seed):
    g = torch.Generator().manual_seed(seed)
    lstm = torch.nn.LSTM(D, H, 1, batch_first=True)
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_(torch.empty(p.shape).uniform_(-0.4, 0.4, generator=g))
    x = torch.randn(B, S, D, generator=g)
    h0 = 0.3 * torch.randn(1, B, H, generator=g)
    c0 = 0.3 * torch.randn(1, B, H, generator=g)
    dh = torch.randn(B, S, H, generator=g)
    flat = lstm_flat(lstm).to(DEV)
    o = 0
    Wih = flat[o:o + 4 * H * D]; o += 4 * H * D
    Whh = flat[o:o + 4 * H * H]; o += 4 * H * H
    bih = flat[o:o + 4 * H]; o += 4 * H
    bhh = flat[o:o + 4 * H]
    st = L.stream()
    ldx = D + pad
    xt = _padded(x.transpose(0, 1).reshape(S * B, D), pad)       # [S][B] rows of ldx floats
    xproj = torch.empty(S, B, 4 * H, device=DEV)
    L.call('smi_linear_forward', L.ptr(xt), ldx, S * B, D, L.ptr(Wih), D, L.ptr(bih), 4 * H, 0,
           L.ptr(xproj), 4 * H, st)
    hbuf = torch.full((S + 1, B, H), NAN, device=DEV)
    cbuf = torch.full((S + 1, B, H), NAN, device=DEV)
    gates = torch.full((S, B, 4 * H), NAN, device=DEV)
    h0d, c0d = h0[0].contiguous().to(DEV), c0[0].contiguous().to(DEV)
    L.call('smi_lstm_forward', L.ptr(xproj), L.ptr(Whh), L.ptr(bhh), L.ptr(h0d), L.ptr(c0d),
           S, B, H, L.ptr(hbuf), L.ptr(cbuf), L.ptr(gates), st)
    assert _last() == f_fwd
    out, (hn, cn) = lstm(x, (h0, c0))
    l64 = torch.nn.LSTM(D, H, 1, batch_first=True).double()
    l64.load_state_dict({k: v.double() for k, v in lstm.state_dict().items()})
    out64, (hn64, cn64) = l64(x.double(), (h0.double(), c0.double()))
    _fp32_as_good_as_torch(hbuf[1:].transpose(0, 1).cpu(), out.detach(), out64.detach(), 2e-6)
    _fp32_as_good_as_torch(cbuf[S].cpu(), cn[0].detach(), cn64[0].detach(), 2e-6)
    assert torch.equal(hbuf[0].cpu(), h0[0]) and torch.equal(cbuf[0].cpu(), c0[0])
    assert bool(torch.isfinite(gates).all())
    # the fused input projection, or its xproj GEMM + recurrence fallback
    hbx, cbx = torch.full_like(hbuf, NAN), torch.full_like(cbuf, NAN)
    gx, xps = torch.full_like(gates, NAN), torch.empty_like(xproj)
    L.call('smi_lstm_forward_x', L.ptr(xt), ldx, D, L.ptr(Wih), L.ptr(bih), L.ptr(Whh), L.ptr(bhh),
           L.ptr(h0d), L.ptr(c0d), S, B, H, L.ptr(hbx), L.ptr(cbx), L.ptr(gx), L.ptr(xps), st)
    assert _last() == f_fwdx
    _fp32_as_good_as_torch(hbx[1:].transpose(0, 1).cpu(), out.detach(), out64.detach(), 2e-6)
    _fp32_as_good_as_torch(cbx[S].cpu(), cn[0].detach(), cn64[0].detach(), 2e-6)
    assert torch.equal(hbx[0].cpu(), h0[0]) and torch.equal(cbx[0].cpu(), c0[0])
    torch.testing.assert_close(gx.cpu(), gates.cpu(), rtol=0, atol=2e-5)
    # backward: loss = sum(out * dh)
    dht = dh.transpose(0, 1).contiguous().to(DEV)
    dgates = torch.full((S, B, 4 * H), NAN, device=DEV)
    L.call('smi_lstm_backward', L.ptr(dht), L.ptr(gates), L.ptr(cbuf), L.ptr(Whh), S, B, H,
           L.ptr(dgates), st)
    assert _last() == f_bwd
    (out64 * dh.double()).sum().backward()
    (out * dh).sum().backward()
    dg = dgates.reshape(S * B, 4 * H)
    hprev = hbuf[:S].reshape(S * B, H)
    gWih = torch.empty(4 * H, D, device=DEV)
    gWhh = torch.empty(4 * H, H, device=DEV)
    gb = torch.empty(4 * H, device=DEV)
    gb2 = torch.empty(4 * H, device=DEV)
    L.call('smi_linear_backward_weight', L.ptr(dg), 4 * H, S * B, 4 * H, L.ptr(xt), ldx, D,
           L.ptr(gWih), D, L.ptr(gb), 0, st)
    L.call('smi_linear_backward_weight', L.ptr(dg), 4 * H, S * B, 4 * H, L.ptr(hprev), H, H,
           L.ptr(gWhh), H, L.ptr(gb2), 0, st)
    for got, p32, p64 in ((gWih, lstm.weight_ih_l0, l64.weight_ih_l0),
                          (gWhh, lstm.weight_hh_l0, l64.weight_hh_l0),
                          (gb, lstm.bias_ih_l0, l64.bias_ih_l0),
                          (gb2, lstm.bias_hh_l0, l64.bias_hh_l0)):
        _fp32_as_good_as_torch(got.cpu(), p32.grad, p64.grad, 4e-6)


# (big, S, din, H, ldx - din, forward, fused-input forward, BPTT); big: CUs + 1
# segments (the 4-segment MFMA forms) instead of a handful (the K-split forms).
# A fused-input form with x columns 0 is the xproj GEMM + recurrence fallback.
LSTM_CASES = [
    # B <= CUs: W_hh layout w2 / w1 / w0 by H % 4 / H % 2, KQ by H; BPTT K-split
    # (H % 4 == 0; BR 16 / 25 / 32) or the row forms 64 / 104 / 128
    (0, 3, 7, 18, 0, _q(16, 0, 1), _q(16, 12, 1), _bv(64)),
    (0, 3, 7, 19, 0, _q(16, 0, 0), _q(16, 12, 0), _bv(64)),
    (0, 3, 7, 68, 0, _q(28, 0, 2), _q(28, 12, 2), _bq(25)),
    (0, 3, 7, 98, 0, _q(26, 0, 1), _q(26, 12, 1), _bv(104)),
    (0, 3, 7, 99, 0, _q(26, 0, 0), _q(26, 12, 0), _bv(104)),
    (0, 3, 8, 104, 0, _q(28, 0, 2), _q(28, 12, 2, True), _bq(32)),
    (0, 3, 8, 112, 0, _q(28, 0, 2), _q(28, 0, 2), _bq(32)),          # H > 104: not fused
    (0, 3, 7, 113, 0, _q(32, 0, 0), _q(32, 0, 0), _bv(128)),
    (0, 3, 8, 114, 0, _q(32, 0, 1), _q(32, 0, 1), _bv(128)),
    (0, 2, 8, 128, 0, _q(32, 0, 2), _q(32, 0, 2), _bq(32)),
    # fused input at B <= CUs: x columns per lane 12 (din <= 48) / 16, the
    # matrix-core x parts for an even din
    (0, 3, 47, 100, 3, _q(28, 0, 2), _q(28, 12, 2), _bq(25)),
    (0, 3, 48, 100, 3, _q(28, 0, 2), _q(28, 12, 2, True), _bq(25)),
    (0, 3, 50, 100, 0, _q(28, 0, 2), _q(28, 16, 2, True), _bq(25)),
    (0, 3, 64, 50, 0, _q(16, 0, 1), _q(16, 16, 1, True), _bv(64)),
    (0, 3, 51, 99, 0, _q(26, 0, 0), _q(26, 16, 0), _bv(104)),
    (0, 3, 65, 100, 0, _q(28, 0, 2), _q(28, 0, 2), _bq(25)),         # din > 64: not fused
    # B = CUs + 1, fused input: KP 64 / 104 x KX 48 / 64, vf (H % 4 == 0 and an
    # even din) on and off; unfused KP 32 / 64 / 104 / 128
    (1, 3, 47, 64, 3, _r4(64, 0, True), _r4(64, 48, False), _br4(32)),
    (1, 2, 8, 20, 0, _r4(32, 0, True), _r4(64, 48, True), _br4(32)),
    (1, 2, 7, 18, 0, _r4(32, 0, False), _r4(64, 48, False), _br4(32)),
    (1, 3, 50, 50, 0, _r4(64, 0, False), _r4(64, 64, False), _br4(32)),
    (1, 2, 64, 60, 0, _r4(64, 0, True), _r4(64, 64, True), _br4(32)),
    (1, 3, 47, 102, 0, _r4(104, 0, False), _r4(104, 48, False), _br4(104)),
    (1, 3, 48, 100, 3, _r4(104, 0, True), _r4(104, 48, True), _br4(104)),
    (1, 2, 63, 98, 0, _r4(104, 0, False), _r4(104, 64, False), _br4(104)),
    (1, 2, 64, 100, 0, _r4(104, 0, True), _r4(104, 64, True), _br4(104)),
    (1, 2, 65, 100, 0, _r4(104, 0, True), _r4(104, 0, True), _br4(104)),
    (1, 2, 9, 126, 0, _r4(128, 0, False), _r4(128, 0, False), _br4(128)),
    # hidden size limits: the 16-segment streaming forms beyond H = 128
    (0, 2, 9, 129, 0, 'lstm_fwd_kernel<4>', 'lstm_fwd_kernel<4>', 'lstm_bwd_kernel<4>'),
    (0, 2, 9, 256, 0, 'lstm_fwd_kernel<4>', 'lstm_fwd_kernel<4>', 'lstm_bwd_kernel<4>'),
]


@pytest.mark.parametrize('big,S,D,H,pad,f_fwd,f_fwdx,f_bwd', LSTM_CASES,
                         ids=[f'{"cu1" if c[0] else "few"}-S{c[1]}-D{c[2]}-H{c[3]}' for c in LSTM_CASES])
def test_lstm_forms(big, S, D, H, pad, f_fwd, f_fwdx, f_bwd):
    cus = _cus()
    B = cus + 1 if big else min(5, cus)
    _lstm_check(B, S, D, H, pad, f_fwd, f_fwdx, f_bwd, seed=1000 * H + D)


def _fwd_v_lds(S, kx, blk):
    """lstm_fwd_v_lds (lstm_cell.hpp) at one segment per workgroup: bytes of
    the staged x sequence + the x parts."""
    return (((S * kx + 3) & ~3) + S * blk) * 4


@pytest.mark.parametrize('over', [0, 1])
def test_lstm_fused_lds_budget_edge(over):
    """H = 100, din = 42, 3 segments: the longest sequence whose staged x and x
    parts fit the fused form's LDS budget (kVxMax = 120 KiB) runs fused; one
    step more takes the xproj GEMM + recurrence."""
    H, D, B = 100, 42, 3
    blk = (4 * H + 63) & ~63
    S = 1
    while _fwd_v_lds(S + 1, 48, blk) <= 120 * 1024:
        S += 1
    assert _fwd_v_lds(S, 48, blk) <= 120 * 1024 < _fwd_v_lds(S + 1, 48, blk)
    fwdx = _q(28, 0, 2) if over else _q(28, 12, 2, True)
    _lstm_check(B, S + over, D, H, 0, _q(28, 0, 2), fwdx, _bq(25), seed=77)


def test_lstm_zero_steps():
    """S = 0: smi_lstm_forward_x and smi_lstm_backward launch nothing and leave
    every buffer untouched; smi_lstm_forward writes row 0 (h0 / c0) only
    (include/surreal_mi.h)."""
    B, H, D = 3, 20, 7
    g = torch.Generator().manual_seed(5)
    Wih, Whh = (torch.randn(4 * H, k, generator=g).to(DEV) for k in (D, H))
    bih, bhh = (torch.randn(4 * H, generator=g).to(DEV) for _ in range(2))
    h0, c0 = (torch.randn(B, H, generator=g) for _ in range(2))
    h0d, c0d = h0.to(DEV), c0.to(DEV)
    x = torch.full((B, D), NAN, device=DEV)              # one step's worth, never read
    xproj = torch.full((1, B, 4 * H), NAN, device=DEV)
    st = L.stream()
    # a launch of another family first: the calls that launch nothing leave it
    y = torch.empty(B, 4 * H, device=DEV)
    L.call('smi_linear_forward', L.ptr(h0d), H, B, H, L.ptr(Whh), H, L.ptr(bhh), 4 * H, 0, L.ptr(y),
           4 * H, st)
    before = _last()
    assert before.startswith('gemm_')

    def bufs():
        return (torch.full((2, B, H), NAN, device=DEV), torch.full((2, B, H), NAN, device=DEV),
                torch.full((1, B, 4 * H), NAN, device=DEV))
    hb, cb, gt = bufs()
    rc = L.lib().smi_lstm_forward_x(L.ptr(x), D, D, L.ptr(Wih), L.ptr(bih), L.ptr(Whh), L.ptr(bhh),
                                    L.ptr(h0d), L.ptr(c0d), 0, B, H, L.ptr(hb), L.ptr(cb), L.ptr(gt),
                                    L.ptr(xproj), st)
    assert rc == 0 and _last() == before
    for t in (hb, cb, gt, xproj):
        assert bool(torch.isnan(t).all())
    dg = torch.full((1, B, 4 * H), NAN, device=DEV)
    rc = L.lib().smi_lstm_backward(L.ptr(hb), L.ptr(gt), L.ptr(cb), L.ptr(Whh), 0, B, H, L.ptr(dg), st)
    assert rc == 0 and _last() == before and bool(torch.isnan(dg).all())
    hb, cb, gt = bufs()
    rc = L.lib().smi_lstm_forward(L.ptr(xproj), L.ptr(Whh), L.ptr(bhh), L.ptr(h0d), L.ptr(c0d), 0, B, H,
                                  L.ptr(hb), L.ptr(cb), L.ptr(gt), st)
    assert rc == 0 and _last() == _q(16, 0, 2)
    assert torch.equal(hb[0].cpu(), h0) and torch.equal(cb[0].cpu(), c0)
    for t in (hb[1], cb[1], gt):
        assert bool(torch.isnan(t).all())


# ------------------------------------------------------------------ heads
def _head_flat(W1, b1, W2, b2, W3, b3):
    return torch.cat([W1.reshape(-1), b1, W2.reshape(-1), b2, W3.reshape(-1), b3]).float()


# (rows, in, h1, h2, out, tanh, dx0, dxn, forward slots, backward slots): the
# width slots are ceil(ceil(w / 16) / 4) 16-column tiles per wave rounded up to
# an instantiation, edges at 128 / 192 / 256 / 320; layer 1 and the backward's
# h1 side use {2, 5, 8}, the backward's dX side {2, 5} (dxn <= 128 or beyond)
HEAD_CASES = [
    (37, 4, 128, 128, 1, 0, 1, 3, '2,2', '2,2'),
    (37, 320, 128, 132, 8, 1, 2, 129, '2,3', '2,5'),
    (37, 4, 128, 196, 16, 0, 1, 3, '2,4', '2,2'),
    (37, 320, 128, 260, 1, 0, 2, 128, '2,5', '2,2'),
    (37, 4, 128, 324, 8, 0, 1, 3, '2,8', '2,2'),
    (37, 320, 132, 128, 16, 1, 2, 128, '5,2', '5,2'),
    (37, 4, 320, 192, 1, 0, 1, 3, '5,3', '5,2'),
    (37, 320, 132, 256, 8, 0, 2, 129, '5,4', '5,5'),
    (37, 4, 320, 320, 16, 0, 1, 3, '5,5', '5,2'),
    (37, 320, 132, 512, 1, 0, 3, 317, '5,8', '5,5'),
    (37, 4, 324, 128, 8, 1, 1, 3, '8,2', '8,2'),
    (37, 320, 512, 192, 16, 0, 2, 128, '8,3', '8,2'),
    (37, 4, 324, 256, 1, 0, 1, 3, '8,4', '8,2'),
    (37, 320, 512, 320, 8, 0, 2, 129, '8,5', '8,5'),
    (37, 320, 324, 512, 16, 1, 2, 318, '8,8', '8,5'),
    # two row tiles per workgroup (rows >= 16384), the last tile ragged
    (16384 + 5, 100, 300, 200, 8, 1, 2, 98, '5,4', '5,2'),
]


@pytest.mark.parametrize('rows,din,h1,h2,out,tanh_out,dx0,dxn,f_fwd,f_bwd', HEAD_CASES,
                         ids=[f'r{c[0]}-{c[1]}x{c[2]}x{c[3]}x{c[4]}' for c in HEAD_CASES])
def test_head_forms(rows, din, h1, h2, out, tanh_out, dx0, dxn, f_fwd, f_bwd):
    rt = 'rt2' if rows >= 16384 else 'rt1'
    g = torch.Generator().manual_seed(rows + din + h1 + h2)
    lins = [torch.nn.Linear(din, h1), torch.nn.Linear(h1, h2), torch.nn.Linear(h2, out)]
    (W1, b1), (W2, b2), (W3, b3) = ((l.weight.detach(), l.bias.detach()) for l in lins)
    x = torch.randn(rows, din, generator=g)
    dz = torch.randn(rows, out, generator=g)
    P = _head_flat(W1, b1, W2, b2, W3, b3).cuda()
    ldx = din + 4                                          # the fused head takes ldx % 4 == 0
    xd, dzd = _padded(x, 4), dz.cuda()
    ha1 = torch.full((rows, h1), NAN, device=DEV)
    ha2 = torch.full((rows, h2), NAN, device=DEV)
    y = torch.full((rows, out), NAN, device=DEV)
    wT = torch.empty(din * h1 + h1 * h2, device=DEV)
    st = L.stream()
    L.call('smi_head_forward', L.ptr(P), din, h1, h2, out, tanh_out, L.ptr(xd), ldx, rows,
           L.ptr(ha1), L.ptr(ha2), L.ptr(y), L.ptr(wT), st)
    assert _last() == f'head_fwd_kernel<{f_fwd},{rt}>'
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
    # backward from dz with the GPU's masks, dX over columns [dx0, dx0 + dxn)
    m1, m2 = (ha1 > 0).cpu(), (ha2 > 0).cpu()
    dh2 = torch.full((rows, h2), NAN, device=DEV)
    dh1 = torch.full((rows, h1), NAN, device=DEV)
    dx = torch.full((rows, dxn), NAN, device=DEV)
    L.call('smi_head_backward_input', L.ptr(P), din, h1, h2, out, L.ptr(wT), L.ptr(dzd), rows,
           L.ptr(ha1), L.ptr(ha2), L.ptr(dh2), L.ptr(dh1), dx0, dxn, L.ptr(dx), dxn, None, 0, st)
    assert _last() == f'head_bwd_kernel<{f_bwd},{rt}>'

    def bwd(dt):
        d2 = (dz.to(dt) @ W3.to(dt)) * m2
        d1 = (d2 @ W2.to(dt)) * m1
        return d2, d1, d1 @ W1.to(dt)[:, dx0:dx0 + dxn]
    b32, b64 = bwd(torch.float32), bwd(torch.float64)
    for got, e32, e64 in zip((dh2, dh1, dx), b32, b64):
        _fp32_as_good_as_torch(got.cpu(), e32, e64)
    # with a mask on dX
    mask = torch.randn(rows, dxn, generator=g).cuda()
    dx.fill_(NAN)
    L.call('smi_head_backward_input', L.ptr(P), din, h1, h2, out, L.ptr(wT), L.ptr(dzd), rows,
           L.ptr(ha1), L.ptr(ha2), L.ptr(dh2), L.ptr(dh1), dx0, dxn, L.ptr(dx), dxn, L.ptr(mask),
           dxn, st)
    assert _last() == f'head_bwd_kernel<{f_bwd},{rt}>'
    mk = (mask > 0).cpu()
    _fp32_as_good_as_torch(dx.cpu(), b32[2] * mk, b64[2] * mk)


# ------------------------------------------------------------------ GEMMs
RED = 'gemm_splitk_reduce_kernel<%s>'
# (op, rows, k, n, form) of a Linear(k, n) layer over `rows` rows
GEMM_CASES = [
    # row panels (>= 4096 rows): 16-column tiles per column group by the cost rule
    ('fwd', 4100, 68, 24, 'gemm_panel_kernel<fwd,2>'),
    ('fwd', 4100, 68, 60, 'gemm_panel_kernel<fwd,4>'),
    ('fwd', 4100, 68, 72, 'gemm_panel_kernel<fwd,5>'),
    # the input gradient's panel from 96 columns up: 6 tiles -> groups of 2,
    # 8 -> 4, 15 -> 5 (7 and 9..10 tiles take 7 and 10, covered by test_gpu_ddpg)
    ('dx', 4100, 96, 20, 'gemm_panel_kernel<dx,2>'),
    ('dx', 4100, 116, 12, 'gemm_panel_kernel<dx,4>'),
    ('dx', 4100, 128, 20, 'gemm_panel_kernel<dx,4>'),
    ('dx', 4100, 228, 12, 'gemm_panel_kernel<dx,5>'),
    ('dx', 4100, 240, 20, 'gemm_panel_kernel<dx,5>'),
    # K <= 16 on the small-K forward
    ('fwd', 2050, 12, 40, 'gemm_smallk_fwd_kernel<4>'),
    ('fwd', 2050, 16, 33, 'gemm_smallk_fwd_kernel<4>'),
    # the input gradient through a layer of 2 outputs
    ('dx', 777, 100, 2, 'dx_smallk_kernel<2,v4>'),
    ('dx', 777, 99, 2, 'dx_smallk_kernel<2>'),
    # the short-batch kernel's longest K (8 chunks of 16 per wave) and its neighbour
    ('fwd', 300, 512, 40, 'gemm_t16_kernel<fwd>'),
    ('fwd', 300, 516, 40, RED % 'gemm_kernel<fwd>'),
    ('dx', 300, 40, 512, 'gemm_t16_kernel<dx>'),
    ('dx', 300, 40, 516, RED % 'gemm_kernel<dx>'),
    # 128 x 128 weight-gradient tiles: an output side > 512 and >= 1024 rows
    ('dw', 1100, 96, 516, RED % 'gemm_dw128_kernel'),
    ('dw_group', 1100, 96, 516, RED % 'gemm_dw128_kernel'),
]


@pytest.mark.parametrize('op,rows,k,n,form', GEMM_CASES,
                         ids=[f'{c[0]}-{c[1]}x{c[2]}x{c[3]}' for c in GEMM_CASES])
def test_gemm_forms(op, rows, k, n, form):
    g = torch.Generator().manual_seed(rows + k + n)
    x = torch.randn(rows, k, generator=g)
    lin = torch.nn.Linear(k, n)
    W, b = lin.weight.detach(), lin.bias.detach()
    dy = torch.randn(rows, n, generator=g)
    xd, wd, bd, dyd = x.cuda(), W.cuda().contiguous(), b.cuda(), dy.cuda()
    st = L.stream()
    if op == 'fwd':
        y = torch.full((rows, n), NAN, device=DEV)
        L.call('smi_linear_forward', L.ptr(xd), k, rows, k, L.ptr(wd), k, L.ptr(bd), n, 1, L.ptr(y), n, st)
        assert _last() == form
        _fp32_as_good_as_torch(y.cpu(), torch.relu(x @ W.t() + b),
                               torch.relu(x.double() @ W.double().t() + b.double()))
        return
    if op == 'dx':
        dx = torch.full((rows, k), NAN, device=DEV)
        L.call('smi_linear_backward_input', L.ptr(dyd), n, rows, n, L.ptr(wd), k, k, L.ptr(xd), k,
               L.ptr(dx), k, st)
        assert _last() == form
        _fp32_as_good_as_torch(dx.cpu(), (dy @ W) * (x > 0), (dy.double() @ W.double()) * (x > 0))
        return
    dw = torch.full((n, k), NAN, device=DEV)
    db = torch.full((n,), NAN, device=DEV)
    mw = float((dy.abs().t() @ x.abs()).max())
    mb = float(dy.abs().sum(0).max())
    grouped = op == 'dw_group'
    if grouped:      # too large to join the group: launches at once inside the bracket
        L.call('smi_dw_group_begin')
    for acc in (0, 1):                                   # plain, then accumulating
        L.call('smi_linear_backward_weight', L.ptr(dyd), n, rows, n, L.ptr(xd), k, k, L.ptr(dw), k,
               L.ptr(db), acc, st)
        assert _last() == form
        f = 1 + acc
        _fp32_as_good_as_torch(dw.cpu(), f * (dy.t() @ x), f * (dy.double().t() @ x.double()), 1e-6,
                               f * mw)
        _fp32_as_good_as_torch(db.cpu(), f * dy.sum(0), f * dy.double().sum(0), 1e-6, f * mb)
    if grouped:
        L.call('smi_dw_group_flush', st)
        assert _last() == form                           # nothing was queued
        _fp32_as_good_as_torch(dw.cpu(), 2 * (dy.t() @ x), 2 * (dy.double().t() @ x.double()), 1e-6,
                               2 * mw)


# -------------------------------------------------------------------- GAE
# the generic window kernel: T + 1 > 64 rows, or windows longer than 16 steps
# with more than one window per segment; lanes per window by H / 3
@pytest.mark.parametrize('B,T,H,form', [(9, 70, 5, 'gae_windows_kernel<lg1>'),
                                        (7, 40, 20, 'gae_windows_kernel<lg4>'),
                                        (5, 70, 48, 'gae_windows_kernel<lg8>')])
def test_gae_forms(B, T, H, form):
    g = torch.Generator().manual_seed(B + T)
    v = torch.randn(B, T + 1, generator=g)
    r = torch.randn(B, T, generator=g)
    d = (torch.rand(B, T, generator=g) < 0.1).float()
    gamma, lam = 0.99, 0.95
    radv, rret = R.gae_and_return(v.clone(), r, d, gamma, lam, T, H, True, norm_adv=False)
    idx = torch.tensor(range(T), dtype=torch.float32)
    gtd, ltd = torch.pow(gamma, idx).to(DEV), torch.pow(lam, idx).to(DEV)
    E = T - H + 1
    vd, rd, dd = v.to(DEV), r.to(DEV), d.to(DEV)
    adv = torch.full((B, E), NAN, device=DEV)
    ret = torch.full((B, E), NAN, device=DEV)
    part = torch.zeros(2 * 2048, dtype=torch.float64, device=DEV)
    n = ctypes.c_int(0)
    L.call('smi_gae_windows', L.ptr(vd), L.ptr(vd), L.ptr(rd), L.ptr(dd), B, T, H, L.ptr(gtd),
           L.ptr(ltd), float(gamma), float(gamma ** H), L.ptr(adv), L.ptr(ret), L.ptr(part),
           ctypes.byref(n), L.stream())
    assert _last() == form
    adv, ret = adv.cpu(), ret.cpu()
    assert max_rel_err(adv, radv.reshape(B, -1)) < RTOL
    assert max_rel_err(ret, rret.reshape(B, -1)) < RTOL
    vref = v.clone(); vref[:, 1:] *= 1 - d
    assert torch.equal(vd.cpu(), vref)
    s = part[:2 * n.value].cpu().view(-1, 2).sum(0)
    assert abs(float(s[0]) - float(adv.double().sum())) <= 1e-9 * (1 + float(adv.double().abs().sum()))
    # (the second partial: the fp64 sum of squares of the stored fp32 advantages)
    sq = float(adv.double().pow(2).sum())
    assert abs(float(s[1]) - sq) <= 1e-9 * (1 + sq)
