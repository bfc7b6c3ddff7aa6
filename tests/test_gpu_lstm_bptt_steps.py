"""The 4-segment BPTT (lstm_bwd_r4_kernel<KW>) at the step counts, hidden sizes
and batch tails where its step pipeline changes shape.

The kernel loads a step's inputs (activated gates, c_t, c_{t-1}, dh_t) two
steps ahead into two register sets alternated by step parity, from addresses
clamped at step 0 and at the last row, sums the K-split partial sums of
dh_rec in one LDS trip (8 partials at H <= 64, 4 beyond) and computes the
gate-only factors of the cell backward a phase early.  So:

  S = 1         no MFMA phase, nothing prefetched
  S = 2, 3      the two-ahead fetch clamps at step 0
  S = 6, 7      both register sets used three times; even / odd step counts
                end on either set
  H = 64        KW 32, 8 partial sums        H = 65   KW 104, the smallest
  H = 100       the C3 form                            two-group shape
  H = 128       KW 128
  B = CUs + 1, + 3, + 4 (rounded to 1, 3, 0 mod 4): one, three valid rows in
                the last workgroup, and no tail

Every case goes through the C ABI as test_gpu_forms._lstm_check does
(smi_lstm_forward_x for the gates and cells, then smi_lstm_backward), asserts
the form by smi_last_launch and compares on _lstm_check's bars: h / c 2e-6 and
the weight gradients assembled from dgates 4e-6, each "as good as torch's own
fp32" against fp64 autograd on the CPU.  dgates itself is compared the same way
(2e-6: element-wise like h / c, one 4H-term dot per step) with an fp64
restatement of the cell backward computed here from the kernel's own inputs;
the fp32 side is the same restatement in fp32.

The BPTT's inputs sit inside larger NaN-filled allocations, once at the start
and once at the very end (a whole step of NaN beside them), and dgates starts
as NaN: a prefetch one step or one row outside its data, or an element never
written, shows as a NaN in the result without reading outside an allocation.
"""
import pytest
import torch

from surreal_amd import _lib as L
from tests.helpers import lstm_flat
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
D = 7


def setup_module(m):
    L.ensure_workspace(DEV)       # split-K partials of the weight-gradient GEMMs


def _last():
    return L.lib().smi_last_launch().decode()


def _batch(tail):
    """the smallest B > CUs with B % 4 == tail"""
    n = torch.cuda.get_device_properties(0).multi_processor_count + 1
    return n + (tail - n) % 4


def _kw(H):
    return 32 if H <= 64 else 104 if H <= 104 else 128


def _cell_backward(gates, cbuf, dh, whh):
    """dgates [S][B][4H] from the activated gates [S][B][4H], cbuf [S+1][B][H],
    dh [S][B][H] and W_hh [4H][H], in the dtype of its arguments."""
    S, B, H = dh.shape
    out = torch.empty_like(gates)
    dhrec = torch.zeros(B, H, dtype=dh.dtype)
    dcn = torch.zeros(B, H, dtype=dh.dtype)
    for t in range(S - 1, -1, -1):
        ig, fg, cg, og = gates[t].split(H, dim=1)
        d = dh[t] + dhrec
        tc = torch.tanh(cbuf[t + 1])
        dc = d * og * (1 - tc * tc) + dcn
        out[t] = torch.cat([dc * cg * (ig * (1 - ig)), dc * cbuf[t] * (fg * (1 - fg)),
                            dc * ig * (1 - cg * cg), d * tc * (og * (1 - og))], dim=1)
        dcn = dc * fg
        dhrec = out[t] @ whh
    return out


def _placed(x, pad, at_end):
    """x flattened inside a NaN-filled allocation with `pad` more floats, at its
    start or at its very end; returns (allocation, view of x's place)."""
    n = x.numel()
    buf = torch.full((n + pad,), NAN, device=DEV)
    view = buf[pad:] if at_end else buf[:n]
    view.copy_(x.reshape(-1))
    return buf, view


CASES = [(S, H, tail) for H in (64, 65, 100, 128) for S in (1, 2, 3, 6, 7) for tail in (1, 3, 0)]


@pytest.mark.parametrize('S,H,tail', CASES, ids=[f'S{s}-H{h}-tail{r}' for s, h, r in CASES])
def test_bptt_r4_steps(S, H, tail):
    B = _batch(tail)
    g = torch.Generator().manual_seed(10000 * S + 10 * H + tail)
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
    xt = x.transpose(0, 1).reshape(S * B, D).contiguous().to(DEV)
    hbuf = torch.full((S + 1, B, H), NAN, device=DEV)
    cbuf = torch.full((S + 1, B, H), NAN, device=DEV)
    gates = torch.full((S, B, 4 * H), NAN, device=DEV)
    xps = torch.empty(S, B, 4 * H, device=DEV)
    h0d, c0d = h0[0].contiguous().to(DEV), c0[0].contiguous().to(DEV)
    L.call('smi_lstm_forward_x', L.ptr(xt), D, D, L.ptr(Wih), L.ptr(bih), L.ptr(Whh), L.ptr(bhh),
           L.ptr(h0d), L.ptr(c0d), S, B, H, L.ptr(hbuf), L.ptr(cbuf), L.ptr(gates), L.ptr(xps), st)
    out, (hn, cn) = lstm(x, (h0, c0))
    l64 = torch.nn.LSTM(D, H, 1, batch_first=True).double()
    l64.load_state_dict({k: v.double() for k, v in lstm.state_dict().items()})
    out64, (hn64, cn64) = l64(x.double(), (h0.double(), c0.double()))
    _fp32_as_good_as_torch(hbuf[1:].transpose(0, 1).cpu(), out.detach(), out64.detach(), 2e-6)
    _fp32_as_good_as_torch(cbuf[S].cpu(), cn[0].detach(), cn64[0].detach(), 2e-6)
    assert bool(torch.isfinite(gates).all()) and bool(torch.isfinite(cbuf).all())
    (out64 * dh.double()).sum().backward()
    (out * dh).sum().backward()

    dht = dh.transpose(0, 1).contiguous()
    gc, cc, whc = gates.cpu(), cbuf.cpu(), Whh.cpu().reshape(4 * H, H)
    ref32 = _cell_backward(gc, cc, dht, whc)
    ref64 = _cell_backward(gc.double(), cc.double(), dht.double(), whc.double())
    hprev = hbuf[:S].reshape(S * B, H)
    results = []
    for at_end in (False, True):
        gbuf, gv = _placed(gates, B * 4 * H, at_end)
        cbuf_p, cv = _placed(cbuf, B * H, at_end)
        dbuf, dv = _placed(dht, B * H, at_end)
        dgates = torch.full((S, B, 4 * H), NAN, device=DEV)
        L.call('smi_lstm_backward', L.ptr(dv), L.ptr(gv), L.ptr(cv), L.ptr(Whh), S, B, H,
               L.ptr(dgates), st)
        assert _last() == f'lstm_bwd_r4_kernel<{_kw(H)}>'
        torch.cuda.synchronize()
        where = 'end' if at_end else 'start'
        assert bool(torch.isfinite(dgates).all()), f'NaN in dgates (inputs at the {where})'
        _fp32_as_good_as_torch(dgates.cpu(), ref32, ref64, 2e-6)
        results.append(dgates)
        del gbuf, cbuf_p, dbuf
    assert torch.equal(results[0], results[1]), 'dgates depend on where the inputs sit'

    dg = results[0].reshape(S * B, 4 * H)
    gWih = torch.empty(4 * H, D, device=DEV)
    gWhh = torch.empty(4 * H, H, device=DEV)
    gb = torch.empty(4 * H, device=DEV)
    gb2 = torch.empty(4 * H, device=DEV)
    L.call('smi_linear_backward_weight', L.ptr(dg), 4 * H, S * B, 4 * H, L.ptr(xt), D, D,
           L.ptr(gWih), D, L.ptr(gb), 0, st)
    L.call('smi_linear_backward_weight', L.ptr(dg), 4 * H, S * B, 4 * H, L.ptr(hprev), H, H,
           L.ptr(gWhh), H, L.ptr(gb2), 0, st)
    for got, p32, p64 in ((gWih, lstm.weight_ih_l0, l64.weight_ih_l0),
                          (gWhh, lstm.weight_hh_l0, l64.weight_hh_l0),
                          (gb, lstm.bias_ih_l0, l64.bias_ih_l0),
                          (gb2, lstm.bias_hh_l0, l64.bias_hh_l0)):
        _fp32_as_good_as_torch(got.cpu(), p32.grad, p64.grad, 4e-6)
