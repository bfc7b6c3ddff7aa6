"""The pixel stem of free shape: smi_stem_* against torch (tests/stem_ref.py).

smi_stem_forward / smi_stem_backward against torch's Conv2d / Linear in fp32
and fp64 under the failure rule of tests/cnn_ref.py (the GPU error against fp64
is bounded by torch-fp32's own error plus slack; CR.FWD_SLACK 2e-6 forward,
CR.BWD_SLACK 4e-6 gradients; the backward with the ReLU masks of the forward
under test).  tests/test_cpu_stem_ref.py shows on the host that these checks
pass a correct fp32 stem at every case below and fail one with H and W swapped,
pix_next ignored, a stale row of the row map, a missing / 255, a `>=` mask, a
layer's stride off by one or two layers' biases swapped.

| spec (cout@k,s) -> F            | C,H,W    | rows (B,T) | purpose |
|---------------------------------|----------|------------|---------|
| default -> 8                    | 4,20,20  | 9 (3,2)    | channel count the fused stem refuses; pix_next for every segment |
| default -> 24                   | 3,32,22  | 7 (4,2)    | W % 4 != 0; row count ends inside a time step |
| default -> 16                   | 3,84,100 | 3 (3,1)    | conv-2 output of 99 pixels |
| default -> 8                    | 1,21,23  | 5 (5,1)    | one channel, odd frame, uncovered trailing columns, pixel pointer offset by 1 byte |
| 8@3,1 -> 5                      | 2,9,11   | 6 (2,2)    | one layer; no input gradient anywhere |
| 8@5,2 . 12@3,1 . 20@2,2 -> 16   | 3,30,26  | 8 (2,3)    | three layers; two masked input gradients |
| 72@4,3 -> 8                     | 5,19,16  | 4 (4,1)    | two 64-row weight tiles; stride not dividing k |
| 4@2,1 x4 -> 8                   | 3,12,12  | 3 (3,1)    | the layer limit |
| default -> 24                   | 3,36,52  | 8 (2,3)    | fused dispatch: smi_stem_fused == 1; bit-equal to smi_cnn_* |

Operands (tests/views.py): feat at ldf = F + 3 behind one float, dz at lddz =
F + 4, a tight activation buffer and gradient image with a NaN tail, canaries
checked on every output, and a NaN-filled scratch: the kernels write every
gradient image and partial slab before reading it, so a NaN in grad is a read
before a write.
"""
import ctypes

import pytest
import torch

from surreal_amd import _lib as L
from tests import cnn_ref as CR
from tests import stem_ref as SR
from tests import views as V
from tests.helpers import seq_flat

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
IDS = [c.id for c in SR.CASES]


def _p(t):
    return L.ptr(t) if t is not None else None


class _Run:
    """one forward (and backward) of the stem on view operands."""

    def __init__(self, case, flat, pix, pixn):
        self.c = case
        self.n = len(case.spec[0])
        self.shapes = SR.layer_shapes(case.spec, case.cam)
        self.acts = [sh[3] * sh[6] * sh[7] for sh in self.shapes]
        self.spec = L.stem_spec(*case.spec) + tuple(case.cam) + (case.F,)
        self.flat = flat.to(DEV)
        assert int(L.lib().smi_stem_param_count(*self.spec)) == self.flat.numel()
        # the pixels behind pix_off bytes: element alignment only
        raw = torch.zeros(pix.numel() + case.pix_off + 64, dtype=torch.uint8, device=DEV)
        raw[case.pix_off:case.pix_off + pix.numel()] = pix.reshape(-1).to(DEV)
        self.raw = raw
        self.pix = ctypes.c_void_p(raw.data_ptr() + case.pix_off)
        self.pixn = pixn.to(DEV) if case.rows > case.B * case.T else None   # only where it is read
        self.ldf, self.offf, self.lddz = case.F + 3, 1, case.F + 4
        self.nact = case.rows * sum(self.acts)
        assert int(L.lib().smi_stem_act_floats(case.rows, *self.spec)) == self.nact
        self.nbytes = int(L.lib().smi_stem_scratch_bytes(case.rows, *self.spec))
        assert self.nbytes > 0 and self.nbytes % 4 == 0
        self.skip = None

    def _scratch(self):
        return torch.full((self.nbytes // 4 + V.TAIL,), NAN, device=DEV)

    def forward(self, with_act=True):
        """[A_1 .. A_n] (None without the activation buffer) and feat."""
        c = self.c
        self.pa, self.ba = V.make_out(1, self.nact, self.nact, 0, device=DEV)
        self.pf, self.bf = V.make_out(c.rows, c.F, self.ldf, self.offf, device=DEV)
        self.scr = self._scratch()
        rc = L.lib().smi_stem_forward(L.ptr(self.flat), self.pix, _p(self.pixn), c.B, c.T, c.rows,
                                      *self.spec, self.pa if with_act else None, L.ptr(self.scr),
                                      self.nbytes, self.pf, self.ldf, _p(self.skip), L.stream())
        assert rc == 0, L.lib().smi_last_error()
        V.assert_untouched(self.scr, 1, self.nbytes // 4, self.nbytes // 4, 0)
        if self.skip is not None:
            return None, None
        if with_act:
            a = V.check_out(self.ba, 1, self.nact, self.nact, 0).reshape(-1)
            acts = [t.reshape(c.rows, -1) for t in torch.split(a, [c.rows * n for n in self.acts])]
        else:
            V.assert_untouched(self.ba, 0, 1, 1, 0)
            acts = None
        return acts, V.check_out(self.bf, c.rows, c.F, self.ldf, self.offf)

    def backward(self, dz):
        """on the activations the last forward left on the device."""
        c = self.c
        total = self.flat.numel()
        pz, self.bz = V.make_in(dz, self.lddz, 0, device=DEV)
        self.pg, self.bg = V.make_out(1, total, total, 0, device=DEV)
        self.scr = self._scratch()
        rc = L.lib().smi_stem_backward(L.ptr(self.flat), self.pix, _p(self.pixn), c.B, c.T, c.rows,
                                       *self.spec, self.pa, pz, self.lddz, self.pg,
                                       L.ptr(self.scr), self.nbytes, _p(self.skip), L.stream())
        assert rc == 0, L.lib().smi_last_error()
        V.assert_untouched(self.scr, 1, self.nbytes // 4, self.nbytes // 4, 0)
        V.assert_untouched(self.ba, 1, self.nact, self.nact, 0)         # the inputs are inputs
        if self.skip is not None:
            return None
        return V.check_out(self.bg, 1, total, total, 0).reshape(-1)


def _setup(case):
    torch.manual_seed(100 * case.B + case.rows)
    net, net64 = SR.nets(case.spec, case.cam, case.F)
    pix, pixn = SR.images(case.B, case.T, case.cam, case.rows, case.rows)
    return net, net64, pix, pixn, _Run(case, seq_flat(net), pix, pixn)


def _report(tag, names, got, ref32, ref64):
    for name, a, r32, r64 in zip(names, got, ref32, ref64):
        a, r32, r64 = (t.double().reshape(-1) for t in (a, r32, r64))
        print(f'{tag} {name}: e_gpu {float((a - r64).abs().max()):.3e} '
              f'e_torch32 {float((r32 - r64).abs().max()):.3e} scale {float(r64.abs().max()):.3e}')


@pytest.mark.parametrize('case', SR.CASES, ids=IDS)
def test_stem_parity(case):
    """forward and backward of every case under the failure rule at the slacks
    of the fused stem's parity tests (CR.FWD_SLACK, CR.BWD_SLACK)."""
    n = len(case.spec[0])
    net, net64, pix, pixn, run = _setup(case)
    assert int(L.lib().smi_stem_fused(*run.spec)) == int(case.fused), 'the case tests the other form'
    x = SR.timemajor_images(pix, pixn, case.rows)
    acts, feat = run.forward()
    s32, s64 = SR.stages(net, x, n), SR.stages(net64, x, n)
    _report(case.id, SR.fwd_names(n), acts + [feat], s32, s64)
    bad = SR.failures(SR.fwd_names(n), acts + [feat], s32, s64, CR.FWD_SLACK)
    assert not bad, bad
    dy = torch.randn(case.rows, case.F, generator=torch.Generator().manual_seed(7))
    dz = (dy * (s32[n] > 0)).contiguous()
    grad = run.backward(dz)
    masks = [a.reshape(r.shape) > 0 for a, r in zip(acts, s32)]
    g32 = SR.masked_grads(net, x, masks, dz, n)
    g64 = SR.masked_grads(net64, x, masks, dz, n)
    got = torch.split(grad, [t.numel() for t in g32])
    _report(case.id, SR.grad_names(n), got, g32, g64)
    bad = SR.failures(SR.grad_names(n), got, g32, g64, CR.BWD_SLACK)
    assert not bad, bad


def test_fused_dispatch_is_bit_equal_to_smi_cnn():
    """where the fused stem runs, smi_stem_* gives the activations, feat and
    gradient of smi_cnn_* bit for bit."""
    case = SR.CASES[-1]
    assert case.fused
    _, _, pix, pixn, run = _setup(case)
    assert int(L.lib().smi_stem_fused(*run.spec)) == 1
    acts, feat = run.forward()
    dy = torch.randn(case.rows, case.F, generator=torch.Generator().manual_seed(7))
    dz = (dy * (feat > 0)).contiguous()
    grad = run.backward(dz)
    rows, F, cam = case.rows, case.F, case.cam
    a1 = torch.full((rows, run.acts[0]), NAN, device=DEV)
    a2 = torch.full((rows, run.acts[1]), NAN, device=DEV)
    ft = torch.full((rows, F), NAN, device=DEV)
    pixd, pixnd = pix.to(DEV), pixn.to(DEV)
    L.call('smi_cnn_forward', L.ptr(run.flat), L.ptr(pixd), L.ptr(pixnd), case.B, case.T, rows, *cam,
           F, L.ptr(a1), L.ptr(a2), L.ptr(ft), F, L.stream())
    nb = int(L.lib().smi_cnn_scratch_bytes(rows, *cam, F))
    scratch = torch.full((nb // 4,), NAN, device=DEV)
    g = torch.full((run.flat.numel(),), NAN, device=DEV)
    dzd = dz.to(DEV)
    L.call('smi_cnn_backward', L.ptr(run.flat), L.ptr(pixd), L.ptr(pixnd), case.B, case.T, rows, *cam,
           F, L.ptr(a1), L.ptr(a2), L.ptr(dzd), F, L.ptr(g), L.ptr(scratch), nb, L.stream())
    assert torch.equal(acts[0], a1.cpu()) and torch.equal(acts[1], a2.cpu())
    assert torch.equal(feat, ft.cpu())
    assert torch.equal(grad, g.cpu())
    assert float(grad.abs().max()) > 0


@pytest.mark.parametrize('case', SR.CASES, ids=IDS)
def test_reruns_and_null_act_bit_equal(case):
    """feat without an activation buffer (acting: the intermediates in scratch)
    is the bits of the run with it; forward and backward run twice give the
    same bits (fixed-order sums of the partials, no float atomics)."""
    _, _, _, _, run = _setup(case)
    acts, feat = run.forward()
    _, featn = run.forward(with_act=False)
    assert torch.equal(featn, feat)
    acts2, feat2 = run.forward()
    assert all(torch.equal(a, b) for a, b in zip(acts, acts2)) and torch.equal(feat2, feat)
    dy = torch.randn(case.rows, case.F, generator=torch.Generator().manual_seed(7))
    dz = (dy * (feat > 0)).contiguous()
    g1 = run.backward(dz)
    g2 = run.backward(dz)
    assert torch.equal(g1, g2)
    assert float(g1.abs().max()) > 0


@pytest.mark.parametrize('case', [SR.CASES[5], SR.CASES[8]], ids=[IDS[5], IDS[8]])
def test_set_skip_flag_writes_nothing(case):
    """with the device stop flag set, neither form writes an activation, a
    feature, a gradient or a float of scratch; with it clear the call runs."""
    _, _, _, _, run = _setup(case)
    acts, feat = run.forward()                      # the activations a backward would read
    pa, ba = run.pa, run.ba
    dz = torch.ones(case.rows, case.F)
    run.skip = torch.ones(1, dtype=torch.int32, device=DEV)
    run.forward()
    V.assert_untouched(run.ba, 0, 1, 1, 0)
    V.assert_untouched(run.bf, 0, 1, 1, 0)
    V.assert_untouched(run.scr, 0, 1, 1, 0)
    run.forward(with_act=False)
    V.assert_untouched(run.bf, 0, 1, 1, 0)
    V.assert_untouched(run.scr, 0, 1, 1, 0)
    run.pa, run.ba = pa, ba
    run.backward(dz)
    V.assert_untouched(run.bg, 0, 1, 1, 0)
    V.assert_untouched(run.scr, 0, 1, 1, 0)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)      # a clear flag: the call runs
    c = case
    pf, bf = V.make_out(c.rows, c.F, run.ldf, run.offf, device=DEV)
    scr = run._scratch()
    L.call('smi_stem_forward', L.ptr(run.flat), run.pix, _p(run.pixn), c.B, c.T, c.rows, *run.spec,
           None, L.ptr(scr), run.nbytes, pf, run.ldf, L.ptr(flag), L.stream())
    assert torch.equal(V.check_out(bf, c.rows, c.F, run.ldf, run.offf), feat)


# ---------------------------------------------------------------- rejections
# Host checks: nothing is launched, and every output keeps its NaN fill.
def _call(case_spec, cam, which, F=8, rows=2, B=2, T=1, pixn=False, null=None, scratch_bytes=None,
          act=True):
    """one smi_stem_forward ('fwd') or smi_stem_backward ('bwd') on zero inputs
    and NaN-filled outputs: (return code, smi_last_error(), outputs)."""
    spec = L.stem_spec(*case_spec) + tuple(cam) + (F,)
    n = max(cam[0] * cam[1] * cam[2], 16)
    flat = torch.zeros(1 << 16, device=DEV)
    pix = torch.zeros(B * T * n + 64, dtype=torch.uint8, device=DEV)
    nxt = torch.zeros(B * n + 64, dtype=torch.uint8, device=DEV)
    outs = {k: torch.full((1 << 16,), NAN, device=DEV) for k in ('act', 'feat', 'grad', 'scratch')}
    if which == 'bwd':
        outs['act'].zero_()                                         # an input there
    dz = torch.zeros(rows * F + 64, device=DEV)
    nbytes = max(int(L.lib().smi_stem_scratch_bytes(rows, *spec)), 0)
    assert nbytes <= 4 * (1 << 16)
    if scratch_bytes is not None:
        nbytes = scratch_bytes
    pn = L.ptr(nxt) if pixn else None
    ptr = {k: L.ptr(v) for k, v in outs.items()}
    ptr.update(flat=L.ptr(flat), pix=L.ptr(pix), dz=L.ptr(dz))
    if null:
        ptr[null] = None
    st = L.stream()
    if which == 'fwd':
        rc = L.lib().smi_stem_forward(ptr['flat'], ptr['pix'], pn, B, T, rows, *spec,
                                      ptr['act'] if act else None, ptr['scratch'], nbytes,
                                      ptr['feat'], F, None, st)
    else:
        rc = L.lib().smi_stem_backward(ptr['flat'], ptr['pix'], pn, B, T, rows, *spec, ptr['act'],
                                       ptr['dz'], F, ptr['grad'], ptr['scratch'], nbytes, None, st)
        del outs['act']
    err = L.lib().smi_last_error().decode(errors='replace')
    torch.cuda.synchronize()
    return rc, err, outs


def _untouched(outs):
    for buf in outs.values():
        V.assert_untouched(buf, 0, 1, 1, 0)


def _rejected(spec, cam, why, **kw):
    for which in ('fwd', 'bwd'):
        rc, err, outs = _call(spec, cam, which, **kw)
        assert rc == -1, (which, rc)                                # SMI_E_ARG
        assert why in err, (which, err)
        _untouched(outs)


@pytest.mark.parametrize('spec,cam,why', [
    (((16, 32), (8, 9), (4, 2)), (3, 84, 84), 'layer 2'),          # k > 8
    (((16, 32), (8, 4), (5, 2)), (3, 84, 84), 'layer 1'),          # stride > 4
    (((16, 129), (8, 4), (4, 2)), (3, 84, 84), 'layer 2'),         # channels > 128
    (((16, 32), (8, 2), (4, 3)), (3, 84, 84), 'layer 2'),          # stride > k
    (SR.DEFAULT, (3, 16, 16), 'layer 2'),                          # a frame smaller than a layer
    (SR.DEFAULT, (3, 7, 84), 'layer 1'),
    (((4,) * 5, (2,) * 5, (1,) * 5), (3, 12, 12), '1 to 4'),
    (((), (), ()), (3, 12, 12), '1 to 4'),
], ids=lambda v: None)
def test_rejects_specs_and_frames(spec, cam, why):
    _rejected(spec, cam, why)
    s = L.stem_spec(*spec) + tuple(cam) + (8,)
    assert L.lib().smi_stem_param_count(*s) == -1 and L.lib().smi_stem_act_floats(2, *s) == -1
    assert L.lib().smi_stem_scratch_bytes(2, *s) == -1 and L.lib().smi_stem_fused(*s) == -1


def test_rejects_bad_pointers_rows_and_scratch():
    spec, cam = ((8,), (3,), (1,)), (2, 9, 11)
    assert _call(spec, cam, 'fwd')[0] == 0 and _call(spec, cam, 'bwd')[0] == 0   # otherwise fine
    for which, nulls in (('fwd', ('flat', 'pix', 'feat')), ('bwd', ('flat', 'pix', 'act', 'dz', 'grad'))):
        for null in nulls:
            rc, err, outs = _call(spec, cam, which, null=null)
            assert rc == -1 and 'null pointer' in err, (which, null, rc, err)
            _untouched(outs)
    _rejected(spec, cam, 'pix_next', rows=3, B=2, T=1)               # rows > B * T without pix_next
    assert _call(spec, cam, 'fwd', rows=3, B=2, T=1, pixn=True)[0] == 0
    assert _call(spec, cam, 'bwd', rows=3, B=2, T=1, pixn=True)[0] == 0
    s = L.stem_spec(*spec) + cam + (8,)
    need_b = int(L.lib().smi_stem_scratch_bytes(2, *s))
    need_f = 4 * int(L.lib().smi_stem_act_floats(2, *s))             # the general forward's intermediates
    rc, err, outs = _call(spec, cam, 'fwd', act=False, scratch_bytes=need_f - 4)
    assert rc == -1 and 'scratch' in err, (rc, err)
    _untouched(outs)
    assert _call(spec, cam, 'fwd', act=False, scratch_bytes=need_f)[0] == 0
    assert _call(spec, cam, 'fwd', scratch_bytes=0)[0] == 0          # with its activation buffer: none needed
    rc, err, outs = _call(spec, cam, 'bwd', scratch_bytes=need_b - 4)
    assert rc == -1 and 'scratch' in err, (rc, err)
    _untouched(outs)
    rc, err, outs = _call(spec, cam, 'fwd', act=False, null='scratch')
    assert rc == -1 and 'scratch' in err, (rc, err)


def test_zero_rows_is_ok_without_a_launch():
    for which in ('fwd', 'bwd'):
        rc, _, outs = _call(SR.DEFAULT, (4, 20, 20), which, rows=0)
        assert rc == 0
        _untouched(outs)
