"""Pixel stem parity beyond 3x84x84: frame shapes, 9 channels, both backward forms.

smi_cnn_forward / smi_cnn_backward against torch's Conv2d / Linear in fp32 and
fp64 (tests/cnn_ref.py; the bars of tests/test_gpu_cnn.py: slack 2e-6 forward,
4e-6 gradients, the backward with the ReLU masks of the forward under test).
tests/test_cpu_cnn_ref.py shows on the host that these checks pass a correct
fp32 stem at every frame below and fail one with H and W swapped, a stale image
row, pix_next ignored, an unwritten pixel, a missing / 255 or a `>=` mask.

| C, H, W   | H1 x W1, P1 | H2 x W2, P2 | purpose |
|-----------|-------------|-------------|---------|
| 3, 20, 20 | 4x4, 16     | 1x1, 1      | smallest legal frame; one tile each |
| 3, 24, 20 | 5x4, 20     | 1x1, 1      | odd H1; P1 % 16 != 0 |
| 3, 64, 36 | 15x8, 120   | 6x3, 18     | tall; odd H1; A1 row 14 outside every conv-2 window |
| 3, 36, 52 | 8x12, 96    | 3x5, 15     | wide; P2 < 16 |
| 3, 68,116 | 16x28, 448  | 7x13, 91    | prefetch form at its limit (4 * P1 == KA * 256) |
| 3, 28,324 | 6x80, 480   | 2x39, 78    | C = 3 non-prefetch backward; two-pass forward staging; backward LDS > 64 KB |
| 9, 20, 20 | 4x4, 16     | 1x1, 1      | C = 9 smallest |
| 9, 36, 52 | 8x12, 96    | 3x5, 15     | C = 9 rectangular |
| 9, 40,212 | 9x52, 468   | 3x25, 75    | C = 9 non-prefetch backward; odd H1; 106 KB forward LDS |
| 9, 84, 84 | 20x20, 400  | 9x9, 81     | DDPG's stack, direct |

Each frame runs at 3..9 rows (time-major with pix_next, rows = (T + 1) * B;
rows < B * T ending inside a time step; plain batches), and six of them at
more rows than the forward grid can hold workgroups, so a workgroup processes
several images.  Operands (tests/views.py): feat at ldf = F + 3 behind one
float, dz at lddz = F + 4, tight A1 / A2 / grad with a NaN tail, canaries
checked on every output, and a NaN-filled backward scratch: the kernels write
dA2 and every partial slab before reading them, so a NaN in grad is a read
before a write.  Every case asserts the backward form it was written for
(smi_cnn_backward_prefetch).
"""
import ctypes

import pytest
import torch

from surreal_amd import _lib as L
from tests import cnn_ref as CR
from tests import views as V
from tests.helpers import seq_flat
from tests.test_gpu_cnn import _run_pixel

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')

# (C, H, W), B, T, rows, F, prefetch form
CASES = [
    ((3, 20, 20), 3, 2, 9, 8, True),         # rows = (T + 1) * B: pix_next for every segment
    ((3, 24, 20), 4, 2, 7, 24, True),        # rows < B * T, rows % B != 0, no pix_next
    ((3, 64, 36), 5, 1, 5, 40, True),
    ((3, 36, 52), 2, 3, 8, 24, True),        # rows = (T + 1) * B
    ((3, 68, 116), 2, 2, 5, 16, True),       # one row of the last time step
    ((3, 28, 324), 5, 1, 5, 24, False),
    ((9, 20, 20), 3, 3, 7, 8, True),         # rows < B * T, rows % B != 0
    ((9, 36, 52), 2, 2, 6, 40, True),        # rows = (T + 1) * B
    ((9, 40, 212), 4, 1, 4, 16, False),
    ((9, 84, 84), 2, 1, 4, 24, True),        # rows = (T + 1) * B
]
# more rows than forward workgroups (and, beyond 512, than backward workgroups):
# (C, H, W), prefetch form, least rows.  9x40x212 holds one forward workgroup per
# CU; 515 rows make the backward's 512 workgroups loop in the C = 9 non-prefetch form
MULTI = [((3, 20, 20), True, 0), ((9, 36, 52), True, 0), ((3, 84, 84), True, 0),
         ((9, 84, 84), True, 0), ((3, 28, 324), False, 0), ((9, 40, 212), False, 515)]
MULTI_B, MULTI_F = 7, 16


def _cam_id(cam):
    return 'x'.join(map(str, cam))


def _fwd_grid_bound(cam):
    """no forward grid exceeds this: 8 wave slots per SIMD (a workgroup is one
    wave on each of the 4) and 160 KiB of LDS per CU."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return min(8, 163840 // CR.geom(*cam).fwd_lds) * cus


def _p(t):
    return L.ptr(t) if t is not None else None


class _Run:
    """one forward (and backward) of the stem on view operands."""

    def __init__(self, cam, B, T, rows, F, flat, pix, pixn):
        self.cam, self.B, self.T, self.rows, self.F = cam, B, T, rows, F
        self.g = CR.geom(*cam)
        self.flat = flat.to(DEV)
        self.pix = pix.to(DEV)
        self.pixn = pixn.to(DEV) if rows > B * T else None      # only where it is read
        self.n1, self.n2 = 16 * self.g.P1, 32 * self.g.P2
        self.ldf, self.offf = F + 3, 1
        self.lddz = F + 4

    def forward(self, with_a1=True):
        rows, F = self.rows, self.F
        self.p1, self.b1 = V.make_out(rows, self.n1, self.n1, 0, device=DEV)
        self.p2, self.b2 = V.make_out(rows, self.n2, self.n2, 0, device=DEV)
        self.pf, self.bf = V.make_out(rows, F, self.ldf, self.offf, device=DEV)
        L.call('smi_cnn_forward', L.ptr(self.flat), L.ptr(self.pix), _p(self.pixn), self.B, self.T,
               rows, *self.cam, F, self.p1 if with_a1 else None, self.p2, self.pf, self.ldf,
               L.stream())
        if with_a1:
            a1 = V.check_out(self.b1, rows, self.n1, self.n1, 0)
        else:
            V.assert_untouched(self.b1, 0, self.n1, self.n1, 0)
            a1 = None
        a2 = V.check_out(self.b2, rows, self.n2, self.n2, 0)
        feat = V.check_out(self.bf, rows, F, self.ldf, self.offf)
        return a1, a2, feat

    def backward(self, dz):
        """on the A1 / A2 the last forward left on the device."""
        rows, F = self.rows, self.F
        total = self.flat.numel()
        pz, bz = V.make_in(dz, self.lddz, 0, device=DEV)
        pg, bg = V.make_out(1, total, total, 0, device=DEV)
        nbytes = int(L.lib().smi_cnn_scratch_bytes(rows, *self.cam, F))
        assert nbytes % 4 == 0
        scratch = torch.full((nbytes // 4 + V.TAIL,), NAN, device=DEV)
        L.call('smi_cnn_backward', L.ptr(self.flat), L.ptr(self.pix), _p(self.pixn), self.B, self.T,
               rows, *self.cam, F, self.p1, self.p2, pz, self.lddz, pg, L.ptr(scratch), nbytes,
               L.stream())
        V.assert_untouched(scratch, 1, nbytes // 4, nbytes // 4, 0)
        # the inputs are inputs
        V.assert_untouched(self.b1, rows, self.n1, self.n1, 0)
        V.assert_untouched(self.b2, rows, self.n2, self.n2, 0)
        return V.check_out(bg, 1, total, total, 0).reshape(-1)


def _setup(cam, B, T, rows, F):
    torch.manual_seed(100 * B + rows)
    net, net64 = CR.nets(*cam, F)
    pix, pixn = CR.images(B, T, cam, rows, rows)
    return net, net64, pix, pixn, _Run(cam, B, T, rows, F, seq_flat(net), pix, pixn)


def _report(tag, names, got, ref32, ref64):
    for name, a, r32, r64 in zip(names, got, ref32, ref64):
        a, r32, r64 = (t.double().reshape(-1) for t in (a, r32, r64))
        print(f'{tag} {name}: e_gpu {float((a - r64).abs().max()):.3e} '
              f'e_torch32 {float((r32 - r64).abs().max()):.3e} scale {float(r64.abs().max()):.3e}')


def _parity(cam, B, T, rows, F, prefetch):
    g = CR.geom(*cam)
    assert g.ok
    assert bool(L.lib().smi_cnn_backward_prefetch(*cam)) == prefetch, 'the case tests the other form'
    net, net64, pix, pixn, run = _setup(cam, B, T, rows, F)
    x = CR.timemajor_images(pix, pixn, rows)
    a1, a2, feat = run.forward()
    s32, s64 = CR.stages(net, x), CR.stages(net64, x)
    tag = f'{_cam_id(cam)} rows {rows}'
    _report(tag, CR.FWD_NAMES, (a1, a2, feat), s32, s64)
    bad = CR.failures(CR.FWD_NAMES, (a1, a2, feat), s32, s64, CR.FWD_SLACK)
    assert not bad, bad
    dy = torch.randn(rows, F, generator=torch.Generator().manual_seed(7))
    dz = (dy * (s32[2] > 0)).contiguous()
    grad = run.backward(dz)
    m1, m2 = a1.reshape(s32[0].shape) > 0, a2 > 0
    g32 = CR.masked_grads(net, x, m1, m2, dz)
    g64 = CR.masked_grads(net64, x, m1, m2, dz)
    got = torch.split(grad, [t.numel() for t in g32])
    _report(tag, CR.GRAD_NAMES, got, g32, g64)
    bad = CR.failures(CR.GRAD_NAMES, got, g32, g64, CR.BWD_SLACK)
    assert not bad, bad


@pytest.mark.parametrize('cam,B,T,rows,F,prefetch', CASES,
                         ids=[f'{_cam_id(c[0])}-r{c[3]}' for c in CASES])
def test_stem_geometry(cam, B, T, rows, F, prefetch):
    _parity(cam, B, T, rows, F, prefetch)


@pytest.mark.parametrize('cam,prefetch,least', MULTI, ids=[_cam_id(c[0]) for c in MULTI])
def test_stem_several_images_per_workgroup(cam, prefetch, least):
    """rows = the forward grid's bound + 3 (or `least`), time-major over 7 segments with the
    last rows on pix_next.  rows * P1, the terms of a conv-1 gradient entry,
    stays at or below the 250,000 of tests/test_gpu_cnn.py's 624-row case whose
    gradient bar is used here, except at 3x84x84, where one workgroup per image
    slot of a 256-CU part needs 771 rows (308,400 terms)."""
    bound = _fwd_grid_bound(cam)
    rows = max(bound + 3, least)
    assert rows > bound
    B, T = MULTI_B, (rows - 1) // MULTI_B
    assert B * T < rows <= B * (T + 1)
    if cam != (3, 84, 84):
        assert rows * CR.geom(*cam).P1 <= 250000
    if cam in ((9, 36, 52), (3, 84, 84), (3, 28, 324), (9, 40, 212)):
        assert rows > 512                       # the backward's workgroups loop too
    _parity(cam, B, T, rows, MULTI_F, prefetch)


BITWISE = [((3, 24, 20), 4, 2, 7, 24), ((3, 28, 324), 5, 1, 5, 24), ((9, 36, 52), 2, 2, 6, 40),
           ((9, 84, 84), 7, 37, 260, 16), ((3, 20, 20), 7, 86, 605, 16)]
# (9x84x84: one workgroup per CU, so 260 rows make those of a 256-CU part loop in the forward;
# 3x20x20 at 605 rows: the backward's 512 workgroups loop)


@pytest.mark.parametrize('cam,B,T,rows,F', BITWISE,
                         ids=[f'{_cam_id(c[0])}-r{c[3]}' for c in BITWISE])
def test_stem_reruns_and_null_a1_bit_equal(cam, B, T, rows, F):
    """A2 and feat without A1 (a1 = NULL: acting) are the bits of the run with
    it; forward and backward run twice give the same bits (the slab reducer
    sums the workgroups' partials in a fixed order)."""
    net, _, pix, pixn, run = _setup(cam, B, T, rows, F)
    a1, a2, feat = run.forward()
    _, a2n, featn = run.forward(with_a1=False)
    assert torch.equal(a2n, a2) and torch.equal(featn, feat)
    a1b, a2b, featb = run.forward()
    assert torch.equal(a1b, a1) and torch.equal(a2b, a2) and torch.equal(featb, feat)
    dy = torch.randn(rows, F, generator=torch.Generator().manual_seed(7))
    dz = (dy * (feat > 0)).contiguous()
    g1 = run.backward(dz)
    g2 = run.backward(dz)
    assert torch.equal(g1, g2)
    assert float(g1.abs().max()) > 0


def test_stem_zero_rows():
    cam, F = (3, 24, 20), 8
    g = CR.geom(*cam)
    flat = torch.zeros(int(L.lib().smi_cnn_param_count(*cam, F)), device=DEV)
    pix = torch.zeros((1, 1) + cam, dtype=torch.uint8, device=DEV)
    outs = [V.make_out(2, n, n, 0, device=DEV) for n in (16 * g.P1, 32 * g.P2, F, flat.numel())]
    (p1, b1), (p2, b2), (pf, bf), (pg, bg) = outs
    st = L.stream()
    assert L.lib().smi_cnn_forward(L.ptr(flat), L.ptr(pix), None, 1, 1, 0, *cam, F, p1, p2, pf, F,
                                   st) == 0
    scratch = torch.full((64,), NAN, device=DEV)
    assert L.lib().smi_cnn_backward(L.ptr(flat), L.ptr(pix), None, 1, 1, 0, *cam, F, p1, p2, pf, F,
                                    pg, L.ptr(scratch), 0, st) == 0
    for _, buf in outs:
        V.assert_untouched(buf, 0, 1, 1, 0)
    V.assert_untouched(scratch, 0, 1, 1, 0)


# ---------------------------------------------------------------- rejections
# Host checks: nothing is launched (the operands are zero-filled and large
# enough for the frame all the same).
def _calls(cam, rows=2, B=2, T=1, F=8, pix_off=0, pixn=False, scratch_short=0):
    C, H, W = cam
    n = max(C * H * W, 16)
    flat = torch.zeros(max(int(L.lib().smi_cnn_param_count(C, H, W, F)), 64), device=DEV)
    pix = torch.zeros(B * T * n + 64, dtype=torch.uint8, device=DEV)
    nxt = torch.zeros(B * n + 64, dtype=torch.uint8, device=DEV)
    g = CR.geom(C, max(H, 20), max(W, 20))
    a1 = torch.zeros(rows * 16 * g.P1 + 64, device=DEV)
    a2 = torch.zeros(rows * 32 * g.P2 + 64, device=DEV)
    feat = torch.zeros(rows * F + 64, device=DEV)
    grad = torch.zeros_like(flat)
    nbytes = max(int(L.lib().smi_cnn_scratch_bytes(rows, C, H, W, F)), 0)
    scratch = torch.zeros(nbytes // 4 + 64, device=DEV)
    pp = ctypes.c_void_p(pix.data_ptr() + pix_off)
    pn = L.ptr(nxt) if pixn else None
    st = L.stream()
    keep = (flat, pix, nxt, a1, a2, feat, grad, scratch)
    rf = L.lib().smi_cnn_forward(L.ptr(flat), pp, pn, B, T, rows, C, H, W, F, L.ptr(a1), L.ptr(a2),
                                 L.ptr(feat), F, st)
    ef = L.lib().smi_last_error().decode(errors='replace')
    rb = L.lib().smi_cnn_backward(L.ptr(flat), pp, pn, B, T, rows, C, H, W, F, L.ptr(a1), L.ptr(a2),
                                  L.ptr(feat), F, L.ptr(grad), L.ptr(scratch),
                                  nbytes - scratch_short, st)
    eb = L.lib().smi_last_error().decode(errors='replace')
    torch.cuda.synchronize()
    del keep
    return rf, ef, rb, eb


@pytest.mark.parametrize('cam,why', [
    ((4, 84, 84), 'channels'),
    ((3, 16, 16), 'smaller than'),
    ((3, 32, 22), 'W % 4'),                  # only W % 4 fails (W1 = 4, 2112 bytes)
    ((3, 84, 88), 'W % 4'),                  # odd W1 (21)
    ((3, 84, 100), '96 pixels'),             # P2 = 99
    ((3, 21, 20), 'W % 4'),                  # only C*H*W % 16 fails (1260 bytes)
], ids=lambda v: _cam_id(v) if isinstance(v, tuple) else None)
def test_stem_rejects_unsupported_frames(cam, why):
    assert not CR.geom(*cam).ok
    rf, ef, rb, eb = _calls(cam)
    assert rf == -1 and rb == -1, (rf, rb)       # SMI_E_ARG
    assert why in ef and why in eb, (ef, eb)


def test_stem_rejects_bad_pointers():
    cam = (3, 24, 20)
    assert _calls(cam)[::2] == (0, 0)                        # the operands are otherwise fine
    rf, ef, rb, eb = _calls(cam, pix_off=4)                  # both entry points
    assert rf == -1 and rb == -1, (rf, rb)
    assert '16-byte aligned' in ef and '16-byte aligned' in eb, (ef, eb)
    rf, ef, rb, eb = _calls(cam, rows=3, B=2, T=1)           # rows > B * T without pix_next
    assert rf == -1 and rb == -1 and 'pix_next' in ef and 'pix_next' in eb, (rf, ef, rb, eb)
    assert _calls(cam, rows=3, B=2, T=1, pixn=True)[::2] == (0, 0)
    rf, ef, rb, eb = _calls(cam, scratch_short=1)
    assert rf == 0 and rb == -1 and 'scratch' in eb, (rf, rb, eb)


def test_geom_accepts_what_the_library_accepts():
    """cnn_ref.geom() against the library over every frame of a sweep (rows = 0:
    the frame is checked before the row count, nothing is launched): cnn_check's
    conditions, and the LDS of a CU for frames that pass them, which the backward
    (staging dA2 as well) reaches first."""
    z = torch.zeros(64, device=DEV)
    zb = torch.zeros(64, dtype=torch.uint8, device=DEV)
    st = L.stream()

    def accepted(C, H, W):
        rf = L.lib().smi_cnn_forward(L.ptr(z), L.ptr(zb), None, 1, 1, 0, C, H, W, 8, None, L.ptr(z),
                                     L.ptr(z), 8, st)
        rb = L.lib().smi_cnn_backward(L.ptr(z), L.ptr(zb), None, 1, 1, 0, C, H, W, 8, L.ptr(z),
                                      L.ptr(z), L.ptr(z), 8, L.ptr(z), L.ptr(z), 1 << 40, st)
        assert rf in (0, -1) and rb in (0, -1), (C, H, W, rf, rb)
        return rf == 0, rb == 0

    def expected(C, H, W):
        g = CR.geom(C, H, W)
        return g.ok and g.fwd_lds <= CR.CU_LDS, g.ok and g.bwd_lds <= CR.CU_LDS

    n_ok = 0
    for C in (1, 3, 4, 9):
        for H in list(range(8, 46)) + [64, 68, 84, 100, 116]:
            for W in range(8, 130) if H < 64 else range(8, 130, 4):
                got = accepted(C, H, W)
                assert got == expected(C, H, W), (C, H, W, got)
                n_ok += got[0]
    assert n_ok > 100
    for cam in CR.TABLE + [(3, 84, 84), (3, 20, 780), (9, 28, 396)]:
        assert accepted(*cam) == (True, True) == expected(*cam), cam
    # wide 9-channel frames that pass cnn_check: 162,736 B forward / 177,240 B
    # backward, and 190,064 B forward
    assert CR.geom(9, 20, 668).ok and CR.geom(9, 20, 780).ok
    assert accepted(9, 20, 668) == (True, False) == expected(9, 20, 668)
    assert accepted(9, 20, 780) == (False, False) == expected(9, 20, 780)
    assert 'LDS' in L.lib().smi_last_error().decode(errors='replace')


# ------------------------------------------------------------------ learner
def test_pixel_mlp_learn_off_the_square():
    """the non-RNN pixel learner on a 3x36x52 camera against the oracle, one
    policy and one value update (the bars of test_pixel_mlp_learn_matches_oracle):
    the learner's scratch carve (conv partials, dA2, A1) and the features written
    into the head input's column block at a frame other than 84x84."""
    rep = _run_pixel('adapt', B=24, T=6, H=6, D=7, A=3, Hd=0, hidden=(32, 24), F=32, iters=1,
                     epochs=(1, 1), rnn=False, cam=(3, 36, 52))
    print('pixel mlp parity, 3x36x52:', rep)
