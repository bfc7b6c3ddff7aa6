"""The bf16 form of the general convolution layer (surreal_amd/csrc/
conv_bf16_kernels.hip, smi_conv2d_*_bf16) and model.conv_dtype = 'bf16'.

Layer parity is qconv_ref.check_layer with its fp32 bars on operands that are
exact in bf16: the kernel then computes the sums torch fp32 computes.  The
rounding itself is checked bit for bit against operands rounded on the host.

The learner is held to a reference that rounds where the kernels round
(_RoundingRef, fp64).  Its bar is d / 4, d the largest scaled deviation between
that reference and the plain fp64 one: a boundary flip moves one term by one
bf16 ulp, a missing or misplaced rounding lands at ~d.  At pix_small d is
4.5e-3 (both references are computed here, on the CPU); the same reference in
fp32 on the CPU lies 9.7e-7 from it, the learner on one MI355X 4.6e-5."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from surreal_amd import _lib as L
from surreal_amd.dqn import FFQfunc
from tests import qconv_ref as Q
from tests import views as V
from tests.test_gpu_conv2d import DEV, E_ARG, NAN, _cases, _in
from tests.test_gpu_dqn_pixel import _bits_equal, _dev, _learner

pytestmark = pytest.mark.gpu


def _bf16(t):
    return t.float().bfloat16().to(t.dtype)


class Bf16Layer(object):
    """the impl interface of qconv_ref.check_layer over the bf16 C ABI, on
    NaN-canaried views at float offset `off` (test_gpu_conv2d.GpuLayer's)"""

    def __init__(self, off):
        self.off = off

    def forward(self, c, div255, act=1):
        cin, H, W, cout, k, s, p = c.geom
        (px, _x), (pw, _w), (pb, _b) = (_in(t, self.off) for t in (c.x, c.w, c.b))
        ny = c.n * cout * c.ho * c.wo
        py, by = V.make_out(1, ny, ny, self.off, device=DEV)
        L.call('smi_conv2d_forward_bf16', px, int(c.u8), int(div255), c.n, cin, H, W, pw, pb, cout, k,
               s, p, act, py, L.stream())
        return V.check_out(by, 1, ny, ny, self.off).reshape(c.n, cout, c.ho, c.wo)

    def backward_input(self, c, dz):
        cin, H, W, cout, k, s, p = c.geom
        (pdy, _d), (pw, _w), (pm, _m) = (_in(t, self.off) for t in (dz, c.w, c.mask))
        nx = c.n * cin * H * W
        pdx, bdx = V.make_out(1, nx, nx, self.off, device=DEV)
        L.call('smi_conv2d_backward_input_bf16', pdy, c.n, cin, H, W, pw, cout, k, s, p, pm, pdx,
               L.stream())
        return V.check_out(bdx, 1, nx, nx, self.off).reshape(c.n, cin, H, W)

    def backward_weight(self, c, dz, div255, raw=False):
        cin, H, W, cout, k, s, p = c.geom
        (pdy, _d), (px, _x) = (_in(t, self.off) for t in (dz, c.x))
        nw = cout * cin * k * k
        # one gradient image [dw | 3 floats that must survive | db], NaN scratch
        pg, bg = V.make_out(1, nw + 3 + cout, nw + 3 + cout, self.off, device=DEV)
        nbytes = int(L.lib().smi_conv2d_scratch_bytes_bf16(c.n, *c.geom))
        scratch = torch.full((nbytes // 4 + 8,), NAN, device=DEV)
        L.call('smi_conv2d_backward_weight_bf16', pdy, px, int(c.u8), int(div255), c.n, cin, H, W,
               cout, k, s, p, pg, ctypes.c_void_p(pg.value + 4 * (nw + 3)), L.ptr(scratch), nbytes,
               L.stream())
        V.assert_untouched(bg, 1, nw + 3 + cout, nw + 3 + cout, self.off)
        img = V.read_out(bg, 1, nw + 3 + cout, nw + 3 + cout, self.off).reshape(-1)
        assert bool(torch.isnan(img[nw:nw + 3]).all()), 'floats between dw and db were written'
        return img if raw else (img[:nw].reshape(cout, cin, k, k), img[nw + 3:])


def _rounded(c):
    c.w, c.dy = _bf16(c.w), _bf16(c.dy)
    if not c.u8:
        c.x = _bf16(c.x)
    return c


@pytest.mark.parametrize('name,n,div255', list(_cases()))
def test_layer_against_torch_on_bf16_exact_operands(name, n, div255):
    Q.check_layer(Bf16Layer(off=0 if n == 1 else 1), _rounded(Q.LayerCase(name, n)), div255)


@pytest.mark.parametrize('name,n', [('parity_3x10x13', 5), ('u8_4x20x20', 1)])
def test_staging_rounds_to_nearest_even(name, n):
    """unrounded operands give the bits of the same operands rounded on the
    host; ties both ways, -0.0 and a value just under the largest finite bf16
    are planted in w and dy (db, the sum of dy as given, is exempt)"""
    c = Q.LayerCase(name, n)
    big = float(torch.tensor(0x7f7effff, dtype=torch.int32).view(torch.float32))
    plant = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -1 - 2.0 ** -8, -0.0, big])
    c.w.view(-1)[:5], c.dy.view(-1)[:5] = plant, plant
    assert not torch.equal(_bf16(c.w), c.w) and float(_bf16(c.w).view(-1)[0]) == 1.0 \
        and float(_bf16(c.w).view(-1)[1]) == 1 + 2.0 ** -6
    r = _rounded(Q.LayerCase(name, n))
    r.w, r.dy = _bf16(c.w), _bf16(c.dy)
    impl, div = Bf16Layer(1), c.u8
    bits = lambda t: t.contiguous().view(torch.int32)                      # noqa: E731
    assert torch.equal(bits(impl.forward(c, div, act=0)), bits(impl.forward(r, div, act=0)))
    if not c.u8:
        assert torch.equal(bits(impl.backward_input(c, c.dy)), bits(impl.backward_input(r, r.dy)))
    assert torch.equal(bits(impl.backward_weight(c, c.dy, div)[0]),
                       bits(impl.backward_weight(r, r.dy, div)[0]))


def test_weight_gradient_twice_is_bit_identical():
    c = Q.LayerCase('tiles_64x12x12', 5)
    dz = c.dy * (c.dy > 0.3)
    a = Bf16Layer(1).backward_weight(c, dz, False, raw=True)
    b = Bf16Layer(1).backward_weight(c, dz, False, raw=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('entry', ['forward', 'backward_input', 'backward_weight'])
def test_argument_errors_leave_the_outputs_untouched(entry):
    lib, P, st = L.lib(), L.ptr, L.stream()
    c = Q.LayerCase('halo_2x5x7', 2)
    x, w, b, dy = c.x.to(DEV), c.w.to(DEV), c.b.to(DEV), c.dy.to(DEV)
    outs = {'forward': [torch.full_like(dy, NAN)], 'backward_input': [torch.full_like(x, NAN)],
            'backward_weight': [torch.full_like(w, NAN), torch.full_like(b, NAN)]}[entry]
    nbytes = int(lib.smi_conv2d_scratch_bytes_bf16(2, *c.geom))
    scratch = torch.full((nbytes // 4 + 8,), NAN, device=DEV)

    def call(n=2, cin=c.geom[0], cout=c.geom[3], k=c.geom[4], s=c.geom[5], p=c.geom[6], act=1,
             nbytes=nbytes):
        H, W = c.geom[1:3]
        if entry == 'forward':
            return lib.smi_conv2d_forward_bf16(P(x), 0, 0, n, cin, H, W, P(w), P(b), cout, k, s, p, act,
                                               P(outs[0]), st)
        if entry == 'backward_input':
            return lib.smi_conv2d_backward_input_bf16(P(dy), n, cin, H, W, P(w), cout, k, s, p, None,
                                                      P(outs[0]), st)
        return lib.smi_conv2d_backward_weight_bf16(P(dy), P(x), 0, 0, n, cin, H, W, cout, k, s, p,
                                                   P(outs[0]), P(outs[1]), P(scratch), nbytes, st)
    bad = [dict(k=9), dict(k=0), dict(s=0), dict(s=4), dict(p=3), dict(p=-1), dict(cin=129),
           dict(cin=0), dict(cout=129), dict(cout=0), dict(n=-1)]
    bad.append({'forward': dict(act=2), 'backward_input': dict(k=8, s=5, p=3),
                'backward_weight': dict(nbytes=nbytes - 4)}[entry])
    for kw in bad:
        assert call(**kw) == E_ARG, kw
        assert lib.smi_last_error()
    assert lib.smi_conv2d_scratch_bytes_bf16(2, 2, 5, 7, 3, 9, 1, 1) == -1
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs + [scratch])
    assert call() == 0                                   # and the same operands do run
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in outs)


# ------------------------------------------------------------ model and learner
def _ste(x):
    return x + (_bf16(x) - x).detach()


class _RoundingQ(Q.QConvRef):
    """QConvRef that rounds what the kernels round: each conv layer's weight and
    (unless it is the exact uint8 frame) input, straight through, and the
    gradient arriving at each conv output (not the one db sums)"""

    def features(self, x):
        if self.is_uint8:
            x = x / 255.0
        for i, conv in enumerate(self.conv_layers):
            z = F.conv2d(x if i == 0 and self.is_uint8 else _ste(x), _ste(conv.weight), None,
                         conv.stride, conv.padding)
            if z.requires_grad:
                z.register_hook(_bf16)
            x = torch.relu(z + conv.bias.view(1, -1, 1, 1))
        return x.flatten(1)


class _RoundingRef(Q.PixLearnerRef):
    def __init__(self, *a):
        Q.PixLearnerRef.__init__(self, *a)
        self.q_func.__class__ = self.q_target.__class__ = _RoundingQ


def _ref_step(cls, lc, shape, A, init, b):
    ref = cls(lc, shape, A, torch.float64)
    ref.load(init)
    td = ref.optimize(b['obs'], b['actions'], b['rewards'], b['obs_next'], b['dones'],
                      b.get('weights'))[1]
    return dict(ref.q_func.state_dict(), td_error=td)


def _deviation(got, ref):
    """largest max|got - ref| / max|ref| over the parameters and td_error"""
    return max(float((torch.as_tensor(got[k]).double().cpu() - ref[k]).abs().max() / ref[k].abs().max())
               for k in ref)


def test_learn_forward_and_graph_replay_with_bf16_convs():
    lc, shape, A, init, batches = Q.pix_case('pix_small')
    lc.model.conv_dtype = 'bf16'
    b = batches[0]
    rounding = _ref_step(_RoundingRef, lc, shape, A, init, b)
    d = _deviation(_ref_step(Q.PixLearnerRef, lc, shape, A, init, b), rounding)
    eager, graph = _learner(lc, shape, A, init), _learner(lc, shape, A, init, use_graph=True)
    assert eager.q_func.conv_dtype == eager.q_target.conv_dtype == 'bf16'
    before, dev = eager.q_func.clone(), _dev(b)
    eager.learn(dev)
    got = _deviation(dict(eager.q_func.state_dict(), td_error=eager.td_error), rounding)
    print(f'd = {d:.3e}, learner within {got:.3e} of the rounding reference (bar d / 4)')
    assert 0 < got <= d / 4
    # FFQfunc.forward's launches are the learner's online forward
    adv, val = before.logits(dev['obs'])
    assert isinstance(before, FFQfunc) and before.conv_dtype == 'bf16'
    assert torch.equal(adv, eager._bufs['q_out_0']) and torch.equal(val, eager._bufs['q_out_1'])
    # replayed steps against eager ones
    graph.learn(dev)
    for bb in batches[1:]:
        assert _bits_equal(eager, graph)
        eager.learn(_dev(bb))
        graph.learn(_dev(bb))
    torch.cuda.synchronize()
    assert _bits_equal(eager, graph) and graph._graph is not None
