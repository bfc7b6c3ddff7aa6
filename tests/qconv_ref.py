"""Test-side restatement of FFQfunc WITH conv_layers (surreal/model/q_net.py:
68-119) in torch on the CPU, the learner reference over it, and the checkers
the GPU tests of the general convolution layer and of the pixel DQN learner
use (test infrastructure only).

  conv layer     LayerCase / check_layer: one layer (forward, input gradient,
                 weight and bias gradient) of an implementation `impl` against
                 torch fp32 and fp64 on the CPU with the pixel stem's bars
                 (tests/test_gpu_cnn.py): _fp32_as_good_as_torch, slack 2e-6
                 for the forward and 4e-6 for the gradients, `mag` (the largest
                 sum of |terms|) for the weight and bias gradients, whose long
                 sums over n Ho Wo cancel.  The backward runs on the ReLU mask of
                 the forward UNDER TEST.  TorchLayer is a correct fp32 impl;
                 FAULTY maps a fault's name to an impl that carries it
                 (tests/test_cpu_qconv_ref.py shows the checker catches each).
  QConvRef       nn.Conv2d(padding = k // 2) + ReLU per layer, x / 255.0 when
                 is_uint8, flatten, then the dueling heads of dqn_ref.FFQfuncRef
  PixLearnerRef  dqn_ref.DQNLearnerRef's step over a QConvRef
  envelope_check_pixels   dqn_ref.envelope_check for uint8 observations: pixels
                 are exact, so the ulp variants perturb the weights, rewards and
                 IS weights only
"""
import copy

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import dqn_ref as R
from tests import views as V

# (cin, H, W), cout, k, stride, pad, uint8 input
GEOMS = {
    'halo_2x5x7': ((2, 5, 7), 3, 3, 1, 1, False),
    'u8_4x20x20': ((4, 20, 20), 8, 8, 4, 4, True),
    'even_16x6x6': ((16, 6, 6), 32, 4, 2, 2, False),
    'odd_3x9x11': ((3, 9, 11), 5, 4, 2, 2, False),
    'parity_3x10x13': ((3, 10, 13), 6, 5, 3, 2, False),
    'k1_7x4x4': ((7, 4, 4), 9, 1, 1, 0, False),
    'tiles_64x12x12': ((64, 12, 12), 64, 3, 1, 1, False),
    'valid_3x8x8': ((3, 8, 8), 4, 8, 4, 0, False),
    'limits_128x3x3': ((128, 3, 3), 128, 3, 1, 1, False),
}
NS = (1, 5)
FWD_SLACK, GRAD_SLACK = 2e-6, 4e-6


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def fp32_as_good_as_torch(got, ref32, ref64, slack, mag=None):
    """tests/test_gpu_ddpg.py::_fp32_as_good_as_torch (the GEMM parity bar) on
    tensors whose shapes must agree"""
    from tests.test_gpu_ddpg import _fp32_as_good_as_torch
    assert tuple(got.shape) == tuple(ref64.shape), (tuple(got.shape), tuple(ref64.shape))
    assert bool(torch.isfinite(torch.as_tensor(got)).all()), 'non-finite values in the result'
    _fp32_as_good_as_torch(got, ref32, ref64, slack, mag)


# ----------------------------------------------------------------- one layer
class LayerCase(object):
    """operands of one layer at n images, generated once (CPU tensors)"""

    def __init__(self, name, n, seed=0):
        (cin, H, W), cout, k, s, p, u8 = GEOMS[name]
        self.name, self.n, self.u8 = name, n, u8
        self.geom = (cin, H, W, cout, k, s, p)
        self.ho, self.wo = out_hw(H, W, k, s, p)
        g = torch.Generator().manual_seed(1000 * seed + 17 * n + sum(map(ord, name)))
        if u8:
            self.x = torch.randint(0, 256, (n, cin, H, W), generator=g, dtype=torch.uint8)
        else:
            self.x = torch.randn(n, cin, H, W, generator=g)
        self.w = torch.randn(cout, cin, k, k, generator=g) / float(np.sqrt(cin * k * k))
        self.b = 0.5 * torch.randn(cout, generator=g)
        self.dy = torch.randn(n, cout, self.ho, self.wo, generator=g)
        # the layer's own input activation as the mask of dx: exact zeros and a few -0.0
        self.mask = V.relu_mask(n, cin * H * W, g).reshape(n, cin, H, W)


def ref_forward(c, dtype, div255, act=True):
    cin, H, W, cout, k, s, p = c.geom
    x = c.x.to(dtype)
    if div255:
        x = x / 255.0
    y = F.conv2d(x, c.w.to(dtype), c.b.to(dtype), stride=s, padding=p)
    return torch.relu(y) if act else y


def ref_backward(c, dtype, div255, dz, mask=True):
    """(dx, dw, db) of sum(y * dz) for the pre-activation y; dx masked by c.mask > 0"""
    cin, H, W, cout, k, s, p = c.geom
    x = c.x.to(dtype)
    if div255:
        x = x / 255.0
    x = x.clone().requires_grad_(True)
    w = c.w.to(dtype).clone().requires_grad_(True)
    b = c.b.to(dtype).clone().requires_grad_(True)
    y = F.conv2d(x, w, b, stride=s, padding=p)
    y.backward(dz.to(dtype))
    dx = x.grad * (c.mask > 0) if mask else x.grad
    return dx, w.grad, b.grad


def grad_mags(c, div255, dz):
    """largest sum of |terms| of one dw and of one db element"""
    cin, H, W, cout, k, s, p = c.geom
    x = c.x.double().abs()
    if div255:
        x = x / 255.0
    x = x.requires_grad_(True)
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, None, stride=s, padding=p).backward(dz.double().abs())
    return float(w.grad.max()), float(dz.double().abs().sum(dim=(0, 2, 3)).max())


def check_layer(impl, c, div255=False):
    """every output of `impl` on LayerCase c against torch; raises AssertionError.
    impl.forward(c, div255) -> y (ReLU applied); impl.backward_input(c, dz) -> dx
    masked by c.mask; impl.backward_weight(c, dz, div255) -> (dw, db)."""
    y = torch.as_tensor(impl.forward(c, div255)).cpu()
    fp32_as_good_as_torch(y, ref_forward(c, torch.float32, div255),
                          ref_forward(c, torch.float64, div255), FWD_SLACK)
    dz = c.dy * (y > 0)                      # the masks of the forward under test
    dx32, dw32, db32 = ref_backward(c, torch.float32, div255, dz)
    dx64, dw64, db64 = ref_backward(c, torch.float64, div255, dz)
    if not c.u8:                             # (the first layer needs no input gradient)
        dx = torch.as_tensor(impl.backward_input(c, dz)).cpu()
        fp32_as_good_as_torch(dx, dx32, dx64, GRAD_SLACK)
        assert not bool((dx[c.mask <= 0] != 0).any()), 'dx is not zero where the mask is <= 0'
    dw, db = impl.backward_weight(c, dz, div255)
    mw, mb = grad_mags(c, div255, dz)
    fp32_as_good_as_torch(torch.as_tensor(dw).cpu(), dw32, dw64, GRAD_SLACK, mw)
    fp32_as_good_as_torch(torch.as_tensor(db).cpu(), db32, db64, GRAD_SLACK, mb)


class TorchLayer(object):
    """a correct fp32 layer in torch (and the base of the faulty ones)"""

    def conv(self, c, x, w, b):
        cin, H, W, cout, k, s, p = c.geom
        return F.conv2d(x, w, b, stride=s, padding=p)

    def scale(self, x, div255):
        return x / 255.0 if div255 else x

    def forward(self, c, div255):
        return torch.relu(self.conv(c, self.scale(c.x.float(), div255), c.w, c.b))

    def _grads(self, c, dz, div255):
        x = self.scale(c.x.float(), div255).clone().requires_grad_(True)
        w, b = c.w.clone().requires_grad_(True), c.b.clone().requires_grad_(True)
        y = self.conv(c, x, w, b)
        if y.shape != dz.shape:
            raise AssertionError('output shape')
        y.backward(dz)
        return x.grad, w.grad, b.grad

    def backward_input(self, c, dz):
        return self._grads(c, dz, False)[0] * (c.mask > 0)

    def backward_weight(self, c, dz, div255):
        return self._grads(c, dz, div255)[1:]


class _OneSidePad(TorchLayer):             # zero halo on the top / left only
    def conv(self, c, x, w, b):
        cin, H, W, cout, k, s, p = c.geom
        x = F.pad(x, (p, 0, p, 0))
        if p:
            x = F.pad(x, (0, p, 0, p), mode='replicate')
        return F.conv2d(x, w, b, stride=s)


class _TfSame(TorchLayer):                 # TF 'SAME': total pad from ceil(H / s), extra at the end
    def conv(self, c, x, w, b):
        cin, H, W, cout, k, s, p = c.geom
        ph = max((-(-H // s) - 1) * s + k - H, 0)
        pw = max((-(-W // s) - 1) * s + k - W, 0)
        return F.conv2d(F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)), w, b, stride=s)


class _PadKm1(TorchLayer):                 # pad = (k - 1) // 2 where k // 2 was asked for
    def conv(self, c, x, w, b):
        cin, H, W, cout, k, s, p = c.geom
        return F.conv2d(x, w, b, stride=s, padding=(k - 1) // 2 if p == k // 2 else p)


class _SwapHW(TorchLayer):                 # the image read as [W][H]
    def conv(self, c, x, w, b):
        cin, H, W, cout, k, s, p = c.geom
        y = F.conv2d(x.reshape(x.shape[0], cin, W, H), w, b, stride=s, padding=p)
        return y.reshape(y.shape[0], cout, y.shape[3], y.shape[2])


class _StrideOneAxis(TorchLayer):          # stride ignored along x
    def conv(self, c, x, w, b):
        cin, H, W, cout, k, s, p = c.geom
        return F.conv2d(x, w, b, stride=(s, 1), padding=p)[..., :c.wo]


class _NoDiv255(TorchLayer):
    def scale(self, x, div255):
        return x


class _GeMask(TorchLayer):
    def backward_input(self, c, dz):
        return self._grads(c, dz, False)[0] * (c.mask >= 0)


class _DwDropsLast(TorchLayer):
    def backward_weight(self, c, dz, div255):
        db = self._grads(c, dz, div255)[2]
        cut = dz.clone()
        cut[-1] = 0
        return self._grads(c, cut, div255)[1], db


class _NoDb(TorchLayer):
    def backward_weight(self, c, dz, div255):
        dw, db = self._grads(c, dz, div255)[1:]
        return dw, torch.zeros_like(db)


# fault -> (impl, (geometry, n, div255) of a case the checker must fail on)
FAULTY = {
    'pad_one_side': (_OneSidePad(), ('halo_2x5x7', 5, False)),
    'tf_same': (_TfSame(), ('u8_4x20x20', 1, True)),
    'pad_k_minus_1': (_PadKm1(), ('even_16x6x6', 5, False)),
    'swap_hw': (_SwapHW(), ('odd_3x9x11', 1, False)),
    'stride_one_axis': (_StrideOneAxis(), ('parity_3x10x13', 5, False)),
    'no_div255': (_NoDiv255(), ('u8_4x20x20', 5, True)),
    'ge_mask': (_GeMask(), ('tiles_64x12x12', 1, False)),
    'dw_drops_last_image': (_DwDropsLast(), ('halo_2x5x7', 5, False)),
    'no_db': (_NoDb(), ('k1_7x4x4', 1, False)),
}


# ------------------------------------------------------------------ the model
def conv_shapes(input_shape, convs):
    """[(cin, H, W, cout, k, s, pad)] per layer and the pre-FC shape (q_net.py:85-102)"""
    C, H, W = input_shape
    out = []
    for cout, k, s in convs:
        out.append((C, H, W, cout, k, s, k // 2))
        H, W = out_hw(H, W, k, s, k // 2)
        C = cout
    return out, (C, H, W)


class QConvRef(R.FFQfuncRef):
    def __init__(self, input_shape, A, convs, hidden, dueling, is_uint8, dtype=torch.float32):
        nn.Module.__init__(self)
        self.is_uint8 = bool(is_uint8)
        layers, shape = conv_shapes(input_shape, convs)
        self.conv_layers = nn.ModuleList(
            [nn.Conv2d(ci, co, k, stride=s, padding=p) for ci, _, _, co, k, s, p in layers])
        if min(shape) < 1:
            raise ValueError('Pre-FC shape has invalid size: {}'.format(shape))
        self.prelinear_size = int(np.prod(shape))
        self.dueling = bool(dueling)
        hiddens = [self.prelinear_size] + list(hidden)
        mk = lambda out: nn.ModuleList([nn.Linear(a, b) for a, b in               # noqa: E731
                                        zip(hiddens + [out], (hiddens + [out])[1:])])
        self.fc_action_layers = mk(A)
        if self.dueling:
            self.fc_state_layers = mk(1)
        self.to(dtype)
        self.trace = None

    def features(self, x):
        if self.is_uint8:
            x = x / 255.0
        for conv in self.conv_layers:
            z = conv(x)
            if self.trace is not None and z.requires_grad:
                z.retain_grad()
                self.trace.append((conv, x, z))
            x = torch.relu(z)
        return x.flatten(1)

    def streams(self, x):
        return R.FFQfuncRef.streams(self, self.features(x))


class PixLearnerRef(R.DQNLearnerRef):
    def __init__(self, lc, input_shape, A, dtype=torch.float32, fault=None):
        self.algo, self.dtype, self.fault, self.A = lc.algo, dtype, fault, A
        self.q_func = QConvRef(input_shape, A, lc.model.convs, lc.model.fc_hidden_sizes,
                               lc.model.dueling, lc.model.get('is_uint8', True), dtype)
        self.q_target = copy.deepcopy(self.q_func)
        self.optimizer = torch.optim.Adam(self.q_func.parameters(), lr=self.algo.lr, eps=1e-4)
        self.tracker = R.RefTracker(self.algo.target_network_update_freq)
        self.last = {}


class QAgentPixRef(R.QAgentRef):
    def __init__(self, lc, input_shape, A, agent_mode='training'):
        R.QAgentRef.__init__(self, lc, 1, A, agent_mode)
        self.q_func = QConvRef(input_shape, A, lc.model.convs, lc.model.fc_hidden_sizes,
                               lc.model.dueling, lc.model.get('is_uint8', True))


# name -> (B, input shape, convs, hidden, A, dueling, double_q, weights, is_uint8, seed);
# seeds picked on the CPU for the arg-max margin (tests/test_cpu_qconv_ref.py)
NATURE = [[32, 8, 4], [64, 4, 2], [64, 3, 1]]
PIX_CASES = {
    'pix_small': (24, (4, 20, 20), [[8, 8, 4], [16, 4, 2], [16, 3, 1]], [32], 3, True, True, True,
                  True, 0),
    'pix_plain': (24, (2, 9, 11), [[6, 3, 2]], [16, 8], 3, False, False, False, False, 0),
    'pix_atari': (8, (4, 84, 84), NATURE, [64], 6, True, True, True, True, 0),
}
PIX_STEPS = 3


def pix_config(B, convs, hidden, dueling=True, double_q=True, is_uint8=True):
    lc = R.dqn_config(B, hidden, dueling, double_q)
    lc.model.convs = [list(c) for c in convs]
    lc.model.is_uint8 = bool(is_uint8)
    return lc


def pix_init(lc, input_shape, A, seed):
    out = {}
    for name, s in (('q_func', 1000 + seed), ('q_target', 2000 + seed)):
        torch.manual_seed(s)
        net = QConvRef(input_shape, A, lc.model.convs, lc.model.fc_hidden_sizes, lc.model.dueling,
                       lc.model.is_uint8)
        out[name] = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return out


def pix_batches(B, input_shape, A, seed, weights=True, steps=PIX_STEPS):
    """dqn_ref.dqn_batches with uint8 frames"""
    out = []
    for it in range(steps):
        g = torch.Generator().manual_seed(31 * seed + it + 5)
        b = {'obs': torch.randint(0, 256, (B,) + tuple(input_shape), generator=g,
                                  dtype=torch.uint8).numpy(),
             'actions': torch.randint(0, A, (B, 1), generator=g).numpy().astype(np.int32),
             'rewards': (1.5 * torch.randn(B, 1, generator=g)).numpy(),
             'obs_next': torch.randint(0, 256, (B,) + tuple(input_shape), generator=g,
                                       dtype=torch.uint8).numpy(),
             'dones': (torch.rand(B, 1, generator=g) < 0.2).float().numpy()}
        if weights:
            b['weights'] = (0.3 + 0.7 * torch.rand(B, 1, generator=g)).numpy()
        out.append(b)
    return out


def pix_case(name):
    B, shape, convs, hidden, A, dueling, double_q, weights, u8, seed = PIX_CASES[name]
    lc = pix_config(B, convs, hidden, dueling, double_q, u8)
    return lc, shape, A, pix_init(lc, shape, A, seed), pix_batches(B, shape, A, seed, weights)


# ------------------------------------------------------------------ envelope
NOISY_KEYS = ('rewards', 'weights')


class _PixVariant(R._Variant):
    def __init__(self, kind, key, lc, shape, A, init):
        self.kind, self.key = kind, key
        self.ref = PixLearnerRef(lc, shape, A, torch.float32 if kind == 'order' else torch.float64)
        self.gen = torch.Generator().manual_seed(555 + 13 * key if kind == 'ulp' else 0)
        self.ref.load(init, self._noisy if kind == 'ulp' else None)

    def optimize(self, b, it):
        B = b['rewards'].shape[0]
        if self.kind == 'order':
            p = (np.arange(B) if self.key == 'given' else np.arange(B)[::-1].copy()
                 if self.key == 'reversed' else np.random.RandomState(50 + it).permutation(B))
            x = {k: np.asarray(v)[p] for k, v in b.items()}
        else:
            p = np.arange(B)
            x = {k: (self._noisy(v) if k in NOISY_KEYS else v) for k, v in b.items()}
        stats, td = self.ref.optimize(x['obs'], x['actions'], x['rewards'], x['obs_next'],
                                      x['dones'], x.get('weights'))
        out = np.empty(B)
        out[p] = td.double().numpy()
        return stats, out


def run_pix_reference(lc, shape, A, init, batches, dtype=torch.float32, fault=None):
    ref = PixLearnerRef(lc, shape, A, dtype, fault)
    ref.load(init)
    got = []
    for b in batches:
        stats, td = ref.optimize(b['obs'], b['actions'], b['rewards'], b['obs_next'], b['dones'],
                                 b.get('weights'))
        got.append((ref.state(), stats, td.double().numpy()))
    return got


def envelope_check_pixels(lc, shape, A, init, batches, got, n_ulp=6):
    """dqn_ref.envelope_check (same bars) over PixLearnerRef and uint8 frames"""
    from tests import parity as P
    r64 = PixLearnerRef(lc, shape, A, torch.float64)
    r64.load(init)
    vs = [_PixVariant('order', k, lc, shape, A, init) for k in R.ORDERS]
    vs += [_PixVariant('ulp', k, lc, shape, A, init) for k in range(1, n_ulp + 1)]
    report = {}
    for it, b in enumerate(batches):
        f64 = lambda k: torch.as_tensor(b[k], dtype=torch.float32).double()        # noqa: E731
        s64, td64 = r64.optimize(b['obs'], b['actions'], f64('rewards'), b['obs_next'],
                                 f64('dones'), f64('weights') if 'weights' in b else None)
        res = [v.optimize(b, it) for v in vs]
        state, stats, td = got[it]
        p64 = r64.state()
        for k in p64:
            w, sc = P.width(p64[k], [v.ref.state()[k] for v in vs])
            P.check(f'{k}@{it}', state[k], p64[k], w, sc, report)
        w, sc = P.width(td64.numpy(), [r[1] for r in res])
        P.check(f'td_error@{it}', td, td64.numpy(), w, sc, report)
        for k in s64:
            w = max(abs(r[0][k] - s64[k]) for r in res)
            e, sc = abs(stats[k] - s64[k]), max(abs(s64[k]), 1e-30)
            bar = max(2 * w + 1e-6 * sc, 1e-5 * sc)
            ok = e <= bar
            report[f'stat:{k}@{it}'] = (e / sc, bar / sc, ok, w / sc)
            if not ok:
                report.setdefault('_fail', []).append(f'stat:{k}@{it}')
    return report
