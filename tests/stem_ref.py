"""Host-side references of the pixel stem of free shape (test infrastructure only).

The stem of smi_stem_* on obs / 255: n x [Conv2d(cout_i, k_i, stride_i), no
padding -> ReLU] -> Flatten -> Linear(F) -> ReLU, 1 <= n <= 4.

  * factory(): the torch stem (nn.Sequential, the module positions of
    builders.py:11-18); with the default spec it is oracle.ppo_ref.cnn_stem_ref;
  * the stem in fp32 and fp64: stage activations, and the masked backward (the
    ReLU masks are those of the forward under test, as in tests/cnn_ref.py);
  * the GPU case table of tests/test_gpu_stem.py;
  * an emulated stem in plain torch fp32 that follows the kernels' arithmetic
    (raw byte values through unfold, the layer-1 sums divided by 255 in the
    epilogue, explicit einsum / fold gradients, dW1 divided by 255 at the end)
    with one-line fault variants: tests/test_cpu_stem_ref.py shows that the
    emulation passes the failure rule at every case of the table and that each
    fault fails it.

Time-major rows (n = t B + b -> pix[b][t] | pix_next[b]), the images and the
failure rule are those of tests/cnn_ref.py.
"""
import collections

import torch
import torch.nn as nn
import torch.nn.functional as Fn

from tests import cnn_ref as CR

DEFAULT = ((16, 32), (8, 4), (4, 2))

Case = collections.namedtuple('Case', 'id spec F cam B T rows pix_off fused')
# spec = (out_channels, kernel_sizes, strides); the purposes are in tests/test_gpu_stem.py
CASES = [
    Case('c4-20x20', DEFAULT, 8, (4, 20, 20), 3, 2, 9, 0, False),
    Case('w22', DEFAULT, 24, (3, 32, 22), 4, 2, 7, 0, False),
    Case('84x100', DEFAULT, 16, (3, 84, 100), 3, 1, 3, 0, False),
    Case('c1-21x23-off1', DEFAULT, 8, (1, 21, 23), 5, 1, 5, 1, False),
    Case('one-layer', ((8,), (3,), (1,)), 5, (2, 9, 11), 2, 2, 6, 0, False),
    Case('three-layers', ((8, 12, 20), (5, 3, 2), (2, 1, 2)), 16, (3, 30, 26), 2, 3, 8, 0, False),
    Case('72ch-k4s3', ((72,), (4,), (3,)), 8, (5, 19, 16), 4, 1, 4, 0, False),
    Case('four-layers', ((4,) * 4, (2,) * 4, (1,) * 4), 8, (3, 12, 12), 3, 1, 3, 0, False),
    Case('fused-36x52', DEFAULT, 24, (3, 36, 52), 2, 3, 8, 0, True),
]

FAULTS = ('hw_swap', 'no_pix_next', 'prev_row', 'no_255', 'mask_ge', 'stride_off', 'bias_swap')


def layer_shapes(spec, cam):
    """[(cin, h, w, cout, k, s, ho, wo)] per conv layer."""
    c, h, w = cam
    out = []
    for co, k, s in zip(*spec):
        assert h >= k and w >= k, (spec, cam)
        ho, wo = (h - k) // s + 1, (w - k) // s + 1
        out.append((c, h, w, co, k, s, ho, wo))
        c, h, w = co, ho, wo
    return out


def factory(C, H, W, F, channels=DEFAULT[0], kernel_sizes=DEFAULT[1], strides=DEFAULT[2]):
    """CNNStemNetwork (builders.py:8-33) for a conv_spec: conv i at position 2i,
    the Linear at 2n + 1."""
    mods = []
    for cin, _, _, co, k, s, _, _ in layer_shapes((channels, kernel_sizes, strides), (C, H, W)):
        mods += [nn.Conv2d(cin, co, k, s), nn.ReLU()]
    sh = layer_shapes((channels, kernel_sizes, strides), (C, H, W))[-1]
    return nn.Sequential(*mods, nn.Flatten(), nn.Linear(sh[3] * sh[6] * sh[7], F), nn.ReLU())


def nets(spec, cam, F):
    """the torch stem in fp32 and the same weights in fp64 (seed set by the caller)."""
    net = factory(*cam, F, *spec)
    net64 = factory(*cam, F, *spec).double()
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    return net, net64


def fwd_names(n):
    return tuple(f'A{i + 1}' for i in range(n)) + ('feat',)


def grad_names(n):
    return tuple(x for i in range(n) for x in (f'dW{i + 1}', f'db{i + 1}')) + ('dWf', 'dbf')


def _dtype(model):
    return next(model.parameters()).dtype


def stages(model, x, n):
    """[A_1 .. A_n ([N, cout, Ho, Wo]), feat [N, F]] of uint8 images x, in the model's dtype."""
    out = []
    with torch.no_grad():
        h = x.to(_dtype(model)) / 255.0
        for i in range(n):
            h = torch.relu(model[2 * i](h))
            out.append(h)
        out.append(model[2 * n:](h))
    return out


def masked_grads(model, x, masks, dz, n):
    """Gradients of sum(fc(z_n) * dz) with the ReLUs replaced by the given masks
    (masks[i]: bool, A_{i+1}'s shape): the 2n + 2 parameter blocks in module order."""
    dt = _dtype(model)
    model.zero_grad()
    h = x.to(dt) / 255.0
    for i in range(n):
        h = model[2 * i](h)
        h = h * masks[i].reshape(h.shape).to(dt)
    (model[2 * n + 1](h.reshape(x.shape[0], -1)) * dz.to(dt)).sum().backward()
    return [p.grad.detach() for p in model.parameters()]


# ------------------------------------------------------------ emulated stem
def split(flat, shapes, F):
    """the flat parameter vector as [(W_i [cout][cin k k], b_i)] + [(Wf, bf)]."""
    out, o = [], 0
    for cin, _, _, co, k, _, _, _ in shapes:
        nw = co * cin * k * k
        out.append((flat[o:o + nw].reshape(co, -1), flat[o + nw:o + nw + co]))
        o += nw + co
    fl = shapes[-1][3] * shapes[-1][6] * shapes[-1][7]
    out.append((flat[o:o + F * fl].reshape(F, fl), flat[o + F * fl:o + F * fl + F]))
    assert o + F * fl + F == flat.numel()
    return out


def _fault_layer(n):
    """the layer the stride fault sits in: the second, or the only one"""
    return min(1, n - 1)


def _cols(inp, i, sh, n, fault):
    """patches of layer i's input ([N][cin][h][w] floats; raw byte values for
    layer 0): [N][cin k k][Ho Wo]."""
    cin, h, w, co, k, s, ho, wo = sh
    if i == 0 and fault == 'prev_row':
        inp = torch.roll(inp, 1, 0)
    if i == 0 and fault == 'hw_swap':
        # the window offset oy s W + ox s with H in W's place (kept inside the image)
        kk = torch.arange(cin * k * k)
        p = torch.arange(ho * wo)
        ko = (kk // (k * k)) * (h * w) + ((kk // k) % k) * w + kk % k
        po = (p // wo) * s * h + (p % wo) * s
        idx = (ko[:, None] + po[None, :]) % (cin * h * w)
        return inp.reshape(inp.shape[0], -1)[:, idx]
    if fault == 'stride_off' and i == _fault_layer(n):
        # windows at stride s + 1; what lies beyond the frame reads as 0
        need_h, need_w = (ho - 1) * (s + 1) + k, (wo - 1) * (s + 1) + k
        big = Fn.pad(inp, (0, max(need_w - w, 0), 0, max(need_h - h, 0)))
        c = Fn.unfold(big, k, stride=s + 1)
        nw = (big.shape[3] - k) // (s + 1) + 1
        c = c.reshape(inp.shape[0], cin * k * k, -1, nw)[:, :, :ho, :wo]
        return c.reshape(inp.shape[0], cin * k * k, ho * wo)
    return Fn.unfold(inp, k, stride=s)


def _biases(blocks, fault):
    bs = [b for _, b in blocks]
    if fault == 'bias_swap':            # layer 1 adds the Linear layer's bias and the reverse
        b0, bf = bs[0], bs[-1]
        bs[0] = bf[torch.arange(b0.numel()) % bf.numel()]
        bs[-1] = b0[torch.arange(bf.numel()) % b0.numel()]
    return bs


def emu_forward(flat, x, spec, cam, F, fault=None):
    """[A_1 .. A_n, feat] in the kernels' arithmetic."""
    shapes = layer_shapes(spec, cam)
    n = len(shapes)
    blocks = split(flat, shapes, F)
    bs = _biases(blocks, fault)
    N = x.shape[0]
    h = x.float()
    out = []
    for i, sh in enumerate(shapes):
        ssum = torch.einsum('ok,nkp->nop', blocks[i][0], _cols(h, i, sh, n, fault))
        if i == 0 and fault != 'no_255':
            ssum = ssum / 255.0
        h = torch.relu(ssum + bs[i][None, :, None]).reshape(N, sh[3], sh[6], sh[7])
        out.append(h)
    out.append(torch.relu(h.reshape(N, -1) @ blocks[n][0].t() + bs[n]))
    return out


def emu_backward(flat, x, spec, cam, F, acts, dz, fault=None):
    """the 2n + 2 gradient blocks (torch parameter shapes) from the stored
    activations and dz, the gradient at the Linear pre-activation."""
    shapes = layer_shapes(spec, cam)
    n = len(shapes)
    blocks = split(flat, shapes, F)
    N = x.shape[0]
    mask = (lambda a: a >= 0) if fault == 'mask_ge' else (lambda a: a > 0)
    an = acts[n - 1].reshape(N, -1)
    tail = [dz.t() @ an, dz.sum(0)]
    da = ((dz @ blocks[n][0]) * mask(an)).reshape(acts[n - 1].shape)
    grads = [None] * n
    for i in range(n - 1, -1, -1):
        cin, h, w, co, k, s, ho, wo = shapes[i]
        inp = x.float() if i == 0 else acts[i - 1]
        d = da.reshape(N, co, ho * wo)
        dW = torch.einsum('nop,nkp->ok', d, _cols(inp, i, shapes[i], n, fault))
        if i == 0 and fault != 'no_255':
            dW = dW / 255.0
        grads[i] = [dW.reshape(co, cin, k, k), d.sum((0, 2))]
        if i > 0:
            dc = torch.einsum('ok,nop->nkp', blocks[i][0], d)
            da = Fn.fold(dc, (h, w), k, stride=s) * mask(acts[i - 1])
    return [g for pair in grads for g in pair] + tail


failures = CR.failures
images = CR.images
timemajor_images = CR.timemajor_images
