"""Host-side references of the pixel stem (test infrastructure only).

CNNStemNetwork on obs / 255: conv 8x8/4 (C -> 16) -> ReLU -> conv 4x4/2
(16 -> 32) -> ReLU -> Flatten -> Linear(F) -> ReLU, for any frame shape.

  * geom(): the frame arithmetic and the library's acceptance conditions
    (cnn_check, cnn_kernels.hip), restated;
  * the torch stem (oracle.ppo_ref.cnn_stem_ref) in fp32 and fp64: stage
    activations, and the masked backward: the ReLU masks are those of the
    forward under test (a pre-activation within fp32 noise of 0 may take either
    side in any two implementations, and the backward is exactly linear given
    the masks), the gradients come from autograd;
  * the time-major row mapping n = t * B + b -> pix[b][t] | pix_next[b];
  * an emulated stem in plain torch fp32 that follows the kernels' arithmetic
    (raw byte values through unfold, the conv-1 sums divided by 255 in the
    epilogue, explicit einsum / fold gradients, dW1 divided by 255 at the end),
    with one-line fault variants.  tests/test_cpu_cnn_ref.py shows that the
    emulation passes the parity bars at every geometry of the GPU case table
    and that each fault fails them: the bars can tell a correct stem from these
    faults at these shapes.
"""
import collections

import torch
import torch.nn.functional as Fn

from oracle import ppo_ref as R
from tests.test_gpu_ddpg import _fp32_as_good_as_torch

FWD_SLACK = 2e-6            # A1, A2, feat (tests/test_gpu_cnn.py)
BWD_SLACK = 4e-6            # the six gradient blocks
FWD_NAMES = ('A1', 'A2', 'feat')
GRAD_NAMES = ('dW1', 'db1', 'dW2', 'db2', 'dWf', 'dbf')

# C, H, W of the GPU case table (tests/test_gpu_cnn_geometry.py carries the purposes)
TABLE = [(3, 20, 20), (3, 24, 20), (3, 64, 36), (3, 36, 52), (3, 68, 116), (3, 28, 324),
         (9, 20, 20), (9, 36, 52), (9, 40, 212), (9, 84, 84)]

FAULTS = ('hw_swap', 'prev_row', 'no_pix_next', 'a1_last_pixel', 'dw2_last_pixel', 'dw1_no_255',
          'mask_ge')

CU_LDS = 160 * 1024         # bytes of LDS of one CU: what one workgroup can have

Geom = collections.namedtuple('Geom', 'C H W H1 W1 P1 H2 W2 P2 img fwd_lds bwd_lds ok')


def geom(C, H, W):
    """Output shapes of the two convolutions, bytes per image, the forward's
    LDS bytes (the 16-byte-aligned image + 16 x P1 floats of A1), the backward's
    (+ dA2, 256 floats of reduction space and the two pixel-offset tables) and
    whether cnn_check accepts the frame (H, W >= 8).  The forward then takes a
    frame with fwd_lds <= CU_LDS, the backward one with bwd_lds <= CU_LDS."""
    H1, W1 = (H - 8) // 4 + 1, (W - 8) // 4 + 1
    H2, W2 = (H1 - 4) // 2 + 1, (W1 - 4) // 2 + 1
    P1, P2 = H1 * W1, H2 * W2
    img = C * H * W
    ok = (C in (3, 9) and H1 >= 4 and W1 >= 4 and H2 >= 1 and W2 >= 1 and (P2 + 15) // 16 <= 6 and
          W % 4 == 0 and img % 16 == 0 and P1 % 4 == 0 and W1 % 2 == 0)
    fwd_lds = (img + 15) // 16 * 16 + 64 * P1
    bwd_lds = fwd_lds + 4 * 32 * P2 + 4 * 256 + 4 * (P1 + P2)
    return Geom(C, H, W, H1, W1, P1, H2, W2, P2, img, fwd_lds, bwd_lds, ok)


def nets(C, H, W, F):
    """the torch stem in fp32 and the same weights in fp64 (seed set by the caller)."""
    net = R.cnn_stem_ref(C, H, W, F)
    net64 = R.cnn_stem_ref(C, H, W, F).double()
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    return net, net64


def _dtype(model):
    return next(model.parameters()).dtype


def stages(model, x):
    """(A1 [N,16,H1,W1], A2 [N, 32*P2], feat [N, F]) of uint8 images x, in the model's dtype."""
    with torch.no_grad():
        xs = x.to(_dtype(model)) / 255.0
        r1 = torch.relu(model[0](xs))
        r2 = torch.relu(model[2](r1))
        out = model[4:](r2)
    return r1, r2.reshape(x.shape[0], -1), out


def masked_grads(model, x, m1, m2, dz):
    """Gradients of sum(fc(z2) * dz) with the ReLUs replaced by the given masks
    (m1 [N,16,H1,W1], m2 [N, 32*P2], bool): the six parameter blocks in module order."""
    dt = _dtype(model)
    rows = x.shape[0]
    model.zero_grad()
    z1 = model[0](x.to(dt) / 255.0) * m1.to(dt)
    z2 = model[2](z1).reshape(rows, -1) * m2.to(dt)
    (model[5](z2) * dz.to(dt)).sum().backward()
    return [p.grad.detach() for p in model.parameters()]


def images(B, T, cam, seed, rows=None):
    """pix [B][T] and pix_next [B][1] of uniform random bytes; with `rows`,
    activation row 0 is all zeros and row rows - 1 all 255."""
    g = torch.Generator().manual_seed(seed)
    pix = torch.randint(0, 256, (B, T) + tuple(cam), generator=g, dtype=torch.uint8)
    pixn = torch.randint(0, 256, (B, 1) + tuple(cam), generator=g, dtype=torch.uint8)
    if rows is not None:
        pix[0, 0] = 0
        t, b = (rows - 1) // B, (rows - 1) % B
        (pix[b, t] if t < T else pixn[b, 0]).fill_(255)
    return pix, pixn


def timemajor_images(pix, pixn, rows, fault=None):
    """[rows] images: row n = t * B + b is pix[b][t] for t < T, pix_next[b] beyond."""
    B, T = pix.shape[:2]
    n = torch.arange(rows)
    t, b = n // B, n % B
    x = pix[b, t.clamp(max=T - 1)]
    late = t >= T
    if bool(late.any()) and fault != 'no_pix_next':
        x[late] = pixn[b[late], 0]
    return x


# ------------------------------------------------------------ emulated stem
def split(flat, g, F):
    """the flat parameter (or gradient) vector as its six blocks, the conv
    weights as [out][in * ky * kx] matrices."""
    sizes = [16 * 64 * g.C, 16, 32 * 256, 32, F * 32 * g.P2, F]
    assert flat.numel() == sum(sizes)
    W1, b1, W2, b2, Wf, bf = torch.split(flat, sizes)
    return W1.reshape(16, -1), b1, W2.reshape(32, 256), b2, Wf.reshape(F, -1), bf


def _cols1(x, g, fault):
    """conv-1 patches of the raw byte values: [N][64 C][P1]."""
    if fault == 'prev_row':
        x = torch.roll(x, 1, 0)
    if fault != 'hw_swap':
        return Fn.unfold(x.float(), 8, stride=4)
    # the window offset oy * 4 * W + ox * 4 with H in W's place (kept inside the image)
    k = torch.arange(64 * g.C)
    p = torch.arange(g.P1)
    ko = (k // 64) * (g.H * g.W) + ((k // 8) % 8) * g.W + k % 8
    po = (p // g.W1) * 4 * g.H + (p % g.W1) * 4
    idx = (ko[:, None] + po[None, :]) % g.img
    return x.reshape(x.shape[0], -1).float()[:, idx]


def emu_forward(flat, x, g, F, fault=None):
    """A1 [N,16,H1,W1], A2 [N, 32*P2], feat [N, F] in the kernels' arithmetic."""
    W1, b1, W2, b2, Wf, bf = split(flat, g, F)
    N = x.shape[0]
    s1 = torch.einsum('ok,nkp->nop', W1, _cols1(x, g, fault))
    a1 = torch.relu(s1 / 255.0 + b1[None, :, None])
    if fault == 'a1_last_pixel':
        a1[:, :, g.P1 - 1] = 0.0
    a1 = a1.reshape(N, 16, g.H1, g.W1)
    s2 = torch.einsum('ok,nkp->nop', W2, Fn.unfold(a1, 4, stride=2))
    a2 = torch.relu(s2 + b2[None, :, None]).reshape(N, -1)
    feat = torch.relu(a2 @ Wf.t() + bf)
    return a1, a2, feat


def emu_backward(flat, x, g, F, a1, a2, dz, fault=None):
    """the six gradient blocks (torch parameter shapes) from the stored A1, A2
    and dz, the gradient at the Linear pre-activation."""
    W1, b1, W2, b2, Wf, bf = split(flat, g, F)
    N = x.shape[0]
    dWf = dz.t() @ a2
    dbf = dz.sum(0)
    da2 = ((dz @ Wf) * (a2 > 0)).reshape(N, 32, g.P2)
    c2 = Fn.unfold(a1, 4, stride=2)
    n2 = g.P2 - 1 if fault == 'dw2_last_pixel' else g.P2
    dW2 = torch.einsum('nop,nkp->ok', da2[:, :, :n2], c2[:, :, :n2])
    db2 = da2.sum((0, 2))
    dc2 = torch.einsum('ok,nop->nkp', W2, da2)
    m1 = (a1 >= 0) if fault == 'mask_ge' else (a1 > 0)
    da1 = (Fn.fold(dc2, (g.H1, g.W1), 4, stride=2) * m1).reshape(N, 16, g.P1)
    dW1 = torch.einsum('nop,nkp->ok', da1, _cols1(x, g, fault))
    if fault != 'dw1_no_255':
        dW1 = dW1 / 255.0
    db1 = da1.sum((0, 2))
    return [dW1.reshape(16, g.C, 8, 8), db1, dW2.reshape(32, 16, 4, 4), db2, dWf, dbf]


# ------------------------------------------------------------------ checks
def failures(names, got, ref32, ref64, slack, mag=None):
    """names of the outputs that miss the parity bar (_fp32_as_good_as_torch);
    mag: {name: largest sum of |terms| of one output} for blocks that use it."""
    bad = []
    for name, a, r32, r64 in zip(names, got, ref32, ref64):
        try:
            _fp32_as_good_as_torch(a.reshape(r32.shape), r32, r64, slack,
                                   None if mag is None else mag.get(name))
        except AssertionError as e:
            bad.append((name, e.args[0] if e.args else None))
    return bad
