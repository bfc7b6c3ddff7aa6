"""smi_mse_grad_weighted_shard (ddpg_kernels.hip) through the C ABI against
smi_mse_grad_weighted on the same rows (whose numeric bars tests/test_gpu_per.py
and tests/test_gpu_ddpg_kernels.py pin): dq and loss bit for bit, the shard's
rows of td_all bit-equal to q - y, +0.0f in every other entry of the draw,
nothing written past it, and the element-wise sum of the ranks' images equal to
the whole batch's td."""
import pytest
import torch

from surreal_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = 'cuda'
QS = 3                      # q is column 1 of a [rows][3] matrix
CANARY, NCANARY = -77.0, 8
SENTINEL = 9.0

# (n_global, n, row0)
SHAPES = [(1, 1, 0), (96, 32, 0), (96, 32, 32), (96, 32, 64), (771, 257, 0), (771, 257, 257),
          (771, 257, 514), (300, 7, 293)]


def _draw(ng, seed):
    """q (a strided column), y, w of a draw of ng rows"""
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(ng, QS, generator=g).to(DEV)
    y = torch.randn(ng, generator=g).to(DEV)
    w = (torch.rand(ng, generator=g) + 0.05).to(DEV)
    return wide, y, w


def _launch(wide, y, w, n, row0, with_w, with_loss, ng=None):
    """rows [row0, row0 + n): the shard entry into a NaN-filled td_all [ng] with
    canaries behind it (ng given), else smi_mse_grad_weighted.  (dq, loss, td)"""
    p = L.ptr
    q, ys, ws = wide[row0:row0 + n, 1], y[row0:row0 + n], w[row0:row0 + n]
    assert ys.is_contiguous() and ws.is_contiguous()
    dq = torch.full((n,), SENTINEL, device=DEV)
    loss = torch.full((1,), SENTINEL, device=DEV)
    td = torch.full(((ng or n) + NCANARY,), float('nan'), device=DEV)
    td[ng or n:] = CANARY
    head = (p(q), QS, p(ys), p(ws) if with_w else None, n)
    tail = (p(dq), p(loss) if with_loss else None, p(td), L.stream())
    if ng is None:
        L.call('smi_mse_grad_weighted', *head, *tail)
    else:
        L.call('smi_mse_grad_weighted_shard', *head, ng, row0, *tail)
    assert L.lib().smi_last_launch().decode() == 'mse_grad_weighted_kernel'
    torch.cuda.synchronize()
    return dq, loss, td


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('with_loss', [True, False], ids=['loss', 'noloss'])
@pytest.mark.parametrize('with_w', [True, False], ids=['w', 'now'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%d_%d_%d' % s)
def test_shard_against_the_whole_batch_entry_on_the_same_rows(shape, with_w, with_loss):
    ng, n, row0 = shape
    wide, y, w = _draw(ng, seed=ng)
    dq0, loss0, td0 = _launch(wide, y, w, n, row0, with_w, with_loss)
    dq, loss, td = _launch(wide, y, w, n, row0, with_w, with_loss, ng=ng)
    assert _bits(dq, dq0) and not (dq == SENTINEL).any()
    assert _bits(loss, loss0)
    assert (loss == SENTINEL).all() != with_loss
    want = wide[row0:row0 + n, 1] - y[row0:row0 + n]              # one fp32 subtraction per row
    assert _bits(td[row0:row0 + n], want) and _bits(td0[:n], want)
    rest = torch.cat([td[:row0], td[row0 + n:ng]])
    assert (rest.view(torch.int32) == 0).all()                    # +0.0f: not NaN, not -0.0f
    assert (td[ng:] == CANARY).all() and (td0[n:] == CANARY).all()


@pytest.mark.parametrize('ng,cuts', [(96, (0, 32, 64, 96)), (771, (0, 257, 514, 771)),
                                     (300, (0, 293, 300))], ids=['96', '771', '300'])
def test_sum_of_the_ranks_images_is_the_whole_batch_td(ng, cuts):
    wide, y, w = _draw(ng, seed=1000 + ng)
    zrow = cuts[1] - 1                           # q = -0.0, y = +0.0: the difference is -0.0
    wide[zrow, 1], y[zrow] = -0.0, 0.0
    _, _, whole = _launch(wide, y, w, ng, 0, True, True)
    whole = whole[:ng]
    neg0 = torch.tensor([-0.0], device=DEV).view(torch.int32)
    assert whole[zrow:zrow + 1].view(torch.int32) == neg0
    images = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        td = _launch(wide, y, w, hi - lo, lo, True, True, ng=ng)[2][:ng]
        if lo <= zrow < hi:
            assert td[zrow:zrow + 1].view(torch.int32) == neg0
        images.append(td)
    for order in (images, images[::-1]):
        total = order[0].clone()
        for t in order[1:]:
            total += t
        assert torch.equal(total, whole)
        keep = torch.arange(ng, device=DEV) != zrow
        assert _bits(total[keep], whole[keep])
        assert int(total[zrow:zrow + 1].view(torch.int32)) == 0      # -0.0 arrives as +0.0
