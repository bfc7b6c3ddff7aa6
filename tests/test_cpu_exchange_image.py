"""device_learner.exchange_image on CPU tensors (no GPU): the layout
[gradient | pad to a multiple of 4 floats | tails...] that one all-reduce of a
data-parallel learn() carries."""
import pytest
import torch

from surreal_amd.device_learner import exchange_image

CEIL4 = {1: 4, 4: 4, 5: 8, 8: 8}


@pytest.mark.parametrize('tails', [(6,), (6, 2)])
@pytest.mark.parametrize('n', [1, 4, 5, 8])
def test_layout(n, tails):
    buf, grad, views = exchange_image(torch.device('cpu'), n, tails)
    n4 = CEIL4[n]
    assert buf.dtype == torch.float32 and buf.dim() == 1 and buf.numel() == n4 + sum(tails)
    assert not buf.any()
    assert len(views) == len(tails)
    base = buf.data_ptr()
    assert grad.data_ptr() == base and tuple(grad.shape) == (n,)
    offsets = [n4, n4 + 6][:len(tails)]
    for v, off, m in zip(views, offsets, tails):
        assert v.data_ptr() == base + 4 * off and tuple(v.shape) == (m,)
    for v in [grad] + list(views):
        assert v.is_contiguous() and v.dtype == torch.float32
    # the views alias the buffer; the pad belongs to none of them and stays zero
    grad.fill_(1.0)
    for k, v in enumerate(views):
        v.fill_(2.0 + k)
    assert torch.equal(buf[:n], torch.ones(n)) and not buf[n:n4].any()
    for k, (off, m) in enumerate(zip(offsets, tails)):
        assert torch.equal(buf[off:off + m], torch.full((m,), 2.0 + k))
