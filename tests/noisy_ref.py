"""Noisy linear layers on the CPU: plain torch in the dtype it is given (the
noisy weight W_mu + W_sig * outer(f_out, f_in) is materialised), and the draw of
smi_noisy_draw by tests.iqn_ref's numpy Philox4x32-10 with Box-Muller in fp32
or fp64."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.iqn_ref import philox


def linear(x, wmu, wsig, bmu, bsig, fi, fo):
    return F.linear(x, wmu + wsig * torch.outer(fo, fi), bmu + bsig * fo)


def draw(seed, step, stream_id, widths, dtype=np.float64):
    """(f, eps) images [sum(in + out)] of the layers [(in, out), ...]"""
    fs, es = [], []
    for l, (k, n) in enumerate(widths):
        e = np.arange(k + n, dtype=np.uint32)
        ctr = np.stack([e, np.full_like(e, l), np.full_like(e, step), np.full_like(e, stream_id)], 1)
        x = philox((seed & 0xFFFFFFFF, seed >> 32), ctr)
        u1, u2 = (((x[:, i] >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23 for i in (0, 1))
        u1, u2 = u1.astype(dtype), u2.astype(dtype)            # exact in fp32
        eps = np.sqrt(dtype(-2) * np.log(u1)) * np.cos(dtype(np.pi) * (dtype(2) * u2))
        es.append(eps.astype(dtype))
        fs.append((np.sign(eps) * np.sqrt(np.abs(eps))).astype(dtype))
    return np.concatenate(fs), np.concatenate(es)

