"""smi_dqn_td_shard (dqn_kernels.hip) through the C ABI against smi_dqn_td on
the same inputs (those of tests/test_gpu_dqn_kernels.py, whose numeric bars pin
smi_dqn_td itself): the whole batch as one shard gives smi_dqn_td's bits, and
two shards of a batch of 300 give the full launch's rows bit for bit, TD
buffers whose element-wise sum is the full launch's td, and statistics that sum
to the full launch's.

The statistics bar: each launch rounds an fp64 sum once to fp32, and the fp32
sum of the two shard values rounds once more; the three terms are positive, so
every rounding is at most half a unit in the last place of the total: 2 ulp in
all with the full launch's own rounding, held to 4."""
import numpy as np
import pytest
import torch

from surreal_amd import _lib as L
from tests.test_gpu_dqn_kernels import FORMS, GAMMA, _case

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD = 3
SENTINEL = -77.0


def _dev(c, lo, hi):
    t = lambda k: torch.as_tensor(c[k][lo:hi], dtype=torch.float32).contiguous().to(DEV)   # noqa: E731
    return {k: t(k) for k in ('adv', 'adv_n', 'adv_t', 'val', 'val_n', 'val_t', 'act', 'rew', 'done', 'w')}


def _launch(name, c, lo, hi, A, dueling, double_q, weighted, extra=(), td_rows=None, ldd=None):
    """one launch over rows [lo, hi) of the case; returns (dadv [B][ldd], dval, td, y, stats)"""
    d = _dev(c, lo, hi)
    B = hi - lo
    ldd = ldd or A
    dadv = torch.full((B, ldd), SENTINEL, device=DEV)
    dval = torch.full((B,), SENTINEL, device=DEV)
    td = torch.full((td_rows or B,), float('nan'), device=DEV)
    y = torch.full((B,), float('nan'), device=DEV)
    stats = torch.full((2,), float('nan'), device=DEV)
    p = L.ptr
    L.call(name, p(d['adv']), A, p(d['adv_n']) if double_q else None, A, p(d['adv_t']), A,
           p(d['val']) if dueling else None, 1, p(d['val_n']) if dueling and double_q else None, 1,
           p(d['val_t']) if dueling else None, 1, p(d['act']), 1, p(d['rew']), 1, p(d['done']), 1,
           p(d['w']) if weighted else None, B, *extra, A, GAMMA, dueling, double_q, p(dadv), ldd,
           p(dval) if dueling else None, p(td), p(y), p(stats), L.stream())
    assert L.lib().smi_last_launch().decode() == f'dqn_td_kernel<{dueling},{double_q}>'
    torch.cuda.synchronize()
    return dadv, dval, td, y, stats


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('A', [1, 6, 18])
@pytest.mark.parametrize('form', FORMS, ids=[f'd{f[0]}q{f[1]}' for f in FORMS])
def test_whole_batch_as_one_shard_has_the_bits_of_dqn_td(form, A):
    dueling, double_q = form
    B = 257                                     # a second pass of the 256 threads
    c = _case(B, A, dueling, double_q, seed=40 + A)
    for weighted in (True, False):
        full = _launch('smi_dqn_td', c, 0, B, A, dueling, double_q, weighted)
        shard = _launch('smi_dqn_td_shard', c, 0, B, A, dueling, double_q, weighted, extra=(B, 0))
        for name, a, b in zip(('dadv', 'dval', 'td', 'y', 'stats'), full, shard):
            assert _bits(a, b), (name, weighted)
        assert not torch.isnan(full[2]).any() and not torch.isnan(full[4]).any()


@pytest.mark.parametrize('form', FORMS, ids=[f'd{f[0]}q{f[1]}' for f in FORMS])
def test_two_shards_of_300_cut_at_row_37(form):
    dueling, double_q = form
    Bg, cut, A = 300, 37, 6                     # 37 rows (< 256) and 263 rows (> 256)
    c = _case(Bg, A, dueling, double_q, seed=9)
    full = _launch('smi_dqn_td', c, 0, Bg, A, dueling, double_q, True)
    td_sum = torch.zeros(Bg, device=DEV)
    stats = []
    for lo, hi in ((0, cut), (cut, Bg)):
        dadv, dval, td_all, y, st = _launch('smi_dqn_td_shard', c, lo, hi, A, dueling, double_q,
                                            True, extra=(Bg, lo), td_rows=Bg, ldd=A + PAD)
        assert _bits(dadv[:, :A], full[0][lo:hi]), (lo, hi)
        assert (dadv[:, A:] == SENTINEL).all()                      # padding columns untouched
        if dueling:
            assert _bits(dval, full[1][lo:hi]), (lo, hi)
        else:
            assert (dval == SENTINEL).all()
        assert _bits(y, full[3][lo:hi])
        assert not torch.isnan(td_all).any()                        # every entry written
        assert _bits(td_all[lo:hi], full[2][lo:hi])
        rest = torch.cat([td_all[:lo], td_all[hi:]])
        assert (rest.view(torch.int32) == 0).all()                  # +0.0f, not -0.0f
        td_sum += td_all
        stats.append(st)
    assert _bits(td_sum, full[2])
    total = (stats[0] + stats[1]).cpu().numpy()                     # the fp32 sum an all-reduce forms
    want = full[4].cpu().numpy()
    assert total.dtype == np.float32 and (want > 0).all()
    ulps = np.abs(total.astype(np.float64) - want.astype(np.float64)) / np.spacing(want).astype(np.float64)
    print('statistics: shard sum against the full launch, ulp:', ulps)
    assert (ulps <= 4).all()
