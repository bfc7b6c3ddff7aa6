"""The kernels of ops_kernels.hip at the edges of their dispatch, against fp64.

Adam with its clips, DiagGauss, the ZFilter apply and column statistics,
moments and the RewardFilter, each at the sizes, alignments and argument
subsets at which the launchers of ops_kernels.hip take another kernel, loop or
tail, compared with the float64 references of tests/ops_ref.py (which
tests/test_cpu_ops_ref.py checks against torch / the oracle).  Bars (ops_ref):
fp32 elementwise outputs 1e-5 (helpers.max_rel_err), Adam's m with the step's
largest effective gradient as the floor, norm_out one fp32 rounding, fp64 sums
1e-9 of the sum of |terms|, fp32 column sums L * 2^-24 * sum |x| with L the
kernels' longest addition chain, and bit equality for guards, skip paths and
the partial / commit pair.

Every output and in-place operand is an interior slice of a larger allocation
filled with a NaN bit pattern; the elements around the slice must come back
bit-unchanged.  Unaligned operands start 1 or 2 floats past a 16-byte boundary.

The NaN tests state the filters' contract: torch.clamp propagates NaN, so a
NaN observation, or a column / reward filter whose variance went negative,
gives NaN exactly where the fp32 oracle has it; +-inf become +-5.
"""
import math

import pytest
import torch

from oracle import ppo_ref as R
from surreal_amd import _lib as L
from tests import ops_ref as O
from tests.helpers import max_rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD = 16                                # guard elements on each side (keeps 16-byte alignment)
SENT32 = 0x7FC5A5A5                     # a quiet NaN: a guard that is read poisons the result
SENT64 = 0x7FF5A5A5A5A5A5A5
SMI_E_NOFIT = -2


def st():
    return L.stream()


def setup_module(m):
    L.ensure_workspace(DEV)


def last():
    return L.lib().smi_last_launch().decode()


class Guarded(object):
    """n elements, `off` elements past a 16-byte boundary, inside a sentinel-filled allocation"""

    def __init__(self, n, off=0, dtype=torch.float32, init=None):
        raw_t, self.sent = (torch.int64, SENT64) if dtype == torch.float64 else (torch.int32, SENT32)
        self.lo, self.hi = PAD + off, PAD + off + n
        self.raw = torch.full((self.hi + PAD,), self.sent, dtype=raw_t, device=DEV)
        self.t = self.raw.view(dtype)[self.lo:self.hi]
        assert self.t.data_ptr() % 16 == (off * self.t.element_size()) % 16
        if init is not None:
            self.t.copy_(init.reshape(-1))

    def ptr(self):
        return L.ptr(self.t)

    def intact(self):
        return bool((self.raw[:self.lo] == self.sent).all()) and bool((self.raw[self.hi:] == self.sent).all())

    def untouched(self):
        return bool((self.raw == self.sent).all())

    def cpu(self):
        return self.t.cpu()


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    return bool(torch.equal(bits(a.cpu()), bits(b.cpu())))


# --------------------------------------------------------------------- Adam
def _adam_call(p, g, m, v, n, step, lr, k, skip=None, norm=None):
    L.call('smi_adam_clip', p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, step.ptr(), L.ptr(lr), O.ADAM_B1,
           O.ADAM_B2, k['eps'], k['wd'], k['max_norm'], k['clip_value'],
           None if skip is None else L.ptr(skip), None if norm is None else norm.ptr(), st())


def _adam_state(n, align):
    offs = O.ADAM_ALIGN[align]
    z = torch.zeros(n)
    p = Guarded(n, offs[0], init=O.adam_params(n, 0))
    g = Guarded(n, offs[1], init=z)
    m, v = Guarded(n, offs[2], init=z), Guarded(n, offs[3], init=z)
    step = Guarded(1, dtype=torch.int32, init=torch.zeros(1, dtype=torch.int32))
    return p, g, m, v, step


def _adam_steps(n, setting, align, steps, ref_dev='cpu', with_norm=True):
    """`steps` steps; after each, p, m, v, norm_out and step against the fp64
    reference stepped from the same fp32 state"""
    k = O.adam_scalars(setting)
    p, g, m, v, step = _adam_state(n, align)
    lr = torch.tensor([O.ADAM_LR], device=DEV)
    norm = Guarded(1) if with_norm else None
    err = O.rel_err_t if ref_dev != 'cpu' else max_rel_err
    for s in range(steps):
        grad = O.adam_grad(n, s, 0)
        g.t.copy_(grad)
        before = [x.t.to(ref_dev, copy=True) for x in (p, m, v)]
        _adam_call(p, g, m, v, n, step, lr, k, norm=norm)
        rp, rm, rv, rnorm, geff = O.adam_ref(before[0], grad.to(ref_dev), before[1], before[2],
                                             s + 1, **k)
        got = [x.t.to(ref_dev) for x in (p, m, v)]
        tag = (n, setting, align, s)
        assert err(got[0], rp) < O.RTOL, tag
        assert err(got[2], rv) < O.RTOL, tag
        assert err(got[1], rm, floor=float(geff.abs().max())) < O.RTOL, tag
        if with_norm:
            assert abs(float(norm.t.item()) - rnorm) <= O.NORM_RTOL * rnorm, tag
        assert int(step.t.item()) == s + 1
        assert same_bits(g.t, grad)
        for x in (p, g, m, v, step) + ((norm,) if with_norm else ()):
            assert x.intact(), tag
    return p, g, m, v, step, lr, k


@pytest.mark.parametrize('align', sorted(O.ADAM_ALIGN))
@pytest.mark.parametrize('setting', O.ADAM_SETTINGS, ids=lambda s: '-'.join(map(str, s)))
@pytest.mark.parametrize('n', O.ADAM_SIZES)
def test_adam_sizes_settings_alignments(n, setting, align):
    # n % 4 != 0: the scalar tail; any operand off a 16-byte boundary: adam_kernel
    # all scalar; g alone decides for sumsq_partial_kernel, so 'p_offset' runs a
    # vector norm and a scalar update, 'g_offset' (the learners' packed gradient)
    # both scalar
    _adam_steps(n, setting, align, O.ADAM_STEPS)


def test_adam_grid_stride_pass():
    # 2048 workgroups x 256 threads x 4 entries + 1029: threads 0..256 take a
    # second float4, one entry is left to the scalar tail
    assert O.ADAM_GRID_STRIDE_N > 2048 * 256 * 4 and O.ADAM_GRID_STRIDE_N % 4 == 1
    _adam_steps(O.ADAM_GRID_STRIDE_N, O.ADAM_SETTINGS[5], 'aligned', 3, ref_dev=DEV)


def test_adam_nontemporal_form():
    # n >= 2^24: adam_kernel<3> (nontemporal loads and stores), 3 entries of tail
    assert O.ADAM_NT_N >= 1 << 24 and O.ADAM_NT_N % 4 == 3
    _adam_steps(O.ADAM_NT_N, O.ADAM_SETTINGS[1], 'aligned', 2, ref_dev=DEV)


@pytest.mark.parametrize('align', ('aligned', 'g_offset'))
@pytest.mark.parametrize('setting', (O.ADAM_SETTINGS[1], O.ADAM_SETTINGS[2]),
                         ids=lambda s: '-'.join(map(str, s)))
def test_adam_skip_flag_and_null_norm(setting, align):
    n = 1025
    # norm_out == NULL: with max_norm > 0 the norm is still formed and applied
    p, g, m, v, step, lr, k = _adam_steps(n, setting, align, 2, with_norm=False)
    # skip != 0: nothing moves, the step counter included
    before = [x.t.clone() for x in (p, g, m, v, step)]
    skip = torch.ones(1, dtype=torch.int32, device=DEV)
    norm = Guarded(1)
    _adam_call(p, g, m, v, n, step, lr, k, skip=skip, norm=norm)
    for x, b in zip((p, g, m, v, step), before):
        assert same_bits(x.t, b) and x.intact()
    assert norm.intact()
    # skip == 0 on the device: a step like any other
    skip.zero_()
    _adam_call(p, g, m, v, n, step, lr, k, skip=skip, norm=norm)
    rp, rm, rv, rnorm, geff = O.adam_ref(before[0].cpu(), before[1].cpu(), before[2].cpu(),
                                         before[3].cpu(), 3, **k)
    assert max_rel_err(p.cpu(), rp) < O.RTOL and max_rel_err(v.cpu(), rv) < O.RTOL
    assert max_rel_err(m.cpu(), rm, floor=float(geff.abs().max())) < O.RTOL
    assert abs(float(norm.t.item()) - rnorm) <= O.NORM_RTOL * rnorm and int(step.t.item()) == 3


# ---------------------------------------------------------------- DiagGauss
DG_OUTS = ('loglik', 'lik', 'kl', 'ent')


def _dg_run(A, rows, outs=DG_OUTS, offs=(0, 0, 0), ref_dev='cpu'):
    """smi_diag_gauss with the outputs `outs` (the others NULL) and the operands
    (actions, prob0, prob1) `offs` floats past a 16-byte boundary"""
    a, p0, p1 = O.dg_inputs(A, rows)
    need_a, need_p1 = 'loglik' in outs or 'lik' in outs, 'kl' in outs
    ga = Guarded(rows * A, offs[0], init=a) if need_a else None
    gp0 = Guarded(rows * 2 * A, offs[1], init=p0)
    gp1 = Guarded(rows * 2 * A, offs[2], init=p1) if need_p1 else None
    o = {name: Guarded(rows) for name in outs}
    L.call('smi_diag_gauss', ga.ptr() if ga else None, gp0.ptr(), gp1.ptr() if gp1 else None, rows, A,
           *[o[name].ptr() if name in o else None for name in DG_OUTS], st())
    used = [off for off, x in zip(offs, (ga, gp0, gp1)) if x is not None]
    rows_form = A <= 8 and not any(used)
    assert last() == ('diag_gauss_rows_kernel' if rows_form else 'diag_gauss_kernel')
    ref = O.dg_ref(a.to(ref_dev) if need_a else None, p0.to(ref_dev),
                   p1.to(ref_dev) if need_p1 else None, A)
    err = O.rel_err_t if ref_dev != 'cpu' else max_rel_err
    for name in outs:
        assert err(o[name].t.to(ref_dev), ref[name]) < O.RTOL, (A, rows, name, offs)
        assert o[name].intact(), (A, rows, name, offs)
    for x, src in ((ga, a), (gp0, p0), (gp1, p1)):
        assert x is None or (x.intact() and same_bits(x.t, src.reshape(-1)))
    return {name: o[name].cpu() for name in outs}


@pytest.mark.parametrize('rows', O.DG_ROWS)
@pytest.mark.parametrize('A', O.DG_ROW_A)
def test_diag_gauss_row_kernels(A, rows):
    # diag_gauss_rows_kernel<A>: float / float2 / float4 row loads by A; rows
    # 1, 2, 255, 257: the clamped loads of the row tail; 513: a second workgroup
    _dg_run(A, rows)


@pytest.mark.parametrize('which,off', (('actions', 1), ('prob0', 2), ('prob1', 1)))
@pytest.mark.parametrize('A', O.DG_ROW_A)
def test_diag_gauss_unaligned_takes_the_lds_kernel(A, which, off):
    offs = tuple(off if which == w else 0 for w in ('actions', 'prob0', 'prob1'))
    _dg_run(A, 257, offs=offs)


@pytest.mark.parametrize('rows', (1, 255, 257, 513))
@pytest.mark.parametrize('A', O.DG_LDS_A)
def test_diag_gauss_lds_kernel(A, rows):
    # A = 12, 16, 32: 16-byte staging; 9, 31: scalar staging; 32: a 192-row tile
    _dg_run(A, rows)


@pytest.mark.parametrize('outs', [(n,) for n in DG_OUTS] + [('lik', 'kl'), ('kl', 'ent')],
                         ids=lambda o: '+'.join(o))
@pytest.mark.parametrize('A', (3, 8, 9, 32))
def test_diag_gauss_output_subsets(A, outs):
    full = _dg_run(A, 300)
    part = _dg_run(A, 300, outs=outs)
    for name in outs:
        assert same_bits(part[name], full[name]), (A, outs, name)


def test_diag_gauss_row_kernel_second_pass():
    rows, A = O.DG_ROWS_2ND_PASS
    assert rows > 2 * 256 * 8192
    _dg_run(A, rows, ref_dev=DEV)


def test_diag_gauss_lds_kernel_second_pass():
    rows, A = O.DG_LDS_2ND_PASS
    assert rows > 4096 * 256 and O.dg_tile_rows(A) == 256
    _dg_run(A, rows, ref_dev=DEV)


def test_diag_gauss_widest_that_fits_and_first_that_does_not():
    A = O.dg_first_rejected()
    assert O.dg_tile_rows(A - 1) == 64
    _dg_run(A - 1, 130, outs=('loglik', 'kl', 'ent'))              # three 64-row tiles
    a, p0, p1 = O.dg_inputs(A, 3)
    ga, gp0, gp1 = Guarded(3 * A, init=a), Guarded(6 * A, init=p0), Guarded(6 * A, init=p1)
    o = [Guarded(3) for _ in DG_OUTS]
    rc = L.lib().smi_diag_gauss(ga.ptr(), gp0.ptr(), gp1.ptr(), 3, A, *[x.ptr() for x in o], st())
    torch.cuda.synchronize()
    assert rc == SMI_E_NOFIT
    assert all(x.untouched() for x in o)


# ------------------------------------------------------------ ZFilter apply
@pytest.mark.parametrize('mode', ('aligned', 'offset', 'in_place', 'in_place_offset'))
@pytest.mark.parametrize('rows,dim', O.ZF_SHAPES)
def test_zfilter_apply_shapes(rows, dim, mode):
    # dim < 4: a float4 spans several rows (the column wraps inside it); dim =
    # 1025, 17: rows that start off a 16-byte boundary; offset: all scalar
    state = O.zf_state(dim)
    x = O.zf_input(rows, dim)
    n = rows * dim
    offx, offo = {'aligned': (0, 0), 'offset': (1, 2), 'in_place': (0, 0), 'in_place_offset': (1, 1)}[mode]
    gx = Guarded(n, offx, init=x)
    go = gx if mode.startswith('in_place') else Guarded(n, offo)
    sd = [Guarded(s.numel(), init=s) for s in state]
    L.call('smi_zfilter_apply', gx.ptr(), go.ptr(), rows, dim, *[s.ptr() for s in sd],
           O.f32(O.ZF_EPS), st())
    assert last() == 'zfilter_apply_kernel'
    ref = O.zf_apply_ref(x, *state, O.f32(O.ZF_EPS))
    assert max_rel_err(go.cpu().view(rows, dim), ref) < O.RTOL
    assert go.intact() and gx.intact()
    if go is not gx:
        assert same_bits(gx.t, x.reshape(-1))
    for s, src in zip(sd, state):
        assert s.intact() and same_bits(s.t, src)


# -------------------------------------------------------- column statistics
@pytest.mark.parametrize('pad', (0, 3))
@pytest.mark.parametrize('rows,dim', O.COL_SMALL + O.COL_PARTIAL)
def test_column_statistics(rows, dim, pad):
    stride = dim + pad
    host = O.col_input(rows, dim, stride)
    xd = host.to(DEV)
    x = host[:, :dim]
    s, q = O.colsums_ref(x)
    sabs = x.double().abs().sum(0)
    # smi_zfilter_colstats: the sums alone
    form, chain = O.col_chain(rows, dim, False)
    gs, gq = Guarded(dim), Guarded(dim)
    L.call('smi_zfilter_colstats', L.ptr(xd), rows, dim, stride, gs.ptr(), gq.ptr(), st())
    assert last() == form
    assert bool(((gs.cpu().double() - s).abs() <= O.col_bound(chain, sabs)).all())
    assert bool(((gq.cpu().double() - q).abs() <= O.col_bound(chain, q, square=True)).all())
    assert gs.intact() and gq.intact()
    # smi_zfilter_update: added to running buffers that are not zero
    g = torch.Generator().manual_seed(rows + dim)
    rs0 = torch.randn(dim, generator=g) * 5.0 + 3.0
    rq0 = torch.rand(dim, generator=g) * 50.0 + 10.0
    c0 = torch.tensor([123.0 + 1e-5])
    form, chain = O.col_chain(rows, dim, True)
    rs, rq, cnt = Guarded(dim, init=rs0), Guarded(dim, init=rq0), Guarded(1, init=c0)
    L.call('smi_zfilter_update', L.ptr(xd), rows, dim, stride, rs.ptr(), rq.ptr(), cnt.ptr(), st())
    assert last() == form
    assert bool(((rs.cpu().double() - (rs0.double() + s)).abs() <=
                 O.col_bound(chain, rs0.double().abs() + sabs)).all())
    assert bool(((rq.cpu().double() - (rq0.double() + q)).abs() <=
                 O.col_bound(chain, rq0.double() + q, square=True)).all())
    assert same_bits(cnt.t, c0 + torch.tensor([float(rows)]))          # one fp32 addition
    assert rs.intact() and rq.intact() and cnt.intact()
    assert same_bits(xd, host)


# ------------------------------------------------------------------ moments
@pytest.mark.parametrize('off', (0, 1))
@pytest.mark.parametrize('n', O.MOM_SIZES)
def test_moments_sizes(n, off):
    # <= 65536: one workgroup; 65537: 33 workgroups, paired and single float4
    # loads; 65539: + 3 entries of scalar tail; 2^21 + 5: the grid capped at
    # 1024, thread 0 alone takes a third float4; off = 1: all scalar
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 3.0 + 1.0
    gx = Guarded(n, off, init=x)
    out = Guarded(3, dtype=torch.float64)
    L.call('smi_moments', gx.ptr(), n, None, 0, out.ptr(), st())
    assert last() == 'moments_kernel'
    s, q, sabs = O.moments_ref(x)
    o = out.cpu()
    assert abs(float(o[0]) - s) <= O.SUM64_RTOL * sabs
    assert abs(float(o[1]) - q) <= O.SUM64_RTOL * q
    assert float(o[2]) == n
    assert out.intact() and gx.intact() and same_bits(gx.t, x)


@pytest.mark.parametrize('np_', O.MOM_NP)
def test_moments_of_partials(np_):
    g = torch.Generator().manual_seed(np_)
    part = torch.randn(np_, 2, generator=g, dtype=torch.float64) * 100.0
    part[:, 1] = part[:, 1].abs()
    pd = part.to(DEV)
    out = Guarded(3, dtype=torch.float64)
    L.call('smi_moments', None, 12345, L.ptr(pd), np_, out.ptr(), st())
    o = out.cpu()
    assert abs(float(o[0]) - float(part[:, 0].sum())) <= O.SUM64_RTOL * float(part[:, 0].abs().sum())
    assert abs(float(o[1]) - float(part[:, 1].sum())) <= O.SUM64_RTOL * float(part[:, 1].sum())
    assert float(o[2]) == 12345 and out.intact()


# ------------------------------------------------------------- RewardFilter
class _RF(object):
    """a reward filter's three buffers on the device, guarded"""

    def __init__(self, state):
        self.b = [Guarded(1, init=s) for s in state]

    def ptrs(self):
        return [x.ptr() for x in self.b]

    def host(self):
        return [x.cpu() for x in self.b]

    def intact(self):
        return all(x.intact() for x in self.b)


def _rf_check_update(got, before, x32, tag):
    """the filter after update(x32) from `before` (fp32 buffers on the host)"""
    s3, sabs = O.rf_sums_ref(x32)
    new = O.rf_update_ref(*before, s3)
    # running_sum: the fp64 sum (1e-9) is cast to fp32 and added in fp32, two roundings
    assert abs(float(got[0]) - float(new[0])) <= \
        (2 * O.U32 + O.SUM64_RTOL) * (abs(float(before[0])) + sabs), tag
    # running_sumsq: the fp64 sum cast to fp32, one rounding
    assert abs(float(got[1]) - float(new[1])) <= (O.U32 + O.SUM64_RTOL) * float(s3[1]), tag
    # count: one fp32 addition
    assert same_bits(got[2], before[2] + torch.tensor([float(x32.numel())])), tag
    return s3, sabs


@pytest.mark.parametrize('mode', (0, 1, 2, 3))
@pytest.mark.parametrize('n', O.RF_SIZES)
def test_reward_filter_modes(n, mode):
    # one workgroup strides over the rewards: 255, 256, 257 around one trip
    rf = _RF(O.rf_init(mode))
    scale, eps = O.f32(O.RF_SCALE), O.f32(O.RF_EPS)
    for rnd in range(O.RF_ROUNDS):
        r = O.rf_rewards(n, rnd)
        x32 = r * torch.tensor(scale)                              # the kernel's fp32 product
        before = rf.host()
        gr = Guarded(n, init=r)
        L.call('smi_reward_filter', gr.ptr(), n, scale, mode, *rf.ptrs(), eps, st())
        tag = (n, mode, rnd)
        if mode & 1:
            ref = O.rf_forward_ref(x32, *before, eps)
            assert O.same_nans(gr.cpu(), ref), tag
            assert O.max_rel_err_finite(gr.cpu(), ref) < O.RTOL, tag
        else:
            assert same_bits(gr.t, x32), tag
        if mode & 2:
            _rf_check_update(rf.host(), before, x32, tag)
        else:
            assert all(same_bits(a, b) for a, b in zip(rf.host(), before)), tag
        assert gr.intact() and rf.intact(), tag


@pytest.mark.parametrize('n', O.RF_SIZES)
def test_reward_filter_partial_commit_is_the_single_call(n):
    one, two = _RF(O.rf_init(3)), _RF(O.rf_init(3))
    scale, eps = O.f32(O.RF_SCALE), O.f32(O.RF_EPS)
    for rnd in range(O.RF_ROUNDS):
        r = O.rf_rewards(n, rnd)
        x32 = r * torch.tensor(scale)
        ga, gb = Guarded(n, init=r), Guarded(n, init=r)
        s3 = Guarded(3, dtype=torch.float64)
        L.call('smi_reward_filter', ga.ptr(), n, scale, 3, *one.ptrs(), eps, st())
        before = two.host()
        L.call('smi_reward_filter_partial', gb.ptr(), n, scale, 1, *two.ptrs(), eps, s3.ptr(), st())
        assert all(same_bits(a, b) for a, b in zip(two.host(), before))      # _partial only reads
        ref3, sabs = O.rf_sums_ref(x32)
        got3 = s3.cpu()
        assert abs(float(got3[0]) - float(ref3[0])) <= O.SUM64_RTOL * sabs
        assert abs(float(got3[1]) - float(ref3[1])) <= O.SUM64_RTOL * float(ref3[1])
        assert float(got3[2]) == n
        L.call('smi_reward_filter_commit', s3.ptr(), *two.ptrs(), st())
        assert same_bits(ga.t, gb.t), (n, rnd)
        assert all(same_bits(a, b) for a, b in zip(one.host(), two.host())), (n, rnd)
        assert ga.intact() and gb.intact() and s3.intact() and one.intact() and two.intact()


@pytest.mark.parametrize('n', (257, 5000))
def test_reward_filter_two_ranks(n):
    # two _partial calls, the sums added in fp64, one _commit: the filter and
    # the rewards of the whole batch
    rf = _RF(O.rf_init(3))
    scale, eps = O.f32(O.RF_SCALE), O.f32(O.RF_EPS)
    h = n // 2 + 1
    for rnd in range(O.RF_ROUNDS):
        r = O.rf_rewards(n, rnd)
        x32 = r * torch.tensor(scale)
        before = rf.host()
        parts = [Guarded(h, init=r[:h]), Guarded(n - h, init=r[h:])]
        sums = [Guarded(3, dtype=torch.float64) for _ in parts]
        for gr, s3 in zip(parts, sums):
            L.call('smi_reward_filter_partial', gr.ptr(), gr.t.numel(), scale, 1, *rf.ptrs(), eps,
                   s3.ptr(), st())
        tot = Guarded(3, dtype=torch.float64, init=sums[0].t + sums[1].t)
        L.call('smi_reward_filter_commit', tot.ptr(), *rf.ptrs(), st())
        tag = (n, rnd)
        ref = O.rf_forward_ref(x32, *before, eps)
        got = torch.cat([p.cpu() for p in parts])
        assert O.same_nans(got, ref) and O.max_rel_err_finite(got, ref) < O.RTOL, tag
        _rf_check_update(rf.host(), before, x32, tag)
        assert all(x.intact() for x in parts + sums) and rf.intact(), tag


# ---------------------------------------------------------- NaN faithfulness
def _oracle_zf(dim, state):
    zf = R.ZFilterRef(dim, eps=O.f32(O.ZF_EPS))
    for buf, val in zip((zf.running_sum, zf.running_sumsq, zf.count), state):
        buf.copy_(val)
    return zf


def _check_filtered(got, x, state, tag=None):
    """`got` = the z-filtered x [rows, dim]: NaN exactly where the fp32 oracle
    has it, +-5 for +-inf, every other entry on the numeric bar"""
    dim = x.shape[-1]
    oracle = _oracle_zf(dim, state)(x)
    ref = O.zf_apply_ref(x, *state, O.f32(O.ZF_EPS))
    assert O.same_nans(oracle, ref)
    nan_got, nan_exp = torch.isnan(got), torch.isnan(oracle)
    assert torch.equal(nan_got, nan_exp), \
        (tag, 'NaN expected, got', got[nan_exp & ~nan_got][:4].tolist())
    col = torch.isfinite(state[1] / state[2] - (state[0] / state[2]) ** 2) & \
        (state[1] / state[2] - (state[0] / state[2]) ** 2 >= 0)
    pinf, ninf = torch.isposinf(x) & col, torch.isneginf(x) & col
    assert bool((got[pinf] == 5).all()) and bool((got[ninf] == -5).all()), tag
    assert O.max_rel_err_finite(got, ref) < O.RTOL, tag


@pytest.mark.parametrize('off', (0, 1))
@pytest.mark.parametrize('rows,dim', ((23, 8), (9, 5)))
def test_nan_zfilter_apply(rows, dim, off):
    state, x = O.nan_filter_state(dim), O.nan_filter_input(rows, dim)
    gx, go = Guarded(rows * dim, off, init=x), Guarded(rows * dim, off)
    sd = [s.to(DEV) for s in state]
    L.call('smi_zfilter_apply', gx.ptr(), go.ptr(), rows, dim, *[L.ptr(s) for s in sd],
           O.f32(O.ZF_EPS), st())
    _check_filtered(go.cpu().view(rows, dim), x, state)
    assert go.intact()


@pytest.mark.parametrize('B,T,S,D,ldo', ((7, 3, 4, 8, 8), (5, 2, 3, 7, 8), (3, 2, 3, 71, 72),
                                         (9, 3, 4, 42, 44), (70, 3, 4, 6, 8)))
def test_nan_zfilter_tmajor_forms(B, T, S, D, ldo):
    state = O.nan_filter_state(D)
    full = O.nan_filter_input(B * S, D).view(B, S, D)
    obs, nxt = full[:, :T].contiguous(), full[:, T:].contiguous()
    exp_x = full.transpose(0, 1).reshape(S * B, D)
    od, nd = obs.to(DEV), nxt.to(DEV)
    sd = [s.to(DEV) for s in state]
    ran = []
    for form in (1, 2, 3, 4, 5):
        if (form == 2 and D % 2) or (form >= 4 and ldo != (D + 3) // 4 * 4):
            continue
        out = torch.full((S * B, ldo), -7.0, device=DEV)
        L.call('smi_zfilter_tmajor', L.ptr(od), L.ptr(nd), B, T, S, D, 1, *[L.ptr(s) for s in sd],
               O.f32(O.ZF_EPS), L.ptr(out), ldo, form, st())
        _check_filtered(out.cpu()[:, :D], exp_x, state, tag=form)
        ran.append(form)
    assert 1 in ran and 3 in ran


@pytest.mark.parametrize('neg_var', (False, True))
def test_nan_mlp_forward_with_zfilter(neg_var):
    # a NaN observation makes its row of the output NaN and no other; a column
    # with negative variance makes every row NaN
    rows, d_in, h, d_out = 70, 8, 16, 2
    torch.manual_seed(11)
    m = R.MLP3(d_in, h, h, d_out, True)
    state, x = O.nan_filter_state(d_in, neg_var), O.nan_filter_input(rows, d_in)
    zf = _oracle_zf(d_in, state)
    oracle = m(zf(x)).detach()
    ref = m.double()(O.zf_apply_ref(x, *state, O.f32(O.ZF_EPS))).detach()
    assert O.same_nans(oracle, ref)
    nan_rows = torch.isnan(oracle).any(1)
    assert bool(nan_rows.all()) if neg_var else (0 < int(nan_rows.sum()) < rows)
    fd, xd = m.float().flat().to(DEV), x.to(DEV)
    sd = [s.to(DEV) for s in state]
    out = Guarded(rows * d_out)
    L.call('smi_mlp_forward', L.ptr(fd), d_in, h, h, d_out, 2, 0, L.ptr(xd), rows, d_in, 1,
           *[L.ptr(s) for s in sd], O.f32(O.ZF_EPS), out.ptr(), st())
    got = out.cpu().view(rows, d_out)
    assert torch.equal(torch.isnan(got), torch.isnan(oracle)), got[nan_rows][:3].tolist()
    assert O.max_rel_err_finite(got, ref) < O.RTOL
    assert out.intact()


@pytest.mark.parametrize('neg_var', (False, True))
def test_nan_critic_gae_values(neg_var):
    # the z-filter inside smi_ppo_critic_gae: values[b][t] is NaN for a NaN
    # observation (b, t) and for no other
    B, T, D, h = 9, 4, 8, 16
    torch.manual_seed(12)
    m = R.MLP3(D, h, h, 1, False)
    state = O.nan_filter_state(D, neg_var)
    full = O.nan_filter_input(B * (T + 1), D).view(B, T + 1, D)
    full[:, :, 2] = torch.nan_to_num(full[:, :, 2], nan=0.25)     # NaN in three observations only
    for b, t in ((1, 0), (4, T), (6, 2)):
        full[b, t, 2] = float('nan')
    zf = _oracle_zf(D, state)
    oracle = m(zf(full)).detach().view(B, T + 1)
    ref = m.double()(O.zf_apply_ref(full, *state, O.f32(O.ZF_EPS))).detach().view(B, T + 1)
    fd = m.float().flat().to(DEV)
    od, nd = full[:, :T].contiguous().to(DEV), full[:, T].contiguous().to(DEV)
    rew, dones = torch.ones(B, T, device=DEV), torch.zeros(B, T, device=DEV)
    idx = torch.arange(T, dtype=torch.float32)
    gt, lt = torch.pow(0.99, idx).to(DEV), torch.pow(0.95, idx).to(DEV)
    sd = [s.to(DEV) for s in state]
    vals, adv, ret = Guarded(B * (T + 1)), Guarded(B), Guarded(B)
    L.call('smi_ppo_critic_gae', L.ptr(fd), D, h, h, 1, *[L.ptr(s) for s in sd], O.f32(O.ZF_EPS),
           L.ptr(od), L.ptr(nd), L.ptr(rew), L.ptr(dones), B, T, L.ptr(gt), L.ptr(lt), 0.99,
           0.99 ** T, vals.ptr(), adv.ptr(), ret.ptr(), st())
    got = vals.cpu().view(B, T + 1)
    assert torch.equal(torch.isnan(got), torch.isnan(oracle)), got[torch.isnan(oracle)][:4].tolist()
    assert O.max_rel_err_finite(got, ref) < O.RTOL
    seg_nan = torch.isnan(oracle).any(1)
    assert bool(seg_nan.all()) if neg_var else 0 < int(seg_nan.sum()) < B
    # the advantage sums the TD errors of every step, the return reads values[:, T] alone
    assert torch.equal(torch.isnan(adv.cpu()), seg_nan)
    assert torch.equal(torch.isnan(ret.cpu()), torch.isnan(oracle[:, T]))
    assert vals.intact() and adv.intact() and ret.intact()


def _oracle_rf(state):
    rf = R.RewardFilterRef(eps=O.f32(O.RF_EPS))
    rf.running_sum, rf.running_sumsq, rf.count = (s.clone().reshape(()) for s in state)
    return rf


@pytest.mark.parametrize('partial', (False, True))
def test_nan_reward_filter_direct_state(partial):
    n = 300
    eps = O.f32(O.RF_EPS)
    r = O.rf_rewards(n, 0)
    r[::7] = float('nan')
    r[1::7] = float('inf')
    r[2::7] = float('-inf')
    # variance -0.5, variance exactly 0 (std = eps), an ordinary filter; count = 4
    for state in ((4.0, 2.0, 4.0), (8.0, 16.0, 4.0), (2.0, 7.0, 4.0)):
        state = [torch.tensor([v]) for v in state]
        oracle = _oracle_rf(state).forward(r)
        ref = O.rf_forward_ref(r, *state, eps)
        assert O.same_nans(oracle, ref)
        gr, rf = Guarded(n, init=r), _RF(state)
        if partial:
            s3 = Guarded(3, dtype=torch.float64)
            L.call('smi_reward_filter_partial', gr.ptr(), n, 1.0, 1, *rf.ptrs(), eps, s3.ptr(), st())
        else:
            L.call('smi_reward_filter', gr.ptr(), n, 1.0, 1, *rf.ptrs(), eps, st())
        got = gr.cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(oracle)), \
            (state, got[torch.isnan(oracle)][:4].tolist())
        if state[0].item() != 4.0:
            assert bool((got[1::7] == 5).all()) and bool((got[2::7] == -5).all())
        assert O.max_rel_err_finite(got, ref) < O.RTOL
        assert gr.intact() and rf.intact()


def test_nan_reward_filter_onset():
    # rewards of mean 1.0, std 0.3: the `=` of the update makes the variance
    # negative from the third batch on; NaN from the same round as the oracle
    oracle, rf = _oracle_rf(O.rf_init(3)), _RF(O.rf_init(3))
    eps = O.f32(O.RF_EPS)
    onset = onset_exp = None
    for rnd, x in enumerate(O.rf_nan_sequence()):
        before = rf.host()
        exp = oracle.forward(x)
        oracle.update(x)
        gr = Guarded(x.numel(), init=x)
        L.call('smi_reward_filter', gr.ptr(), x.numel(), 1.0, 3, *rf.ptrs(), eps, st())
        got = gr.cpu()
        if onset_exp is None and bool(torch.isnan(exp).any()):
            onset_exp = rnd
        if onset is None and bool(torch.isnan(got).any()):
            onset = rnd
        assert torch.equal(torch.isnan(got), torch.isnan(exp)), (rnd, got[:4].tolist())
        assert O.max_rel_err_finite(got, O.rf_forward_ref(x, *before, eps)) < O.RTOL, rnd
    assert onset == onset_exp == 2
