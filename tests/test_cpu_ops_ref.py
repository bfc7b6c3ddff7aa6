"""The fp64 references of the ops kernels and the inputs of their GPU tests (host only).

tests/test_gpu_ops_edges.py compares the kernels of ops_kernels.hip with the
references of tests/ops_ref.py.  Here

  * each reference is checked against something independent: Adam against
    torch.optim.Adam with clip_grad_value_ / clip_grad_norm_ in float64,
    DiagGauss and the two filters against oracle.ppo_ref run on doubles, the
    sums against math.fsum;
  * the inputs of the GPU file are shown to exercise what they are meant to:
    rows on both sides of the likelihood clamp and of the filters' +-5 clamp,
    gradients on both sides of the value and norm clips, the NaN onset of the
    reward filter's `=`;
  * the fp32 oracle (torch in float32) is shown to stay inside every bar on
    those inputs, so a bar is never tighter than fp32 itself allows.
"""
import math

import pytest
import torch

from oracle import ppo_ref as R
from tests import ops_ref as O
from tests.helpers import max_rel_err


def _torch_adam(n, setting, dtype, betas, seed=0):
    """torch.optim.Adam over ADAM_STEPS steps; yields (state before, grad, state after, norm)"""
    wd, max_norm, clip_value, eps = setting
    p = torch.nn.Parameter(O.adam_params(n, seed).to(dtype))
    opt = torch.optim.Adam([p], lr=O.f32(O.ADAM_LR), betas=betas, eps=O.f32(eps),
                           weight_decay=O.f32(wd))
    for step in range(O.ADAM_STEPS):
        grad = O.adam_grad(n, step, seed)
        st = opt.state[p]
        before = (p.detach().clone(),
                  st['exp_avg'].clone() if st else torch.zeros(n, dtype=dtype),
                  st['exp_avg_sq'].clone() if st else torch.zeros(n, dtype=dtype))
        p.grad = grad.to(dtype).clone()
        norm = None
        if clip_value > 0:
            torch.nn.utils.clip_grad_value_([p], O.f32(clip_value))
        if max_norm > 0:
            norm = float(torch.nn.utils.clip_grad_norm_([p], O.f32(max_norm)))
        opt.step()
        st = opt.state[p]
        yield step, before, grad, (p.detach().clone(), st['exp_avg'].clone(),
                                   st['exp_avg_sq'].clone()), norm


@pytest.mark.parametrize('setting', O.ADAM_SETTINGS)
@pytest.mark.parametrize('n', (5, 1025))
def test_adam_ref_is_torch_adam_in_fp64(n, setting):
    k = O.adam_scalars(setting)
    for step, before, grad, after, norm in _torch_adam(n, setting, torch.float64, (k['b1'], k['b2'])):
        p, m, v, rnorm, _ = O.adam_ref(*before[:1], grad, *before[1:], step + 1, **k)
        for got, exp in zip((p, m, v), after):
            assert max_rel_err(got, exp) < 1e-12
        if norm is not None:
            assert abs(rnorm - norm) <= 1e-12 * norm


def test_adam_inputs_reach_both_sides_of_the_clips():
    for n in O.ADAM_SIZES:
        for wd, max_norm, clip_value, eps in O.ADAM_SETTINGS:
            for step in range(O.ADAM_STEPS):
                g = O.adam_grad(n, step, 0).double()
                if clip_value > 0 and n >= 1023:
                    share = float((g.abs() > clip_value).double().mean())
                    assert (share > 0.1) if step % 2 == 0 else (share == 0.0), (n, clip_value, step)
                if step == 2 and n >= 3:
                    assert float((g == 0).double().mean()) >= 0.3
    # the norm clip: a setting and step with coefficient < 1 and one with 1, at every size
    for n in O.ADAM_SIZES:
        sides = set()
        for wd, max_norm, clip_value, eps in O.ADAM_SETTINGS:
            if max_norm > 0:
                for step in range(O.ADAM_STEPS):
                    sides.add(float(O.adam_grad(n, step, 0).double().norm()) > max_norm)
        assert sides == {True, False}, n


def test_abi_rounds_beta2():
    # why the references take their scalars rounded to fp32: the library gets
    # beta2 as a float, and 1 - fp32(0.999) is not 1e-3 to the 1e-5 of the bars
    assert abs((1.0 - O.f32(0.999)) / 1e-3 - 1.0) > 1e-5


@pytest.mark.parametrize('setting', O.ADAM_SETTINGS)
def test_fp32_adam_stays_inside_the_bars(setting):
    # torch's fp32 Adam against the reference stepped from the same fp32 state
    # (exact betas here: torch rounds 1 - beta2, not beta2)
    k = O.adam_scalars(setting)
    k['b1'], k['b2'] = O.ADAM_B1, O.ADAM_B2
    for n in (1025, 4099):
        for step, before, grad, after, norm in _torch_adam(n, setting, torch.float32,
                                                           (O.ADAM_B1, O.ADAM_B2)):
            p, m, v, rnorm, geff = O.adam_ref(before[0], grad, before[1], before[2], step + 1, **k)
            assert max_rel_err(after[0], p) < O.RTOL
            assert max_rel_err(after[2], v) < O.RTOL
            assert max_rel_err(after[1], m, floor=float(geff.abs().max())) < O.RTOL


# ---------------------------------------------------------------- DiagGauss
@pytest.mark.parametrize('A', O.DG_ROW_A + O.DG_LDS_A + (O.dg_first_rejected() - 1,))
def test_diag_gauss_ref_inputs_and_fp32(A):
    ref = R.DiagGaussRef(A)
    for rows in O.DG_ROWS:
        a, p0, p1 = O.dg_inputs(A, rows)
        r64 = O.dg_ref(a, p0, p1, A)
        ad, p0d, p1d = a.double(), p0.double(), p1.double()
        assert max_rel_err(r64['loglik'], ref.loglikelihood(ad, p0d).view(-1)) < 1e-12
        assert max_rel_err(r64['lik'], ref.likelihood(ad, p0d).view(-1)) < 1e-12
        assert max_rel_err(r64['kl'], ref.kl(p0d, p1d)) < 1e-12
        assert max_rel_err(r64['ent'], ref.entropy(p0d)) < 1e-12
        # the fp32 oracle inside the bar
        assert max_rel_err(ref.loglikelihood(a, p0).view(-1), r64['loglik']) < O.RTOL
        if A <= 32:     # wider: exp() of a log-likelihood of +-40 magnifies its fp32 rounding past the bar
            assert max_rel_err(ref.likelihood(a, p0).view(-1), r64['lik']) < O.RTOL
        assert max_rel_err(ref.kl(p0, p1), r64['kl']) < O.RTOL
        assert max_rel_err(ref.entropy(p0), r64['ent']) < O.RTOL
        if rows >= 255 and A <= 32:
            clamped = float((r64['loglik'] < math.log(O.CLAMP_LIK)).double().mean())
            assert 0.1 <= clamped <= 0.9, (A, rows, clamped)


def test_diag_gauss_tile_rows():
    for A in range(1, 32):
        assert O.dg_tile_rows(A) == 256            # every width that fit one 256-row tile: unchanged
    assert O.dg_tile_rows(32) == 192
    assert 256 * O.dg_row_floats(32) * 4 == 166912
    A = O.dg_first_rejected()
    assert A == 128 and O.dg_tile_rows(A - 1) == 64
    assert 64 * O.dg_row_floats(A - 1) * 4 <= O.LDS_CAP < 64 * O.dg_row_floats(A) * 4


# ------------------------------------------------------------------ ZFilter
def _oracle_zf(dim, state, dtype):
    zf = R.ZFilterRef(dim, eps=O.f32(O.ZF_EPS)).to(dtype)
    for buf, val in zip((zf.running_sum, zf.running_sumsq, zf.count), state):
        buf.copy_(val.to(dtype))
    return zf


def test_zfilter_ref_inputs_and_fp32():
    lo = hi = tot = 0
    for rows, dim in O.ZF_SHAPES:
        st = O.zf_state(dim)
        x = O.zf_input(rows, dim)
        ref = O.zf_apply_ref(x, *st, O.f32(O.ZF_EPS))
        assert max_rel_err(ref, _oracle_zf(dim, st, torch.float64)(x.double())) < 1e-12
        assert max_rel_err(_oracle_zf(dim, st, torch.float32)(x), ref) < O.RTOL
        lo += int((ref == -5).sum()); hi += int((ref == 5).sum()); tot += ref.numel()
    assert lo >= 0.03 * tot and hi >= 0.03 * tot and lo + hi <= 0.5 * tot


def test_nan_filter_state_in_the_oracle():
    rows, dim = 23, 8
    st, x = O.nan_filter_state(dim), O.nan_filter_input(rows, dim)
    y = _oracle_zf(dim, st, torch.float32)(x)
    ref = O.zf_apply_ref(x, *st, O.f32(O.ZF_EPS))
    assert O.same_nans(y, ref)
    assert bool(torch.isnan(y[:, 0]).all())                       # negative variance
    assert torch.equal(torch.isnan(y[:, 2]), torch.isnan(x[:, 2])) and bool(torch.isnan(y[::3, 2]).all())
    assert not bool(torch.isnan(y[:, [1] + list(range(3, dim))]).any())
    assert bool((y[::2, 1] == 0).all()) and bool((y[1::2, 1].abs() == 5).all())   # std = eps
    assert bool((y[1::5, 3] == 5).all()) and bool((y[2::5, 3] == -5).all())
    assert O.max_rel_err_finite(y, ref) < O.RTOL


# ------------------------------------------------------------------- sums
def test_colsums_and_moments_refs():
    x = O.col_input(37, 5, 8)[:, :5]
    assert O.rel_err_t(x + 1e-3, x) == max_rel_err(x + 1e-3, x)
    s, q = O.colsums_ref(x)
    for c in range(5):
        col = [float(v) for v in x[:, c]]
        assert abs(float(s[c]) - math.fsum(col)) <= 1e-13 * math.fsum(abs(v) for v in col)
        assert abs(float(q[c]) - math.fsum(v * v for v in col)) <= 1e-13 * math.fsum(v * v for v in col)
    v = [float(t) for t in x.reshape(-1)]
    m = O.moments_ref(x.reshape(-1))
    assert abs(m[0] - math.fsum(v)) <= 1e-13 * m[2] and abs(m[1] - math.fsum(t * t for t in v)) <= 1e-13 * m[1]


@pytest.mark.parametrize('rows,dim', O.COL_SMALL + O.COL_PARTIAL)
def test_colstats_forms_and_fp32_inside_the_bound(rows, dim):
    form, L = O.col_chain(rows, dim, False)
    assert form == ('colstats_small_kernel' if (rows, dim) in O.COL_SMALL else 'colstats_finish_kernel')
    assert 1 <= L <= rows + 8
    x = O.col_input(rows, dim, dim + 3)[:, :dim]
    s, q = O.colsums_ref(x)
    assert float(x.double().mean()) > 0.5                                          # a non-zero mean
    assert bool(((x.sum(0).double() - s).abs() <= O.col_bound(L, x.double().abs().sum(0))).all())
    assert bool((((x * x).sum(0).double() - q).abs() <= O.col_bound(L, q, square=True)).all())


# ------------------------------------------------------------- RewardFilter
def _oracle_rf(state, dtype):
    rf = R.RewardFilterRef(eps=O.f32(O.RF_EPS))
    rf.running_sum, rf.running_sumsq, rf.count = (s.to(dtype).reshape(()) for s in state)
    return rf


@pytest.mark.parametrize('n', O.RF_SIZES)
def test_reward_filter_ref_and_fp32(n):
    for mode in (1, 3):
        st = O.rf_init(mode)
        rf32, rf64 = _oracle_rf(st, torch.float32), _oracle_rf(st, torch.float64)
        for rnd in range(O.RF_ROUNDS):
            x = O.rf_rewards(n, rnd) * O.RF_SCALE
            cur = (rf32.running_sum.view(1), rf32.running_sumsq.view(1), rf32.count.view(1))
            ref = O.rf_forward_ref(x, *cur, O.f32(O.RF_EPS))
            # the reference is the oracle run on doubles
            rf64.running_sum, rf64.running_sumsq, rf64.count = (c.double().reshape(()) for c in cur)
            y64 = rf64.forward(x.double())
            assert O.same_nans(ref, y64) and O.max_rel_err_finite(ref, y64) < 1e-12
            # the fp32 oracle inside the bar, NaN where the reference has NaN
            y32 = rf32.forward(x)
            assert O.same_nans(y32, ref), (n, mode, rnd)
            assert O.max_rel_err_finite(y32, ref) < O.RTOL, (n, mode, rnd)
            if mode & 2:
                s3, sabs = O.rf_sums_ref(x)
                new = O.rf_update_ref(*cur, s3)
                rf64.update(x.double())
                assert abs(float(rf64.running_sum) - float(new[0])) <= 1e-12 * sabs
                assert abs(float(rf64.running_sumsq) - float(new[1])) <= 1e-12 * float(s3[1])
                assert float(rf64.count) == float(new[2])
                rf32.update(x)
                assert abs(float(rf32.running_sum) - float(new[0])) <= 1e-5 * sabs
                assert abs(float(rf32.running_sumsq) - float(new[1])) <= 1e-5 * float(s3[1])


def test_reward_filter_nan_onset():
    # mean 1.0, std 0.3: NaN from the third batch on, in fp32 and in fp64
    for dtype in (torch.float32, torch.float64):
        rf = _oracle_rf(O.rf_init(3), dtype)
        onset = None
        for rnd, x in enumerate(O.rf_nan_sequence()):
            y = rf.forward(x.to(dtype))
            if onset is None and bool(torch.isnan(y).any()):
                onset = rnd
                assert bool(torch.isnan(y).all())
            rf.update(x.to(dtype))
        assert onset == 2
